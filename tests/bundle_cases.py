"""Shared by tests/test_bundles_cpu.py and tests/test_bundles_gpu.py: the rendered boards of the bundle tests, their bundles, and the
oracle's records on them -- each computed once per process and never changed afterwards."""
import math

import numpy as np

from isaac_ros_apriltag_amd import synth
from oracle import pyoracle as po
import parity_util as pu

FAM = ("tag36h11",)
_cache = {}


def board_members(cols, rows, pitch, size, first_id=0, family_index=0):
    """Members of a cols x rows board, row-major ids from first_id, centres on a grid of `pitch` metres about the board origin."""
    return [(family_index, first_id + r * cols + c, (c - (cols - 1) / 2.0) * pitch, (r - (rows - 1) / 2.0) * pitch, size)
            for r in range(rows) for c in range(cols)]


def board_tags(members, R, t, K, skip=(), codes=None):
    """Render records ({family, id, H}) of the members of a board with pose (R, t) under K; codes: id -> code word to paint instead."""
    tags = []
    for (_, tid, x, y, size) in members:
        if tid in skip:
            continue
        tg = {"family": FAM[0], "id": tid, "H": synth.homography_from_pose(R, np.asarray(t) + R @ np.array([x, y, 0.0]), K, size)}
        if codes and tid in codes:
            tg["code"] = codes[tid]
        tags.append(tg)
    return tags


def lone_tag(tid, cx, cy, side):
    """A fronto-parallel tag of `side` pixels centred at (cx, cy)."""
    return {"family": FAM[0], "id": tid, "H": np.array([[side / 2.0, 0, cx], [0, side / 2.0, cy], [0, 0, 1.0]])}


# ---- case 1: 640 x 480, a 3 x 2 board at 64 px sides ------------------------------------------------------------------------------------
W1, H1 = 640, 480
SIZE1, PITCH1 = 0.064, 0.088
K1 = np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]])
R1 = synth.rot_xyz(math.radians(6.0), math.radians(-9.0), math.radians(4.0))
T1 = np.array([0.01, 0.045, 0.6])
MEMBERS1 = board_members(3, 2, PITCH1, SIZE1)
BUNDLE1 = {"name": "board", "members": MEMBERS1, "max_hamming": 0, "min_decision_margin": 0.0, "min_tags": 1}
LONE_ID = 7
# per-frame intrinsics of a three-frame submission (fx, fy, cx, cy) and skews: distinct, the middle frame with a skew
INTR1 = ((600.0, 600.0, 320.0, 240.0), (598.5, 601.25, 318.75, 241.5), (603.0, 597.0, 322.5, 238.25))
SKEW1 = (0.0, 0.75, 0.0)
CONTENT = ("all_six", "painted_over", "non_member", "duplicate", "hamming", "no_tags")
# content case -> (submission, slot): two three-frame submissions
SLOTS = {"all_six": (0, 0), "painted_over": (0, 1), "non_member": (0, 2), "duplicate": (1, 0), "hamming": (1, 1), "no_tags": (1, 2)}


def content_frame(name):
    """The 640 x 480 frame of a content case."""
    if ("frame", name) not in _cache:
        codes36 = synth.family_codes(FAM[0])[0]
        if name == "no_tags":
            tags = []
        elif name == "painted_over":
            tags = board_tags(MEMBERS1, R1, T1, K1, skip=(4,))
        elif name == "hamming":   # one data bit of tag 2 painted wrong: decoded with hamming 1
            tags = board_tags(MEMBERS1, R1, T1, K1, codes={2: codes36[2] ^ (1 << 17)})
        else:
            tags = board_tags(MEMBERS1, R1, T1, K1)
        if name == "non_member":
            tags.append(lone_tag(LONE_ID, 84.0, 80.0, 56.0))
        if name == "duplicate":   # a second copy of member 1, away from the board
            tags.append(lone_tag(1, 84.0, 80.0, 56.0))
        _cache[("frame", name)] = np.ascontiguousarray(synth.render(W1, H1, tags, background=150, sigma=1.0, seed=11 + CONTENT.index(name)))
    return _cache[("frame", name)]


def oracle_records(img, intr, skew=0.0, tag_size=SIZE1, **more):
    """The oracle's records of a frame under the intrinsics (fx, fy, cx, cy) and skew the submission carries."""
    K = np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1.0]])
    if skew:
        more = dict(more, skew=float(skew))
    return po.detect(img, families=FAM, params=pu.oracle_params(K, tag_size=tag_size, **more))[0]


def content_records(name):
    if ("rec", name) not in _cache:
        slot = SLOTS[name][1]
        _cache[("rec", name)] = oracle_records(content_frame(name), INTR1[slot], SKEW1[slot])
    return _cache[("rec", name)]


# ---- case 2: 640 x 576, a 9 x 8 board, 72 tags at 48 px sides ---------------------------------------------------------------------------
W2, H2 = 640, 576
SIZE2, PITCH2 = 0.048, 0.064
K2 = np.array([[800.0, 0, 320.0], [0, 800.0, 288.0], [0, 0, 1]])
R2 = synth.rot_xyz(math.radians(3.0), math.radians(-4.0), math.radians(1.5))
T2 = np.array([0.002, -0.001, 0.8])
MEMBERS2 = board_members(9, 8, PITCH2, SIZE2)
BUNDLE2 = {"name": "board72", "members": MEMBERS2, "max_hamming": 2, "min_decision_margin": 0.0, "min_tags": 4}
INTR2 = (800.0, 800.0, 320.0, 288.0)


def frame72():
    if "frame72" not in _cache:
        _cache["frame72"] = np.ascontiguousarray(synth.render(W2, H2, board_tags(MEMBERS2, R2, T2, K2), background=150, sigma=1.0, seed=72))
    return _cache["frame72"]


def records72():
    if "rec72" not in _cache:
        _cache["rec72"] = oracle_records(frame72(), INTR2, tag_size=SIZE2)
    return _cache["rec72"]


# ---- case 3: two bundles in one frame, and a one-tag bundle (the non_member frame) ------------------------------------------------------
BUNDLES3 = [{"name": "top", "members": MEMBERS1[:3], "max_hamming": 2, "min_decision_margin": 0.0, "min_tags": 2},
            {"name": "bottom", "members": MEMBERS1[3:], "max_hamming": 2, "min_decision_margin": 0.0, "min_tags": 2},
            {"name": "lone", "members": [(0, LONE_ID, 0.0, 0.0, SIZE1)], "max_hamming": 2, "min_decision_margin": 0.0, "min_tags": 1}]

# ---- composition: a made-up planar layout over scene_c2's ten ids (a 5 x 2 grid) ---------------------------------------------------------
BUNDLE_C2 = {"name": "grid", "members": board_members(5, 2, 0.5, 0.22), "max_hamming": 2, "min_decision_margin": 0.0, "min_tags": 3}
