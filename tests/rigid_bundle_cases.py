"""Shared by tests/test_rigid_bundles_cpu.py and tests/test_rigid_bundles_gpu.py: the rendered rigs of the rigid-bundle tests, their
bundles, the oracle's records on them and the reference's bundle records -- each computed once per process and never changed
afterwards.  Every frame is rendered by synth.render, where every tag has its own H."""
import math

import numpy as np

from isaac_ros_apriltag_amd import synth
import bundle_cases as bc
import rigid_bundle_ref as rr

FAM = bc.FAM
FAMS = list(FAM)
_cache = {}
I3 = np.eye(3)


def frame_axes(ex, ez):
    """The rotation whose columns are the tag's x axis, z x x, and its z axis (which points INTO the surface, away from the viewer)."""
    ex, ez = np.asarray(ex, dtype=np.float64), np.asarray(ez, dtype=np.float64)
    return np.stack([ex, np.cross(ez, ex), ez], axis=1)


def rigid_tags(members, Rb, tb, K, only=None, codes=None):
    """Render records ({family, id, H}) of the members of a rigid bundle with pose (Rb, tb) under K; only: the ids to render."""
    tags = []
    for (_, tid, Rm, tm, size) in members:
        if only is not None and tid not in only:
            continue
        R = np.asarray(Rb) @ np.asarray(Rm)
        t = np.asarray(tb) + np.asarray(Rb) @ np.asarray(tm)
        tg = {"family": FAM[0], "id": tid, "H": synth.homography_from_pose(R, t, K, size)}
        if codes and tid in codes:
            tg["code"] = codes[tid]
        tags.append(tg)
    return tags


# ---- the cube corner: three mutually orthogonal faces of 2 x 2 tags, the cube in the negative octant of the bundle frame ------------------
SIZE_C, PITCH_C, MARGIN_C = 0.056, 0.074, 0.050
EX, EY, EZ = np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0])


def _face(first_id, ea, eb, en):
    """2 x 2 tags on the face spanned by -ea, -eb from the corner, outward normal en; the tag's x axis is ea."""
    R = frame_axes(ea, -en)
    out = []
    for r in range(2):
        for c in range(2):
            centre = -(MARGIN_C + c * PITCH_C) * ea - (MARGIN_C + r * PITCH_C) * eb
            out.append((0, first_id + 2 * r + c, R, centre, SIZE_C))
    return out


CUBE_MEMBERS = _face(0, EX, EY, EZ) + _face(4, EY, EZ, EX) + _face(8, EZ, EX, EY)
CUBE = {"name": "cube", "iterations": rr.ITERATIONS, "members": CUBE_MEMBERS, "max_hamming": 0, "min_decision_margin": 0.0, "min_tags": 2}
LONE_ID = 20
LONE = {"name": "lone", "iterations": rr.ITERATIONS, "members": [(0, LONE_ID, I3, np.zeros(3), bc.SIZE1)], "max_hamming": 2,
        "min_decision_margin": 0.0, "min_tags": 1}
CUBE_BUNDLES = [CUBE, LONE]
W1, H1, K1 = bc.W1, bc.H1, bc.K1


def _look_at_corner(yaw_deg, extra):
    """A bundle pose under which the camera looks at the cube's corner along its diagonal, turned about it by yaw_deg."""
    d = -np.array([1.0, 1.0, 1.0]) / math.sqrt(3.0)             # the viewing direction in the bundle frame
    up = np.array([0.0, 0.0, 1.0])
    x = np.cross(d, up)
    x = x / np.linalg.norm(x)
    y = np.cross(d, x)
    Rb = np.stack([x, y, d], axis=0)                            # rows: the camera's axes in the bundle frame
    return synth.rot_xyz(0.0, 0.0, math.radians(yaw_deg)) @ synth.rot_xyz(*[math.radians(v) for v in extra]) @ Rb


CUBE_POSES = {"cube_a": (_look_at_corner(8.0, (4.0, -6.0, 0.0)), np.array([0.005, 0.035, 0.62])),
              "cube_b": (_look_at_corner(-25.0, (-7.0, 9.0, 0.0)), np.array([-0.02, 0.03, 0.66]))}
# one face in view: the z = 0 face alone (ids 0 .. 3), seen obliquely, and the lone tag beside it
FACE_POSE = (synth.rot_xyz(math.radians(28.0), math.radians(-20.0), math.radians(10.0)) @ np.diag([1.0, -1.0, -1.0]), np.array([0.09, -0.06, 0.55]))
CUBE_FRAMES = ("cube_a", "one_face", "cube_b")   # the slots of the three-frame submission (bc.INTR1 / bc.SKEW1)


def cube_frame(name):
    if ("frame", name) not in _cache:
        if name == "one_face":
            tags = rigid_tags(CUBE_MEMBERS, FACE_POSE[0], FACE_POSE[1], K1, only=(0, 1, 2, 3)) + [bc.lone_tag(LONE_ID, 90.0, 84.0, 56.0)]
        else:
            tags = rigid_tags(CUBE_MEMBERS, CUBE_POSES[name][0], CUBE_POSES[name][1], K1)
        _cache[("frame", name)] = np.ascontiguousarray(synth.render(W1, H1, tags, background=150, sigma=1.0, seed=31 + CUBE_FRAMES.index(name)))
    return _cache[("frame", name)]


def cube_records(name):
    if ("rec", name) not in _cache:
        slot = CUBE_FRAMES.index(name)
        _cache[("rec", name)] = bc.oracle_records(cube_frame(name), bc.INTR1[slot], bc.SKEW1[slot])
    return _cache[("rec", name)]


def cube_solved(name):
    """The reference's records of the frame's two bundles."""
    if ("sol", name) not in _cache:
        slot = CUBE_FRAMES.index(name)
        _cache[("sol", name)] = [rr.solve(cube_records(name), b, FAMS, bc.INTR1[slot], bc.SKEW1[slot], bundle_index=i) for i, b in enumerate(CUBE_BUNDLES)]
    return _cache[("sol", name)]


# ---- quarter turns: bundle_cases' 3 x 2 board with member i turned by i quarter turns in the plane ----------------------------------------
def _turn(q):
    c, s = (1.0, 0.0, -1.0, 0.0)[q % 4], (0.0, 1.0, 0.0, -1.0)[q % 4]
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


TURNED_MEMBERS = [(0, tid, _turn(i), np.array([x, y, 0.0]), size) for i, (_, tid, x, y, size) in enumerate(bc.MEMBERS1)]
TURNED = {"name": "turned", "iterations": rr.ITERATIONS, "members": TURNED_MEMBERS, "max_hamming": 0, "min_decision_margin": 0.0, "min_tags": 1}


def turned_frame():
    if "turned" not in _cache:
        _cache["turned"] = np.ascontiguousarray(synth.render(W1, H1, rigid_tags(TURNED_MEMBERS, bc.R1, bc.T1, K1), background=150, sigma=1.0, seed=41))
    return _cache["turned"]


def turned_records():
    if "turned_rec" not in _cache:
        _cache["turned_rec"] = bc.oracle_records(turned_frame(), bc.INTR1[0])
    return _cache["turned_rec"]


def turned_solved():
    if "turned_sol" not in _cache:
        _cache["turned_sol"] = rr.solve(turned_records(), TURNED, FAMS, bc.INTR1[0])
    return _cache["turned_sol"]


# ---- planar layouts restated with identity member rotations --------------------------------------------------------------------------------
def restated(bundle, iterations=rr.ITERATIONS, members=None):
    """A bundle_cases bundle as a rigid one: every member at (x, y, 0) with the identity rotation."""
    mem = bundle["members"] if members is None else members
    return dict(bundle, iterations=iterations, members=[(f, tid, I3, np.array([x, y, 0.0]), size) for (f, tid, x, y, size) in mem])


BUNDLE1 = restated(bc.BUNDLE1)


def content_solved(name):
    if ("content", name) not in _cache:
        slot = bc.SLOTS[name][1]
        _cache[("content", name)] = rr.solve(bc.content_records(name), BUNDLE1, FAMS, bc.INTR1[slot], bc.SKEW1[slot])
    return _cache[("content", name)]


# the 72-tag board: all 64 lanes of the wave hold a tag (ids 0 .. 63 are members, 8 records are none of them); and 12 members from both
# ends of the id range, whose records fall into both 64-record chunks of the canonical order.  Ten steps keep the reference quick.
ITER72 = 10
FULL_WAVE = restated(dict(bc.BUNDLE2, name="wave"), ITER72, [m for m in bc.MEMBERS2 if m[1] < 64])
ENDS_IDS = tuple(range(6)) + tuple(range(66, 72))
BOTH_ENDS = restated(dict(bc.BUNDLE2, name="ends"), ITER72, [m for m in bc.MEMBERS2 if m[1] in ENDS_IDS])


def solved72(which):
    if ("72", which) not in _cache:
        _cache[("72", which)] = rr.solve(bc.records72(), {"wave": FULL_WAVE, "ends": BOTH_ENDS}[which], FAMS, bc.INTR2)
    return _cache[("72", which)]


# two rigid bundles in one frame: the board's rows (bundle_cases.BUNDLES3 without the lone tag)
TWO = [restated(bc.BUNDLES3[0]), restated(bc.BUNDLES3[1])]


def pose_errors(R, t, R_true, t_true):
    """(rotation error in degrees, translation error in metres)."""
    from pose_refine_ref import rot_angle_deg
    return rot_angle_deg(R, R_true), float(np.linalg.norm(np.asarray(t) - np.asarray(t_true)))
