"""Shared by tests/test_rig_bundles_cpu.py and tests/test_rig_bundles_gpu.py: the camera rigs of the rig tests, their rendered
frames, the oracle's records on them and the reference's rig records -- each computed once per process and never changed
afterwards.  A camera is (Rc, tc), the rig frame in the camera frame: X_cam = Rc X_rig + tc."""
import math

import numpy as np

from isaac_ros_apriltag_amd import synth
import bundle_cases as bc
import rigid_bundle_cases as rc
import rigid_bundle_ref as rr
import rig_pose_ref as gr

FAMS = rc.FAMS
NO_CAMERA = 0xFFFFFFFF
_cache = {}
I3 = np.eye(3)


def camera_at(centre, yaw_deg, pitch_deg=0.0, roll_deg=0.0):
    """(Rc, tc) of a camera whose centre is `centre` in the rig frame and whose axes are the rig's turned by the angles."""
    Rw = synth.rot_xyz(math.radians(pitch_deg), math.radians(yaw_deg), math.radians(roll_deg))   # camera axes in the rig frame
    Rc = Rw.T
    return Rc, -Rc @ np.asarray(centre, dtype=np.float64)


def in_camera(cam, Rb, tb):
    """The bundle pose (Rb, tb) of the rig frame in the camera's frame: Rc Rb, Rc tb + tc."""
    Rc, tc = cam
    return Rc @ np.asarray(Rb), Rc @ np.asarray(tb) + tc


def K_of(intr, skew=0.0):
    return np.array([[intr[0], skew, intr[2]], [0.0, intr[1], intr[3]], [0.0, 0.0, 1.0]])


# ---- the stereo pair: two cameras 0.3 m apart, toed in on a point 0.62 m ahead, the rig frame between them --------------------------------
PAIR = (camera_at((-0.15, 0.004, 0.0), 13.0, 1.5, -0.8), camera_at((0.15, -0.003, 0.01), -14.0, -1.0, 1.2))
TRIPLE = PAIR + (camera_at((0.0, -0.12, 0.02), 1.0, -11.0, 0.5),)
# per-slot intrinsics of the four-frame submission (distinct) and skews (one slot with a skew)
INTR4 = bc.INTR1 + ((601.5, 599.25, 321.25, 239.5),)
SKEW4 = (0.0, 0.75, 0.0, 0.0)
# the cube's poses in the RIG frame at the two instants
POSES = (rc.CUBE_POSES["cube_a"], rc.CUBE_POSES["cube_b"])
# what each camera sees of the cube: a different pair of faces (ids 0 .. 3, 4 .. 7, 8 .. 11 are the faces)
SEEN = (tuple(range(0, 8)), tuple(range(4, 12)))
SLOTS4 = ((0, 0), (0, 1), (1, 0), (1, 1))   # the default map of a two-camera rig
CUBE = dict(rc.CUBE, name="cube")
# split visibility: members on different faces, each seen by one camera only; and the same tag in both cameras
SPLIT = {"name": "split", "iterations": rr.ITERATIONS, "members": [rc.CUBE_MEMBERS[0], rc.CUBE_MEMBERS[8]], "max_hamming": 0,
         "min_decision_margin": 0.0, "min_tags": 2}
STEREO = {"name": "stereo", "iterations": rr.ITERATIONS, "members": [rc.CUBE_MEMBERS[4]], "max_hamming": 0, "min_decision_margin": 0.0,
          "min_tags": 1}
W1, H1 = rc.W1, rc.H1


def pair_frame(slot):
    """Frame `slot` of the four-frame submission: the cube at instant slot // 2 as camera slot % 2 sees it, under that slot's K."""
    if ("frame", slot) not in _cache:
        Rb, tb = in_camera(PAIR[slot % 2], *POSES[slot // 2])
        tags = rc.rigid_tags(rc.CUBE_MEMBERS, Rb, tb, K_of(INTR4[slot], SKEW4[slot]), only=SEEN[slot % 2])
        _cache[("frame", slot)] = np.ascontiguousarray(synth.render(W1, H1, tags, background=150, sigma=1.0, seed=61 + slot))
    return _cache[("frame", slot)]


def pair_records(slot):
    if ("rec", slot) not in _cache:
        _cache[("rec", slot)] = bc.oracle_records(pair_frame(slot), INTR4[slot], SKEW4[slot])
    return _cache[("rec", slot)]


def frames_of(records, intrinsics, skews, slots, cams):
    """The submission as rig_pose_ref.solve_submission reads it: per batch slot {"records", "intrinsics", "skew", "camera"}, and the
    slot map with None for a slot without camera."""
    frames, smap = [], []
    for i, recs in enumerate(records):
        g, c = slots[i]
        none = c is None or c == NO_CAMERA
        frames.append({"records": recs, "intrinsics": intrinsics[i], "skew": skews[i], "camera": (I3, np.zeros(3)) if none else cams[c]})
        smap.append((g, None if none else c))
    return frames, smap


def pair_solved(bundles_name, slots=SLOTS4, records=None, **forms):
    """The reference's records [group][bundle] of the four-frame submission under a slot map, for a named layout."""
    key = ("sol", bundles_name, tuple(slots), tuple(sorted(forms.items())), records is None)
    if key not in _cache or records is not None:
        recs = records if records is not None else [pair_records(s) for s in range(4)]
        frames, smap = frames_of(recs, INTR4, SKEW4, slots, PAIR)
        out = gr.solve_submission(frames, smap, LAYOUTS[bundles_name], FAMS, **forms)
        if records is not None:
            return out
        _cache[key] = out
    return _cache[key]


LAYOUTS = {"cube": [CUBE], "split": [SPLIT, STEREO]}
# an explicit map: slot 1 without a camera, so that group 0 has camera 0 alone; the second instant's pair as group 2; groups 1 and 3
# are named by nobody
SLOTS_ABSENT = ((0, 0), (0, NO_CAMERA), (2, 0), (2, 1))

# ---- the observation slots: the 72-tag frame in both slots of a two-camera group ------------------------------------------------------------
# 32 members whose records lie in both 64-record chunks of the canonical order (which is by id): 2 x 32 = 64 observations, every slot
# filled and none dropped; and 33 members: 66 used, 64 in slots, 2 dropped
IDS32 = tuple(range(16)) + tuple(range(56, 72))
IDS33 = IDS32 + (16,)
FULL = rc.restated(dict(bc.BUNDLE2, name="full"), rc.ITER72, [m for m in bc.MEMBERS2 if m[1] in IDS32])
OVER = rc.restated(dict(bc.BUNDLE2, name="over"), rc.ITER72, [m for m in bc.MEMBERS2 if m[1] in IDS33])
PAIR72 = (camera_at((-0.02, 0.0, 0.0), 1.5), camera_at((0.02, 0.001, 0.0), -1.0, 0.5))


def solved72(which, **forms):
    key = ("72", which, tuple(sorted(forms.items())))
    if key not in _cache:
        frames, smap = frames_of([bc.records72()] * 2, [bc.INTR2] * 2, [0.0, 0.0], ((0, 0), (0, 1)), PAIR72)
        _cache[key] = gr.solve_submission(frames, smap, [{"full": FULL, "over": OVER}[which]], FAMS, **forms)
    return _cache[key]


# ---- the duplicate rule is per frame: bundle_cases' duplicate frame in camera 0, the all_six frame in camera 1 -------------------------------
DUP_INTR = (bc.INTR1[0], bc.INTR1[1])
DUP_SKEW = (0.0, 0.75)


def dup_records(slot):
    if ("dup", slot) not in _cache:
        _cache[("dup", slot)] = bc.oracle_records(bc.content_frame(("duplicate", "all_six")[slot]), DUP_INTR[slot], DUP_SKEW[slot])
    return _cache[("dup", slot)]


def dup_solved():
    if "dup_sol" not in _cache:
        frames, smap = frames_of([dup_records(0), dup_records(1)], DUP_INTR, DUP_SKEW, ((0, 0), (0, 1)), PAIR)
        _cache["dup_sol"] = gr.solve_submission(frames, smap, [rc.BUNDLE1], FAMS)
    return _cache["dup_sol"]


# ---- exact projections of the cube into a rig: the truth cases of the CPU test -------------------------------------------------------------
def exact_group(cams, intrinsics, skews, Rb, tb, noise_px=0.0, seen=None):
    """Records ({family, id, p, H}) of the cube's members projected exactly into every camera (float intrinsics, as the library holds
    them), with a deterministic corner noise of +-noise_px; a group for rig_pose_ref.solve."""
    group = []
    for c, cam in enumerate(cams):
        R, t = in_camera(cam, Rb, tb)
        K = K_of([rr.f32(v) for v in intrinsics[c]], rr.f32(skews[c]))
        recs = []
        for (_, tid, Rm, tm, size) in rc.CUBE_MEMBERS:
            if seen is not None and tid not in seen[c]:
                continue
            H = synth.homography_from_pose(R @ np.asarray(Rm), t + R @ np.asarray(tm), K, size)
            p = []
            for k, (x, y) in enumerate(rr.CORNERS):
                u, v = synth.project(H, x, y)
                s = noise_px * (1.0 if (tid + k + c) % 2 else -1.0)
                p.append((u + s, v - s * (1.0 if (tid + 2 * k) % 3 else -0.5)))
            recs.append({"family": FAMS[0], "id": tid, "hamming": 0, "decision_margin": 100.0, "H": H, "p": np.array(p), "c": np.zeros(2)})
        group.append({"slot": c, "records": recs, "intrinsics": intrinsics[c], "skew": skews[c], "camera": cam})
    return group


TRUTH_POSE = (rc.CUBE_POSES["cube_b"][0], rc.CUBE_POSES["cube_b"][1] + np.array([0.01, -0.02, 0.03]))
TRUTH_RIGS = {"two": (PAIR, INTR4[:2], SKEW4[:2]), "three": (TRIPLE, INTR4[:3], (0.0, 0.75, 0.0))}
