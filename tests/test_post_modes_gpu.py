"""One handle walked through the combinations of the stages behind k_reconcile (post_plan.h): corner undistortion, planar and rigid
bundles, pose refinement and pose covariance.  The other suites check each stage against its reference; this one checks that the
stages compose on one handle whatever the order they were switched in: after every setter call the handle hands out the bytes of a
fresh handle that only ever had the final settings, the getters of the stages that are off refuse, the second submission replays a
graph, and the graph counts are what the retirement table of tests/test_post_plan_cpu.py predicts.  No tolerance: equal settings on
equal frames give equal bytes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from isaac_ros_apriltag_amd import capi, synth  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402
import bundle_cases as bc  # noqa: E402
import rigid_bundle_cases as rg  # noqa: E402
import test_post_plan_cpu as pp  # noqa: E402

INVALID_ARGUMENT = 1
W, H, B = 320, 240, 3
SIZE, PITCH = 0.05, 0.075                 # a 2 x 2 board of 30-pixel tags, 45 pixels apart, half a metre away
K = np.array([[300.0, 0, 160.0], [0, 300.0, 120.0], [0, 0, 1.0]])
INTR = (300.0, 300.0, 160.0, 120.0)
MEMBERS = bc.board_members(2, 2, PITCH, SIZE)
PLANAR = {"name": "board", "members": MEMBERS, "max_hamming": 2, "min_decision_margin": 0.0, "min_tags": 1}
RIGID = rg.restated(PLANAR)
CAMERA = (np.array([[296.0, 0, 161.5], [0, 295.0, 118.75], [0, 0, 1.0]]), [-0.11, 0.03, 0.0012, -0.0009, -0.004], K, "plumb_bob", None)
MAX_DETS = 3                              # below the four tags of frames 0 and 2: frames x min(nout, ostride) records
# the values a stage is switched on with, by the request's name in tests/test_post_plan_cpu.py
IT, SG = pp.IT, pp.SG


def _frames():
    """Frames 0 and 2: the whole board; frame 1: tags 1 and 2 covered."""
    R, t = synth.rot_xyz(0.10, -0.14, 0.06), np.array([0.004, -0.006, 0.5])
    whole = synth.render(W, H, bc.board_tags(MEMBERS, R, t, K), background=150, sigma=1.0, seed=5)
    two = synth.render(W, H, bc.board_tags(MEMBERS, R, t, K, skip=(1, 2)), background=150, sigma=1.0, seed=5)
    return torch.from_numpy(np.ascontiguousarray(np.stack([whole, two, whole]))).cuda()


def _set(det, what, v):
    """A request of tests/test_post_plan_cpu.py on a handle: v is the count, iteration number or sigma (0: off)."""
    if what == "planar":
        det.set_bundles([PLANAR] * v)
    elif what == "rigid":
        det.set_bundles_ex([RIGID] * v)
    elif what == "refine":
        det.set_pose_refinement(v)
    elif what == "cov":
        det.set_pose_covariance(v)
    else:
        det.set_corner_undistortion([CAMERA] * v)


def _blob(x):
    if isinstance(x, dict):
        return b"".join(k.encode() + _blob(v) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return b"[" + b"".join(_blob(v) for v in x) + b"]"
    return np.ascontiguousarray(x).tobytes()


def _code(fn):
    with pytest.raises(capi.AprilTagsError) as e:
        fn()
    return e.value.code


def _getters(det, mode):
    """(getter, its stages are on in `mode`) for all six."""
    nb, nr, it, sg, nu = mode
    return [(lambda: det.bundle_poses(B), nb > 0), (lambda: det.bundle_poses_ex(B), nr > 0),
            (lambda: det.bundle_pose_covariances_ex(B), nr > 0 and sg > 0), (lambda: det.refined_poses(B), it > 0),
            (lambda: det.refined_pose_covariances(B), it > 0 and sg > 0), (lambda: det.undistorted_detections(B), nu > 0)]


def _submit_twice(det, prep, mode):
    """Two submissions (the second replays); the records and what every getter hands out, as bytes, None for a getter that must refuse."""
    det.run_prepared(prep)
    det.run_prepared(prep)
    assert det.last_graph_nodes() > 0
    out = [bytes(prep["out"]), bytes(prep["cnt"])]
    for get, on in _getters(det, mode):
        if on:
            out.append(_blob(get()))
        else:
            assert _code(get) == INVALID_ARGUMENT
            out.append(None)
    return out


def _fresh(frames, mode):
    """What a handle hands out on which only the settings of `mode` were ever applied."""
    det = AprilTagDetector(W, H, tag_size=SIZE, intrinsics=INTR, max_batch=B)
    for what, v in zip(("planar", "rigid", "refine", "cov", "undistort"), mode):
        if v:
            _set(det, what, v)
    out = _submit_twice(det, det.prepare(frames, max_dets=MAX_DETS), mode)
    assert det.late_waits() == 0
    det.close()
    return out


# every on / off bit in both directions, the planar -> rigid and rigid -> planar switches, a value changed under the same bits, and the
# covariance toggled where no launch has a covariance instance
WALK = [("refine", IT), ("cov", SG), ("planar", 1), ("undistort", 1), ("rigid", 1), ("refine", 7), ("cov", 0), ("refine", 0),
        ("planar", 1), ("undistort", 0), ("cov", 0.25), ("planar", 0), ("rigid", 1), ("refine", IT), ("undistort", 1)]


def test_one_handle_through_the_combinations(built):
    frames = _frames()
    det = AprilTagDetector(W, H, tag_size=SIZE, intrinsics=INTR, max_batch=B)
    prep = det.prepare(frames, max_dets=MAX_DETS)
    mode, retired = (0, 0, 0, 0, 0), 0
    want = _fresh(frames, mode)
    assert _submit_twice(det, prep, mode) == want and det.graph_replay() == (True, 1, 0)
    assert list(prep["cnt"]) == [3, 2, 3]   # (four, two and four tags kept, three slots)
    for what, v in WALK:
        mode, retires = pp.setters_as_they_were(mode, what, v)
        _set(det, what, v)
        retired += int(retires)             # (one live graph at every call: each submission pair below captures one)
        assert det.graph_replay() == (True, 0 if retires else 1, retired), (what, v)
        want = _fresh(frames, mode)
        assert _submit_twice(det, prep, mode) == want, (what, v, mode)
        assert det.graph_replay() == (True, 1, retired), (what, v)
    assert retired == len(WALK) - 1   # (only the new iteration number left the bits and the graph alone)
    assert mode == (0, 1, IT, 0.25, 1)
    # the debug entry points overwrite batch slot 0: nothing of the last submission is handed out afterwards, and the next one is whole
    records = np.frombuffer(bytes(prep["out"]), dtype=capi.DET_DTYPE)[:3].copy()
    for debug in (lambda: det.debug_reconcile(records), lambda: det.debug_undistort(records, CAMERA)):
        debug()
        for get, _ in _getters(det, mode):
            assert _code(get) == INVALID_ARGUMENT
        assert _submit_twice(det, prep, mode) == want
        assert det.graph_replay() == (True, 1, retired)
    assert det.late_waits() == 0
    det.close()
