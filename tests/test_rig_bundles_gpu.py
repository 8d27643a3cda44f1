"""Camera rigs inside the submission (amdAprilTagsSetRig, k_bundle_rig).  The definition under test is DESIGN.md section 7j, stated in
Python by tests/rig_pose_ref.py: fed the oracle's records of the frames of a submission -- which the library's own records equal bit
for bit -- the reference gives the rig record the library must hand out, every double compared as its 64 bits with
numpy.array_equal, the counts, seeds and chosen with ==.  The oracle-side preconditions (which tags each frame holds, the
observations per case, the reference against truth and against numpy, the wrong builds' forms) are asserted in
tests/test_rig_bundles_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from isaac_ros_apriltag_amd import capi  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402
import bundle_cases as bc  # noqa: E402
import parity_util as pu  # noqa: E402
import rig_cases as gc  # noqa: E402
import rig_pose_ref as gr  # noqa: E402
import rigid_bundle_cases as rc  # noqa: E402
import rigid_bundle_ref as rr  # noqa: E402
import undistort_cases as uc  # noqa: E402
import undistort_ref as ur  # noqa: E402

FAMS = gc.FAMS
INVALID_ARGUMENT = 1
# launch set and how the submission goes out: replayed from a captured graph (the second of two submissions), or as plain enqueues
MODES = ("latency-graph", "latency-plain", "throughput-plain")
_cache = {}


def _code(fn):
    with pytest.raises(capi.AprilTagsError) as e:
        fn()
    return e.value.code


def _exact(frames):
    """Records of a getter with every double as its 64 bits: what == compares."""
    return [[{k: (rr.bits(v).tolist() if isinstance(v, (np.ndarray, float)) else v) for k, v in p.items()} for p in f] for f in frames]


def _handle(mode, width, height, **kw):
    path, how = mode.split("-")
    if how == "plain" and path == "latency":
        kw["no_graph_replay"] = 1
    det = AprilTagDetector(width, height, **kw)
    det.set_submission_path(path)
    return det


def _submit(det, mode, frames, max_dets, intrinsics):
    """One submission in the mode's way; (records per frame, rigid bundle records per frame, rig records per group)."""
    prep = det.prepare(frames, max_dets=max_dets, intrinsics=intrinsics)
    graph = mode.endswith("graph")
    for _ in range(2 if graph else 1):   # (graph: captured by the first submission, replayed by the second)
        det.submit_prepared(prep)
        det.wait_prepared(prep)
    assert det.last_submission_path() == mode.split("-")[0]
    assert (det.last_graph_nodes() > 0) == graph, (mode, det.last_graph_nodes())
    return det.unpack(prep), det.bundle_poses_ex(prep["n"]), det.rig_bundle_poses(prep["n"])


def _check(label, got, want):
    errs = gr.compare(got, want, label + ": ")
    print("%s: status %d nobs %d nskipped %d ndropped %d ncams %d seed %d/%d chosen %d err %.3e sq_err_sum %.4f %s"
          % (label, got["status"], got["nobs"], got["nskipped"], got["ndropped"], got["ncams"], got["seed_frame"], got["seed"], got["chosen"],
             got["err"], got["sq_err_sum"], errs))
    return errs


def _check_all(label, got, want):
    assert len(got) == len(want)
    errs = []
    for g, (gg, ww) in enumerate(zip(got, want)):
        assert len(gg) == len(ww)
        for b, (x, y) in enumerate(zip(gg, ww)):
            errs += _check("%s group %d bundle %d" % (label, g, b), x, y)
    return errs


def _pair_frames():
    if "frames" not in _cache:
        _cache["frames"] = torch.from_numpy(np.stack([gc.pair_frame(s) for s in range(4)])).cuda()
    return _cache["frames"]


def _pair(mode):
    """The four-frame submission of the stereo pair (two instants, two cameras) in `mode`, under the cube layout, the split / stereo
    layout and the explicit slot map with an absent camera: name -> (records, rigid records, rig records)."""
    if ("pair", mode) not in _cache:
        det = _handle(mode, gc.W1, gc.H1, max_batch=4, tag_size=bc.SIZE1, bundles_ex=gc.LAYOUTS["cube"], rig=gc.PAIR)
        det.set_frame_skews(gc.SKEW4)
        out = {"cube": _submit(det, mode, _pair_frames(), 64, list(gc.INTR4))}
        det.set_bundles_ex(gc.LAYOUTS["split"])   # (a change of layout: the same graph)
        out["split"] = _submit(det, mode, _pair_frames(), 64, list(gc.INTR4))
        det.set_bundles_ex(gc.LAYOUTS["cube"])
        det.set_rig_slots(gc.SLOTS_ABSENT)          # (a new slot map: the same graph)
        out["absent"] = _submit(det, mode, _pair_frames(), 64, list(gc.INTR4))
        # the submit-time refusals: a group index at the frame count, a camera index at the rig's count, one (group, camera) twice
        prep = det.prepare(_pair_frames(), max_dets=64, intrinsics=list(gc.INTR4))
        for bad in (((0, 0), (4, 1), (1, 0), (1, 1)), ((0, 0), (0, 2), (1, 0), (1, 1)), ((0, 0), (0, 1), (0, 0), (1, 1))):
            det.set_rig_slots(bad)
            assert _code(lambda: det.submit_prepared(prep)) == INVALID_ARGUMENT
            assert _code(lambda: det.wait_prepared(prep)) == INVALID_ARGUMENT   # (nothing was enqueued)
        det.set_rig_slots(None)
        out["again"] = _submit(det, mode, _pair_frames(), 64, list(gc.INTR4))
        assert det.late_waits() == 0
        det.close()
        _cache[("pair", mode)] = out
    return _cache[("pair", mode)]


def _records_equal(recs, label=""):
    for s in range(4):
        assert not pu.compare_detections(recs[s], gc.pair_records(s), exact=True), (label, s)   # the input of the reference is the input of the kernel


# ---- 1. two cameras, two instants -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_two_cameras_two_instants(built, mode):
    """640 x 480, a four-frame submission of two groups: cameras 0.3 m apart and toed in see different face pairs of the cube, distinct
    intrinsics per slot, a skew on slot 1, another cube pose at the second instant.  The rig records equal the reference's; the
    per-frame rigid records of the same submission equal rigid_bundle_ref's, as on a handle without a rig; and the rig's translation
    error against truth is no larger than the larger of the two cameras' own."""
    recs, rigid, rig = _pair(mode)["cube"]
    _records_equal(recs, mode)
    errs = _check_all("pair %s" % mode, rig, gc.pair_solved("cube"))
    assert not errs, errs
    for s in range(4):
        want = rr.solve(gc.pair_records(s), gc.CUBE, FAMS, gc.INTR4[s], gc.SKEW4[s])
        assert not rr.compare(rigid[s][0], want), (mode, s)
    for g in (0, 1):
        Rt, tt = gc.POSES[g]
        dr, dt = rc.pose_errors(rig[g][0]["R"], rig[g][0]["t"], Rt, tt)
        own = []
        for c in (0, 1):
            Rc, tc = gc.in_camera(gc.PAIR[c], Rt, tt)
            own.append(rc.pose_errors(rigid[2 * g + c][0]["R"], rigid[2 * g + c][0]["t"], Rc, tc))
        print("truth %s group %d: rig %.4f deg %.3f mm; camera 0 alone %.4f deg %.3f mm; camera 1 alone %.4f deg %.3f mm"
              % (mode, g, dr, 1e3 * dt, own[0][0], 1e3 * own[0][1], own[1][0], 1e3 * own[1][1]))
        assert rig[g][0]["status"] == capi.BUNDLE_SOLVED and rig[g][0]["nobs"] == 16 and rig[g][0]["ncams"] == 2
        assert dt <= max(own[0][1], own[1][1])
    assert all(rig[g][0]["status"] == capi.BUNDLE_TOO_FEW_TAGS and not rig[g][0]["R"].any() for g in (2, 3))
    # the default map again behind the refused submissions: the same records
    assert not _check_all("again %s" % mode, _pair(mode)["again"][2], gc.pair_solved("cube"))


# ---- 2, 3. split visibility and stereo --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_split_visibility_and_stereo(built, mode):
    """A two-member bundle with its members on different faces, min_tags = 2, each camera seeing exactly one of them: both per-frame
    rigid records read TOO_FEW_TAGS, the rig record is SOLVED with nobs = 2, ncams = 2.  And a one-member bundle whose tag both cameras
    see: two observations of one tag."""
    recs, rigid, rig = _pair(mode)["split"]
    _records_equal(recs, mode)
    errs = _check_all("split %s" % mode, rig, gc.pair_solved("split"))
    assert not errs, errs
    for g in (0, 1):
        assert [rigid[2 * g + c][0]["status"] for c in (0, 1)] == [capi.BUNDLE_TOO_FEW_TAGS] * 2
        assert [rigid[2 * g + c][0]["ntags"] for c in (0, 1)] == [1, 1]
        assert (rig[g][0]["status"], rig[g][0]["nobs"], rig[g][0]["ncams"]) == (capi.BUNDLE_SOLVED, 2, 2)
        assert (rig[g][1]["status"], rig[g][1]["nobs"], rig[g][1]["ncams"]) == (capi.BUNDLE_SOLVED, 2, 2)


# ---- 4. absent cameras ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_absent_cameras(built, mode):
    """An explicit slot map: slot 1 has no camera, so group 0 is camera 0 alone under its non-identity extrinsic; the second instant's
    pair is group 2; groups 1 and 3 are named by nobody and read too few tags with zeros.  (The three submit-time refusals are asserted
    where the submissions are made.)"""
    recs, rigid, rig = _pair(mode)["absent"]
    _records_equal(recs, mode)
    errs = _check_all("absent %s" % mode, rig, gc.pair_solved("cube", gc.SLOTS_ABSENT))
    assert not errs, errs
    assert [(g[0]["status"], g[0]["nobs"], g[0]["ncams"]) for g in rig] == [(0, 8, 1), (1, 0, 0), (0, 16, 2), (1, 0, 0)]
    for g in (1, 3):
        assert not rig[g][0]["R"].any() and not rig[g][0]["t"].any() and rig[g][0]["err"] == 0.0 and rig[g][0]["group"] == g
    assert all(r[0]["status"] == capi.BUNDLE_SOLVED for r in rigid)   # (the slot without camera is detected and solved per frame as usual)


# ---- 5. identity ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_one_camera_identity_rig(built, mode):
    """A one-camera rig with the identity and zero under the default map, on the cube submission of the rigid bundle test:
    rig_bundle_poses equals bundle_poses_ex bit for bit, group by frame."""
    det = _handle(mode, rc.W1, rc.H1, max_batch=3, tag_size=bc.SIZE1, bundles_ex=rc.CUBE_BUNDLES, rig=[(np.eye(3), np.zeros(3))])
    det.set_frame_skews(bc.SKEW1)
    frames = torch.from_numpy(np.stack([rc.cube_frame(n) for n in rc.CUBE_FRAMES])).cuda()
    recs, rigid, rig = _submit(det, mode, frames, 64, list(bc.INTR1))
    assert det.late_waits() == 0
    det.close()
    solved = 0
    for f, name in enumerate(rc.CUBE_FRAMES):
        assert not pu.compare_detections(recs[f], rc.cube_records(name), exact=True)
        for b in range(2):
            x, y = rig[f][b], rigid[f][b]
            assert not rr.compare(y, rc.cube_solved(name)[b])
            assert (x["group"], x["bundle"], x["status"], x["nobs"], x["nskipped"], x["seed_frame"], x["seed"], x["chosen"]) == \
                (f, b, y["status"], y["ntags"], y["nskipped"], f if y["status"] == 0 else 0, y["seed"], y["chosen"])
            for k in rr.FIELDS:
                assert np.array_equal(rr.bits(x[k]), rr.bits(y[k])), (mode, name, b, k)
            solved += x["status"] == capi.BUNDLE_SOLVED
    assert solved == 4


# ---- 6. the observation slots -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_observation_slots(built, mode):
    """640 x 576, the 72-tag frame in both slots of a two-camera group.  32 members: exactly 64 observations, every lane of the wave,
    none dropped.  33 members: 66 used, 64 in slots, 2 dropped.  Both have used records in the second 64-record chunk of a frame;
    with max_dets = 8 the hand-out ends at eight records and the solve still reads all 72."""
    det = _handle(mode, bc.W2, bc.H2, max_batch=2, tag_size=bc.SIZE2, intrinsics=bc.INTR2, bundles_ex=[gc.FULL], rig=gc.PAIR72)
    frames = torch.from_numpy(np.stack([bc.frame72(), bc.frame72()])).cuda()
    recs, _, rig = _submit(det, mode, frames, 128, None)
    assert not pu.compare_detections(recs[0], bc.records72(), exact=True) and not pu.compare_detections(recs[1], bc.records72(), exact=True)
    errs = _check_all("full %s" % mode, rig, gc.solved72("full"))
    assert (rig[0][0]["nobs"], rig[0][0]["ndropped"]) == (64, 0)
    det.set_bundles_ex([gc.OVER])
    for max_dets in (128, 8):
        recs, _, rig = _submit(det, mode, frames, max_dets, None)
        assert len(recs[0]) == min(max_dets, 72)
        errs += _check_all("over %s max_dets %d" % (mode, max_dets), rig, gc.solved72("over"))
        assert (rig[0][0]["nobs"], rig[0][0]["ndropped"]) == (64, 2)
    assert det.late_waits() == 0
    det.close()
    assert not errs, errs


@pytest.mark.parametrize("mode", MODES)
def test_duplicate_rule_is_per_frame(built, mode):
    """bundle_cases' duplicate frame in camera 0 and its all_six frame in camera 1: the duplicated id contributes camera 1's observation
    only, and both of camera 0's records of it count as skipped."""
    det = _handle(mode, bc.W1, bc.H1, max_batch=2, tag_size=bc.SIZE1, bundles_ex=[rc.BUNDLE1], rig=gc.PAIR)
    det.set_frame_skews(gc.DUP_SKEW)
    frames = torch.from_numpy(np.stack([bc.content_frame("duplicate"), bc.content_frame("all_six")])).cuda()
    recs, _, rig = _submit(det, mode, frames, 64, list(gc.DUP_INTR))
    assert det.late_waits() == 0
    det.close()
    for s in (0, 1):
        assert not pu.compare_detections(recs[s], gc.dup_records(s), exact=True)
    errs = _check_all("dup %s" % mode, rig, gc.dup_solved())
    assert not errs, errs
    assert (rig[0][0]["nobs"], rig[0][0]["nskipped"], rig[0][0]["ncams"]) == (11, 2, 2)


# ---- 7. twins -------------------------------------------------------------------------------------------------------------------------------------
def _twin_camera(slot):
    K = gc.K_of(gc.INTR4[slot])
    return (K, [-0.05, 0.01, 0.0004, -0.0003, 0.0], K, "plumb_bob", None)


def test_twins(built):
    """Case 1 with the corner undistortion on (the frames taken as raw frames of a mildly distorted camera per slot): the rig stage reads
    the undistorted twins in the raw records' place, as the other pose launches do."""
    det = AprilTagDetector(gc.W1, gc.H1, max_batch=4, tag_size=bc.SIZE1, bundles_ex=gc.LAYOUTS["cube"], rig=gc.PAIR,
                           corner_undistortion=[_twin_camera(s) for s in range(4)])
    det.set_frame_skews(gc.SKEW4)
    prep = det.prepare(_pair_frames(), max_dets=64, intrinsics=list(gc.INTR4))
    det.run_prepared(prep)
    recs, rig, rigid = det.unpack(prep), det.rig_bundle_poses(4), det.bundle_poses_ex(4)
    assert det.late_waits() == 0
    det.close()
    _records_equal(recs, "twins")
    feed = [ur.for_consumers(ur.records(gc.pair_records(s), _twin_camera(s), gc.INTR4[s], bc.SIZE1, gc.SKEW4[s])) for s in range(4)]
    assert all(t["status"] == ur.OK for f in feed for t in f)
    want = gc.pair_solved("cube", records=feed)
    errs = _check_all("twins", rig, want)
    assert not errs, errs
    assert gr.compare(rig[0][0], gc.pair_solved("cube")[0][0])   # (the twins are not the raw records)
    for s in range(4):
        assert not rr.compare(rigid[s][0], rr.solve(feed[s], gc.CUBE, FAMS, gc.INTR4[s], gc.SKEW4[s]))


# ---- 8. the contract --------------------------------------------------------------------------------------------------------------------------------
def test_off_means_off_retirement_and_the_contract(built):
    frames = _pair_frames()[:2]
    intr = list(gc.INTR4[:2])
    det = AprilTagDetector(gc.W1, gc.H1, tag_size=bc.SIZE1, max_batch=2, bundles_ex=gc.LAYOUTS["cube"], pose_refinement=5)
    never = AprilTagDetector(gc.W1, gc.H1, tag_size=bc.SIZE1, max_batch=2, bundles_ex=gc.LAYOUTS["cube"], pose_refinement=5)
    L, h = capi.lib(), det._h

    def run(d=det):
        prep = d.prepare(frames, max_dets=64, intrinsics=intr)
        d.run_prepared(prep)
        return bytes(prep["out"]), list(prep["cnt"]), _exact(d.bundle_poses_ex(2)), _exact(d.refined_poses(2))

    def rig_ok(slots=gc.SLOTS4[:2], cams=gc.PAIR):
        fr, sm = gc.frames_of([gc.pair_records(0), gc.pair_records(1)], gc.INTR4[:2], (0.0, 0.0), slots, cams)
        return not _check_all("contract", det.rig_bundle_poses(2), gr.solve_submission(fr, sm, gc.LAYOUTS["cube"], FAMS))

    # off is the default: nothing to hand out, no memory, the same launches
    bytes0 = det.device_bytes()
    off = run()
    run()
    nodes_off = det.last_graph_nodes()
    assert nodes_off > 0 and never.device_bytes() == bytes0
    assert _code(lambda: det.rig_bundle_poses(1)) == INVALID_ARGUMENT
    det.set_rig(None)
    det.set_rig_slots([(0, 0)])
    det.set_rig_slots(None)
    assert det.device_bytes() == bytes0 and det.graph_replay() == (True, 1, 0)
    # on: every other stage's output is the same bytes, exactly one launch more in the graph; on retires the graphs once
    det.set_rig(gc.PAIR)
    assert det.graph_replay() == (True, 0, 1)
    assert run() == off and run() == off and det.last_graph_nodes() == nodes_off + 1 and rig_ok()
    state = det.graph_replay()
    assert _code(lambda: det.rig_bundle_poses(3)) == INVALID_ARGUMENT   # beyond the last submission's frames
    # new extrinsics and a new slot map retire nothing and are solved
    other = (gc.PAIR[1], gc.PAIR[0])
    det.set_rig(other)
    assert det.graph_replay() == state and run() == off and det.last_graph_nodes() == nodes_off + 1 and rig_ok(cams=other)
    det.set_rig_slots([(1, 1), (1, 0)])
    assert det.graph_replay() == state and run() == off and det.last_graph_nodes() == nodes_off + 1 and rig_ok(slots=((1, 1), (1, 0)), cams=other)
    det.set_rig_slots(None)
    det.set_rig(gc.PAIR)
    # every setter refusal leaves the previous setting in force and retires nothing
    ok = (np.eye(3), np.zeros(3))
    for bad in ([(np.diag([1.0, 1.0, -1.0]), np.zeros(3))], [(1.001 * np.eye(3), np.zeros(3))], [(np.eye(3), (float("nan"), 0, 0))],
                [(np.diag([1.0, float("inf"), 1.0]), np.zeros(3))], [ok] * 17):
        assert _code(lambda: det.set_rig(bad)) == INVALID_ARGUMENT
    assert _code(lambda: det.set_rig_slots([(0, 0)] * 3)) == INVALID_ARGUMENT   # above max_batch
    assert L.amdAprilTagsSetRig(h, 1, None) == INVALID_ARGUMENT and L.amdAprilTagsSetRigSlots(h, 1, None) == INVALID_ARGUMENT
    assert L.amdAprilTagsSetRig(None, 0, None) == INVALID_ARGUMENT and L.amdAprilTagsSetRigSlots(None, 0, None) == INVALID_ARGUMENT
    assert L.amdAprilTagsGetRigBundlePoses(h, None, 1) == INVALID_ARGUMENT and L.amdAprilTagsGetRigBundlePoses(None, None, 1) == INVALID_ARGUMENT
    assert run() == off and rig_ok() and det.graph_replay() == state
    # between Submit and Wait the setters and the getter are refused
    prep = det.prepare(frames, max_dets=64, intrinsics=intr)
    det.submit_prepared(prep)
    assert _code(lambda: det.set_rig(None)) == INVALID_ARGUMENT and _code(lambda: det.set_rig_slots(None)) == INVALID_ARGUMENT
    assert _code(lambda: det.rig_bundle_poses(1)) == INVALID_ARGUMENT
    det.wait_prepared(prep)
    assert rig_ok() and det.graph_replay() == state
    # the stage's inputs absent: with the rigid kind off nothing is launched and the getter refuses; every other output as without a rig
    det.set_bundles_ex(None)
    never.set_bundles_ex(None)

    def run_plain(d):
        prep = d.prepare(frames, max_dets=64, intrinsics=intr)
        d.run_prepared(prep)
        d.run_prepared(prep)
        return bytes(prep["out"]), list(prep["cnt"]), _exact(d.refined_poses(2)), d.last_graph_nodes()

    assert run_plain(det) == run_plain(never)
    assert _code(lambda: det.rig_bundle_poses(1)) == INVALID_ARGUMENT and _code(lambda: det.bundle_poses_ex(1)) == INVALID_ARGUMENT
    det.set_bundles_ex(gc.LAYOUTS["cube"])
    never.set_bundles_ex(gc.LAYOUTS["cube"])
    assert run() == off and rig_ok()
    # ThresholdOnly never solves: afterwards there is nothing to hand out
    det.threshold_only(frames)
    assert _code(lambda: det.rig_bundle_poses(1)) == INVALID_ARGUMENT
    # off again retires the graphs once, and the handle is one that never had the setting
    run()
    capturing, live, retired = det.graph_replay()
    det.set_rig(None)
    assert det.graph_replay() == (True, 0, retired + live)
    assert run() == off and run() == off and det.last_graph_nodes() == nodes_off
    assert _code(lambda: det.rig_bundle_poses(1)) == INVALID_ARGUMENT
    assert run(never) == off and never.device_bytes() == bytes0
    assert det.late_waits() == 0 and never.late_waits() == 0
    det.close()
    never.close()


# ---- 9. the node shell --------------------------------------------------------------------------------------------------------------------------
def test_node_shell(built):
    """AprilTagMultiCameraNode with three streams and rig_cameras (the cube's members by id, position, quaternion and size): a full round
    and a round with one stream missing.  One "rig_bundle:cube" transform under rig_frame_id behind the first served stream's
    transforms, from the record's chosen pose -- the translation as it stands, the rotation through the float quaternion a tag's
    takes -- and the records equal the reference's on the served streams' frames."""
    from isaac_ros_apriltag_amd import build as b
    from isaac_ros_apriltag_amd import node
    from test_rigid_bundles_gpu import _quat_of, _quat_matrix
    b.build_node()
    shell = [dict(gc.CUBE, members=[(m[1], tuple(m[3]), _quat_of(m[2]), m[4]) for m in gc.CUBE["members"]])]
    # three streams: the pair's two cameras at the first instant, and camera 0's frame of the second instant as a third camera
    frames = [gc.pair_frame(0), gc.pair_frame(1), gc.pair_frame(2)]
    k9 = [[gc.INTR4[s][0], gc.SKEW4[s], gc.INTR4[s][2], 0.0, gc.INTR4[s][1], gc.INTR4[s][3], 0.0, 0.0, 1.0] for s in range(3)]
    multi = node.AprilTagMultiCameraNode(3, size=bc.SIZE1, backends="HIP", auto_flush=False, rigid_bundles=shell, rig_cameras=gc.TRIPLE,
                                         rig_frame_id="rig_base")
    nodes = [multi]
    try:
        for served in ((0, 1, 2), (0, 2)):
            for s in served:
                assert multi.on_frame(s, frames[s].ctypes.data, False, "mono8", gc.W1, gc.H1, gc.W1, k9[s], "cam%d" % s, (7, s))
            assert multi.flush() == len(served)
            fr, sm = gc.frames_of([gc.pair_records(s) for s in served], [gc.INTR4[s] for s in served], [gc.SKEW4[s] for s in served],
                                  [(0, s) for s in served], gc.TRIPLE)
            want = gr.solve_submission(fr, sm, [gc.CUBE], FAMS)[0][0]
            poses = multi.rig_bundle_poses()
            assert [p["name"] for p in poses] == ["cube"]
            p = poses[0]
            rec = dict(p, group=0, bundle=0, seed_frame=served.index(p["seed_stream"]), R=np.array(p["R"]).reshape(3, 3), t=np.array(p["t"]),
                       R_alt=np.array(p["R_alt"]).reshape(3, 3), t_alt=np.array(p["t_alt"]))
            errs = _check("node shell %s" % (served,), rec, want)
            assert not errs, errs
            assert p["status"] == capi.BUNDLE_SOLVED and p["ncams"] == len(served) and p["nobs"] == 8 * len(served)
            for s in served:
                tfs = multi.transforms(s)
                names = [t["child_frame_id"] for t in tfs]
                own = ["tag36h11:%d" % r["id"] for r in gc.pair_records(s)] + ["bundle:cube"]
                assert names == own + (["rig_bundle:cube"] if s == served[0] else []), (s, names)
            tf = multi.transforms(served[0])[-1]
            assert tf["frame_id"] == "rig_base" and tf["stamp"] == (7, served[0]) and tf["translation"] == p["t"]
            assert np.abs(_quat_matrix(tf["rotation_xyzw"]) - np.array(p["R"]).reshape(3, 3)).max() < 1e-6   # (float quaternion)
        bad = node.AprilTagMultiCameraNode(3, size=bc.SIZE1, backends="HIP", rigid_bundles=shell, rig_cameras=gc.PAIR)
        nodes.append(bad)
        with pytest.raises(RuntimeError):   # one camera per stream: refused when the handle is created, at the first frame
            bad.on_frame(0, frames[0].ctypes.data, False, "mono8", gc.W1, gc.H1, gc.W1, k9[0], "cam0", (7, 0))
    finally:
        [x.close() for x in nodes]


# ---- 10. the suite bites ------------------------------------------------------------------------------------------------------------------------
_SELECT = "(test_two_cameras_two_instants or test_split_visibility_and_stereo or test_absent_cameras or test_one_camera_identity_rig " \
          "or test_observation_slots or test_duplicate_rule_is_per_frame) and throughput"
_GEOMETRY = ("test_two_cameras_two_instants[throughput-plain]", "test_split_visibility_and_stereo[throughput-plain]",
             "test_absent_cameras[throughput-plain]", "test_duplicate_rule_is_per_frame[throughput-plain]")
_SLOTS = ("test_observation_slots[throughput-plain]",)
_IDENTITY = ("test_one_camera_identity_rig[throughput-plain]",)
_WRONG_BUILDS = {
    # the ray origin left out of the translation statement: every rig whose cameras are not at the rig's origin; the identity rig does not see it
    46: {"must_fail": _GEOMETRY + _SLOTS, "must_pass": _IDENTITY},
    # Rc in place of its transpose for the ray direction: every rig with a turned camera
    47: {"must_fail": _GEOMETRY + _SLOTS, "must_pass": _IDENTITY},
    # the slots cut at 63: only where 64 or more observations are used
    48: {"must_fail": _SLOTS, "must_pass": _GEOMETRY + _IDENTITY},
}


@pytest.mark.parametrize("mutant", sorted(_WRONG_BUILDS))
def test_the_rig_tests_fail_on_the_wrong_builds(built, mutant):
    """libapriltag_amd_mut46.so .. _mut48.so (csrc/tools_hooks.h, AMDAT_MUTATE): the rig cases on the throughput set, in a process of
    their own, must FAIL on the wrong build exactly where its error lives, and all of them pass on the product library.  The three
    wrong builds change values only."""
    import subprocess
    from isaac_ros_apriltag_amd import build as bld
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(bld.lib_mutant(mutant)):
        bld.build_mutants()
    spec = _WRONG_BUILDS[mutant]

    def run(lib):
        env = dict(os.environ)
        env.pop("AMDAT_LIB", None)
        if lib:
            env["AMDAT_LIB"] = lib
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-rA", "-p", "no:cacheprovider",
                              "-k", _SELECT], capture_output=True, text=True, timeout=600, cwd=root, env=env)
        ids = lambda word: sorted(l.split("::", 1)[1].split(" ")[0] for l in out.stdout.splitlines() if l.startswith(word + " ") and "::" in l)
        return out, ids("PASSED"), ids("FAILED")
    out, passed, failed = run("mut%d" % mutant)
    assert out.returncode == 1, (out.stdout[-1500:], out.stderr[-1500:])
    assert sorted(failed) == sorted(spec["must_fail"]), (failed, passed)
    assert sorted(passed) == sorted(spec["must_pass"]), (failed, passed)
    assert "differ" in out.stdout   # what differs: fields of the rig record
    if "ok" not in _cache:   # (the product run is the same for the three wrong builds)
        _cache["ok"] = run(None)
    out_ok, passed_ok, failed_ok = _cache["ok"]
    assert out_ok.returncode == 0 and not failed_ok and sorted(passed_ok) == sorted(passed + failed), (out_ok.stdout[-1500:], failed_ok)
