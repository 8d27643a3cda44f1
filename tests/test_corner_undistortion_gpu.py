"""Raw-frame mode inside the submission (amdAprilTagsSetCornerUndistortion, k_undistort_records).  The definition under test is DESIGN.md
section 7h, stated by tests/undistort_ref.py: fed the records a raw frame keeps -- the oracle's, which the library's own records equal
bit for bit -- the reference gives the undistorted twins the library must hand out, every double compared as its 64 bits.  The
consumers' references (bundle_ref, rigid_bundle_ref, pose_refine_ref, pose_cov_ref) are fed those twins.  The oracle-side preconditions
are asserted in tests/test_corner_undistortion_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from isaac_ros_apriltag_amd import capi  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
import bundle_cases as bc  # noqa: E402
import bundle_ref as br  # noqa: E402
import parity_util as pu  # noqa: E402
import pose_cov_ref as pv  # noqa: E402
import pose_refine_cases as pc  # noqa: E402
import pose_refine_ref as pr  # noqa: E402
import resize_cases as zc  # noqa: E402
import rigid_bundle_ref as rr  # noqa: E402
import undistort_cases as uc  # noqa: E402
import undistort_ref as ur  # noqa: E402

FAMS = list(bc.FAM)
INVALID_ARGUMENT = 1
SIGMA = 0.3
MODES = ("latency-graph", "latency-plain", "throughput-plain")
_cache = {}
# under this camera the outer tags of the nine-tag frame lie beyond the fisheye's 90 degrees: valid and invalid twins in one frame
PARTLY_INVALID = (np.array([[80.0, 0, 326.5], [0, 80.0, 236.25], [0, 0, 1.0]]), uc.D_FISHEYE, uc.KNEW, "equidistant", None)


def _code(fn):
    with pytest.raises(capi.AprilTagsError) as e:
        fn()
    return e.value.code


def _handle(mode, width, height, **kw):
    path, how = mode.split("-")
    if how == "plain" and path == "latency":
        kw["no_graph_replay"] = 1
    det = AprilTagDetector(width, height, **kw)
    det.set_submission_path(path)
    return det


def _run(det, mode, prep):
    graph = mode.endswith("graph")
    for _ in range(2 if graph else 1):   # (graph: captured by the first submission, replayed by the second)
        det.submit_prepared(prep)
        det.wait_prepared(prep)
    assert det.last_submission_path() == mode.split("-")[0]
    assert (det.last_graph_nodes() > 0) == graph, (mode, det.last_graph_nodes())


def _compare_twins(got, want, label=""):
    if len(got) != len(want):
        return ["%s%d undistorted records, the reference has %d" % (label, len(got), len(want))]
    errs = []
    for i, (g, w) in enumerate(zip(got, want)):
        errs += ["%srecord %d: %s" % (label, i, e) for e in ur.compare(g, w)]
    return errs


# ---- 1. the stage alone -----------------------------------------------------------------------------------------------------------------------
STAGE_CAMERAS = dict(uc.CAMERAS, folded=uc.FOLDED, behind=uc.BEHIND, narrow_fisheye=uc.FISHEYE_NARROW)


def _as_array(recs):
    a = np.zeros(len(recs), dtype=capi.DET_DTYPE)
    for i, r in enumerate(recs):
        a[i]["family"], a[i]["id"], a[i]["hamming"], a[i]["decision_margin"] = 0, r["id"], r["hamming"], r["decision_margin"]
        a[i]["p"] = r["p"]
        a[i]["c"] = r["center"]
    return a


def _special_records():
    """Four equal corners (a singular H), three collinear ones (nearly so), a NaN and an infinity in a corner."""
    out = uc.stage_records(4, 5)
    out[0]["p"] = np.full((4, 2), 200.0)
    out[1]["p"] = np.array([[100.0, 100.0], [150.0, 150.0], [200.0, 200.0], [100.0, 200.0]])
    out[2]["p"] = np.array(out[2]["p"])
    out[2]["p"][1, 0] = float("nan")
    out[3]["p"] = np.array(out[3]["p"])
    out[3]["p"][3, 1] = float("inf")
    return out


@pytest.mark.parametrize("cam", sorted(STAGE_CAMERAS))
def test_stage_alone(built, cam):
    """amdAprilTagsDebugUndistort on 0, 1, 8, 9 (one more than a wave's eight) and 257 chosen records, a third of them with corners
    outside the image, and on records whose H is singular or whose corners are not finite: the public records and the device twins
    against the reference, bit for bit.  The cameras: every kind with and without R, and each INVALID cause."""
    camera = STAGE_CAMERAS[cam]
    det = AprilTagDetector(uc.W, uc.H, tag_size=bc.SIZE1, intrinsics=uc.INTR)
    errs, seen = [], set()
    for n in (0, 1, 8, 9, 257, "special"):
        recs = _special_records() if n == "special" else uc.stage_records(n, 100 + n, spread=1.0 if n < 9 else 1.5)
        pub, tw = det.debug_undistort(_as_array(recs), camera)
        want = ur.records(recs, camera, uc.INTR, bc.SIZE1)
        assert len(pub) == len(tw) == len(recs)
        for i, w in enumerate(want):
            g = {"status": int(pub[i]["status"]), "H": pub[i]["H"].reshape(3, 3), "center": pub[i]["c"], "p": pub[i]["p"],
                 "R": pub[i]["R"].reshape(3, 3), "t": pub[i]["t"]}
            errs += ["%s n=%s record %d: %s" % (cam, n, i, e) for e in ur.compare(g, w)]
            t = {"status": w["status"], "H": tw[i]["H"].reshape(3, 3), "center": tw[i]["c"], "p": tw[i]["p"], "R": tw[i]["R"].reshape(3, 3),
                 "t": tw[i]["t"]}
            errs += ["%s n=%s twin %d: %s" % (cam, n, i, e) for e in ur.compare(t, w)]
            if (int(tw[i]["hamming"]), int(tw[i]["id"]), float(tw[i]["decision_margin"])) != (w["hamming_dev"], w["id"], w["decision_margin"]):
                errs.append("%s n=%s twin %d: hamming, id or margin differ" % (cam, n, i))
            seen.add(w["status"])
            assert np.isfinite(pub[i]["H"]).all() and np.isfinite(pub[i]["R"]).all() and np.isfinite(pub[i]["t"]).all() and np.isfinite(pub[i]["p"]).all()
        if n == "special":
            assert [want[i]["status"] for i in (0, 2, 3)] == [ur.INVALID] * 3   # (the collinear corners are no longer collinear once undistorted)
    det.close()
    print("%s: %s" % (cam, errs[:4]))
    assert not errs, errs[:8]
    assert seen == ({ur.OK, ur.INVALID})   # (every camera sees valid records and, at the least, the special ones)


# ---- 2. one submission of three frames ----------------------------------------------------------------------------------------------------------
FRAMES3 = ("nine", "none", "one")
SKEW3 = (0.0, 0.0, 0.5)


def _frames3():
    return torch.from_numpy(np.stack([uc.raw(n, c) for n, c in zip(FRAMES3, uc.KINDS3)])).cuda()


@pytest.mark.parametrize("mode", MODES)
def test_three_frame_submission(built, mode):
    """Nine tags, none and one under one camera of each kind (ncams = 3), with the planar bundle of the nine on: the undistorted records
    against the reference, the DetectionEx records against the same handle with the mode off byte for byte, and -- with max_dets = 4,
    below the nine kept -- the bundle still solved from all nine twins."""
    det = _handle(mode, uc.W, uc.H, max_batch=3, tag_size=bc.SIZE1, bundles=[uc.BUNDLE9])
    det.set_frame_skews(SKEW3)
    frames = _frames3()
    want_raw = [uc.raw_records(n, c, uc.INTR, s) for n, c, s in zip(FRAMES3, uc.KINDS3, SKEW3)]
    want_tw = [uc.twins(n, c, uc.INTR, s) for n, c, s in zip(FRAMES3, uc.KINDS3, SKEW3)]
    assert [len(w) for w in want_raw] == [9, 0, 1]
    errs = []
    for max_dets in (64, 4):
        prep = det.prepare(frames, max_dets=max_dets, intrinsics=[uc.INTR] * 3)
        det.set_corner_undistortion(None)
        _run(det, mode, prep)
        off = (bytes(prep["out"]), list(prep["cnt"]))
        assert _code(lambda: det.undistorted_detections(3)) == INVALID_ARGUMENT
        det.set_corner_undistortion([uc.CAMERAS[c] for c in uc.KINDS3])
        _run(det, mode, prep)
        assert (bytes(prep["out"]), list(prep["cnt"])) == off          # the raw frame's records, whether the mode is on or off
        recs, got = det.unpack(prep), det.undistorted_detections(3)
        poses = det.bundle_poses(3)
        for f in range(3):
            assert not pu.compare_detections(recs[f], want_raw[f][:max_dets], exact=True)
            errs += _compare_twins(got[f], want_tw[f][:max_dets], "max_dets %d frame %d: " % (max_dets, f))
            errs += br.compare(poses[f][0], br.solve(ur.for_consumers(want_tw[f]), uc.BUNDLE9, FAMS, uc.INTR, SKEW3[f]))
        assert poses[0][0]["ntags"] == 9 and poses[1][0]["ntags"] == 0 and poses[2][0]["ntags"] == 0
    assert det.late_waits() == 0
    det.close()
    print("three frames %s: %s" % (mode, errs[:4]))
    assert not errs, errs[:8]


# ---- 3. composition -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ("rational", "partly_invalid"))
def test_composition(built, case):
    """The nine-tag raw frame with the planar bundle, the refinement and its covariance on, then with the rigid bundle and its covariance:
    every record equals the existing reference fed the reference's twins.  partly_invalid: a camera under which the outer tags have no
    preimage -- their twins are INVALID, the bundles skip and count them, their refined records are DEGENERATE with zero fields and
    their covariance records zero."""
    camera = uc.CAMERAS["rational"] if case == "rational" else PARTLY_INVALID
    frame = torch.from_numpy(uc.raw("nine", "rational")).cuda()
    raw = uc.raw_records("nine", "rational")
    tw = ur.records(raw, camera, uc.INTR, bc.SIZE1)
    feed = ur.for_consumers(tw)
    ninvalid = sum(t["status"] for t in tw)
    assert ninvalid == 0 if case == "rational" else 0 < ninvalid < 9
    errs = []
    det = AprilTagDetector(uc.W, uc.H, tag_size=bc.SIZE1, intrinsics=uc.INTR, corner_undistortion=[camera], bundles=[uc.BUNDLE9],
                           pose_refinement=pc.ITERATIONS, pose_covariance=SIGMA)
    prep = det.prepare(frame, max_dets=64)
    det.run_prepared(prep)
    det.run_prepared(prep)
    assert det.last_graph_nodes() > 0
    assert not pu.compare_detections(det.unpack(prep)[0], raw, exact=True)
    errs += _compare_twins(det.undistorted_detections(1)[0], tw)
    planar = det.bundle_poses(1)[0][0]
    errs += br.compare(planar, br.solve(feed, uc.BUNDLE9, FAMS, uc.INTR))
    refined = ur.refined(tw, uc.INTR, 0.0, bc.SIZE1, pc.ITERATIONS)
    got_refined = det.refined_poses(1)[0]
    errs += pr.compare_frames(got_refined, refined)
    errs += pv.compare_frames(det.refined_pose_covariances(1)[0], ur.covariances(tw, uc.INTR, 0.0, bc.SIZE1, refined, SIGMA))
    assert (planar["ntags"], planar["nskipped"]) == (9 - ninvalid, ninvalid)
    assert [g["status"] == capi.POSE_DEGENERATE for g in got_refined] == [t["status"] == ur.INVALID for t in tw]
    # the rigid kind in the planar kind's place
    det.set_bundles_ex([uc.RIGID9])
    det.run_prepared(prep)
    det.run_prepared(prep)
    want_rigid = rr.solve(feed, uc.RIGID9, FAMS, uc.INTR)
    rigid = det.bundle_poses_ex(1)[0][0]
    errs += rr.compare(rigid, want_rigid)
    errs += pv.compare(det.bundle_pose_covariances_ex(1)[0][0], pv.bundle_record_of(feed, uc.RIGID9, FAMS, uc.INTR, 0.0, want_rigid, SIGMA))
    assert (rigid["ntags"], rigid["nskipped"]) == (9 - ninvalid, ninvalid)
    for rec in [planar, rigid] + got_refined:
        assert all(np.isfinite(np.asarray(v, dtype=np.float64)).all() for v in rec.values())
    assert det.late_waits() == 0
    det.close()
    print("composition %s: %s" % (case, errs[:4]))
    assert not errs, errs[:8]


# ---- 4. modes -----------------------------------------------------------------------------------------------------------------------------------
def test_with_resize(built):
    """The nine-tag raw frame resized to 480 x 360 inside the submission, K, Knew and the pose intrinsics scaled as image_proc scales a
    camera: the records of the oracle on the resized frame, and their twins under the scaled camera."""
    K, D, Kn, kind, R = uc.CAMERAS["plumb_bob+R"]
    camera = (zc.scaled_k(K, 640, 480, 480, 360), D, zc.scaled_k(Kn, 640, 480, 480, 360), kind, R)
    intr = tuple(float(v) for v in (camera[2][0, 0], camera[2][1, 1], camera[2][0, 2], camera[2][1, 2]))
    raw = uc.raw("nine", "plumb_bob+R")
    want_raw = bc.oracle_records(po.resize_mono8(raw, 480, 360), intr)
    want = ur.records(want_raw, camera, intr, bc.SIZE1)
    det = AprilTagDetector(480, 360, tag_size=bc.SIZE1, resize=[(480, 360)], corner_undistortion=[camera])
    recs = det.detect_batch_ex(torch.from_numpy(raw).cuda(), max_dets=64, intrinsics=[intr])[0]
    got = det.undistorted_detections(1)[0]
    det.close()
    assert len(want_raw) == 9 and not pu.compare_detections(recs, want_raw, exact=True)
    errs = _compare_twins(got, want)
    assert not errs and all(w["status"] == ur.OK for w in want), errs[:8]


def test_with_per_frame_sizes(built):
    """A 420 x 400 window at (110, 40) of the nine-tag raw frame, at the full image's pitch, beside the whole one-tag frame: K's
    principal point moves with the window, Knew and the pose intrinsics stay -- the twins are those of the full frame's records."""
    x0, y0, w, h = 110, 40, 420, 400
    K, D, Kn, kind, R = uc.CAMERAS["equidistant"]
    Kw = K.copy()
    Kw[0, 2] -= x0
    Kw[1, 2] -= y0
    cams = [(Kw, D, Kn, kind, R), uc.CAMERAS["rational+R"]]
    full = torch.from_numpy(uc.raw("nine", "equidistant")).cuda()
    one = torch.from_numpy(uc.raw("one", "rational+R")).cuda()
    want_raw = [bc.oracle_records(np.ascontiguousarray(uc.raw("nine", "equidistant")[y0:y0 + h, x0:x0 + w]), uc.INTR), uc.raw_records("one", "rational+R")]
    want = [ur.records(want_raw[0], cams[0], uc.INTR, bc.SIZE1), uc.twins("one", "rational+R")]
    det = AprilTagDetector(uc.W, uc.H, tag_size=bc.SIZE1, max_batch=2, per_frame_sizes=True, corner_undistortion=cams)
    recs = det.detect_batch_ex([(full.data_ptr() + y0 * uc.W + x0, uc.W, w, h), (one.data_ptr(), uc.W, uc.W, uc.H)], max_dets=64,
                               intrinsics=[uc.INTR, uc.INTR])
    got = det.undistorted_detections(2)
    det.close()
    assert [len(r) for r in want_raw] == [9, 1]
    errs = []
    for f in range(2):
        assert not pu.compare_detections(recs[f], want_raw[f], exact=True)
        errs += _compare_twins(got[f], want[f], "frame %d: " % f)
    assert not errs, errs[:8]


def test_on_off_on_and_the_refusals(built):
    """The mode on, off and on again: each switch retires the live graph against the budget, a change of models alone does not; the
    mutual refusal with rectification; the getter's refusals."""
    import ctypes as C
    frame = torch.from_numpy(uc.raw("one", "rational")).cuda()
    want = uc.twins("one", "rational")
    det = AprilTagDetector(uc.W, uc.H, tag_size=bc.SIZE1, intrinsics=uc.INTR, max_batch=2)
    prep = det.prepare(frame, max_dets=64)

    def run():
        det.run_prepared(prep)
        det.run_prepared(prep)
        return det.last_graph_nodes()

    bytes0 = det.device_bytes()
    nodes_off = run()
    assert nodes_off > 0 and det.graph_replay() == (True, 1, 0)
    det.set_corner_undistortion(None)
    assert det.device_bytes() == bytes0 and det.graph_replay() == (True, 1, 0)
    retired = 0
    for _ in range(2):
        det.set_corner_undistortion([uc.CAMERAS["rational"]])
        retired += 1
        assert det.graph_replay() == (True, 0, retired)
        assert run() == nodes_off + 1
        assert not _compare_twins(det.undistorted_detections(1)[0], want)
        det.set_corner_undistortion([uc.CAMERAS["plumb_bob"], uc.CAMERAS["rational"]])   # other models: the same graph
        assert det.graph_replay() == (True, 1, retired)
        assert run() == nodes_off + 1 and det.graph_replay() == (True, 1, retired)
        assert _compare_twins(det.undistorted_detections(1)[0], want)                      # (slot 0 now has another camera)
        # rectification is refused while the mode is on, and the mode stays as it was
        assert _code(lambda: det.set_rectification([uc.CAMERAS["rational"]])) == INVALID_ARGUMENT
        assert _code(lambda: det.set_rectification([uc.CAMERAS["plumb_bob"][:3]])) == INVALID_ARGUMENT
        det.set_rectification(None)
        assert det.graph_replay() == (True, 1, retired)
        # the setter's other refusals leave the setting in force
        bad = list(uc.CAMERAS["rational"])
        bad[1] = [float("nan")] + list(bad[1][1:])
        assert _code(lambda: det.set_corner_undistortion([tuple(bad)])) == INVALID_ARGUMENT
        assert _code(lambda: det.set_corner_undistortion([uc.CAMERAS["rational"]] * 3)) == INVALID_ARGUMENT   # ncams > max_batch
        assert det.graph_replay() == (True, 1, retired)
        L, h = capi.lib(), det._h
        n = C.c_uint32(99)
        out = (capi.UndistortedDetection * 4)()
        assert L.amdAprilTagsGetUndistortedDetections(h, 1, out, 4, C.byref(n)) == INVALID_ARGUMENT and n.value == 99
        assert L.amdAprilTagsGetUndistortedDetections(h, 0, out, 0, C.byref(n)) == INVALID_ARGUMENT and n.value == 1
        assert L.amdAprilTagsGetUndistortedDetections(h, 0, None, 4, C.byref(n)) == INVALID_ARGUMENT
        assert L.amdAprilTagsGetUndistortedDetections(h, 0, out, 4, None) == INVALID_ARGUMENT
        det.submit_prepared(prep)
        assert _code(lambda: det.set_corner_undistortion(None)) == INVALID_ARGUMENT
        assert _code(lambda: det.undistorted_detections(1)) == INVALID_ARGUMENT
        det.wait_prepared(prep)
        det.threshold_only(frame)
        assert _code(lambda: det.undistorted_detections(1)) == INVALID_ARGUMENT
        det.set_corner_undistortion(None)
        retired += 1
        assert det.graph_replay() == (True, 0, retired)
        assert run() == nodes_off
        assert _code(lambda: det.undistorted_detections(1)) == INVALID_ARGUMENT
    # the other way round: with rectification on, the mode is refused
    det.set_rectification([uc.CAMERAS["rational"]])
    assert _code(lambda: det.set_corner_undistortion([uc.CAMERAS["rational"]])) == INVALID_ARGUMENT
    det.set_corner_undistortion(None)   # (turning it off is never refused)
    det.set_rectification(None)
    det.set_corner_undistortion([uc.CAMERAS["rational"]])
    run()
    assert not _compare_twins(det.undistorted_detections(1)[0], want)
    assert det.graph_replay()[0] and det.graph_replay()[2] <= 24 and det.late_waits() == 0
    det.close()


# ---- 5. the node shell ---------------------------------------------------------------------------------------------------------------------------
def test_node_shell_publishes_the_undistorted_poses(built):
    """AprilTagNode and a two-stream AprilTagMultiCameraNode with undistort_corners (rectify="corners") on raw host frames: corners and
    centre are the raw frame's, position and "family:id" transform the twin's pose in float -- which the raw record's pose a plain node
    publishes is not -- and both kinds of rectification beside it are refused."""
    from isaac_ros_apriltag_amd import build as b
    from isaac_ros_apriltag_amd import node
    b.build_node()
    p12 = [600.0, 0.0, 320.0, 0.0, 0.0, 600.0, 240.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    k9 = [float(v) for v in uc.K_RAW.reshape(-1)]

    def feed(n, frame_name, cam, stream=None, stamp=(3, 0)):
        K, D, Kn, kind, R = uc.CAMERAS[cam]
        frame = uc.raw(frame_name, cam)
        args = (frame.ctypes.data, False, "mono8", uc.W, uc.H, uc.W, k9, "cam", stamp)
        more = {"D": list(D), "distortion_model": kind, "P12": p12, "R": R}
        return n.on_frame(*args, **more) if stream is None else n.on_frame(stream, *args, **more)

    def check(dets, tfs, frame_name, cam):
        raw, tw = uc.raw_records(frame_name, cam), uc.twins(frame_name, cam)
        assert [d["id"] for d in dets] == [r["id"] for r in raw] and len(tfs) == len(raw)
        for d, tf, r, t in zip(dets, tfs, raw, tw):
            assert t["status"] == ur.OK
            assert d["position"] == [float(np.float32(v)) for v in t["t"]] == tf["translation"]
            assert d["position"] != [float(np.float32(v)) for v in r["t"]]
            assert d["orientation_xyzw"] == tf["rotation_xyzw"]
            assert np.abs(np.asarray(d["center"]) - r["center"]).max() < 1e-3      # the raw frame's centre (float in the message)

    nodes = []
    try:
        n = node.AprilTagNode(size=bc.SIZE1, rectify="corners")
        nodes.append(n)
        dets, _ = feed(n, "nine", "rational+R")
        check(dets, n.transforms(), "nine", "rational+R")
        multi = node.AprilTagMultiCameraNode(2, size=bc.SIZE1, rectify="corners")
        nodes.append(multi)
        pairs = (("nine", "equidistant"), ("one", "plumb_bob+R"))
        for s, (f, c) in enumerate(pairs):
            assert feed(multi, f, c, s, (4, s))
        for s, (f, c) in enumerate(pairs):
            assert multi.publishes(s) == 1
            check(multi.last(s)[0], multi.transforms(s), f, c)
    finally:
        [x.close() for x in nodes]


def test_node_shell_keeps_the_identity_for_an_invalid_twin_under_refinement(built):
    """undistort_corners beside pose_refinement (and the covariance) under the camera that makes three of the nine twins invalid, on both
    node shells: a valid tag publishes the chosen refined pose of its twin; an invalid one a zero translation and the identity
    quaternion (0, 0, 0, 1) -- not its DEGENERATE refined record's zeros -- in the detection and in the transform, and a zero covariance."""
    from isaac_ros_apriltag_amd import build as b
    from isaac_ros_apriltag_amd import node
    b.build_node()
    K, D, Kn, kind, R = PARTLY_INVALID
    k9 = [float(v) for v in K.reshape(-1)]
    p12 = [600.0, 0.0, 320.0, 0.0, 0.0, 600.0, 240.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    frame = uc.raw("nine", "rational")
    raw = uc.raw_records("nine", "rational")
    tw = ur.records(raw, PARTLY_INVALID, uc.INTR, bc.SIZE1)
    refined = ur.refined(tw, uc.INTR, 0.0, bc.SIZE1, pc.ITERATIONS)
    assert 0 < sum(t["status"] for t in tw) < 9

    def check(dets, tfs, covs=None):
        assert [d["id"] for d in dets] == [r["id"] for r in raw] and len(tfs) == len(raw)
        for i, (d, tf, t, o) in enumerate(zip(dets, tfs, tw, refined)):
            assert d["orientation_xyzw"] == tf["rotation_xyzw"] and d["position"] == tf["translation"]
            assert abs(sum(q * q for q in d["orientation_xyzw"]) - 1.0) < 1e-6          # a rotation, whatever the twin
            if t["status"] == ur.INVALID:
                assert d["position"] == [0.0, 0.0, 0.0] and d["orientation_xyzw"] == [0.0, 0.0, 0.0, 1.0]
                assert covs is None or not np.asarray(covs[i]).any()
            else:
                assert o["status"] == capi.POSE_REFINED and d["position"] == [float(np.float32(v)) for v in o["t"]]
                assert covs is None or np.asarray(covs[i]).any()

    more = {"D": list(D), "distortion_model": kind, "P12": p12, "R": R}
    nodes = []
    try:
        n = node.AprilTagNode(size=bc.SIZE1, rectify="corners", pose_refinement=pc.ITERATIONS, pose_covariance=SIGMA)
        nodes.append(n)
        dets, _ = n.on_frame(frame.ctypes.data, False, "mono8", uc.W, uc.H, uc.W, k9, "cam", (3, 0), **more)
        check(dets, n.transforms(), n.covariances())
        multi = node.AprilTagMultiCameraNode(2, size=bc.SIZE1, rectify="corners", pose_refinement=pc.ITERATIONS, auto_flush=False)
        nodes.append(multi)
        assert multi.on_frame(1, frame.ctypes.data, False, "mono8", uc.W, uc.H, uc.W, k9, "cam", (4, 1), **more)
        assert multi.flush() == 1
        check(multi.last(1)[0], multi.transforms(1))
    finally:
        [x.close() for x in nodes]


# ---- 6. the suite bites -------------------------------------------------------------------------------------------------------------------------
_SELECT = "test_stage_alone or test_composition or (test_three_frame_submission and throughput)"
_STAGE = tuple("test_stage_alone[%s]" % c for c in sorted(STAGE_CAMERAS))
_WITH_R = tuple("test_stage_alone[%s]" % c for c in sorted(STAGE_CAMERAS) if c.endswith("+R") or c == "behind")
_COMPOSITION = ("test_composition[rational]", "test_composition[partly_invalid]")
_THREE = ("test_three_frame_submission[throughput-plain]",)
_WRONG_BUILDS = {
    # R taken as the identity: wrong under every camera with a rotation (two of the three frames' slots have one)
    28: {"must_fail": _WITH_R + _THREE, "says": "p differ"},
    # the pose launches read the raw records: the twins themselves are right, every consumer's record is not
    29: {"must_fail": _COMPOSITION + _THREE, "says": "R differ"},
    # every frame under cams[0]: wrong from the second slot on
    30: {"must_fail": _THREE, "says": "frame 2: record 0"},
}


@pytest.mark.parametrize("mutant", sorted(_WRONG_BUILDS))
def test_the_undistortion_tests_fail_on_the_wrong_builds(built, mutant):
    """libapriltag_amd_mut28.so .. _mut30.so (csrc/tools_hooks.h, AMDAT_MUTATE): the stage, composition and three-frame tests, in a
    process of their own, must FAIL on the wrong build exactly where its error lives, and all of them pass on the product library.  None
    of the three changes an index bound, a launch size or a loop count."""
    import subprocess
    from isaac_ros_apriltag_amd import build as bld
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(bld.lib_mutant(mutant)):
        bld.build_mutants()
    spec = _WRONG_BUILDS[mutant]
    everything = _STAGE + _COMPOSITION + _THREE

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
    assert sorted(passed) == sorted(set(everything) - set(spec["must_fail"])), (failed, passed)
    assert spec["says"] in out.stdout
    if "ok" not in _cache:   # (the product run is the same for all three wrong builds)
        _cache["ok"] = run(None)
    out_ok, passed_ok, failed_ok = _cache["ok"]
    assert out_ok.returncode == 0 and not failed_ok and sorted(passed_ok) == sorted(everything), (out_ok.stdout[-1500:], failed_ok)
