"""Pose covariance inside the submission (amdAprilTagsSetPoseCovariance, k_pose_refine<true>, k_bundle_rigid<true>).  The definition
under test is DESIGN.md section 7g, stated in Python by tests/pose_cov_ref.py: a pure function of the reported pose, the points, the
camera and sigma.  Fed the reference's refined records and rigid bundle records of a frame -- which the library's own equal bit for
bit, as asserted here again -- it gives the covariance records the library must hand out, every double compared as its 64 bits, the
valid word with ==.  The reference-side preconditions are asserted in tests/test_pose_covariance_cpu.py."""
import ctypes as C
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
import pose_cov_ref as pv  # noqa: E402
import pose_refine_cases as pc  # noqa: E402
import pose_refine_ref as pr  # noqa: E402
import rigid_bundle_cases as rc  # noqa: E402
import rigid_bundle_ref as rr  # noqa: E402

FAMS = rc.FAMS
INVALID_ARGUMENT = 1
SIGMA = 0.3
# launch set and how the submission goes out: replayed from a captured graph (the second of two submissions), or as plain enqueues
MODES = ("latency-graph", "latency-plain", "throughput-plain")
_cache = {}


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


def _submit(det, mode, frames, max_dets, intrinsics):
    """One submission in the mode's way; the prepared submission (results in it and in the handle)."""
    prep = det.prepare(frames, max_dets=max_dets, intrinsics=intrinsics)
    graph = mode.endswith("graph")
    for _ in range(2 if graph else 1):   # (graph: captured by the first submission, replayed by the second)
        det.submit_prepared(prep)
        det.wait_prepared(prep)
    assert det.last_submission_path() == mode.split("-")[0]
    assert (det.last_graph_nodes() > 0) == graph, (mode, det.last_graph_nodes())
    return prep


def _refined_bytes(det, frame, n):
    arr = (capi.RefinedPose * max(n, 1))()
    cnt = C.c_uint32(0)
    assert capi.lib().amdAprilTagsGetRefinedPoses(det._h, frame, arr, n, C.byref(cnt)) == 0 and cnt.value == n
    return bytes(arr)[:n * C.sizeof(capi.RefinedPose)]


def _tag_check(label, got, records, intr, skew, size, refined, sigma=SIGMA):
    errs = pv.compare_frames(got, pv.tag_records(records, intr, skew, size, refined, sigma), label + ": ")
    print("%s: %d covariance records, valid %s %s" % (label, len(got), [int(g["valid"]) for g in got][:8], errs[:4]))
    return errs


# ---- 1. oblique tags: four records, idle tail groups in the wave ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_oblique_tags(built, mode):
    """Four tags at 35 .. 60 degrees of tilt in one wave: cov, cov_alt, residuals and valid bits of every record bit for bit; the refined
    pose records and the detection records are the bytes of a handle with the mode off."""
    frame = torch.from_numpy(pc.oblique_frame()).cuda()
    want_recs = pc.oblique_records()
    refined = pc.refined("oblique", want_recs, pc.INTR_O, 0.0, pc.SIZE_O)
    out = {}
    for sigma in (SIGMA, 0.0):
        det = _handle(mode, pc.WO, pc.HO, tag_size=pc.SIZE_O, intrinsics=pc.INTR_O, pose_refinement=pc.ITERATIONS, pose_covariance=sigma)
        prep = _submit(det, mode, frame, 64, None)
        assert not pu.compare_detections(det.unpack(prep)[0], want_recs, exact=True)
        assert not pr.compare_frames(det.refined_poses(1)[0], refined)
        out[sigma] = (bytes(prep["out"]), int(prep["cnt"][0]), _refined_bytes(det, 0, 4))
        if sigma:
            got = det.refined_pose_covariances(1)[0]
        else:
            assert _code(lambda: det.refined_pose_covariances(1)) == INVALID_ARGUMENT
        assert det.late_waits() == 0
        det.close()
    assert out[SIGMA] == out[0.0]
    errs = _tag_check("oblique %s" % mode, got, want_recs, pc.INTR_O, 0.0, pc.SIZE_O, refined)
    assert not errs, errs
    assert len(got) == 4 and all(int(g["valid"]) == 3 and (np.diag(g["cov"]) > 0).all() and np.array_equal(g["cov"], g["cov"].T) for g in got)
    # the alternative, tens of degrees away, has another covariance
    assert all(not np.array_equal(g["cov"], g["cov_alt"]) for g in got)


# ---- 2. content frames: per-frame cameras, a skew on the middle slot -----------------------------------------------------------------------
def _content(mode):
    if ("content", mode) not in _cache:
        det = _handle(mode, bc.W1, bc.H1, max_batch=3, tag_size=bc.SIZE1, pose_refinement=pc.ITERATIONS, pose_covariance=SIGMA)
        det.set_frame_skews(bc.SKEW1)
        out = {}
        for sub in (0, 1):
            names = [n for n in bc.CONTENT if bc.SLOTS[n][0] == sub]
            names.sort(key=lambda n: bc.SLOTS[n][1])
            frames = torch.from_numpy(np.stack([bc.content_frame(n) for n in names])).cuda()
            prep = _submit(det, mode, frames, 64, list(bc.INTR1))
            recs, poses, covs = det.unpack(prep), det.refined_poses(3), det.refined_pose_covariances(3)
            for slot, n in enumerate(names):
                out[n] = (recs[slot], poses[slot], covs[slot])
        assert det.late_waits() == 0
        det.close()
        _cache[("content", mode)] = out
    return _cache[("content", mode)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", bc.CONTENT)
def test_content(built, name, mode):
    """640 x 480, the six-tag content frames of the bundle tests in two three-frame submissions with distinct per-frame intrinsics and a
    skew of 0.75 on the middle slot; the tag-free frame has no record."""
    recs, poses, got = _content(mode)[name]
    slot = bc.SLOTS[name][1]
    want_recs = bc.content_records(name)
    assert not pu.compare_detections(recs, want_recs, exact=True)
    assert not pr.compare_frames(poses, pc.content_refined(name))
    errs = _tag_check("%s %s" % (name, mode), got, want_recs, bc.INTR1[slot], bc.SKEW1[slot], bc.SIZE1, pc.content_refined(name))
    assert not errs, errs
    assert len(got) == len(want_recs)
    if name == "no_tags":
        assert len(got) == 0
    else:
        assert all(int(g["valid"]) == 3 for g in got)


# ---- 3. more records than one wave; the last wave clipped by the hand-out ------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_board72(built, mode):
    """640 x 576, 72 tags.  max_dets = 13: two waves, the second one's tail clipped by the records handed out; then all 72, nine full
    waves."""
    det = _handle(mode, bc.W2, bc.H2, tag_size=bc.SIZE2, intrinsics=bc.INTR2, pose_refinement=pc.ITERATIONS, pose_covariance=SIGMA)
    frame = torch.from_numpy(bc.frame72()).cuda()
    refined = pc.refined("board72", bc.records72(), bc.INTR2, 0.0, bc.SIZE2)
    errs = []
    for max_dets in (13, 128):
        prep = _submit(det, mode, frame, max_dets, None)
        n = min(max_dets, 72)
        assert not pu.compare_detections(det.unpack(prep)[0], bc.records72()[:max_dets], exact=True)
        assert not pr.compare_frames(det.refined_poses(1)[0], refined[:max_dets])
        got = det.refined_pose_covariances(1)[0]
        assert len(got) == n
        errs += _tag_check("board72 %s max_dets %d" % (mode, max_dets), got, bc.records72()[:n], bc.INTR2, 0.0, bc.SIZE2, refined[:n])
    assert det.late_waits() == 0
    det.close()
    assert not errs, errs


# ---- 4. rigid bundles ------------------------------------------------------------------------------------------------------------------------
def _bundle_check(label, got, records, bundle, intr, skew, solved):
    want = pv.bundle_record_of(records, bundle, FAMS, intr, skew, solved, SIGMA)
    errs = pv.compare(got, want, label + ": ")
    print("%s: status %d valid %d (the reference %d) %s" % (label, solved["status"], int(got["valid"]), want["valid"], errs[:3]))
    return errs, want


@pytest.mark.parametrize("mode", MODES)
def test_rigid_cube(built, mode):
    """The three-frame cube submission with two bundles (a skew on the middle slot): a non-coplanar set, a coplanar set with its
    alternative, a one-tag bundle, and the zeroed record of a bundle with too few tags."""
    det = _handle(mode, rc.W1, rc.H1, max_batch=3, tag_size=bc.SIZE1, bundles_ex=rc.CUBE_BUNDLES, pose_covariance=SIGMA)
    det.set_frame_skews(bc.SKEW1)
    frames = torch.from_numpy(np.stack([rc.cube_frame(n) for n in rc.CUBE_FRAMES])).cuda()
    prep = _submit(det, mode, frames, 64, list(bc.INTR1))
    recs, poses, covs = det.unpack(prep), det.bundle_poses_ex(3), det.bundle_pose_covariances_ex(3)
    assert det.late_waits() == 0
    det.close()
    assert covs.shape == (3, 2)
    errs, valid = [], {}
    for slot, name in enumerate(rc.CUBE_FRAMES):
        assert not pu.compare_detections(recs[slot], rc.cube_records(name), exact=True)
        for b, bundle in enumerate(rc.CUBE_BUNDLES):
            solved = rc.cube_solved(name)[b]
            assert not rr.compare(poses[slot][b], solved)
            e, want = _bundle_check("%s %s %s" % (name, bundle["name"], mode), covs[slot][b], rc.cube_records(name), bundle, bc.INTR1[slot],
                                    bc.SKEW1[slot], solved)
            errs += e
            valid[(name, bundle["name"])] = want["valid"]
    assert not errs, errs
    assert valid == {("cube_a", "cube"): 3, ("cube_a", "lone"): 0, ("one_face", "cube"): 3, ("one_face", "lone"): 3, ("cube_b", "cube"): 3,
                     ("cube_b", "lone"): 0}
    assert not covs[0][1]["cov"].any() and not covs[0][1]["cov_alt"].any()   # too few tags: zeros


@pytest.mark.parametrize("mode", MODES)
def test_rigid_full_wave_and_across_chunks(built, mode):
    """640 x 576, 72 records: 64 used tags, one on every lane; then 12 members from both ends of the id range."""
    det = _handle(mode, bc.W2, bc.H2, tag_size=bc.SIZE2, intrinsics=bc.INTR2, bundles_ex=[rc.FULL_WAVE], pose_covariance=SIGMA)
    frame = torch.from_numpy(bc.frame72()).cuda()
    errs = []
    for which, bundle in (("wave", rc.FULL_WAVE), ("ends", rc.BOTH_ENDS)):
        det.set_bundles_ex([bundle])
        prep = _submit(det, mode, frame, 128, None)
        assert not pu.compare_detections(det.unpack(prep)[0], bc.records72(), exact=True)
        assert not rr.compare(det.bundle_poses_ex(1)[0][0], rc.solved72(which))
        e, want = _bundle_check("%s %s" % (which, mode), det.bundle_pose_covariances_ex(1)[0][0], bc.records72(), bundle, bc.INTR2, 0.0, rc.solved72(which))
        errs += e
        assert want["valid"] & 1
    assert det.late_waits() == 0
    det.close()
    assert not errs, errs


def test_tags_and_bundles_together(built):
    """Pose refinement and rigid bundles in one submission, both as their covariance instances, replayed from a graph."""
    det = AprilTagDetector(bc.W1, bc.H1, tag_size=bc.SIZE1, intrinsics=bc.INTR1[0], bundles_ex=[rc.BUNDLE1], pose_refinement=pc.ITERATIONS,
                           pose_covariance=SIGMA)
    prep = det.prepare(torch.from_numpy(bc.content_frame("all_six")).cuda(), max_dets=64)
    det.run_prepared(prep)
    det.run_prepared(prep)
    assert det.last_graph_nodes() > 0
    want_recs = bc.content_records("all_six")
    assert not pu.compare_detections(det.unpack(prep)[0], want_recs, exact=True)
    solved = rc.content_solved("all_six")
    assert not rr.compare(det.bundle_poses_ex(1)[0][0], solved) and not pr.compare_frames(det.refined_poses(1)[0], pc.content_refined("all_six"))
    errs, _ = _bundle_check("together", det.bundle_pose_covariances_ex(1)[0][0], want_recs, rc.BUNDLE1, bc.INTR1[0], 0.0, solved)
    errs += _tag_check("together", det.refined_pose_covariances(1)[0], want_recs, bc.INTR1[0], 0.0, bc.SIZE1, pc.content_refined("all_six"))
    assert det.late_waits() == 0
    det.close()
    assert not errs, errs


# ---- 5. off means off; the setter's contract ---------------------------------------------------------------------------------------------
def test_off_means_off_and_the_setter_contract(built):
    frame = torch.from_numpy(pc.oblique_frame()).cuda()
    det = AprilTagDetector(pc.WO, pc.HO, tag_size=pc.SIZE_O, intrinsics=pc.INTR_O, pose_refinement=pc.ITERATIONS)
    L, h = capi.lib(), det._h
    recs = pc.oblique_records()
    refined = pc.refined("oblique", recs, pc.INTR_O, 0.0, pc.SIZE_O)
    prep = det.prepare(frame, max_dets=64)

    def run():
        det.run_prepared(prep)
        return bytes(prep["out"]), int(prep["cnt"][0]), _refined_bytes(det, 0, 4)

    # off is the default: both getters refuse, turning it off again changes nothing, no device memory
    bytes0 = det.device_bytes()
    off = run()
    assert run() == off
    nodes = det.last_graph_nodes()
    assert nodes > 0
    out = (capi.PoseCovariance * 8)()
    n = C.c_uint32(99)
    assert L.amdAprilTagsGetRefinedPoseCovariances(h, 0, out, 8, C.byref(n)) == INVALID_ARGUMENT and n.value == 99
    assert L.amdAprilTagsGetBundlePoseCovariancesEx(h, out, 1) == INVALID_ARGUMENT
    det.set_pose_covariance(0.0)
    assert det.device_bytes() == bytes0 and det.graph_replay() == (True, 1, 0)
    # the setter's refusals leave the setting and the graphs alone
    for bad in (float("nan"), float("inf"), float("-inf"), -0.5):
        assert _code(lambda: det.set_pose_covariance(bad)) == INVALID_ARGUMENT
    assert det.graph_replay() == (True, 1, 0) and run() == off
    # on: the graph captured with the other instance is retired, once; the launch count stays; the records are the same bytes
    det.set_pose_covariance(SIGMA)
    assert det.graph_replay() == (True, 0, 1)
    assert run() == off and det.last_graph_nodes() == nodes
    first = det.refined_pose_covariances(1)[0].tobytes()
    assert not _tag_check("on", det.refined_pose_covariances(1)[0], recs, pc.INTR_O, 0.0, pc.SIZE_O, refined)
    assert run() == off and det.refined_pose_covariances(1)[0].tobytes() == first   # a replayed submission: the same bytes
    assert L.amdAprilTagsGetBundlePoseCovariancesEx(h, out, 1) == INVALID_ARGUMENT   # (no rigid bundles in that submission)
    # the getter's refusals
    assert L.amdAprilTagsGetRefinedPoseCovariances(h, 1, out, 8, C.byref(n)) == INVALID_ARGUMENT and n.value == 99
    assert L.amdAprilTagsGetRefinedPoseCovariances(h, 0, out, 3, C.byref(n)) == INVALID_ARGUMENT and n.value == 4
    assert L.amdAprilTagsGetRefinedPoseCovariances(h, 0, None, 8, C.byref(n)) == INVALID_ARGUMENT
    assert L.amdAprilTagsGetRefinedPoseCovariances(h, 0, out, 8, None) == INVALID_ARGUMENT
    assert L.amdAprilTagsGetRefinedPoseCovariances(h, 0, out, 4, C.byref(n)) == 0 and n.value == 4
    # another sigma: no graph is retired, and the result is the reference's at the new value
    state = det.graph_replay()
    assert state == (True, 1, 1)
    for sigma in (1.25, SIGMA):
        det.set_pose_covariance(sigma)
        assert run() == off and det.last_graph_nodes() == nodes and det.graph_replay() == state
        assert not _tag_check("sigma %g" % sigma, det.refined_pose_covariances(1)[0], recs, pc.INTR_O, 0.0, pc.SIZE_O, refined, sigma)
    assert det.refined_pose_covariances(1)[0].tobytes() == first
    assert _code(lambda: det.set_pose_covariance(float("nan"))) == INVALID_ARGUMENT and det.graph_replay() == state
    # between Submit and Wait the setter and the getter are refused
    det.submit_prepared(prep)
    assert _code(lambda: det.set_pose_covariance(0.0)) == INVALID_ARGUMENT
    assert _code(lambda: det.set_pose_covariance(0.5)) == INVALID_ARGUMENT
    assert _code(lambda: det.refined_pose_covariances(1)) == INVALID_ARGUMENT
    det.wait_prepared(prep)
    assert det.refined_pose_covariances(1)[0].tobytes() == first and det.graph_replay() == state
    # pose refinement off: nothing to hand out, though the mode is on
    det.set_pose_refinement(0)
    det.run_prepared(prep)
    assert _code(lambda: det.refined_pose_covariances(1)) == INVALID_ARGUMENT
    det.set_pose_refinement(pc.ITERATIONS)
    assert run() == off and det.refined_pose_covariances(1)[0].tobytes() == first
    # off again: the graphs are retired, the getter refuses, the bytes stay
    _, live, retired = det.graph_replay()
    det.set_pose_covariance(0.0)
    assert det.graph_replay() == (True, 0, retired + live)
    assert run() == off and run() == off and det.last_graph_nodes() == nodes
    assert _code(lambda: det.refined_pose_covariances(1)) == INVALID_ARGUMENT
    assert det.late_waits() == 0
    det.close()


# ---- 6. the node shell ------------------------------------------------------------------------------------------------------------------------
def test_node_shell_publishes_the_covariance(built):
    """AprilTagNode and a two-stream AprilTagMultiCameraNode with pose_refinement and pose_covariance on, on the oblique frame:
    detection.pose.pose.covariance is the chosen pose's 36 doubles, bit for bit; the rigid bundle's covariance is published the same
    way; with the option at 0 everything stays zero."""
    from isaac_ros_apriltag_amd import build as b
    from isaac_ros_apriltag_amd import node
    b.build_node()
    k9 = [600.0, 0.0, 320.0, 0.0, 600.0, 240.0, 0.0, 0.0, 1.0]
    frame = pc.oblique_frame()
    recs = pc.oblique_records()
    want = pv.tag_records(recs, pc.INTR_O, 0.0, pc.SIZE_O, pc.refined("oblique", recs, pc.INTR_O, 0.0, pc.SIZE_O), SIGMA)
    # a one-tag rigid bundle on tag 8 of the frame: (id, (x, y, z), (qw, qx, qy, qz), size)
    shell_bundle = {"name": "eight", "iterations": pc.ITERATIONS, "members": [(8, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), pc.SIZE_O)],
                    "max_hamming": 0, "min_decision_margin": 0.0, "min_tags": 1}
    ref_bundle = {"name": "eight", "iterations": pc.ITERATIONS, "members": [(0, 8, np.eye(3), np.zeros(3), pc.SIZE_O)], "max_hamming": 0,
                  "min_decision_margin": 0.0, "min_tags": 1}
    solved = rr.solve(recs, ref_bundle, FAMS, pc.INTR_O)
    want_bundle = pv.bundle_record_of(recs, ref_bundle, FAMS, pc.INTR_O, 0.0, solved, SIGMA)
    assert solved["status"] == rr.SOLVED and want_bundle["valid"] & 1 and all(w["valid"] & 1 for w in want)

    def check(dets, covs, bundle_covs):
        assert [d["id"] for d in dets] == [r["id"] for r in recs] and len(covs) == len(recs)
        for c, w in zip(covs, want):
            assert np.array_equal(pr.bits(c), pr.bits(w["cov"]))
        assert len(bundle_covs) == 1 and np.array_equal(pr.bits(bundle_covs[0]), pr.bits(want_bundle["cov"]))

    nodes = []
    try:
        n = node.AprilTagNode(size=pc.SIZE_O, pose_refinement=pc.ITERATIONS, rigid_bundles=[shell_bundle], pose_covariance=SIGMA)
        nodes.append(n)
        dets, _ = n.on_frame(frame.ctypes.data, False, "mono8", pc.WO, pc.HO, pc.WO, k9, "cam", (3, 0))
        check(dets, n.covariances(), n.rigid_bundle_covariances())
        for kw in ({"pose_refinement": pc.ITERATIONS}, {"rigid_bundles": [shell_bundle]}):
            plain = node.AprilTagNode(size=pc.SIZE_O, **kw)
            nodes.append(plain)
            pdets, _ = plain.on_frame(frame.ctypes.data, False, "mono8", pc.WO, pc.HO, pc.WO, k9, "cam", (3, 0))
            assert len(pdets) == len(recs) and len(plain.covariances()) == len(recs) and not any(c.any() for c in plain.covariances())
            assert not any(c.any() for c in plain.rigid_bundle_covariances())
        multi = node.AprilTagMultiCameraNode(2, size=pc.SIZE_O, pose_refinement=pc.ITERATIONS, rigid_bundles=[shell_bundle], pose_covariance=SIGMA)
        nodes.append(multi)
        for s in (0, 1):
            assert multi.on_frame(s, frame.ctypes.data, False, "mono8", pc.WO, pc.HO, pc.WO, k9, "cam", (4, s))
        for s in (0, 1):
            assert multi.publishes(s) == 1
            check(multi.last(s)[0], multi.covariances(s), multi.rigid_bundle_covariances(s))
        with pytest.raises(ValueError):
            node.AprilTagNode(size=pc.SIZE_O, pose_covariance=SIGMA)   # (nothing to act on: refused by this view)
    finally:
        [x.close() for x in nodes]


# ---- 7. the suite bites -----------------------------------------------------------------------------------------------------------------------
_SELECT = "(test_content or test_rigid_cube) and throughput"
_CONTENT_IDS = {n: "test_content[%s-throughput-plain]" % n for n in bc.CONTENT}
_CUBE_ID = "test_rigid_cube[throughput-plain]"
_SKEWED = tuple(_CONTENT_IDS[n] for n in bc.CONTENT if n != "no_tags" and bc.SKEW1[bc.SLOTS[n][1]] != 0.0)
_WITH_TAGS = tuple(_CONTENT_IDS[n] for n in bc.CONTENT if n != "no_tags")
_WRONG_BUILDS = {
    # no skew term in J_u: wrong on the middle slot of every submission, whose camera has a skew -- tags and bundles alike
    25: {"must_fail": _SKEWED + (_CUBE_ID,), "says": "cov differ"},
    # the second quad at chain 0's pose: the alternative's covariance of every tag is the chosen one's; bundles are untouched
    26: {"must_fail": _WITH_TAGS, "says": "cov_alt differ"},
    # centred object points: every bundle whose points do not average to the origin; tags are untouched
    27: {"must_fail": (_CUBE_ID,), "says": "cov differ"},
}


@pytest.mark.parametrize("mutant", sorted(_WRONG_BUILDS))
def test_the_pose_covariance_tests_fail_on_the_wrong_builds(built, mutant):
    """libapriltag_amd_mut25.so .. _mut27.so (csrc/tools_hooks.h, AMDAT_MUTATE): the content cases and the cube submission on the
    throughput set, in a process of their own, must FAIL on the wrong build exactly where its error lives, and all of them pass on the
    product library.  All three wrong builds change values only."""
    import subprocess
    from isaac_ros_apriltag_amd import build as bld
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(bld.lib_mutant(mutant)):
        bld.build_mutants()
    spec = _WRONG_BUILDS[mutant]
    everything = sorted(_CONTENT_IDS.values()) + [_CUBE_ID]

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
    assert spec["says"] in out.stdout   # what differs: fields of the covariance record
    if "ok" not in _cache:   # (the product run is the same for all wrong builds)
        _cache["ok"] = run(None)
    out_ok, passed_ok, failed_ok = _cache["ok"]
    assert out_ok.returncode == 0 and not failed_ok and sorted(passed_ok) == sorted(everything), (out_ok.stdout[-1500:], failed_ok)
