"""Orthogonal-iteration tag pose with both minima inside the submission (amdAprilTagsSetPoseRefinement, k_pose_refine).  The definition
under test is DESIGN.md section 7e, stated in Python by tests/pose_refine_ref.py: fed the oracle's records of a frame -- which the
library's own records equal bit for bit -- the reference gives the refined records the library must hand out, every double compared as
its 64 bits with numpy.array_equal, status and chosen with ==.  The oracle-side preconditions (the oblique tags are found and their
two minima differ, 72 records on the large board, the wrong builds' forms differ) are asserted in tests/test_pose_refine_cpu.py."""
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
import bundle_ref as br  # noqa: E402
import parity_util as pu  # noqa: E402
import pose_refine_cases as pc  # noqa: E402
import pose_refine_ref as pr  # noqa: E402

FAMS = list(bc.FAM)
INVALID_ARGUMENT = 1
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
    """One submission in the mode's way; (records per frame, refined records per frame)."""
    prep = det.prepare(frames, max_dets=max_dets, intrinsics=intrinsics)
    graph = mode.endswith("graph")
    for _ in range(2 if graph else 1):   # (graph: captured by the first submission, replayed by the second)
        det.submit_prepared(prep)
        det.wait_prepared(prep)
    assert det.last_submission_path() == mode.split("-")[0]
    assert (det.last_graph_nodes() > 0) == graph, (mode, det.last_graph_nodes())
    return det.unpack(prep), det.refined_poses(prep["n"])


# ---- 1. content frames ----------------------------------------------------------------------------------------------------------------------
def _content(mode):
    """The two three-frame submissions of bundle_cases' content frames in `mode`: content case -> (records, refined records)."""
    if ("content", mode) not in _cache:
        det = _handle(mode, bc.W1, bc.H1, max_batch=3, tag_size=bc.SIZE1, pose_refinement=pc.ITERATIONS)
        det.set_frame_skews(bc.SKEW1)
        out = {}
        for sub in (0, 1):
            names = [n for n in bc.CONTENT if bc.SLOTS[n][0] == sub]
            names.sort(key=lambda n: bc.SLOTS[n][1])
            frames = torch.from_numpy(np.stack([bc.content_frame(n) for n in names])).cuda()
            recs, poses = _submit(det, mode, frames, 64, list(bc.INTR1))
            for slot, n in enumerate(names):
                out[n] = (recs[slot], poses[slot])
        assert det.late_waits() == 0
        det.close()
        _cache[("content", mode)] = out
    return _cache[("content", mode)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", bc.CONTENT)
def test_content(built, name, mode):
    """640 x 480, the six-tag content frames of the bundle tests in two three-frame submissions with distinct per-frame intrinsics and a
    skew on the middle slot; the tag-free frame has no refined record."""
    recs, got = _content(mode)[name]
    want_recs = bc.content_records(name)
    assert not pu.compare_detections(recs, want_recs, exact=True)   # the input of the reference is the input of the kernel
    errs = pr.compare_frames(got, pc.content_refined(name))
    print("%s %s: %d refined records %s" % (name, mode, len(got), errs[:4]))
    assert not errs, errs
    assert len(got) == len(want_recs)
    if name == "no_tags":
        assert got == []
    else:
        assert all(g["status"] == capi.POSE_REFINED and g["err"] <= g["err_homography"] for g in got)


# ---- 2. oblique tags: two distinct minima ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_oblique_tags(built, mode):
    """Four tags at 35 .. 60 degrees of tilt: the alternative is another pose, tens of degrees away."""
    det = _handle(mode, pc.WO, pc.HO, tag_size=pc.SIZE_O, intrinsics=pc.INTR_O, pose_refinement=pc.ITERATIONS)
    recs, poses = _submit(det, mode, torch.from_numpy(pc.oblique_frame()).cuda(), 64, None)
    det.close()
    want_recs = pc.oblique_records()
    assert len(want_recs) == 4 and not pu.compare_detections(recs[0], want_recs, exact=True)
    errs = pr.compare_frames(poses[0], pc.refined("oblique", want_recs, pc.INTR_O, 0.0, pc.SIZE_O))
    print("oblique %s: %s" % (mode, errs[:4]))
    assert not errs, errs
    assert all(g["status"] == capi.POSE_REFINED and pr.rot_angle_deg(g["R"], g["R_alt"]) > 20.0 for g in poses[0])


# ---- 3. more records than one wave, and than one hand-out -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_board72(built, mode):
    """640 x 576, 72 tags: nine waves of eight records.  With max_dets = 8 eight records are handed out and eight refined."""
    det = _handle(mode, bc.W2, bc.H2, tag_size=bc.SIZE2, intrinsics=bc.INTR2, pose_refinement=pc.ITERATIONS)
    frame = torch.from_numpy(bc.frame72()).cuda()
    want = pc.refined("board72", bc.records72(), bc.INTR2, 0.0, bc.SIZE2)
    assert len(want) == 72
    errs = []
    for max_dets in (128, 8):
        recs, poses = _submit(det, mode, frame, max_dets, None)
        assert len(recs[0]) == min(max_dets, 72) == len(poses[0])
        assert not pu.compare_detections(recs[0], bc.records72()[:max_dets], exact=True)
        errs += pr.compare_frames(poses[0], want[:max_dets], "max_dets %d: " % max_dets)
    det.close()
    print("board72 %s: %s" % (mode, errs[:4]))
    assert not errs, errs


# ---- 4. the iteration count lives in device memory ------------------------------------------------------------------------------------------
def test_iteration_count_changes_no_graph(built):
    """1 and 50 iterations on one handle: the graph captured with one count is replayed with the other."""
    det = AprilTagDetector(pc.WO, pc.HO, tag_size=pc.SIZE_O, intrinsics=pc.INTR_O, pose_refinement=1)
    prep = det.prepare(torch.from_numpy(pc.oblique_frame()).cuda(), max_dets=64)
    errs = []
    state = None
    for it in (1, pc.ITERATIONS, 1):
        det.set_pose_refinement(it)
        det.run_prepared(prep)
        det.run_prepared(prep)
        assert det.last_graph_nodes() > 0
        if state is None:
            state = det.graph_replay()
        assert det.graph_replay() == state == (True, 1, 0)
        errs += pr.compare_frames(det.refined_poses(1)[0], pc.refined("oblique", pc.oblique_records(), pc.INTR_O, 0.0, pc.SIZE_O, iterations=it),
                                  "%d iterations: " % it)
    det.close()
    one = pc.refined("oblique", pc.oblique_records(), pc.INTR_O, 0.0, pc.SIZE_O, iterations=1)
    assert all(pr.compare(a, b) for a, b in zip(one, pc.refined("oblique", pc.oblique_records(), pc.INTR_O, 0.0, pc.SIZE_O)))   # (the counts differ)
    assert not errs, errs


# ---- 5. together with bundles ---------------------------------------------------------------------------------------------------------------
def test_together_with_bundles(built):
    """Both launches behind k_reconcile in one submission: both record sets equal their references, replayed from a graph."""
    det = AprilTagDetector(bc.W1, bc.H1, tag_size=bc.SIZE1, intrinsics=bc.INTR1[0], bundles=[bc.BUNDLE1], pose_refinement=pc.ITERATIONS)
    prep = det.prepare(torch.from_numpy(bc.content_frame("all_six")).cuda(), max_dets=64)
    det.run_prepared(prep)
    det.run_prepared(prep)
    assert det.last_graph_nodes() > 0
    recs = det.unpack(prep)[0]
    want_recs = bc.oracle_records(bc.content_frame("all_six"), bc.INTR1[0])
    assert not pu.compare_detections(recs, want_recs, exact=True)
    errs = br.compare(det.bundle_poses(1)[0][0], br.solve(want_recs, bc.BUNDLE1, FAMS, bc.INTR1[0]))
    errs += pr.compare_frames(det.refined_poses(1)[0], pc.refined("all_six-0", want_recs, bc.INTR1[0], 0.0, bc.SIZE1))
    det.close()
    assert not errs, errs


# ---- 6. off means off; the setter's contract ------------------------------------------------------------------------------------------------
def test_off_means_off_and_the_setter_contract(built):
    import ctypes as C
    frame = torch.from_numpy(bc.content_frame("all_six")).cuda()
    det = AprilTagDetector(bc.W1, bc.H1, tag_size=bc.SIZE1, intrinsics=bc.INTR1[0], max_batch=2)
    L, h = capi.lib(), det._h
    want = pc.refined("all_six-0", bc.oracle_records(bc.content_frame("all_six"), bc.INTR1[0]), bc.INTR1[0], 0.0, bc.SIZE1)

    def run():
        prep = det.prepare(frame, max_dets=64)
        det.run_prepared(prep)
        return bytes(prep["out"]), int(prep["cnt"][0])

    # off is the default: no records to hand out, turning it off again changes nothing, no memory, the parent's launches
    bytes0 = det.device_bytes()
    off_out, off_cnt = run()
    run()
    nodes_off = det.last_graph_nodes()
    assert nodes_off > 0 and off_cnt == 6
    assert _code(lambda: det.refined_poses(1)) == INVALID_ARGUMENT
    det.set_pose_refinement(0)
    assert det.device_bytes() == bytes0 and det.graph_replay() == (True, 1, 0)
    # on: the detection records are the same bytes, one launch more in the graph
    det.set_pose_refinement(pc.ITERATIONS)
    assert det.graph_replay() == (True, 0, 1)   # the graph captured without the launch is retired
    on_out, on_cnt = run()
    assert det.last_graph_nodes() == nodes_off + 1   # (captured by this submission, and replayed at once)
    assert (on_out, on_cnt) == (off_out, off_cnt)
    assert not pr.compare_frames(det.refined_poses(1)[0], want)
    assert run() == (off_out, off_cnt) and det.last_graph_nodes() == nodes_off + 1
    assert not pr.compare_frames(det.refined_poses(1)[0], want)
    # the getter's refusals: a frame beyond the last submission's, a capacity below the count (which still comes back), null pointers
    n = C.c_uint32(99)
    out = (capi.RefinedPose * 8)()
    assert L.amdAprilTagsGetRefinedPoses(h, 1, out, 8, C.byref(n)) == INVALID_ARGUMENT and n.value == 99
    assert L.amdAprilTagsGetRefinedPoses(h, 0, out, 5, C.byref(n)) == INVALID_ARGUMENT and n.value == 6
    assert L.amdAprilTagsGetRefinedPoses(h, 0, None, 8, C.byref(n)) == INVALID_ARGUMENT
    assert L.amdAprilTagsGetRefinedPoses(h, 0, out, 8, None) == INVALID_ARGUMENT
    assert L.amdAprilTagsGetRefinedPoses(h, 0, out, 6, C.byref(n)) == 0 and n.value == 6
    # refused setter calls leave the previous setting in force; nothing is retired
    state = det.graph_replay()
    assert _code(lambda: det.set_pose_refinement(201)) == INVALID_ARGUMENT
    assert L.amdAprilTagsSetPoseRefinement(None, 50) == INVALID_ARGUMENT
    assert det.graph_replay() == state
    assert run() == (off_out, off_cnt) and not pr.compare_frames(det.refined_poses(1)[0], want)
    # between Submit and Wait both calls are refused
    prep = det.prepare(frame, max_dets=64)
    det.submit_prepared(prep)
    assert _code(lambda: det.set_pose_refinement(0)) == INVALID_ARGUMENT
    assert _code(lambda: det.set_pose_refinement(10)) == INVALID_ARGUMENT
    assert _code(lambda: det.refined_poses(1)) == INVALID_ARGUMENT
    det.wait_prepared(prep)
    assert not pr.compare_frames(det.refined_poses(1)[0], want)
    assert det.graph_replay() == state
    # ThresholdOnly never refines: afterwards there is nothing to hand out
    det.threshold_only(frame)
    assert _code(lambda: det.refined_poses(1)) == INVALID_ARGUMENT
    assert run() == (off_out, off_cnt) and not pr.compare_frames(det.refined_poses(1)[0], want)
    # off again: the graphs with the launch are retired, the parent's node count is back, the getter is refused
    capturing, live, retired = det.graph_replay()
    det.set_pose_refinement(0)
    assert det.graph_replay() == (True, 0, retired + live)
    assert run() == (off_out, off_cnt)
    assert run() == (off_out, off_cnt) and det.last_graph_nodes() == nodes_off
    assert _code(lambda: det.refined_poses(1)) == INVALID_ARGUMENT
    assert det.late_waits() == 0
    det.close()


# ---- 7. the node shell ----------------------------------------------------------------------------------------------------------------------
def _quat_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_node_shell_publishes_the_chosen_pose(built):
    """AprilTagNode and a two-stream AprilTagMultiCameraNode with pose_refinement on, on the oblique frame: position and "family:id"
    transform are the chosen refined pose -- the translation as its float, the rotation through the float quaternion -- which the
    homography pose a plain node publishes is not."""
    from isaac_ros_apriltag_amd import build as b
    from isaac_ros_apriltag_amd import node
    b.build_node()
    k9 = [600.0, 0.0, 320.0, 0.0, 600.0, 240.0, 0.0, 0.0, 1.0]
    frame = pc.oblique_frame()
    recs = pc.oblique_records()
    want = pc.refined("oblique", recs, pc.INTR_O, 0.0, pc.SIZE_O)

    def check(dets, tfs, stamp):
        assert [d["id"] for d in dets] == [r["id"] for r in recs]
        assert [t["child_frame_id"] for t in tfs] == ["tag36h11:%d" % r["id"] for r in recs]
        for d, tf, w, r in zip(dets, tfs, want, recs):
            assert tf["frame_id"] == "cam" and tf["stamp"] == stamp
            assert d["position"] == [float(np.float32(v)) for v in w["t"]] == tf["translation"]
            assert d["orientation_xyzw"] == tf["rotation_xyzw"]
            assert np.abs(_quat_matrix(d["orientation_xyzw"]) - w["R"]).max() < 1e-6          # (float quaternion)
            assert np.abs(_quat_matrix(d["orientation_xyzw"]) - r["R"]).max() > 1e-4          # not the homography pose

    nodes = []
    try:
        n = node.AprilTagNode(size=pc.SIZE_O, pose_refinement=pc.ITERATIONS)
        nodes.append(n)
        dets, _ = n.on_frame(frame.ctypes.data, False, "mono8", pc.WO, pc.HO, pc.WO, k9, "cam", (3, 0))
        check(dets, n.transforms(), (3, 0))
        plain = node.AprilTagNode(size=pc.SIZE_O)
        nodes.append(plain)
        pdets, _ = plain.on_frame(frame.ctypes.data, False, "mono8", pc.WO, pc.HO, pc.WO, k9, "cam", (3, 0))
        assert [d["corners"] for d in pdets] == [d["corners"] for d in dets]
        assert [d["position"] for d in pdets] == [[float(np.float32(v)) for v in r["t"]] for r in recs]
        multi = node.AprilTagMultiCameraNode(2, size=pc.SIZE_O, pose_refinement=pc.ITERATIONS)
        nodes.append(multi)
        for s in (0, 1):
            assert multi.on_frame(s, frame.ctypes.data, False, "mono8", pc.WO, pc.HO, pc.WO, k9, "cam", (4, s))
        for s in (0, 1):
            assert multi.publishes(s) == 1
            check(multi.last(s)[0], multi.transforms(s), (4, s))
    finally:
        [x.close() for x in nodes]


# ---- 8. the suite bites ---------------------------------------------------------------------------------------------------------------------
_SELECT = "test_content and throughput"
_WITH_TAGS = tuple("test_content[%s-throughput-plain]" % n for n in bc.CONTENT if n != "no_tags")
_WRONG_BUILDS = {
    # chain 1 starts unmirrored: the alternative of every record is the chosen pose again; a frame without tags has no record
    17: {"must_fail": _WITH_TAGS, "must_pass": ("test_content[no_tags-throughput-plain]",), "says": "R_alt differ"},
    # no t(R) after the last iteration: every record carries another translation
    18: {"must_fail": _WITH_TAGS, "must_pass": ("test_content[no_tags-throughput-plain]",), "says": ": t differ"},
}


@pytest.mark.parametrize("mutant", sorted(_WRONG_BUILDS))
def test_the_pose_refinement_tests_fail_on_the_wrong_builds(built, mutant):
    """libapriltag_amd_mut17.so and _mut18.so (csrc/tools_hooks.h, AMDAT_MUTATE): the content cases on the throughput set, in a process
    of their own, must FAIL on the wrong build exactly where its error lives, and all of them pass on the product library.  Both wrong
    builds change values only."""
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
    assert spec["says"] in out.stdout   # what differs: fields of the refined record
    if "ok" not in _cache:   # (the product run is the same for both wrong builds)
        _cache["ok"] = run(None)
    out_ok, passed_ok, failed_ok = _cache["ok"]
    assert out_ok.returncode == 0 and not failed_ok and sorted(passed_ok) == sorted(passed + failed), (out_ok.stdout[-1500:], failed_ok)
