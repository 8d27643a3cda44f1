"""Rigid 3-D tag bundles inside the submission (amdAprilTagsSetBundlesEx, k_bundle_rigid).  The definition under test is DESIGN.md
section 7f, stated in Python by tests/rigid_bundle_ref.py: fed the oracle's records of a frame -- which the library's own records
equal bit for bit -- the reference gives the rigid bundle record the library must hand out, every double compared as its 64 bits
with numpy.array_equal, the counts, seed and chosen with ==.  The oracle-side preconditions (which tags each frame holds, the slots
they fill, the reference against truth and against numpy, the wrong builds' forms) are asserted in tests/test_rigid_bundles_cpu.py."""
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
import rigid_bundle_cases as rc  # noqa: E402
import rigid_bundle_ref as rr  # noqa: E402

FAMS = rc.FAMS
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
    """One submission in the mode's way; (records per frame, rigid bundle records per frame)."""
    prep = det.prepare(frames, max_dets=max_dets, intrinsics=intrinsics)
    graph = mode.endswith("graph")
    for _ in range(2 if graph else 1):   # (graph: captured by the first submission, replayed by the second)
        det.submit_prepared(prep)
        det.wait_prepared(prep)
    assert det.last_submission_path() == mode.split("-")[0]
    assert (det.last_graph_nodes() > 0) == graph, (mode, det.last_graph_nodes())
    return det.unpack(prep), det.bundle_poses_ex(prep["n"])


def _check(label, got, want):
    errs = rr.compare(got, want, label + ": ")
    print("%s: status %d ntags %d nskipped %d seed %d chosen %d err %.3e sq_err_sum %.4f %s"
          % (label, got["status"], got["ntags"], got["nskipped"], got["seed"], got["chosen"], got["err"], got["sq_err_sum"], errs))
    return errs


# ---- 1, 2, 3. the cube corner, one face of it, and the board with quarter turns, on one 640 x 480 handle -----------------------------------
def _rigs(mode):
    """The three-frame cube submission (cube corner, one face and the lone tag, cube corner again; two bundles) and the one-frame
    quarter-turn submission in `mode`: frame name -> (records, rigid bundle records)."""
    if ("rigs", mode) not in _cache:
        det = _handle(mode, rc.W1, rc.H1, max_batch=3, tag_size=bc.SIZE1, bundles_ex=rc.CUBE_BUNDLES)
        det.set_frame_skews(bc.SKEW1)
        frames = torch.from_numpy(np.stack([rc.cube_frame(n) for n in rc.CUBE_FRAMES])).cuda()
        recs, poses = _submit(det, mode, frames, 64, list(bc.INTR1))
        out = {n: (recs[i], poses[i]) for i, n in enumerate(rc.CUBE_FRAMES)}
        det.set_bundles_ex([rc.TURNED])   # (a change of layout: the same graph)
        recs, poses = _submit(det, mode, torch.from_numpy(rc.turned_frame()).cuda(), 64, [bc.INTR1[0]])
        out["turned"] = (recs[0], poses[0])
        assert det.late_waits() == 0
        det.close()
        _cache[("rigs", mode)] = out
    return _cache[("rigs", mode)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ("cube_a", "cube_b"))
def test_cube_corner(built, name, mode):
    """640 x 480, three mutually orthogonal faces of 2 x 2 tags seen along the cube's diagonal, 12 members, in a three-frame submission
    with distinct per-frame intrinsics: all twelve tags used, one minimum (both chains end in it).  The second bundle of the handle,
    the lone tag, is not in view: too few tags, zeros."""
    recs, got = _rigs(mode)[name]
    assert not pu.compare_detections(recs, rc.cube_records(name), exact=True)   # the input of the reference is the input of the kernel
    want = rc.cube_solved(name)
    errs = _check("%s %s cube" % (name, mode), got[0], want[0]) + _check("%s %s lone" % (name, mode), got[1], want[1])
    assert not errs, errs
    assert got[0]["status"] == capi.BUNDLE_SOLVED and got[0]["ntags"] == 12 and pr.rot_angle_deg(got[0]["R"], got[0]["R_alt"]) < 1e-3
    assert got[1]["status"] == capi.BUNDLE_TOO_FEW_TAGS and not got[1]["R"].any() and not got[1]["t"].any() and got[1]["err"] == 0.0


@pytest.mark.parametrize("mode", MODES)
def test_coplanar_and_one_tag(built, mode):
    """The middle frame of the cube submission (a skew on its slot): one face in view, 4 used of 12 members -- a coplanar set, M of rank
    2, two distinct minima -- and the one-member bundle whose single used tag is all there is."""
    recs, got = _rigs(mode)["one_face"]
    assert not pu.compare_detections(recs, rc.cube_records("one_face"), exact=True)
    want = rc.cube_solved("one_face")
    errs = _check("one_face %s cube" % mode, got[0], want[0]) + _check("one_face %s lone" % mode, got[1], want[1])
    assert not errs, errs
    assert got[0]["status"] == capi.BUNDLE_SOLVED and got[0]["ntags"] == 4 and pr.rot_angle_deg(got[0]["R"], got[0]["R_alt"]) > 20.0
    assert got[1]["status"] == capi.BUNDLE_SOLVED and got[1]["ntags"] == 1


@pytest.mark.parametrize("mode", MODES)
def test_quarter_turns(built, mode):
    """bundle_cases' 3 x 2 board with member i turned by i quarter turns in the plane, which amdAprilTagsSetBundles cannot describe."""
    recs, got = _rigs(mode)["turned"]
    assert not pu.compare_detections(recs, rc.turned_records(), exact=True)
    errs = _check("turned %s" % mode, got[0], rc.turned_solved())
    assert not errs, errs
    assert len(got) == 1 and got[0]["status"] == capi.BUNDLE_SOLVED and got[0]["ntags"] == 6


# ---- 4. content frames ----------------------------------------------------------------------------------------------------------------------
def _content(mode):
    """The two three-frame submissions of bundle_cases' content frames in `mode`: content case -> (records, rigid bundle record)."""
    if ("content", mode) not in _cache:
        det = _handle(mode, bc.W1, bc.H1, max_batch=3, tag_size=bc.SIZE1, bundles_ex=[rc.BUNDLE1])
        det.set_frame_skews(bc.SKEW1)
        out = {}
        for sub in (0, 1):
            names = [n for n in bc.CONTENT if bc.SLOTS[n][0] == sub]
            names.sort(key=lambda n: bc.SLOTS[n][1])
            frames = torch.from_numpy(np.stack([bc.content_frame(n) for n in names])).cuda()
            recs, poses = _submit(det, mode, frames, 64, list(bc.INTR1))
            for slot, n in enumerate(names):
                out[n] = (recs[slot], poses[slot][0])
        assert det.late_waits() == 0
        det.close()
        _cache[("content", mode)] = out
    return _cache[("content", mode)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", bc.CONTENT)
def test_content(built, name, mode):
    """bundle_cases' content frames with BUNDLE1 restated with identity member rotations: all six tags; one painted over; a non-member
    tag in view; a second copy of member 1 (the duplicate rule skips both); tag 2 with a wrong bit (hamming 1: refused); no tags (too
    few tags, zeros)."""
    recs, got = _content(mode)[name]
    assert not pu.compare_detections(recs, bc.content_records(name), exact=True)
    errs = _check("%s %s" % (name, mode), got, rc.content_solved(name))
    assert not errs, errs
    if name == "no_tags":
        assert got["status"] == capi.BUNDLE_TOO_FEW_TAGS and not got["R"].any() and not got["t"].any() and got["sq_err_sum"] == 0.0
    else:
        assert got["status"] == capi.BUNDLE_SOLVED and got["ntags"] >= 4


# ---- 5, 6. every lane of the wave, and used records in both chunks ------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_full_wave_and_across_chunks(built, mode):
    """640 x 576, 72 records.  Members 0 .. 63: 64 used tags, one on every lane, and 8 records of no member.  Then 12 members from both
    ends of the id range: the used records fall into both 64-record chunks; with max_dets = 8 the hand-out ends at eight records and
    the solve still reads all 72."""
    det = _handle(mode, bc.W2, bc.H2, tag_size=bc.SIZE2, intrinsics=bc.INTR2, bundles_ex=[rc.FULL_WAVE])
    frame = torch.from_numpy(bc.frame72()).cuda()
    recs, poses = _submit(det, mode, frame, 128, None)
    assert not pu.compare_detections(recs[0], bc.records72(), exact=True)
    errs = _check("wave %s" % mode, poses[0][0], rc.solved72("wave"))
    assert poses[0][0]["ntags"] == 64
    det.set_bundles_ex([rc.BOTH_ENDS])
    for max_dets in (128, 8):
        recs, poses = _submit(det, mode, frame, max_dets, None)
        assert len(recs[0]) == min(max_dets, 72) and not pu.compare_detections(recs[0], bc.records72()[:max_dets], exact=True)
        errs += _check("ends %s max_dets %d" % (mode, max_dets), poses[0][0], rc.solved72("ends"))
    assert det.late_waits() == 0
    det.close()
    assert not errs, errs


# ---- 7. several bundles in one frame --------------------------------------------------------------------------------------------------------
def test_two_bundles(built):
    """The all_six frame with the board's rows as two rigid bundles."""
    det = AprilTagDetector(bc.W1, bc.H1, tag_size=bc.SIZE1, intrinsics=bc.INTR1[0], bundles_ex=rc.TWO)
    recs = det.detect_batch_ex(torch.from_numpy(bc.content_frame("all_six")).cuda(), max_dets=64)[0]
    poses = det.bundle_poses_ex(1)[0]
    det.close()
    want_recs = bc.oracle_records(bc.content_frame("all_six"), bc.INTR1[0])
    assert not pu.compare_detections(recs, want_recs, exact=True)
    errs = []
    for i, b in enumerate(rc.TWO):
        errs += _check("two %d" % i, poses[i], rr.solve(want_recs, b, FAMS, bc.INTR1[0], 0.0, bundle_index=i))
    assert not errs, errs
    assert [(p["status"], p["ntags"], p["nskipped"]) for p in poses] == [(0, 3, 0), (0, 3, 0)]


# ---- 8, 9. retirement; off means off; the contract ------------------------------------------------------------------------------------------
def test_off_means_off_retirement_and_the_contract(built):
    frame = torch.from_numpy(bc.content_frame("all_six")).cuda()
    det = AprilTagDetector(bc.W1, bc.H1, tag_size=bc.SIZE1, intrinsics=bc.INTR1[0], max_batch=2)
    never = AprilTagDetector(bc.W1, bc.H1, tag_size=bc.SIZE1, intrinsics=bc.INTR1[0], max_batch=2)
    L, h = capi.lib(), det._h
    want_recs = bc.oracle_records(bc.content_frame("all_six"), bc.INTR1[0])
    want = rr.solve(want_recs, rc.BUNDLE1, FAMS, bc.INTR1[0])

    def run(d=det):
        prep = d.prepare(frame, max_dets=64)
        d.run_prepared(prep)
        return bytes(prep["out"]), int(prep["cnt"][0])

    def solved():
        return not rr.compare(det.bundle_poses_ex(1)[0][0], want)

    # off is the default: no records to hand out, turning it off again changes nothing, no memory, the same launches
    bytes0 = det.device_bytes()
    assert never.device_bytes() == bytes0
    off_out, off_cnt = run()
    run()
    nodes_off = det.last_graph_nodes()
    assert nodes_off > 0 and off_cnt == 6
    assert _code(lambda: det.bundle_poses_ex(1)) == INVALID_ARGUMENT
    det.set_bundles_ex(None)
    assert det.device_bytes() == bytes0 and det.graph_replay() == (True, 1, 0)
    # on: the tag records are the same bytes, exactly one launch more in the graph, the layout's memory
    det.set_bundles_ex([rc.BUNDLE1])
    assert det.graph_replay() == (True, 0, 1)   # the graph captured without the launch is retired
    assert det.device_bytes() > bytes0
    bytes_on = det.device_bytes()
    assert run() == (off_out, off_cnt) and det.last_graph_nodes() == nodes_off + 1 and solved()
    assert run() == (off_out, off_cnt) and det.last_graph_nodes() == nodes_off + 1 and solved()
    assert _code(lambda: det.bundle_poses_ex(2)) == INVALID_ARGUMENT   # beyond the last submission's frames
    assert _code(lambda: det.bundle_poses(1)) == INVALID_ARGUMENT      # the planar kind did not run
    # refused calls leave the previous setting in force; nothing is retired
    state = det.graph_replay()
    ok = {"name": "ok", "iterations": 50, "members": [(0, 4, rc.I3, (1.0, 1.0, 0.0), 0.1)]}
    for bad in ([dict(ok, members=[(0, 4, np.diag([1.0, 1.0, -1.0]), (0, 0, 0), 0.1)])], [dict(ok, members=[(0, 4, 1.001 * rc.I3, (0, 0, 0), 0.1)])],
                [dict(ok, iterations=0)], [dict(ok, iterations=201)], [dict(ok, members=[(0, i, rc.I3, (0, 0, 0), 0.1) for i in range(65)])],
                [dict(ok, members=[(0, 4, rc.I3, (float("inf"), 0, 0), 0.1)])], [ok, ok], [dict(ok, min_tags=0)]):
        assert _code(lambda: det.set_bundles_ex(bad)) == INVALID_ARGUMENT
        assert run() == (off_out, off_cnt) and solved()
    assert L.amdAprilTagsSetBundlesEx(h, 1, None) == INVALID_ARGUMENT and L.amdAprilTagsGetBundlePosesEx(h, None, 1) == INVALID_ARGUMENT
    assert det.graph_replay() == state and det.device_bytes() == bytes_on
    # between Submit and Wait the setter and the getter are refused
    prep = det.prepare(frame, max_dets=64)
    det.submit_prepared(prep)
    assert _code(lambda: det.set_bundles_ex(None)) == INVALID_ARGUMENT
    assert _code(lambda: det.set_bundles_ex([ok])) == INVALID_ARGUMENT
    assert _code(lambda: det.bundle_poses_ex(1)) == INVALID_ARGUMENT
    det.wait_prepared(prep)
    assert solved() and det.graph_replay() == state
    # a change of layout, iteration count and gates replays the same graph and solves the new setting
    two = [dict(rc.TWO[0], min_tags=4, iterations=7), dict(rc.TWO[1], iterations=3)]
    det.set_bundles_ex(two)
    assert det.graph_replay() == state and det.device_bytes() == bytes_on
    assert run() == (off_out, off_cnt) and det.last_graph_nodes() == nodes_off + 1 and det.graph_replay() == state
    got = det.bundle_poses_ex(1)[0]
    assert len(got) == 2 and got[0]["status"] == capi.BUNDLE_TOO_FEW_TAGS and got[0]["ntags"] == 3
    for i, b in enumerate(two):
        assert not rr.compare(got[i], rr.solve(want_recs, b, FAMS, bc.INTR1[0], bundle_index=i))
    assert rr.compare(got[1], rr.solve(want_recs, rc.TWO[1], FAMS, bc.INTR1[0], bundle_index=1))   # (three steps are not fifty)
    # rigid -> planar retires, and the planar kind holds; planar -> rigid retires again
    capturing, live, retired = det.graph_replay()
    det.set_bundles([bc.BUNDLE1])
    assert det.graph_replay() == (True, 0, retired + live)
    assert run() == (off_out, off_cnt) and run() == (off_out, off_cnt) and det.last_graph_nodes() == nodes_off + 1
    assert not br.compare(det.bundle_poses(1)[0][0], br.solve(want_recs, bc.BUNDLE1, FAMS, bc.INTR1[0]))
    assert _code(lambda: det.bundle_poses_ex(1)) == INVALID_ARGUMENT
    capturing, live, retired = det.graph_replay()
    det.set_bundles_ex([rc.BUNDLE1])
    assert det.graph_replay() == (True, 0, retired + live)
    assert run() == (off_out, off_cnt) and run() == (off_out, off_cnt) and det.last_graph_nodes() == nodes_off + 1 and solved()
    assert _code(lambda: det.bundle_poses(1)) == INVALID_ARGUMENT
    # together with the pose refinement in one submission: both record sets exact, two launches more than off
    det.set_pose_refinement(pc.ITERATIONS)
    assert run() == (off_out, off_cnt) and run() == (off_out, off_cnt) and det.last_graph_nodes() == nodes_off + 2 and solved()
    assert not pr.compare_frames(det.refined_poses(1)[0], pc.refined("all_six-0", want_recs, bc.INTR1[0], 0.0, bc.SIZE1))
    det.set_pose_refinement(0)
    # ThresholdOnly never solves: afterwards there is nothing to hand out
    det.threshold_only(frame)
    assert _code(lambda: det.bundle_poses_ex(1)) == INVALID_ARGUMENT
    assert run() == (off_out, off_cnt) and solved()
    # off again: the graphs with the launch are retired, and the handle is one that never had the setting
    capturing, live, retired = det.graph_replay()
    det.set_bundles_ex(None)
    assert det.graph_replay() == (True, 0, retired + live)
    assert run() == (off_out, off_cnt)
    assert run() == (off_out, off_cnt) and det.last_graph_nodes() == nodes_off
    assert _code(lambda: det.bundle_poses_ex(1)) == INVALID_ARGUMENT
    assert run(never) == (off_out, off_cnt) and never.device_bytes() == bytes0
    assert det.late_waits() == 0
    det.close()
    never.close()


# ---- 10. the node shell ---------------------------------------------------------------------------------------------------------------------
def _quat_of(R):
    """(qw, qx, qy, qz) of a rotation matrix whose trace is not near -1 (the members' are axis permutations with signs)."""
    R = np.asarray(R, dtype=np.float64)
    cands = [(1 + R[0, 0] + R[1, 1] + R[2, 2], lambda: (1 + R[0, 0] + R[1, 1] + R[2, 2], R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1])),
             (1 + R[0, 0] - R[1, 1] - R[2, 2], lambda: (R[2, 1] - R[1, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], R[0, 1] + R[1, 0], R[0, 2] + R[2, 0])),
             (1 - R[0, 0] + R[1, 1] - R[2, 2], lambda: (R[0, 2] - R[2, 0], R[0, 1] + R[1, 0], 1 - R[0, 0] + R[1, 1] - R[2, 2], R[1, 2] + R[2, 1])),
             (1 - R[0, 0] - R[1, 1] + R[2, 2], lambda: (R[1, 0] - R[0, 1], R[0, 2] + R[2, 0], R[1, 2] + R[2, 1], 1 - R[0, 0] - R[1, 1] + R[2, 2]))]
    q = np.array(max(cands, key=lambda c: c[0])[1]())
    return tuple(float(v) for v in q / np.linalg.norm(q))


def _quat_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_node_shell(built):
    """AprilTagNode and a two-stream AprilTagMultiCameraNode with the cube (members by id, position, quaternion and size) and the lone
    tag, which is not in view, on the cube-corner frame: one "bundle:cube" transform behind the tags', under the camera info's header,
    from the chosen pose -- the translation as it stands, the rotation through the float quaternion a tag's takes -- and none for
    the lone tag.  The members' rotations are axis permutations with signs, which their quaternions give back exactly, so the
    records equal the reference's bit for bit."""
    from isaac_ros_apriltag_amd import build as b
    from isaac_ros_apriltag_amd import node
    b.build_node()
    shell = [dict(bundle, members=[(m[1], tuple(m[3]), _quat_of(m[2]), m[4]) for m in bundle["members"]]) for bundle in rc.CUBE_BUNDLES]
    for bundle in rc.CUBE_BUNDLES:   # (the quaternions give the members' rotations back as they are)
        assert all(np.array_equal(_quat_matrix(_quat_of(m[2])[1:] + _quat_of(m[2])[:1]), np.asarray(m[2])) for m in bundle["members"])
    k9 = [600.0, 0.0, 320.0, 0.0, 600.0, 240.0, 0.0, 0.0, 1.0]
    frame = rc.cube_frame("cube_a")
    recs = rc.cube_records("cube_a")
    want = rc.cube_solved("cube_a")   # (slot 0: bc.INTR1[0] is k9, no skew)

    def check(tfs, poses, stamp):
        assert [t["child_frame_id"] for t in tfs] == ["tag36h11:%d" % r["id"] for r in recs] + ["bundle:cube"]
        tf = tfs[-1]
        assert tf["frame_id"] == "cam" and tf["stamp"] == stamp
        assert [p["name"] for p in poses] == ["cube", "lone"] and poses[1]["status"] == capi.BUNDLE_TOO_FEW_TAGS and poses[1]["ntags"] == 0
        for i, p in enumerate(poses):
            rec = dict(p, bundle=i, R=np.array(p["R"]).reshape(3, 3), t=np.array(p["t"]), R_alt=np.array(p["R_alt"]).reshape(3, 3), t_alt=np.array(p["t_alt"]))
            assert not rr.compare(rec, want[i])
        assert poses[0]["ntags"] == 12 and tf["translation"] == poses[0]["t"]
        assert np.abs(_quat_matrix(tf["rotation_xyzw"]) - np.array(poses[0]["R"]).reshape(3, 3)).max() < 1e-6   # (float quaternion)

    nodes = []
    try:
        n = node.AprilTagNode(size=bc.SIZE1, rigid_bundles=shell)
        nodes.append(n)
        dets, _ = n.on_frame(frame.ctypes.data, False, "mono8", rc.W1, rc.H1, rc.W1, k9, "cam", (3, 0))
        assert len(dets) == 12 and n.bundle_poses() == []
        check(n.transforms(), n.rigid_bundle_poses(), (3, 0))
        multi = node.AprilTagMultiCameraNode(2, size=bc.SIZE1, rigid_bundles=shell)
        nodes.append(multi)
        for s in (0, 1):
            assert multi.on_frame(s, frame.ctypes.data, False, "mono8", rc.W1, rc.H1, rc.W1, k9, "cam", (4, s))
        for s in (0, 1):
            assert multi.publishes(s) == 1
            check(multi.transforms(s), multi.rigid_bundle_poses(s), (4, s))
        with pytest.raises(ValueError):
            node.AprilTagNode(size=bc.SIZE1, rigid_bundles=shell, bundles=[{"name": "b", "members": [(0, 0.0, 0.0, 0.1)]}])
    finally:
        [x.close() for x in nodes]


# ---- 11. the suite bites ----------------------------------------------------------------------------------------------------------------------
_SELECT = "(test_content or test_cube_corner or test_coplanar_and_one_tag or test_quarter_turns) and throughput"
_CONTENT = tuple("test_content[%s-throughput-plain]" % n for n in bc.CONTENT)
_RIGS = ("test_cube_corner[cube_a-throughput-plain]", "test_cube_corner[cube_b-throughput-plain]", "test_coplanar_and_one_tag[throughput-plain]",
         "test_quarter_turns[throughput-plain]")
_WRONG_BUILDS = {
    # the object points without the member's rotation: the cube, its one face and the turned board; identity rotations do not see it
    19: {"must_fail": _RIGS, "must_pass": _CONTENT},
    # the means divided by 4: every bundle with two or more used tags (the one-tag bundle shares its test with the four-tag face)
    20: {"must_fail": _RIGS + tuple(c for c in _CONTENT if "no_tags" not in c), "must_pass": ("test_content[no_tags-throughput-plain]",)},
}


@pytest.mark.parametrize("mutant", sorted(_WRONG_BUILDS))
def test_the_rigid_bundle_tests_fail_on_the_wrong_builds(built, mutant):
    """libapriltag_amd_mut19.so and _mut20.so (csrc/tools_hooks.h, AMDAT_MUTATE): the rig and content cases on the throughput set, in a
    process of their own, must FAIL on the wrong build exactly where its error lives, and all of them pass on the product library.
    Both wrong builds change values only.  Under mut20 the one-tag bundle itself still equals the reference: the lines printed for
    "one_face ... lone" carry no mismatch."""
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
    assert "differ" in out.stdout   # what differs: fields of the rigid bundle record
    lone = [l for l in out.stdout.splitlines() if l.startswith("one_face throughput-plain lone:")]
    assert lone and all(l.rstrip().endswith("[]") for l in lone)   # the one-tag bundle passes on both wrong builds
    if "ok" not in _cache:   # (the product run is the same for both wrong builds)
        _cache["ok"] = run(None)
    out_ok, passed_ok, failed_ok = _cache["ok"]
    assert out_ok.returncode == 0 and not failed_ok and sorted(passed_ok) == sorted(passed + failed), (out_ok.stdout[-1500:], failed_ok)
