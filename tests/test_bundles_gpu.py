"""Board pose inside the submission (amdAprilTagsSetBundles, k_bundle_pose).  The definition under test is DESIGN.md section 7d, stated
in Python by tests/bundle_ref.py: fed the oracle's records of a frame -- which the library's own records equal bit for bit -- the
reference gives the bundle record the library must hand out, R, t and sq_err_sum compared with numpy.array_equal, status, ntags and
nskipped with ==.  The oracle-side preconditions (which tags each content frame holds, the duplicate pair, the hamming-1 record, 72
records on the large board, the reference against truth and against lstsq) are asserted in tests/test_bundles_cpu.py."""
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
import bundle_ref as br  # noqa: E402
import parity_util as pu  # noqa: E402
import rectify_cases as rc  # noqa: E402
import resize_cases as zc  # noqa: E402

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
    """One submission in the mode's way; (records per frame, bundle records per frame)."""
    prep = det.prepare(frames, max_dets=max_dets, intrinsics=intrinsics)
    graph = mode.endswith("graph")
    for _ in range(2 if graph else 1):   # (graph: captured by the first submission, replayed by the second)
        det.submit_prepared(prep)
        det.wait_prepared(prep)
    assert det.last_submission_path() == mode.split("-")[0]
    assert (det.last_graph_nodes() > 0) == graph, (mode, det.last_graph_nodes())
    return det.unpack(prep), det.bundle_poses(prep["n"])


# ---- 1. content cases ---------------------------------------------------------------------------------------------------------------------
def _content(mode):
    """The two three-frame submissions of the content cases in `mode`: content case -> (records, bundle record)."""
    if ("content", mode) not in _cache:
        det = _handle(mode, bc.W1, bc.H1, max_batch=3, tag_size=bc.SIZE1, bundles=[bc.BUNDLE1])
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
    """640 x 480, a 3 x 2 board of tag36h11 at 64 px sides, max_hamming = 0, in two three-frame submissions with distinct per-frame
    intrinsics and a skew on the middle slot: all six tags; one painted over; a non-member tag in view; a second copy of member 1
    elsewhere (the duplicate rule skips both); tag 2 with a wrong bit (hamming 1: refused); no tags (too few tags, zeros)."""
    recs, got = _content(mode)[name]
    slot = bc.SLOTS[name][1]
    want_recs = bc.content_records(name)
    assert not pu.compare_detections(recs, want_recs, exact=True)   # the input of the reference is the input of the kernel
    want = br.solve(want_recs, bc.BUNDLE1, FAMS, bc.INTR1[slot], bc.SKEW1[slot])
    errs = br.compare(got, want)
    print("%s %s: status %d ntags %d nskipped %d rms %.4f px %s" % (name, mode, got["status"], got["ntags"], got["nskipped"], br.rms(got), errs))
    assert not errs, errs
    if name == "no_tags":
        assert got["status"] == capi.BUNDLE_TOO_FEW_TAGS and not got["R"].any() and not got["t"].any() and got["sq_err_sum"] == 0.0
    else:
        assert got["status"] == capi.BUNDLE_SOLVED and got["ntags"] >= 5


# ---- 2. more kept records than lanes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_board72(built, mode):
    """640 x 576, a 9 x 8 board, 72 tags at 48 px sides: two chunks of records.  With max_dets = 8 the hand-out ends at eight records and
    the bundle still sees all 72."""
    det = _handle(mode, bc.W2, bc.H2, tag_size=bc.SIZE2, intrinsics=bc.INTR2, bundles=[bc.BUNDLE2])
    frame = torch.from_numpy(bc.frame72()).cuda()
    want = br.solve(bc.records72(), bc.BUNDLE2, FAMS, bc.INTR2)
    assert want["status"] == br.SOLVED and want["ntags"] == 72
    errs = []
    for max_dets in (128, 8):
        recs, poses = _submit(det, mode, frame, max_dets, None)
        assert len(recs[0]) == min(max_dets, 72)
        assert not pu.compare_detections(recs[0], bc.records72()[:max_dets], exact=True)
        errs += ["max_dets %d: %s" % (max_dets, e) for e in br.compare(poses[0][0], want)]
    det.close()
    print("board72 %s: %s" % (mode, errs))
    assert not errs, errs


# ---- 3. several bundles in one frame ------------------------------------------------------------------------------------------------------
def test_two_bundles_and_a_lone_tag(built):
    """The non_member frame with the board's rows as two bundles and the lone tag as a one-tag bundle.  The one-tag bundle's pose is the
    tag's own up to the arithmetic: both come from the same four corners, through the normal equations here and through the 8 x 8
    system there, and through one pose routine whose three float square roots may each round the other way -- R within 1e-9 (the
    polar factor does not see the scale; the homographies agree to cond(M) 2^-53, about 1e-13), t within 2 * 2^-23 |t|."""
    det = AprilTagDetector(bc.W1, bc.H1, tag_size=bc.SIZE1, intrinsics=bc.INTR1[2], bundles=bc.BUNDLES3)
    frame = torch.from_numpy(bc.content_frame("non_member")).cuda()
    recs = det.detect_batch_ex(frame, max_dets=64)[0]
    poses = det.bundle_poses(1)[0]
    det.close()
    want_recs = bc.oracle_records(bc.content_frame("non_member"), bc.INTR1[2])
    assert not pu.compare_detections(recs, want_recs, exact=True)
    errs = []
    for i, b in enumerate(bc.BUNDLES3):
        errs += br.compare(poses[i], br.solve(want_recs, b, FAMS, bc.INTR1[2], 0.0, bundle_index=i))
    print("bundles3: %s" % errs)
    assert not errs, errs
    assert [(p["status"], p["ntags"], p["nskipped"]) for p in poses] == [(0, 3, 0), (0, 3, 0), (0, 1, 0)]
    lone = [r for r in recs if r["id"] == bc.LONE_ID][0]
    dr, dt = float(np.abs(poses[2]["R"] - lone["R"]).max()), float(np.abs(poses[2]["t"] - lone["t"]).max())
    print("one-tag bundle against the tag's own pose: R %.3g, t %.3g" % (dr, dt))
    assert dr <= 1e-9 and dt <= 2 * 2.0 ** -23 * float(np.abs(lone["t"]).max())


# ---- 5. composition -----------------------------------------------------------------------------------------------------------------------
def test_composes_with_a_window(built):
    """Per-frame sizes: a 360 x 260 window at (150, 150) of the all_six frame, at the full image's pitch, its principal point moved with
    it -- the bundle record of the oracle's records on the cropped array."""
    x0, y0, w, h = 150, 150, 360, 260
    intr = (600.0, 600.0, 320.0 - x0, 240.0 - y0)
    want_recs = bc.oracle_records(np.ascontiguousarray(bc.content_frame("all_six")[y0:y0 + h, x0:x0 + w]), intr)
    assert len(want_recs) == 6
    full = torch.from_numpy(bc.content_frame("all_six")).cuda()
    det = AprilTagDetector(bc.W1, bc.H1, tag_size=bc.SIZE1, per_frame_sizes=True, bundles=[bc.BUNDLE1])
    recs = det.detect_batch_ex([(full.data_ptr() + y0 * bc.W1 + x0, bc.W1, w, h)], max_dets=64, intrinsics=[intr])[0]
    got = det.bundle_poses(1)[0][0]
    det.close()
    assert not pu.compare_detections(recs, want_recs, exact=True)
    errs = br.compare(got, br.solve(want_recs, bc.BUNDLE1, FAMS, intr))
    assert not errs and got["ntags"] == 6, errs


def test_composes_with_rectification(built):
    """scene_c2 rectified with Da, Knew_a inside the submission: the records tests/test_rectify_submission_gpu.py pins, and the bundle
    record of a 5 x 2 layout over its ten ids, with Knew's intrinsics."""
    K, D, Kn = rc.model_a()
    want_recs = rc.oracle_detections("a")
    det = AprilTagDetector(1920, 1080, rectification=[(K, D, Kn)], bundles=[bc.BUNDLE_C2])
    recs = det.detect_batch_ex(torch.from_numpy(rc.scene()[0]).cuda(), max_dets=64, intrinsics=[rc.k4(Kn)])[0]
    got = det.bundle_poses(1)[0][0]
    det.close()
    assert len(want_recs) == 10 and not pu.compare_detections(recs, want_recs, exact=True)
    errs = br.compare(got, br.solve(want_recs, bc.BUNDLE_C2, FAMS, rc.k4(Kn)))
    assert not errs and got["ntags"] == 10 and got["status"] == capi.BUNDLE_SOLVED, errs


def test_composes_with_resize(built):
    """scene_c2 resized to 1280 x 720 inside the submission: the records tests/test_resize_submission_gpu.py pins, the scaled camera."""
    Ks = rc.k4(zc.scaled_k(rc.scene()[1], 1920, 1080, 1280, 720))
    want_recs = zc.oracle_detections(1280, 720)
    det = AprilTagDetector(1280, 720, resize=[(1280, 720)], bundles=[bc.BUNDLE_C2])
    recs = det.detect_batch_ex(torch.from_numpy(rc.scene()[0]).cuda(), max_dets=64, intrinsics=[Ks])[0]
    got = det.bundle_poses(1)[0][0]
    det.close()
    assert len(want_recs) == 10 and not pu.compare_detections(recs, want_recs, exact=True)
    errs = br.compare(got, br.solve(want_recs, bc.BUNDLE_C2, FAMS, Ks))
    assert not errs and got["ntags"] == 10 and got["status"] == capi.BUNDLE_SOLVED, errs


# ---- 6. off means off; the setter's contract ----------------------------------------------------------------------------------------------
def test_off_means_off_and_the_setter_contract(built):
    frame = torch.from_numpy(bc.content_frame("all_six")).cuda()
    empty = torch.from_numpy(bc.content_frame("no_tags")).cuda()
    det = AprilTagDetector(bc.W1, bc.H1, tag_size=bc.SIZE1, intrinsics=bc.INTR1[0], max_batch=2)
    never = AprilTagDetector(bc.W1, bc.H1, tag_size=bc.SIZE1, intrinsics=bc.INTR1[0], max_batch=2)
    L, h = capi.lib(), det._h
    want = br.solve(bc.oracle_records(bc.content_frame("all_six"), bc.INTR1[0]), bc.BUNDLE1, FAMS, bc.INTR1[0])

    def run(d=det, f=frame):
        prep = d.prepare(f, max_dets=64)
        d.run_prepared(prep)
        return bytes(prep["out"]), int(prep["cnt"][0])

    # off is the default: no records to hand out, turning it off again changes nothing, no memory, the same launches
    bytes0 = det.device_bytes()
    assert never.device_bytes() == bytes0
    off_out, off_cnt = run()
    run()
    nodes_off = det.last_graph_nodes()
    assert nodes_off > 0 and off_cnt == 6
    assert _code(lambda: det.bundle_poses(1)) == INVALID_ARGUMENT
    det.set_bundles(None)
    assert det.device_bytes() == bytes0 and det.graph_replay() == (True, 1, 0)
    # on: the tag records are the same bytes, one launch more in the graph, the layout's memory
    det.set_bundles([bc.BUNDLE1])
    assert det.graph_replay() == (True, 0, 1)   # the graph captured without the launch is retired
    table = sum(len(capi.family_info(f)["codes"]) for f in FAMS)
    assert det.device_bytes() - bytes0 >= 1024 * 32 + 2 * table
    bytes_on = det.device_bytes()
    on_out, on_cnt = run()
    assert det.last_graph_nodes() == nodes_off + 1   # (captured by this submission, and replayed at once)
    assert (on_out, on_cnt) == (off_out, off_cnt)
    assert not br.compare(det.bundle_poses(1)[0][0], want)
    assert run() == (off_out, off_cnt) and det.last_graph_nodes() == nodes_off + 1
    assert not br.compare(det.bundle_poses(1)[0][0], want)
    assert _code(lambda: det.bundle_poses(2)) == INVALID_ARGUMENT   # beyond the last submission's frames
    # refused calls leave the previous setting in force; nothing is retired
    state = det.graph_replay()
    ok = {"name": "ok", "members": [(0, 4, 1.0, 1.0, 0.1)]}
    for bad in ([dict(ok, members=[(1, 4, 0, 0, 0.1)])], [dict(ok, members=[(0, 587, 0, 0, 0.1)])], [dict(ok, members=[(0, 4, 0, 0, 0.0)])],
                [dict(ok, members=[(0, 4, float("nan"), 0, 0.1)])], [dict(ok, min_tags=0)], [ok, ok], [ok] * 9,
                [dict(ok, members=[(0, i % 587, 0.0, 0.0, 0.1) for i in range(1025)])]):
        assert _code(lambda: det.set_bundles(bad)) == INVALID_ARGUMENT
        assert run() == (off_out, off_cnt) and not br.compare(det.bundle_poses(1)[0][0], want)
    assert L.amdAprilTagsSetBundles(h, 1, None) == INVALID_ARGUMENT and L.amdAprilTagsSetBundles(None, 0, None) == INVALID_ARGUMENT
    assert L.amdAprilTagsGetBundlePoses(h, None, 1) == INVALID_ARGUMENT
    assert det.graph_replay() == state and det.device_bytes() == bytes_on
    # between Submit and Wait both calls are refused
    prep = det.prepare(frame, max_dets=64)
    det.submit_prepared(prep)
    assert _code(lambda: det.set_bundles(None)) == INVALID_ARGUMENT
    assert _code(lambda: det.set_bundles([ok])) == INVALID_ARGUMENT
    assert _code(lambda: det.bundle_poses(1)) == INVALID_ARGUMENT
    det.wait_prepared(prep)
    assert not br.compare(det.bundle_poses(1)[0][0], want)
    # changing only the layout retires no graph, and the replayed graph solves the new one -- more bundles, other gates
    two = [dict(bc.BUNDLES3[0], min_tags=4), bc.BUNDLES3[1]]
    det.set_bundles(two)
    assert det.graph_replay() == state and det.device_bytes() == bytes_on
    assert run() == (off_out, off_cnt) and det.last_graph_nodes() == nodes_off + 1
    recs = bc.oracle_records(bc.content_frame("all_six"), bc.INTR1[0])
    got = det.bundle_poses(1)[0]
    assert len(got) == 2 and got[0]["status"] == capi.BUNDLE_TOO_FEW_TAGS and got[0]["ntags"] == 3
    for i, b in enumerate(two):
        assert not br.compare(got[i], br.solve(recs, b, FAMS, bc.INTR1[0], bundle_index=i))
    # a two-frame submission: frame-major records, the empty frame with zeros
    det.set_bundles([bc.BUNDLE1])
    prep = det.prepare(torch.stack([empty, frame]), max_dets=64)
    det.run_prepared(prep)
    got = det.bundle_poses(2)
    assert got[0][0]["status"] == capi.BUNDLE_TOO_FEW_TAGS and not got[0][0]["R"].any() and not br.compare(got[1][0], want)
    # off again: the graphs with the launch are retired, and the handle is one that never had the setting
    capturing, live, retired = det.graph_replay()
    det.set_bundles(None)
    assert det.graph_replay() == (True, 0, retired + live)
    assert run() == (off_out, off_cnt)
    assert run() == (off_out, off_cnt) and det.last_graph_nodes() == nodes_off
    assert _code(lambda: det.bundle_poses(1)) == INVALID_ARGUMENT
    assert run(never) == (off_out, off_cnt) and never.device_bytes() == bytes0
    assert det.late_waits() == 0
    det.close()
    never.close()


# ---- 7. the node shell --------------------------------------------------------------------------------------------------------------------
def _quat_matrix(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def test_node_shell(built):
    """AprilTagNode and a two-stream AprilTagMultiCameraNode with the board and a bundle that cannot be solved (a tag that is not in
    view): one "bundle:<name>" transform behind the tags' for the solved bundle, under the camera info's header, equal to the record --
    the translation as it stands, the rotation through the float quaternion a tag's takes -- and none for the other; the records equal
    the reference's."""
    from isaac_ros_apriltag_amd import build as b
    from isaac_ros_apriltag_amd import node
    b.build_node()
    shell = [{"name": "board", "members": [m[1:] for m in bc.MEMBERS1], "max_hamming": 0},
             {"name": "absent", "members": [(100, 0.0, 0.0, bc.SIZE1)]}]
    k9 = [600.0, 0.0, 320.0, 0.0, 600.0, 240.0, 0.0, 0.0, 1.0]
    frames = {"all_six": bc.content_frame("all_six"), "painted_over": bc.content_frame("painted_over")}
    want = {n: br.solve(bc.oracle_records(f, bc.INTR1[0]), bc.BUNDLE1, FAMS, bc.INTR1[0]) for n, f in frames.items()}

    def check(tfs, poses, name, ntags, stamp):
        assert [t["child_frame_id"] for t in tfs] == ["tag36h11:%d" % r["id"] for r in bc.oracle_records(frames[name], bc.INTR1[0])] + ["bundle:board"]
        tf = tfs[-1]
        assert tf["frame_id"] == "cam" and tf["stamp"] == stamp
        assert [p["name"] for p in poses] == ["board", "absent"] and poses[1]["status"] == capi.BUNDLE_TOO_FEW_TAGS and poses[1]["ntags"] == 0
        rec = dict(poses[0], bundle=0, R=np.array(poses[0]["R"]).reshape(3, 3), t=np.array(poses[0]["t"]))
        assert not br.compare(rec, want[name]) and rec["ntags"] == ntags
        assert tf["translation"] == poses[0]["t"]
        assert np.abs(_quat_matrix(tf["rotation_xyzw"]) - rec["R"]).max() < 1e-6   # (float quaternion)

    nodes = []
    try:
        n = node.AprilTagNode(size=bc.SIZE1, bundles=shell)
        nodes.append(n)
        dets, _ = n.on_frame(frames["all_six"].ctypes.data, False, "mono8", bc.W1, bc.H1, bc.W1, k9, "cam", (3, 0))
        assert len(dets) == 6
        check(n.transforms(), n.bundle_poses(), "all_six", 6, (3, 0))
        plain = node.AprilTagNode(size=bc.SIZE1)
        nodes.append(plain)
        pdets, _ = plain.on_frame(frames["all_six"].ctypes.data, False, "mono8", bc.W1, bc.H1, bc.W1, k9, "cam", (3, 0))
        assert pdets == dets and len(plain.transforms()) == 6 and plain.bundle_poses() == []
        multi = node.AprilTagMultiCameraNode(2, size=bc.SIZE1, bundles=shell)
        nodes.append(multi)
        for s, name in enumerate(("all_six", "painted_over")):
            assert multi.on_frame(s, frames[name].ctypes.data, False, "mono8", bc.W1, bc.H1, bc.W1, k9, "cam", (4, s))
        for s, (name, ntags) in enumerate((("all_six", 6), ("painted_over", 5))):
            assert multi.publishes(s) == 1
            check(multi.transforms(s), multi.bundle_poses(s), name, ntags, (4, s))
    finally:
        [x.close() for x in nodes]


# ---- 8. the suite bites -------------------------------------------------------------------------------------------------------------------
_SELECT = "test_content and throughput"
_SOLVED = ["test_content[%s-throughput-plain]" % n for n in bc.CONTENT if n != "no_tags"]
_WRONG_BUILDS = {
    # board corner k paired with p[3 - k]: every solved bundle gets another pose; a frame without tags has nothing to pair
    15: {"must_fail": tuple(_SOLVED), "must_pass": ("test_content[no_tags-throughput-plain]",)},
    # no duplicate rule: only the frame with a second copy of a member differs
    16: {"must_fail": ("test_content[duplicate-throughput-plain]",),
         "must_pass": tuple("test_content[%s-throughput-plain]" % n for n in bc.CONTENT if n != "duplicate")},
}


@pytest.mark.parametrize("mutant", sorted(_WRONG_BUILDS))
def test_the_bundle_tests_fail_on_the_wrong_builds(built, mutant):
    """libapriltag_amd_mut15.so and _mut16.so (csrc/tools_hooks.h, AMDAT_MUTATE): the content cases on the throughput set, in a process
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
    assert "differ" in out.stdout   # what differs: fields of the bundle record
    if "ok" not in _cache:   # (the product run is the same for both wrong builds)
        _cache["ok"] = run(None)
    out_ok, passed_ok, failed_ok = _cache["ok"]
    assert out_ok.returncode == 0 and not failed_ok and sorted(passed_ok) == sorted(passed + failed), (out_ok.stdout[-1500:], failed_ok)
