"""The tag table inside the submission (amdAprilTagsSetTagTable): a size per (family, id) in k_reconcile,
k_undistort_records and k_pose_refine, and listed-only reporting in k_reconcile.  Expected values come from the existing references
-- the oracle, pose_refine_ref, pose_cov_ref, undistort_ref, bundle_ref, reconcile_ref -- run once per distinct size, record i taken
from the run of its own size (tests/tag_table_cases.py); every double is compared as its 64 bits.  The oracle-side preconditions
(which frame holds which record, that two sizes differ, the wrong builds' forms) are asserted in tests/test_tag_table_cpu.py."""
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
import pose_cov_ref as pv  # noqa: E402
import pose_refine_cases as pc  # noqa: E402
import pose_refine_ref as pr  # noqa: E402
import reconcile_cases as rcs  # noqa: E402
import reconcile_ref  # noqa: E402
import tag_table_cases as tc  # noqa: E402
import tag_table_ref as tt  # noqa: E402
import undistort_cases as uc  # noqa: E402
import undistort_ref as ur  # noqa: E402

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
    prep = det.prepare(frames, max_dets=max_dets, intrinsics=intrinsics)
    graph = mode.endswith("graph")
    for _ in range(2 if graph else 1):   # (graph: captured by the first submission, replayed by the second)
        det.submit_prepared(prep)
        det.wait_prepared(prep)
    assert det.last_submission_path() == mode.split("-")[0]
    assert (det.last_graph_nodes() > 0) == graph, (mode, det.last_graph_nodes())
    return prep


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def compare_records(got, want, label=""):
    """Mismatch strings between the library's detection records and the reference's: counts, the integer fields, the margin as a
    float, every double as its 64 bits."""
    if len(got) != len(want):
        return ["%srecords: %d, the reference has %d" % (label, len(got), len(want))]
    errs = []
    for i, (g, o) in enumerate(zip(got, want)):
        for k in ("family", "id", "hamming"):
            if g[k] != o[k]:
                errs.append("%srecord %d: %s %r, the reference has %r" % (label, i, k, g[k], o[k]))
        if np.float32(g["decision_margin"]) != np.float32(o["decision_margin"]):
            errs.append("%srecord %d: margin differs" % (label, i))
        for k in ("H", "center", "p", "R", "t"):
            if not np.array_equal(_bits(g[k]), _bits(o[k])):
                errs.append("%srecord %d (id %d): record field %s differs by %.3e" % (label, i, o["id"], k, np.abs(np.asarray(g[k]) - np.asarray(o[k])).max()))
    return errs


# ---- 1. sizes per record: the content frames in three modes under two tables ----------------------------------------------------------------
def _content(mode):
    """Both tables on one handle, in turn: (table, content case) -> (records, refined records, covariance records)."""
    if ("content", mode) not in _cache:
        det = _handle(mode, bc.W1, bc.H1, max_batch=3, tag_size=bc.SIZE1, pose_refinement=pc.ITERATIONS, pose_covariance=tc.SIGMA)
        det.set_frame_skews(bc.SKEW1)
        out = {}
        for which in tc.CONTENT_TABLES:
            det.set_tag_table(tc.CONTENT_TABLES[which])
            for sub in (0, 1):
                names = [n for n in bc.CONTENT if bc.SLOTS[n][0] == sub]
                names.sort(key=lambda n: bc.SLOTS[n][1])
                frames = torch.from_numpy(np.stack([bc.content_frame(n) for n in names])).cuda()
                prep = _submit(det, mode, frames, 64, list(bc.INTR1))
                recs, poses, covs = det.unpack(prep), det.refined_poses(3), det.refined_pose_covariances(3)
                for slot, n in enumerate(names):
                    out[(which, n)] = (recs[slot], poses[slot], covs[slot])
        assert det.late_waits() == 0
        det.close()
        _cache[("content", mode)] = out
    return _cache[("content", mode)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", sorted(tc.CONTENT_TABLES))
@pytest.mark.parametrize("name", bc.CONTENT)
def test_sizes_records(built, name, which, mode):
    """The detection records: R and t of every record are those of a tag of its own size."""
    got = _content(mode)[(which, name)][0]
    want = tc.content_sized(name, which)[0]
    errs = compare_records(got, want)
    print("%s %s %s: %d records %s" % (name, which, mode, len(got), errs[:4]))
    assert not errs, errs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", sorted(tc.CONTENT_TABLES))
@pytest.mark.parametrize("name", bc.CONTENT)
def test_sizes_refined(built, name, which, mode):
    """The refined poses and their covariances: pr_setup's and the covariance's model points have the tag's own size."""
    _, poses, covs = _content(mode)[(which, name)]
    _, want_poses, want_covs = tc.content_sized(name, which)
    errs = pr.compare_frames(poses, want_poses, "refined: ") + pv.compare_frames(covs, want_covs, "covariance: ")
    print("%s %s %s: %d refined records %s" % (name, which, mode, len(poses), errs[:4]))
    assert not errs, errs
    assert len(poses) == len(want_poses) == len(covs)


# ---- 2. more than one trip: 72 records, three sizes by id % 3 -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_board72(built, mode):
    """640 x 576, 72 tags: the copy loop of k_reconcile goes round a second time, k_pose_refine fills nine waves; with max_dets = 8 the
    first eight come out."""
    det = _handle(mode, bc.W2, bc.H2, tag_size=bc.SIZE2, intrinsics=bc.INTR2, pose_refinement=pc.ITERATIONS, pose_covariance=tc.SIGMA,
                  tags=tc.BOARD72_TABLE)
    frame = torch.from_numpy(bc.frame72()).cuda()
    want, want_poses, want_covs = tc.board72_sized()
    errs = []
    for max_dets in (128, 8):
        prep = _submit(det, mode, frame, max_dets, None)
        recs, poses, covs = det.unpack(prep)[0], det.refined_poses(1)[0], det.refined_pose_covariances(1)[0]
        assert len(recs) == min(max_dets, 72) == len(poses) == len(covs)
        errs += compare_records(recs, want[:max_dets], "max_dets %d: " % max_dets)
        errs += pr.compare_frames(poses, want_poses[:max_dets], "max_dets %d: " % max_dets)
        errs += pv.compare_frames(covs, want_covs[:max_dets], "max_dets %d: " % max_dets)
    assert det.late_waits() == 0
    det.close()
    print("board72 %s: %s" % (mode, errs[:4]))
    assert not errs, errs


# ---- 3. the family is in the key ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(tc.TWO_FAMILY_TABLES))
def test_family_in_the_key(built, which):
    """tag36h11 id 3 and tag25h9 id 3 in one frame of a two-family handle, with different sizes: by exact entries, and by a wildcard on
    family 1 (given by index)."""
    det = AprilTagDetector(tc.W3, tc.H3, families=tc.FAMS2, tag_size=tc.SIZE3, intrinsics=tc.INTR3, pose_refinement=pc.ITERATIONS,
                           pose_covariance=tc.SIGMA, tags=tc.TWO_FAMILY_TABLES[which])
    prep = det.prepare(torch.from_numpy(tc.two_family_frame()).cuda(), max_dets=64)
    det.run_prepared(prep)
    det.run_prepared(prep)
    assert det.last_graph_nodes() > 0
    want, want_poses, want_covs = tc.two_family_sized(which)
    errs = compare_records(det.unpack(prep)[0], want) + pr.compare_frames(det.refined_poses(1)[0], want_poses)
    errs += pv.compare_frames(det.refined_pose_covariances(1)[0], want_covs)
    det.close()
    assert not errs, errs


# ---- 4. listed-only -------------------------------------------------------------------------------------------------------------------------
def _listed_reference(name):
    """(records, refined records) of a content frame under LISTED with listed_only: the parent's kept list less the unlisted, in order."""
    table = tc.table_of(tc.LISTED, FAMS)
    recs, poses, _ = tc.content_sized(name, "listed")
    keep = [i for i, r in enumerate(recs) if tc.listed(table, FAMS, r)]
    return [recs[i] for i in keep], [poses[i] for i in keep]


@pytest.mark.parametrize("max_dets", (64, 5, 3))
def test_listed_only(built, max_dets):
    """All six content frames in one submission, each under its own slot's camera; painted_over holds listed tags only.  Records and
    counts are the parent's less the unlisted, in order, cut to max_dets AFTER the filter: with max_dets = 5, all_six hands out id 5,
    which the parent's cut loses.  Planar bundles see the filtered list."""
    slots = [bc.SLOTS[n][1] for n in bc.CONTENT]
    det = AprilTagDetector(bc.W1, bc.H1, max_batch=6, tag_size=bc.SIZE1, pose_refinement=pc.ITERATIONS, bundles=[bc.BUNDLE1],
                           tags=tc.LISTED, listed_only=True)
    det.set_frame_skews([bc.SKEW1[s] for s in slots])
    frames = torch.from_numpy(np.stack([bc.content_frame(n) for n in bc.CONTENT])).cuda()
    prep = det.prepare(frames, max_dets=max_dets, intrinsics=[bc.INTR1[s] for s in slots])
    det.run_prepared(prep)
    det.run_prepared(prep)
    assert det.last_graph_nodes() > 0
    recs, poses, bundles = det.unpack(prep), det.refined_poses(6), det.bundle_poses(6)
    flags = det.frame_flags(6)
    raw_counts = [len(det.debug(i, capi.DBG_DETS)) for i in range(6)]
    assert det.late_waits() == 0
    det.close()
    errs = []
    for f, name in enumerate(bc.CONTENT):
        want, want_poses = _listed_reference(name)
        errs += compare_records(recs[f], want[:max_dets], "%s: " % name)
        errs += pr.compare_frames(poses[f], want_poses[:max_dets], "%s: " % name)
        errs += ["%s: %s" % (name, e) for e in br.compare(bundles[f][0], br.solve(want, bc.BUNDLE1, FAMS, bc.INTR1[slots[f]], bc.SKEW1[slots[f]]))]
        # the records before reconcile and the overflow flag stay the parent's
        assert raw_counts[f] >= len(bc.content_records(name)) and not (flags[f] & 0x10)
    assert not errs, errs
    if max_dets == 5:
        assert 5 in [r["id"] for r in recs[bc.CONTENT.index("all_six")]]


def _reconcile_reference(records, table, listed_only, default, prm):
    """reconcile_ref followed by the filter; the pose of each kept record at its own size, from the oracle's pose statement."""
    kept = [i for i in reconcile_ref.reconcile(records)
            if not listed_only or tt.lookup(table, int(records["family"][i]), int(records["id"][i]), 0.0)[1]]
    out = records[kept].copy()
    for r in out:
        size = tt.lookup(table, int(r["family"]), int(r["id"]), tt.f32(default))[0]
        R, t = po.pose_from_homography(r["H"], prm.fx, prm.fy, prm.cx, prm.cy, size, prm.skew)
        r["R"], r["t"] = R.reshape(-1), t
    return out


def test_debug_reconcile_runs_with_the_table(built):
    """amdAprilTagsDebugReconcile on chosen records -- runs of one id with overlaps, listed and unlisted ids interleaved, up to 256
    records, the rank sort's fourth trip -- against reconcile_ref followed by the filter; sizes alone without listed_only."""
    det = AprilTagDetector(640, 480, families=("tag36h11", "tag25h9"), decimate=2, intrinsics=rcs.INTRINSICS, tag_size=rcs.TAG_SIZE,
                           max_batch=1, max_detections=rcs.MAX_DETECTIONS)
    table = tt.build(2, (587, 35), tc.RECONCILE_ENTRIES)
    cases = [rcs.crafted(n)[0] for n in ("runs_do_not_see_each_other", "crossing_under_another_family", "chain_c_survives")]
    cases += [rcs.random_case(n) for n in (1, 64, 65, 130, rcs.MAX_DETECTIONS)]
    for listed_only in (True, False):
        det.set_tag_table(tc.RECONCILE_ENTRIES, listed_only)
        for rec in cases:
            got = det.debug_reconcile(rec)
            want = _reconcile_reference(rec, table, listed_only, rcs.TAG_SIZE, rcs.params())
            assert len(got) == len(want), (listed_only, len(rec), len(got), len(want))
            assert rcs.same_records(got, want), (listed_only, len(rec))
    det.set_tag_table(None)
    for rec in cases:
        assert rcs.same_records(det.debug_reconcile(rec), rcs.expected_records(rec))
    det.close()


# ---- 5. raw-frame mode: the twins carry the id's size ---------------------------------------------------------------------------------------
def test_raw_frame_mode(built):
    """corner_undistortion on, nine tags under the rational camera, three sizes by id % 3: the raw records, the twins and the refined
    poses of the twins, each from the reference run of the record's own size; amdAprilTagsDebugUndistort runs with the same table."""
    sizes = (bc.SIZE1, 0.04, 0.15)
    camera = uc.CAMERAS["rational"]
    raw = uc.raw("nine", "rational")
    base = uc.raw_records("nine", "rational")
    ids = [int(r["id"]) for r in base]
    assert len(base) == 9 and {i % 3 for i in ids} == {0, 1, 2}
    tags = [("tag36h11", i, sizes[i % 3]) for i in ids if i % 3]
    det = AprilTagDetector(uc.W, uc.H, tag_size=bc.SIZE1, intrinsics=uc.INTR, corner_undistortion=[camera], pose_refinement=pc.ITERATIONS, tags=tags)
    prep = det.prepare(torch.from_numpy(raw).cuda(), max_dets=64)
    det.run_prepared(prep)
    det.run_prepared(prep)
    assert det.last_graph_nodes() > 0
    recs, twins, poses = det.unpack(prep)[0], det.undistorted_detections(1)[0], det.refined_poses(1)[0]
    want_recs, want_twins, want_poses = [], [], []
    runs = {}
    for i, r in enumerate(base):
        s = sizes[int(r["id"]) % 3]
        if s not in runs:
            raw_s = bc.oracle_records(raw, uc.INTR, tag_size=s)
            tw_s = ur.records(raw_s, camera, uc.INTR, s)
            runs[s] = (raw_s, tw_s, ur.refined(tw_s, uc.INTR, 0.0, s, pc.ITERATIONS))
        for o, g in zip((want_recs, want_twins, want_poses), runs[s]):
            o.append(g[i])
    errs = compare_records(recs, want_recs)
    for i, (g, w) in enumerate(zip(twins, want_twins)):
        errs += ["twin %d: %s" % (i, e) for e in ur.compare(g, w)]
    errs += pr.compare_frames(poses, want_poses)
    assert len(twins) == 9 and not errs, errs
    assert not np.array_equal(want_twins[ids.index(1)]["t"], ur.records(base, camera, uc.INTR, bc.SIZE1)[ids.index(1)]["t"])
    # the stage on its own
    rec = np.zeros(len(base), dtype=capi.DET_DTYPE)
    for i, r in enumerate(base):
        rec["family"][i], rec["id"][i], rec["hamming"][i], rec["p"][i] = 0, r["id"], r["hamming"], r["p"]
    pub, _ = det.debug_undistort(rec, camera)
    for i, w in enumerate(want_twins):
        assert np.array_equal(_bits(pub["t"][i]), _bits(w["t"])) and np.array_equal(_bits(pub["R"][i]).reshape(-1), _bits(w["R"]).reshape(-1)), i
    det.close()


# ---- 6. contents change, graphs stay --------------------------------------------------------------------------------------------------------
def test_contents_change_no_graph(built):
    """One handle: entries replaced and listed_only flipped between replays of the graph captured under the first table."""
    det = AprilTagDetector(bc.W1, bc.H1, tag_size=bc.SIZE1, intrinsics=bc.INTR1[2], pose_refinement=pc.ITERATIONS, tags=tc.CONTENT_TABLES["exact"])
    prep = det.prepare(torch.from_numpy(bc.content_frame("non_member")).cuda(), max_dets=64)
    det.run_prepared(prep)
    det.run_prepared(prep)
    state = det.graph_replay()
    assert state == (True, 1, 0) and det.last_graph_nodes() > 0
    nodes = det.last_graph_nodes()
    table_listed = tc.table_of(tc.LISTED, FAMS)
    errs = []
    for which, listed_only in (("exact", False), ("wild", False), ("listed", True), ("listed", False), ("exact", True), ("wild", True)):
        det.set_tag_table(tc.LISTED if which == "listed" else tc.CONTENT_TABLES[which], listed_only)
        det.run_prepared(prep)
        assert det.graph_replay() == state and det.last_graph_nodes() == nodes
        want, want_poses, _ = tc.content_sized("non_member", which)
        if listed_only and which == "listed":
            keep = [i for i, r in enumerate(want) if tc.listed(table_listed, FAMS, r)]
            want, want_poses = [want[i] for i in keep], [want_poses[i] for i in keep]
            assert len(want) == 5
        elif listed_only and which == "exact":   # ids 1, 4, 5 and the lone tag
            keep = [i for i, r in enumerate(want) if int(r["id"]) in (1, 4, 5, bc.LONE_ID)]
            want, want_poses = [want[i] for i in keep], [want_poses[i] for i in keep]
        errs += compare_records(det.unpack(prep)[0], want, "%s %s: " % (which, listed_only))
        errs += pr.compare_frames(det.refined_poses(1)[0], want_poses, "%s %s: " % (which, listed_only))
    assert det.late_waits() == 0
    det.close()
    assert not errs, errs


# ---- 7. off means off; the setter's contract ------------------------------------------------------------------------------------------------
def test_off_means_off_and_the_setter_contract(built):
    frame = torch.from_numpy(bc.content_frame("all_six")).cuda()
    det = AprilTagDetector(bc.W1, bc.H1, families=("tag36h11", "tag25h9"), tag_size=bc.SIZE1, intrinsics=bc.INTR1[0], max_batch=2)
    L, h = capi.lib(), det._h

    def run():
        prep = det.prepare(frame, max_dets=64)
        det.run_prepared(prep)
        return bytes(prep["out"]), int(prep["cnt"][0])

    def entries(rows):
        arr = (capi.TagEntry * len(rows))()
        for e, (fi, tid, size, res) in zip(arr, rows):
            e.family_index, e.id, e.size, e.reserved = fi, tid, size, res
        return arr

    # off is the default: turning it off again changes nothing
    bytes0 = det.device_bytes()
    off = run()
    assert run() == off and off[1] >= 6
    nodes_off = det.last_graph_nodes()
    assert nodes_off > 0 and det.graph_replay() == (True, 1, 0)
    det.set_tag_table(None)
    det.set_tag_table([])
    assert det.device_bytes() == bytes0 and det.graph_replay() == (True, 1, 0)
    # on: a buffer, the graph captured without a table is retired, the same launches
    det.set_tag_table([("tag36h11", 1, 0.05)])
    assert det.device_bytes() == bytes0 + 16 + 4096 * 12 and det.graph_replay() == (True, 0, 1)
    on = run()
    assert run() == on and on != off and on[1] == off[1] and det.last_graph_nodes() == nodes_off
    state = det.graph_replay()
    # every refusal leaves the table in force and retires nothing
    ok = [(0, 1, 0.05, 0)]
    refused = {
        "null handle": lambda: L.amdAprilTagsSetTagTable(None, 1, entries(ok), 0),
        "entries missing": lambda: L.amdAprilTagsSetTagTable(h, 1, None, 0),
        "reserved": lambda: L.amdAprilTagsSetTagTable(h, 1, entries([(0, 1, 0.05, 1)]), 0),
        "listed_only 2": lambda: L.amdAprilTagsSetTagTable(h, 1, entries(ok), 2),
        "duplicate key": lambda: L.amdAprilTagsSetTagTable(h, 2, entries(ok + ok), 0),
        "family beyond the handle's": lambda: L.amdAprilTagsSetTagTable(h, 1, entries([(2, 1, 0.05, 0)]), 0),
        "id at the code count": lambda: L.amdAprilTagsSetTagTable(h, 1, entries([(1, 35, 0.05, 0)]), 0),
        "negative size": lambda: L.amdAprilTagsSetTagTable(h, 1, entries([(0, 1, -0.05, 0)]), 0),
        "infinite size": lambda: L.amdAprilTagsSetTagTable(h, 1, entries([(0, 1, float("inf"), 0)]), 0),
        "nan size": lambda: L.amdAprilTagsSetTagTable(h, 1, entries([(0, 1, float("nan"), 0)]), 0),
        "4097 entries": lambda: L.amdAprilTagsSetTagTable(h, 4097, entries([(0, i % 587, 0.05, 0) for i in range(4097)]), 0),
    }
    for what, call in refused.items():
        assert call() == INVALID_ARGUMENT, what
        assert det.graph_replay() == state, what
    assert run() == on
    assert L.amdAprilTagsSetTagTable(h, 1, entries([(1, 34, 0.05, 0)]), 1) == 0      # the last id of tag25h9 is taken ...
    assert run()[1] == 0 and det.graph_replay() == state                             # ... and lists nothing of this frame
    det.set_tag_table([("tag36h11", 1, 0.05)])
    # between Submit and Wait the setter is refused, with and without entries
    prep = det.prepare(frame, max_dets=64)
    det.submit_prepared(prep)
    assert _code(lambda: det.set_tag_table([("tag36h11", 2, 0.1)])) == INVALID_ARGUMENT
    assert _code(lambda: det.set_tag_table(None)) == INVALID_ARGUMENT
    det.wait_prepared(prep)
    assert (bytes(prep["out"]), int(prep["cnt"][0])) == on and det.graph_replay() == state
    # off again: the bytes, the memory and the node count of the start
    capturing, live, retired = det.graph_replay()
    det.set_tag_table(None)
    assert det.graph_replay() == (True, 0, retired + live) and det.device_bytes() == bytes0
    assert run() == off
    assert run() == off and det.last_graph_nodes() == nodes_off
    assert det.late_waits() == 0
    det.close()


# ---- 8. the nodes ---------------------------------------------------------------------------------------------------------------------------
def test_nodes_publish_sizes_and_frame_names(built):
    """AprilTagNode and a two-stream AprilTagMultiCameraNode with tags= on the oblique frame: child frames are the given names where
    given and "family:id" otherwise, positions the float of the per-size translation (the refined one with pose_refinement); with
    tags_listed_only the unlisted tag has neither a detection nor a transform; a frame above 47 characters is refused."""
    from isaac_ros_apriltag_amd import build as b
    from isaac_ros_apriltag_amd import node
    b.build_node()
    k9 = [600.0, 0.0, 320.0, 0.0, 600.0, 240.0, 0.0, 0.0, 1.0]
    frame = pc.oblique_frame()
    (recs, refined, _), table = tc.oblique_sized()
    names = {i: f for i, _, f in tc.NODE_TAGS}

    def check(dets, tfs, stamp, want, listed_only):
        pairs = [(r, w) for r, w in zip(recs, want) if not listed_only or tc.listed(table, FAMS, r)]
        assert [d["id"] for d in dets] == [r["id"] for r, _ in pairs] and len(pairs) == (3 if listed_only else 4)
        assert all(d["family"] == "tag36h11" for d in dets)
        assert [t["child_frame_id"] for t in tfs] == [names.get(r["id"]) or "tag36h11:%d" % r["id"] for r, _ in pairs]
        for d, tf, (r, w) in zip(dets, tfs, pairs):
            assert tf["frame_id"] == "cam" and tf["stamp"] == stamp
            assert d["position"] == [float(np.float32(v)) for v in w["t"]] == tf["translation"]

    nodes = []
    try:
        for listed_only in (False, True):
            n = node.AprilTagNode(size=pc.SIZE_O, tags=tc.NODE_TAGS, tags_listed_only=listed_only)
            nodes.append(n)
            dets, _ = n.on_frame(frame.ctypes.data, False, "mono8", pc.WO, pc.HO, pc.WO, k9, "cam", (3, 0))
            check(dets, n.transforms(), (3, 0), recs, listed_only)
            multi = node.AprilTagMultiCameraNode(2, size=pc.SIZE_O, pose_refinement=pc.ITERATIONS, tags=tc.NODE_TAGS, tags_listed_only=listed_only)
            nodes.append(multi)
            for s in (0, 1):
                assert multi.on_frame(s, frame.ctypes.data, False, "mono8", pc.WO, pc.HO, pc.WO, k9, "cam", (4, s))
            for s in (0, 1):
                assert multi.publishes(s) == 1
                check(multi.last(s)[0], multi.transforms(s), (4, s), refined, listed_only)
        with pytest.raises(RuntimeError, match="longer than 47"):
            node.AprilTagNode(size=pc.SIZE_O, tags=[(3, 0.05, "x" * 48)])
        with pytest.raises(RuntimeError, match="longer than 47"):
            node.AprilTagMultiCameraNode(2, size=pc.SIZE_O, tags=[(3, 0.05, "x" * 48)])
        nodes.append(node.AprilTagNode(size=pc.SIZE_O, tags=[(3, 0.05, "x" * 47)]))
    finally:
        [x.close() for x in nodes]


# ---- 9. the suite bites ---------------------------------------------------------------------------------------------------------------------
_SELECT = "(test_sizes_records or test_sizes_refined) and throughput"
_WITH_TAGS = tuple(n for n in bc.CONTENT if n != "no_tags")


def _ids(tests, names, tables):
    return tuple("%s[%s-%s-throughput-plain]" % (t, n, w) for t in tests for n in names for w in tables)


_BOTH = ("test_sizes_records", "test_sizes_refined")
_ALL = _ids(_BOTH, bc.CONTENT, ("exact", "wild"))
_WRONG_BUILDS = {
    # the last key is never found: under "exact" it is the lone tag's, which non_member alone looks up; under "wild" it is the wildcard,
    # which every frame with tags needs
    53: {"must_fail": _ids(_BOTH, ("non_member",), ("exact",)) + _ids(_BOTH, _WITH_TAGS, ("wild",)), "says": "t differ"},
    # the wildcard first: wrong only where an exact entry sits beside it -- "wild", whose exact entries every frame with tags holds
    54: {"must_fail": _ids(_BOTH, _WITH_TAGS, ("wild",)), "says": "t differ"},
    # k_pose_refine with the handle's size: refined records and covariances of every frame with tags, never a detection record
    55: {"must_fail": _ids(("test_sizes_refined",), _WITH_TAGS, ("exact", "wild")), "says": "refined: "},
}


@pytest.mark.parametrize("mutant", sorted(_WRONG_BUILDS))
def test_the_tag_table_tests_fail_on_the_wrong_builds(built, mutant):
    """libapriltag_amd_mut53.so .. _mut55.so (csrc/tools_hooks.h, AMDAT_MUTATE): the sizes cases on the throughput set, in a process of
    their own, must FAIL on the wrong build exactly where its error lives and pass elsewhere, and all of them pass on the product
    library.  The wrong builds change values only."""
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
    assert sorted(passed) == sorted(set(_ALL) - set(spec["must_fail"])), (failed, passed)
    assert spec["says"] in out.stdout
    if "ok" not in _cache:   # (the product run is the same for the three wrong builds)
        _cache["ok"] = run(None)
    out_ok, passed_ok, failed_ok = _cache["ok"]
    assert out_ok.returncode == 0 and not failed_ok and sorted(passed_ok) == sorted(_ALL), (out_ok.stdout[-1500:], failed_ok)
