"""k_decode_wave and k_reconcile as stages, on frames that reach their edges (tests/decode_cases.py): tags within a few pixels of the
frame border -- refinement steps, gray-model samples and bit samples outside the image --, a tag16h5 word equally near two codes, a
duplicate nested inside a tag of its own id, and a frame with more decodable tags than the handle holds records for.  Every frame goes
through parity_util's stage comparison, which includes the records before reconcile (AMDAT_DBG_DETS), and the final records; nothing
has a tolerance.  tests/test_decode_stage_cpu.py holds the preconditions on the oracle alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from isaac_ros_apriltag_amd import capi  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402
import decode_cases as dc  # noqa: E402
import parity_util as pu  # noqa: E402

PATHS = ("latency", "throughput")


def _handle(w, h, families, path, decimate=1, max_batch=1, **more):
    K = dc.K_of(w, h)
    det = AprilTagDetector(w, h, families=families, decimate=decimate, intrinsics=(K[0, 0], K[1, 1], K[0, 2], K[1, 2]), max_batch=max_batch, **more)
    det.set_submission_path(path)
    return det


def _pitched(imgs, fill):
    """The equally sized frames in one device buffer whose rows carry dc.PITCH_PAD bytes of `fill` behind them: (tensor, frames)."""
    h, w = imgs[0].shape
    pitch = w + dc.PITCH_PAD
    buf = np.full((len(imgs), h, pitch), fill, dtype=np.uint8)
    for i, img in enumerate(imgs):
        buf[i, :, :w] = img
    t = torch.from_numpy(buf).cuda()
    return t, [(t.data_ptr() + i * h * pitch, pitch, w, h) for i in range(len(imgs))]


def _raw(det, i):
    rec = det.debug(i, capi.DBG_DETS)
    return rec[pu.record_order(rec)].tobytes()


def _final(dets):
    return [(d["family"], d["id"], d["hamming"], np.float32(d["decision_margin"]).tobytes()) + tuple(d[k].tobytes() for k in ("H", "center", "p", "R", "t"))
            for d in dets]


def _compare(det, i, img, gdets, families, key, decimate=1, **more):
    oracle = dc.oracle_on(key, img, families, decimate, **more)
    errs, odets = pu.compare_stages(det, i, img, families, dc.K_of(img.shape[1], img.shape[0]), decimate, oracle=oracle, **more)
    return errs + pu.compare_detections(gdets, odets), oracle


# ---- border tags ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("sigma", dc.SIGMAS, ids=lambda s: "sigma%d" % s)
@pytest.mark.parametrize("decimate,refine", dc.BORDER_SETTINGS, ids=["dec%d_refine%d" % s for s in dc.BORDER_SETTINGS])
def test_border_tags(built, decimate, refine, sigma, path):
    """The 56 border geometries, each with pixel (0, 0) at 0 and at 255, as one submission of frames whose rows are 19 bytes longer than
    the frame, the padding 0x00: every stage, the records before reconcile and the final records against the oracle.  Then the same
    frames with the padding 0xFF: the same records, raw and final."""
    cases = dc.border_cases(sigma, decimate)
    imgs = [img for _, img in cases]
    det = _handle(dc.W, dc.H, dc.FAM36, path, decimate, max_batch=len(imgs), refine_edges=bool(refine))
    try:
        keep0, frames0 = _pitched(imgs, 0x00)
        g0 = det.detect_batch_ex(frames0, max_dets=16)
        errs, raws, found = [], [], 0
        for i, (name, img) in enumerate(cases):
            e, (odets, _) = _compare(det, i, img, g0[i], dc.FAM36, ("border", name, sigma), decimate, refine_edges=refine)
            errs += ["%s: %s" % (name, x) for x in e]
            raws.append(_raw(det, i))
            found += [d["id"] for d in odets] == [5]
        print("decimate %d refine %d sigma %d %s: the oracle keeps the tag in %d of %d frames; %d mismatches" % (decimate, refine, sigma, path, found, len(cases), len(errs)))
        assert not errs, errs[:6]
        keep1, frames1 = _pitched(imgs, 0xFF)
        g1 = det.detect_batch_ex(frames1, max_dets=16)
        for i, (name, _) in enumerate(cases):
            assert _raw(det, i) == raws[i], "%s: the records before reconcile depend on the padding" % name
            assert _final(g1[i]) == _final(g0[i]), "%s: the final records depend on the padding" % name
    finally:
        det.close()


@pytest.mark.parametrize("path", PATHS)
def test_large_border_tag(built, path):
    """640 x 480, sides of 300 px two pixels from the top and left frame edges: 37 refinement samples a side, so the four sides' 148
    samples take three chunks of 64 lanes."""
    img = dc.large_frame()
    det = _handle(dc.LARGE["w"], dc.LARGE["h"], dc.FAM36, path)
    try:
        keep, frames = _pitched([img], 0xFF)
        g = det.detect_batch_ex(frames, max_dets=16)[0]
        errs, (odets, _) = _compare(det, 0, img, g, dc.FAM36, "large")
        assert not errs and [d["id"] for d in g] == [5], errs
    finally:
        det.close()


# ---- ties -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_tie_keeps_the_first_code(built, path):
    """A word three bits from tag16h5's codes 0 and 15, at four turns: id 0, hamming 3, with the rotation the oracle finds; with
    max_hamming 2 nothing."""
    imgs = [dc.word_frame(dc.tie_word(), t) for t in range(4)]
    for max_hamming in (3, 2):
        det = _handle(dc.W, dc.H, dc.FAM16, path, max_batch=4, max_hamming=max_hamming)
        try:
            keep, frames = _pitched(imgs, 0x00)
            g = det.detect_batch_ex(frames, max_dets=16)
            for t, img in enumerate(imgs):
                errs, _ = _compare(det, t, img, g[t], dc.FAM16, ("tie", t), max_hamming=max_hamming)
                assert not errs, (t, max_hamming, errs)
                assert [(d["id"], d["hamming"]) for d in g[t]] == ([(0, 3)] if max_hamming == 3 else []), (t, max_hamming, g[t])
        finally:
            det.close()


# ---- nested duplicate -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_nested_duplicate(built, path):
    """A small tag inside a white cell of a large tag of the same id: two records before reconcile, the small one kept (containment
    alone decides: no side meets a side); with the next id inside both stay."""
    cases = [(k, inner) for k in dc.NESTED_IDS for inner in (k, k + 1)]
    imgs = [dc.nested_frame(k, inner) for k, inner in cases]
    det = _handle(dc.NW, dc.NH, dc.FAM36, path, max_batch=len(imgs))
    try:
        keep, frames = _pitched(imgs, 0x00)
        g = det.detect_batch_ex(frames, max_dets=16)
        for i, ((k, inner), img) in enumerate(zip(cases, imgs)):
            errs, _ = _compare(det, i, img, g[i], dc.FAM36, ("nested", k, inner))
            assert not errs, (k, inner, errs)
            raw = det.debug(i, capi.DBG_DETS)
            assert sorted(int(v) for v in raw["id"]) == sorted([k, inner]), raw["id"]
            if inner == k:
                assert len(g[i]) == 1 and 60 < np.linalg.norm(g[i][0]["p"][0] - g[i][0]["p"][2]) < 75
            else:
                assert sorted(d["id"] for d in g[i]) == [k, inner]
    finally:
        det.close()


# ---- more decodable tags than max_detections ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_overflow_stays_inside_its_frame(built, path):
    """max_detections 4, two frames: eight decodable tags in frame 0, two in frame 1.  Frame 0 reports AMDAT_FLAG_DETS_OVERFLOW, counts
    every decoded quad, and hands out at most four records, each one of the oracle's, in the canonical order -- which four is the
    scheduler's choice.  Frame 1 is exact and flag-free: nothing spilled into its slots.  Then frame 1 alone on the same handle."""
    f0, f1 = dc.overflow_frames()
    (o0, d0), (o1, d1) = dc.oracle_on("overflow0", f0, dc.FAM36), dc.oracle_on("overflow1", f1, dc.FAM36)
    cap = dc.OVERFLOW_CAPACITY
    det = _handle(dc.W, dc.H, dc.FAM36, path, max_batch=2, max_detections=cap)
    try:
        keep, frames = _pitched([f0, f1], 0x00)
        g = det.detect_batch_ex(frames, max_dets=16)
        assert det.frame_flags(2) == [capi.FLAG_DETS_OVERFLOW, 0]
        counts = det.debug(0, capi.DBG_COUNTS)
        assert int(counts[4]) == len(d0["dets_raw"]) >= 8 and int(counts[5]) == capi.FLAG_DETS_OVERFLOW
        # frame 0's stages up to the quads are exact; only the flag and the record count differ
        errs, _ = pu.compare_stages(det, 0, f0, dc.FAM36, dc.K_of(dc.W, dc.H), oracle=(o0, d0))
        assert errs == ["frame flags 0x10", "records: gpu %d vs oracle %d" % (cap, len(d0["dets_raw"]))], errs
        raw = det.debug(0, capi.DBG_DETS)
        head = lambda r: tuple(r[f].tobytes() for f in ("family", "id", "hamming", "decision_margin", "H", "c", "p"))
        oracle_raw, got_raw = {head(r) for r in d0["dets_raw"]}, [head(r) for r in raw]
        assert len(raw) == cap and len(set(got_raw)) == cap and set(got_raw) <= oracle_raw and not raw["R"].any() and not raw["t"].any()
        # the records handed out: at most four, each bit-equal to the oracle's record of its id (all eight ids are distinct and kept), ordered
        oracle_final = {d["id"]: _final([d])[0] for d in o0}
        assert 1 <= len(g[0]) <= cap and all(_final([d])[0] == oracle_final[d["id"]] for d in g[0])
        assert [d["id"] for d in g[0]] == sorted(d["id"] for d in g[0]) and sorted(d["id"] for d in g[0]) == sorted(int(v) for v in raw["id"])
        errs1, _ = pu.compare_stages(det, 1, f1, dc.FAM36, dc.K_of(dc.W, dc.H), oracle=(o1, d1))
        errs1 += pu.compare_detections(g[1], o1)
        assert not errs1 and len(g[1]) == 2, errs1
        # frame 1 alone afterwards
        keep1, frames1 = _pitched([f1], 0xFF)
        g1 = det.detect_batch_ex(frames1, max_dets=16)
        errs2, _ = pu.compare_stages(det, 0, f1, dc.FAM36, dc.K_of(dc.W, dc.H), oracle=(o1, d1))
        errs2 += pu.compare_detections(g1[0], o1)
        assert not errs2 and det.frame_flags(1) == [0], errs2
    finally:
        det.close()


# ---- four wrong builds ----------------------------------------------------------------------------------------------------------------------
_HERE = os.path.basename(__file__)
_WRONG_BUILDS = {
    # 21: a refinement step with a read outside the image is counted, pixel 0 in that read's place
    21: {"files": (_HERE, "test_gpu_parity.py"), "select": "(test_border_tags and dec1_refine1) or test_large_border_tag or test_stage_and_detection_parity",
         "must_fail": ("test_border_tags[dec1_refine1-sigma0-latency]", "test_border_tags[dec1_refine1-sigma0-throughput]",
                       "test_border_tags[dec1_refine1-sigma1-"),
         "must_pass": ("test_stage_and_detection_parity",), "says": "records"},
    # 22: the code scan's reduction keeps the higher index at equal distance
    22: {"files": (_HERE, "test_gpu_parity.py"), "select": "test_tie_keeps_the_first_code or test_nested_duplicate or test_stage_and_detection_parity",
         "must_fail": ("test_tie_keeps_the_first_code[latency]", "test_tie_keeps_the_first_code[throughput]"),
         "must_pass": ("test_stage_and_detection_parity", "test_nested_duplicate"), "says": "records"},
    # 23: quads_overlap_dev without the containment tests
    23: {"files": (_HERE, "test_reconcile_gpu.py"), "select": "test_nested_duplicate or test_crafted_case or test_tie_keeps_the_first_code",
         "must_fail": ("test_nested_duplicate[latency]", "test_nested_duplicate[throughput]", "test_crafted_case[a_strictly_inside_b]",
                       "test_crafted_case[b_strictly_inside_a]"),
         "must_pass": ("test_crafted_case[crossing_edges]", "test_crafted_case[touching_in_one_corner]", "test_tie_keeps_the_first_code"), "says": "detections"},
    # 24: det_before_dev with margins ascending
    24: {"files": (_HERE, "test_reconcile_gpu.py"), "select": "test_crafted_case or (test_random_case and (64 or 130)) or test_tie_keeps_the_first_code",
         "must_fail": ("test_crafted_case[higher_margin_wins]", "test_random_case[64]", "test_random_case[130]"),
         "must_pass": ("test_crafted_case[lower_hamming_beats_higher_margin]", "test_crafted_case[equal_margin_first_differing_corner]",
                       "test_tie_keeps_the_first_code"), "says": "decision_margin"},
}


@pytest.mark.parametrize("mutant", sorted(_WRONG_BUILDS))
def test_the_decode_stage_tests_fail_on_the_wrong_builds(built, mutant):
    """libapriltag_amd_mut21.so .. _mut24.so (csrc/tools_hooks.h, AMDAT_MUTATE): a selection of these tests and of
    tests/test_reconcile_gpu.py, in a process of its own, must FAIL on the wrong build where its error lives and pass where it does
    not, and all of it passes on the product library.  21 and 22 live in k_decode_wave where only a border tag or a tie reaches them:
    tests/test_gpu_parity.py::test_stage_and_detection_parity still passes on both -- the gap these tests close.  23 and 24 live in
    k_reconcile."""
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
        out = subprocess.run([sys.executable, "-m", "pytest"] + [os.path.join(root, "tests", f) for f in spec["files"]] +
                             ["-m", "gpu", "-q", "-rA", "-p", "no:cacheprovider", "-k", spec["select"]],
                             capture_output=True, text=True, timeout=600, cwd=root, env=env)
        ids = lambda word: sorted(l.split("::", 1)[1].split(" ")[0] for l in out.stdout.splitlines() if l.startswith(word + " ") and "::" in l)
        return out, ids("PASSED"), ids("FAILED")
    out, passed, failed = run("mut%d" % mutant)
    assert out.returncode == 1, (out.stdout[-1500:], out.stderr[-1500:])
    assert len(failed) >= 2
    for want in spec["must_fail"]:
        assert any(t.startswith(want) for t in failed), (want, failed, passed)
    for want in spec["must_pass"]:
        assert any(t.startswith(want) for t in passed) and not any(t.startswith(want) for t in failed), (want, failed, passed)
    assert spec["says"] in out.stdout
    out_ok, passed_ok, failed_ok = run(None)
    assert out_ok.returncode == 0 and not failed_ok and sorted(passed_ok) == sorted(passed + failed), (out_ok.stdout[-1500:], failed_ok)
