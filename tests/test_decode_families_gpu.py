"""k_decode_wave on what the families of the suite so far never brought it (tests/decode_family_cases.py): code tables of several codes
per lane with ties inside a lane (dense16: 3 000 codes of 16 bits), 313 trips per scan (std52: 20 000 codes), a 64-bit word (d8),
border squares of 9 and 10 cells, whose gray-model samples take the sample loop's second trip (d7, through amdAprilTagsRegisterFamily at
its limit, and d8), next to d3 and tag16h5.  Per family, max_hamming 0 .. 3 and launch set: one handle, one submission of the family's
400 tags in at most 14 frames with padded rows; every stage, the records before reconcile and the final records against the oracle with
no tolerance; then the library's own records against the scan of tests/decode_lookup_cases.py, tag by tag.  One more case runs four
families in one handle.  tests/test_decode_families_cpu.py holds the preconditions and the census on the oracle alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from isaac_ros_apriltag_amd import capi  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402
import decode_family_cases as fc  # noqa: E402
import parity_util as pu  # noqa: E402

PATHS = ("latency", "throughput")
CASES = [(n, mh, p) for n in fc.NAMES for mh in fc.MAX_HAMMINGS for p in PATHS]   # (a family's two launch sets share one oracle run)


def _pitched(imgs, fill):
    """The frames in one device buffer whose rows carry fc.PITCH_PAD bytes of `fill` behind them (as tests/test_decode_stage_gpu.py)."""
    h, w = imgs[0].shape
    pitch = w + fc.PITCH_PAD
    buf = np.full((len(imgs), h, pitch), fill, dtype=np.uint8)
    for i, img in enumerate(imgs):
        buf[i, :, :w] = img
    t = torch.from_numpy(buf).cuda()
    return t, [(t.data_ptr() + i * h * pitch, pitch, w, h) for i in range(len(imgs))]


def _submit(names, imgs, oracle, max_hamming, path, max_detections):
    """Registers the families, runs the frames as one submission of one handle and compares every frame with the oracle's (detections,
    dump): (mismatches, the library's records before reconcile per frame).  The registry is process-wide: emptied again in any case."""
    K = fc.K()
    done = []
    try:
        fams = []
        for n in names:
            fams.append(fc.register(n, capi))
            done.append(n)
        det = AprilTagDetector(fc.W, fc.H, families=tuple(fams), intrinsics=(K[0, 0], K[1, 1], K[0, 2], K[1, 2]), max_batch=len(imgs),
                               max_hamming=max_hamming, max_detections=max_detections)
        try:
            det.set_submission_path(path)
            keep, frames = _pitched(imgs, 0x00)
            g = det.detect_batch_ex(frames, max_dets=max_detections)
            errs, records = [], []
            for i, img in enumerate(imgs):
                e, odets = pu.compare_stages(det, i, img, None, K, 1, oracle=oracle[i], max_hamming=max_hamming)
                errs += ["frame %d: %s" % (i, x) for x in e + pu.compare_detections(g[i], odets)]
                records.append(det.debug(i, capi.DBG_DETS))
            return errs, records
        finally:
            det.close()
    finally:
        for n in done:
            fc.unregister(n, capi)


@pytest.mark.parametrize("name,mh,path", CASES, ids=["%s-mh%d-%s" % c for c in CASES])
def test_families(built, name, mh, path):
    oracle = fc.oracle_on(name, mh)
    errs, records = _submit((name,), fc.frames(name), oracle, mh, path, fc.MAX_DETECTIONS)
    assert not errs, errs[:6]
    # the library's own records against the scan: one record on the border square of every tag whose word, as first read, the scan
    # accepts, with the scan's id, hamming and rotation; none on the others
    tg = fc.tags(name)
    ob = fc.observed(records, [d["quads"] for _, d in oracle], name)
    exp = fc.expected_rows(name, mh, [fc.read_orientation(t, o["near"]) for t, o in zip(tg, ob)])
    bad = [(j, fc.row_of(o), tuple(e), len(o["records"])) for j, (o, e) in enumerate(zip(ob, exp))
           if fc.row_of(o) != tuple(e) or len(o["records"]) != e[0]]
    print("%s max_hamming %d %s: %d of %d tags found, %d records in %d frames" %
          (name, mh, path, sum(e[0] for e in exp), len(tg), sum(len(r) for r in records), len(records)))
    assert not bad, ("records against the scan", bad[:5])


@pytest.mark.parametrize("path", PATHS)
def test_four_families_in_one_handle(built, path):
    """tag16h5, dense16, std52 and d8 in one handle -- AT_MAX_FAMILIES -- on the first frames of each: every quad is decoded four times.
    tag16h5 and dense16 share one layout, so one quad yields two records that differ only in the family and reconcile keeps both
    (tests/test_decode_families_cpu.py counts them); every stage and record against the oracle under the same four descriptors."""
    oracle = fc.four_oracle()
    errs, records = _submit(fc.FOUR, fc.four_frames(), oracle, fc.FOUR_MAX_HAMMING, path, fc.FOUR_MAX_DETECTIONS)
    assert not errs, errs[:6]
    assert all({0, 1} <= set(int(v) for v in r["family"]) for r in records[:2 * fc.FOUR_FRAMES])   # both on the h5 and the dense16 frames


# ---- three wrong builds -------------------------------------------------------------------------------------------------------------------------
_HERE = os.path.basename(__file__)
_WRONG_BUILDS = {
    # 56: the in-lane code scan keeps the later code at equal distance
    56: {"files": (_HERE, "test_decode_stage_gpu.py"),
         "select": "(test_families and latency and (dense16-mh2 or dense16-mh3 or h5-mh)) or test_tie_keeps_the_first_code",
         "must_fail": ("test_families[dense16-mh2-latency]", "test_families[dense16-mh3-latency]"),
         "must_pass": ("test_families[h5-mh0-", "test_families[h5-mh1-", "test_families[h5-mh2-", "test_families[h5-mh3-", "test_tie_keeps_the_first_code")},
    # 57: the quarter turn's ballot without lane 63
    57: {"files": (_HERE,), "select": "test_families and mh2 and (d8 or std52 or d7)",
         "must_fail": ("test_families[d8-mh2-latency]", "test_families[d8-mh2-throughput]"),
         "must_pass": ("test_families[std52-mh2-", "test_families[d7-mh2-")},
    # 58: the border samples from index 64 on stored as invalid
    58: {"files": (_HERE, "test_gpu_parity.py"),
         "select": "(test_families and mh1 and latency and (d8 or d7 or std52 or dense16)) or test_stage_and_detection_parity",
         "must_fail": ("test_families[d8-mh1-latency]", "test_families[d7-mh1-latency]"),
         "must_pass": ("test_families[std52-mh1-", "test_families[dense16-mh1-", "test_stage_and_detection_parity")},
}


@pytest.mark.parametrize("mutant", sorted(_WRONG_BUILDS))
def test_the_family_tests_fail_on_the_wrong_builds(built, mutant):
    """libapriltag_amd_mut56.so .. _mut58.so (csrc/tools_hooks.h, AMDAT_MUTATE): a selection of these tests, in a process of its own,
    must FAIL on the wrong build where its error lives -- in the records -- and pass where it does not, and all of it passes on the
    product library.  56 lives where two equally near codes share a lane of the scan: tag16h5's 30 codes and the tie word of
    tests/test_decode_stage_gpu.py never get there.  57 lives in the turn of a 64-bit word, 58 in the gray models of a border square of
    9 or 10 cells: tests/test_gpu_parity.py::test_stage_and_detection_parity passes on it."""
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
    assert "records" in out.stdout
    out_ok, passed_ok, failed_ok = run(None)
    assert out_ok.returncode == 0 and not failed_ok and sorted(passed_ok) == sorted(passed + failed), (out_ok.stdout[-1500:], failed_ok)
