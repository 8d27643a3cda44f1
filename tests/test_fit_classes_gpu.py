"""The quad fit under quads the oracle KEEPS, in every size class and every sort form (tests/fit_frames.py): five k_fit_quads<NT, SPLIT>
instances of 64 .. 1024 threads and k_fit_small<2>; keys sorted in registers with 1, 2 or 4 per lane, in LDS padded and unpadded, and in
global scratch; the moment sweep in both wordings (two doubles up to 2048 pixels a side, 128-bit fixed point above).  Every case goes
through parity_util's comparison -- all stages and quads bit for bit -- and then asserts, on the library's own cluster and quad lists,
that the quads it was built for are there: a later change of a frame cannot hollow a case out unnoticed.  The same census conditions
hold on the oracle alone in tests/test_fit_frames_cpu.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from isaac_ros_apriltag_amd import capi, synth  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
import fit_frames as ff  # noqa: E402
import parity_util as pu  # noqa: E402

PATHS = ("latency", "throughput")
FAM = ("tag36h11",)


def _submit(imgs, path):
    """One submission of the equally sized frames `imgs` on a handle of their size, pinned to launch set `path`: every stage, quad and
    record of every frame against the oracle, then per frame (kept, dropped, cluster list, quad list) -- fit_frames.census on the
    library's own DBG_CLUSTERS and DBG_QUADS."""
    h, w = imgs[0].shape
    K = synth.default_K(w, h)
    det = AprilTagDetector(w, h, families=FAM, decimate=1, intrinsics=(K[0, 0], K[1, 1], K[0, 2], K[1, 2]), max_batch=len(imgs))
    try:
        det.set_submission_path(path)
        g = det.detect_batch_ex(torch.from_numpy(np.stack(imgs)).cuda(), max_dets=64)
        errs, out = [], []
        for i, img in enumerate(imgs):
            e, odets = pu.compare_stages(det, i, img, FAM, K, 1)
            e += pu.compare_detections(g[i], odets)
            errs += ["frame %d: %s" % (i, x) for x in e]
            cl, q = det.debug(i, capi.DBG_CLUSTERS), det.debug(i, capi.DBG_QUADS)
            out.append(ff.census_gpu(cl, q, ff.sort_cap(w, h), ff.has_fit_small(w, h, path)) + (cl, q))
    finally:
        det.close()
    assert not errs, errs[:4]
    return out


# ---- (a) the ladder: one frame with a quad in every class ---------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("content", sorted(ff.LADDER_CONTENT))
@pytest.mark.parametrize("w", ff.LADDER_WIDTHS, ids=["w2048", "w2049"])
def test_ladder(built, w, content, path):
    """Three nested large rectangles, a row of small ones and a checkerboard patch: clean, under sigma-1 noise (4 200 noise clusters
    beside them) and with sides that ripple by 3 pixels.  2048 wide the handle sums moments in two doubles and its throughput set
    has k_fit_small; 2049 wide neither."""
    a, sigma = ff.LADDER_CONTENT[content]
    kept, dropped, _, _ = _submit([ff.ladder(w, a, sigma)], path)[0]
    counts = [n for n, _, _ in kept]
    fit_small = ff.has_fit_small(w, ff.LADDER_H, path)
    assert fit_small == (w == 2048 and path == "throughput")
    if content == "clean":
        assert ff.classes_of(kept) == set(range(ff.NCLASSES)), kept
        forms = ff.forms_of(kept, 0) | ff.forms_of(kept, 1)
        if fit_small:   # clusters up to 128 points sort in k_fit_small's registers; it has them on either side of 64 points
            assert forms == {"fit_small"} | set(ff.ONE_WAVE_FORMS[2:]), forms
            assert min(counts) <= 64 and any(64 < n <= 128 for n in counts)
        else:
            assert forms == set(ff.ONE_WAVE_FORMS), forms
        assert ff.forms_of(kept, 2) | ff.forms_of(kept, 3) | ff.forms_of(kept, 4) | ff.forms_of(kept, 5) == {"lds_padded"}
        # the two light rectangles inside dark ones: clusters of the two largest classes that end at the border direction
        assert [n for n in dropped if n > 128] == [5912, 8152], dropped
    elif content == "noise":
        assert set(counts) >= {1696, 3392, 4427, 7312, 9368} and len(kept) > 200 and len(dropped) > 1500, (counts[-8:], len(dropped))
        assert ff.forms_of(kept, 0) | ff.forms_of(kept, 1) >= set(ff.ONE_WAVE_FORMS[2:])
    else:
        # sides at about half the line-fit limit: kept in the 256- and the 1024-thread class, given up in the 512-thread class and once more
        # in the 1024-thread class
        assert {3, 5} <= ff.classes_of(kept) and {4064, 9088} <= set(counts), kept[-6:]
        assert [n for n in dropped if n > 128] == [4399, 5912, 8152, 12268], dropped
    if w == 2049 and path == "throughput":
        # no k_fit_small in this plan (tests/test_launch_plan_cpu.py): the quads of clusters up to 128 points came from k_fit_quads<64>
        small = ff.forms_of(kept, 0)
        assert small and small <= set(ff.REG_FORMS[:2]), small
        assert content == "noise" or small == set(ff.REG_FORMS[:2])


# ---- (b) the near-limit sweep: the sound early exits on a margin -------------------------------------------------------------------------------
_SWEEP_BATCH = 8


def _sweep_census(dump, rects, w, quad_keys):
    """Per class: how many clusters of the DARK rectangles (fit_frames.rect_of_box on the oracle's points) have a quad in `quad_keys`,
    and how many have none."""
    kept, lost = [0] * ff.NCLASSES, [0] * ff.NCLASSES
    for key, count, box in ff.cluster_boxes(dump):
        i = ff.rect_of_box(box, rects, w, ff.LADDER_H)
        assert i is not None, (count, box)
        if rects[i][5] == ff.D:
            (kept if key in quad_keys else lost)[ff.size_class(count)] += 1
    return kept, lost


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("batch", range(len(ff.SWEEP_SEEDS) // _SWEEP_BATCH), ids=lambda b: "b%d" % b)
@pytest.mark.parametrize("w", ff.LADDER_WIDTHS, ids=["w2048", "w2049"])
def test_near_limit_sweep(built, w, batch, path):
    """24 seeded frames of the ladder's layout whose rectangles ripple by 1.5 .. 6 pixels at seeded periods and angles, eight to a
    submission: in every k_fit_quads class some sides fit a line just inside the limit and some just outside, so the prefilter's sector
    test and the group test after the first walk must pass real quads on a thin margin and may drop only what the oracle drops.  Over
    the 24 frames the oracle keeps at least 8 of the dark rectangles' clusters in each class and gives up at least 5
    (tests/test_fit_frames_cpu.py); each batch of eight holds some of either kind in every class, asserted here on the library's lists."""
    seeds = ff.SWEEP_SEEDS[batch * _SWEEP_BATCH:(batch + 1) * _SWEEP_BATCH]
    imgs = [ff.sweep_frame(s, w) for s in seeds]
    res = _submit(imgs, path)
    K = synth.default_K(w, ff.LADDER_H)
    kept, lost = np.zeros(ff.NCLASSES, int), np.zeros(ff.NCLASSES, int)
    for s, img, (_, _, cl, q) in zip(seeds, imgs, res):
        _, dump = po.detect(img, families=FAM, params=pu.oracle_params(K), want_dump=True)
        k, n = _sweep_census(dump, ff.sweep_rects(s), w, {int(x) for x in q["key"]})
        kept += k
        lost += n
    assert (kept[1:] >= 1).all() and (lost[1:] >= 1).all(), (kept, lost)


# ---- (c) giants: one cluster beyond the 16 384-key LDS array --------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sorted(ff.GIANTS))
def test_giants(built, name, path):
    """One rippling rectangle that fills the frame.  1920 x 1080: the handle's largest cluster is 18 000 points, so the LDS key array is
    raised to 18 048 and the 17 936-point cluster sorts there, unpadded (with a shorter ripple period the boundary exceeds the cap and
    both sides have no cluster at all); 2048 x 2048: the sort runs in global scratch, the sweep in two doubles; 2800 x 1800: global
    scratch and the 128-bit sweep."""
    w, h, _, _, _, _, _, (lo, hi), quad = ff.GIANTS[name]
    kept, dropped, cl, q = _submit([ff.giant(name)], path)[0]
    if not quad:
        assert len(cl) == 0 and len(q) == 0
        return
    form = "lds_unpadded" if name.startswith("1080p") else "global"
    assert len(cl) == 1 and lo <= int(cl["count"][0]) <= hi and ff.sort_cap(w, h) == (18048 if name.startswith("1080p") else 16384)
    assert kept == [(int(cl["count"][0]), 5, form)] and not dropped, (kept, dropped)
    assert np.linalg.norm(q["p"][0][0] - q["p"][0][2]) > 1500


# ---- two wrong builds -----------------------------------------------------------------------------------------------------------------------------
_HERE = os.path.basename(__file__)
_WRONG_BUILDS = {
    # 7: a quarter of the line-fit limit in the group test of k_fit_quads<256, true> and <1024, true>
    7: {"files": (_HERE, "test_gpu_parity.py"),
        "select": "(test_near_limit_sweep and w2048 and b0) or (test_ladder and w2048 and ripple) or test_large_quads_survive_the_prefilter",
        "must_fail": ("test_ladder[w2048-ripple-latency]", "test_ladder[w2048-ripple-throughput]", "test_near_limit_sweep[w2048-"),
        "must_pass": ("test_large_quads_survive_the_prefilter",)},
    # 8: the last wave's totals twice in the chunk carry of the general sweep, k_fit_quads<NT, false> with NT >= 128
    8: {"files": (_HERE,),
        "select": "(test_ladder and not noise) or (test_near_limit_sweep and b0) or (test_giants and (2800 or a1))",
        "must_fail": ("test_ladder[w2049-clean-latency]", "test_ladder[w2049-clean-throughput]", "test_ladder[w2049-ripple-latency]",
                      "test_ladder[w2049-ripple-throughput]", "test_near_limit_sweep[w2049-b0-latency]",
                      "test_near_limit_sweep[w2049-b0-throughput]", "test_giants[2800_global_general-latency]",
                      "test_giants[2800_global_general-throughput]"),
        "must_pass": ("test_ladder[w2048-", "test_near_limit_sweep[w2048-", "test_giants[2048sq_global_split_a1-")},
}


@pytest.mark.parametrize("mutant", sorted(_WRONG_BUILDS))
def test_fit_class_tests_fail_on_the_wrong_builds(built, mutant):
    """libapriltag_amd_mut7.so and _mut8.so (csrc/tools_hooks.h, AMDAT_MUTATE): a selection of this file's cases, in a process of its
    own, must FAIL on the wrong build where its error lives and pass where it does not, and all of it passes on the product library.
    7 lives in the 256- and 1024-thread instances of the two-double sweep: the rippled ladder and the sweep fail 2048 wide, while
    tests/test_gpu_parity.py::test_large_quads_survive_the_prefilter -- whose large quads all sit in the 512-thread class -- still passes:
    the gap these tests close.  8 lives in the general sweep from 128 threads on: every 2049-wide case and the 2800 x 1800 giant fail,
    every 2048-wide case passes."""
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
    for want in spec["must_fail"]:
        assert any(t.startswith(want) for t in failed), (want, failed, passed)
    for want in spec["must_pass"]:
        assert any(t.startswith(want) for t in passed) and not any(t.startswith(want) for t in failed), (want, failed, passed)
    assert "quad" in out.stdout   # the stage that differs: the quad list
    out_ok, passed_ok, failed_ok = run(None)
    assert out_ok.returncode == 0 and not failed_ok and sorted(passed_ok) == sorted(passed + failed), (out_ok.stdout[-1500:], failed_ok)
