"""Host checks of tests/fit_frames.py: its class bounds against the launch plan's, and every census condition of
tests/test_fit_classes_gpu.py on the CPU oracle alone -- which cluster sizes of each frame end in a quad, hence which kernel instance
and sort form a bit-exact comparison of that frame can bite on.  No GPU."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import fit_frames as ff  # noqa: E402
import parity_util as pu  # noqa: E402
import test_launch_plan_cpu as lp  # noqa: E402

from isaac_ros_apriltag_amd import synth  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

FAM = ("tag36h11",)


def _oracle(img):
    h, w = img.shape
    return po.detect(img, families=FAM, params=pu.oracle_params(synth.default_K(w, h)), want_dump=True)[1]


# ---- the census's literals against launch_plan.h ----------------------------------------------------------------------------------------
def test_class_bounds_equal_the_launch_plans(tmp_path):
    exe = str(tmp_path / "launch_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", os.path.join(lp.HERE, "aux_c", "launch_plan_driver.cpp"), "-o", exe])
    sizes = [(1920, 1080), (2048, ff.LADDER_H), (2049, ff.LADDER_H), (2048, 2048), (2800, 1800), (640, 480)]
    lines = "".join("classes %d %d 256 8\n" % ff.handle(w, h) for w, h in sizes)
    out = subprocess.run([exe], input=lines, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    for (w, h), line in zip(sizes, out):
        assert ff.handle(w, h) == lp.handle(w, h)
        rows = [tuple(map(int, r.split())) for r in line.split("|")[0].split(";") if r.strip()]   # nt, sort_cap, lo, hi, grid, slot_cap, pop, kernel
        split = ff.handle(w, h)[1]
        assert ff.has_fit_small(w, h, "throughput") == bool(split) and not ff.has_fit_small(w, h, "latency")
        # class 0 is k_fit_small's where the handle sums in two doubles (and empty otherwise: the one-wave class then starts at 0)
        assert rows[0][2:4] == (0, ff.FIT_SMALL_HI if split else 0) and rows[0][7] == lp.SMALL and rows[1][7] == lp.EMPTY
        quads = rows[2:]
        assert len(quads) == ff.NCLASSES - 1 and all(r[7] == lp.QUADS for r in quads)
        assert [r[0] for r in quads] == list(ff.CLASS_NT[1:])
        assert [r[3] for r in quads[:-1]] == list(ff.CLASS_HI[1:]) and quads[-1][3] == 0x7FFFFFFF
        assert [r[2] for r in quads] == [ff.CLASS_HI[0] if split else 0] + list(ff.CLASS_HI[1:])
        # LDS key arrays: the class's bound (always a power of two from 128 threads on: padded), the largest class's raised or not
        assert [r[1] for r in quads[:-1]] == list(ff.CLASS_HI[1:]) and quads[-1][1] == ff.sort_cap(w, h)
    assert ff.sort_cap(1920, 1080) == 18048 and ff.sort_cap(2048, 2048) == ff.sort_cap(2800, 1800) == ff.sort_cap(640, 480) == 16384


def test_sort_forms_at_their_bounds():
    form = lambda n, **kw: ff.sort_form(n, **kw)
    assert [form(n) for n in (24, 64, 65, 128, 129, 256, 257, 512, 513, 768)] == [
        "reg1", "reg1", "reg2", "reg2", "reg4", "reg4", "lds_padded", "lds_padded", "lds_unpadded", "lds_unpadded"]
    assert [form(n, fit_small=True) for n in (24, 128, 129)] == ["fit_small", "fit_small", "reg4"]
    assert {form(n) for n in (769, 2048, 2049, 4096, 4097, 8192, 8193, 16384)} == {"lds_padded"}
    assert form(16385) == "global" and form(16385, cap=18048) == form(18048, cap=18048) == "lds_unpadded" and form(18049, cap=18048) == "global"
    assert [ff.size_class(n) for n in (24, 128, 129, 768, 769, 2048, 2049, 4096, 4097, 8192, 8193, 40000)] == [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5]


def test_census_maps_quads_to_their_clusters():
    kept, dropped = ff.census(([11, 12, 13, 14], [30, 600, 5000, 17000]), [13, 11, 14])
    assert kept == [(30, 0, "reg1"), (5000, 4, "lds_padded"), (17000, 5, "global")] and dropped == [600]
    assert ff.census(([11, 14], [30, 17000]), [11, 14], 18048, True)[0] == [(30, 0, "fit_small"), (17000, 5, "lds_unpadded")]
    with pytest.raises(AssertionError):
        ff.census(([11], [30]), [12])   # a quad without its cluster


def test_bounding_box_render_equals_whole_frame_arithmetic():
    """The renderer against the formula written out over the whole frame, on rotated, rippled, nested and frame-cut rectangles."""
    w, h = 300, 200
    rects = [(150, 100, 120, 70, 0.3, ff.D, 3.0, 17.0), (150, 100, 60, 40, -0.2, ff.L, 2.0, 11.0), (280, 190, 30, 20, 0.7, ff.D, 1.0, 9.0),
             (20.5, 30.25, 3.2, 3.2, 0.1, ff.D, 0, 37.0)]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full((h, w), float(ff.L))
    for cx, cy, hw, hh, ang, val, amp, per in rects:
        c, s = np.cos(ang), np.sin(ang)
        u, v = (xx - cx) * c + (yy - cy) * s, -(xx - cx) * s + (yy - cy) * c
        img[(np.abs(u) < hw + amp * np.sin(2 * np.pi * v / per)) & (np.abs(v) < hh + amp * np.sin(2 * np.pi * u / per + 1.0))] = val
    assert np.array_equal(ff.render(w, h, rects), img.astype(np.uint8))
    noisy = np.clip(np.rint(img + np.random.default_rng(5).normal(0, 1.0, (h, w))), 0, 255).astype(np.uint8)
    assert np.array_equal(ff.render(w, h, rects, 1.0, 5), noisy)


# ---- (a) the ladder ---------------------------------------------------------------------------------------------------------------------
CLEAN_COUNTS = [104, 120, 216, 400, 600, 1696, 3392, 4427, 7312, 9368]   # the rectangles' clusters that end in a quad (56 is too small)


@pytest.mark.parametrize("content", sorted(ff.LADDER_CONTENT))
@pytest.mark.parametrize("w", ff.LADDER_WIDTHS)
def test_ladder_census_on_the_oracle(built, w, content):
    a, sigma = ff.LADDER_CONTENT[content]
    img = ff.ladder(w, a, sigma)
    assert img.shape == (ff.LADDER_H, w) and np.array_equal(img[:, :2048], ff.ladder(2048, a, sigma)) == (sigma == 0 or w == 2048)
    kept, dropped = ff.census_oracle(_oracle(img), ff.sort_cap(w, ff.LADDER_H))
    counts = [n for n, _, _ in kept]
    if content == "clean":
        assert [n for n in counts if n > 71] == CLEAN_COUNTS and dropped == [55, 56, 5912, 8152]   # (55: the checkerboard's cut corner cell)
        assert sorted(set(n for n in counts if n <= 71)) == [62, 68, 70, 71]   # the checkerboard's cells, cut and whole
        assert ff.classes_of(kept) == set(range(ff.NCLASSES))
        assert ff.forms_of(kept, 0) == {"reg1", "reg2"} and ff.forms_of(kept, 1) == {"reg4", "lds_padded", "lds_unpadded"}
        assert {c: ff.CLASS_NT[c] for _, c, _ in kept if c >= 3} == {3: 256, 4: 512, 5: 1024}
    elif content == "noise":
        assert set(counts) >= {1696, 3392, 4427, 7312, 9368} and len(kept) > 200 and len(dropped) > 1500
        assert {5912, 8152} <= set(dropped) and sum(1 for n in dropped if n > 2048) >= 8   # noise blobs of the large classes beside them
        assert ff.forms_of(kept, 0) | ff.forms_of(kept, 1) >= set(ff.ONE_WAVE_FORMS[2:])
    else:
        assert {3, 5} <= ff.classes_of(kept) and [n for n in counts if n > 2048] == [4064, 9088]
        assert [n for n in dropped if n > 128] == [4399, 5912, 8152, 12268]


# ---- (b) the near-limit sweep -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sweep_batch(w, batch):
    """(kept, given up) per class among the dark rectangles' clusters of sweep frames 8 batch .. 8 batch + 7."""
    kept, lost = np.zeros(ff.NCLASSES, int), np.zeros(ff.NCLASSES, int)
    for seed in ff.SWEEP_SEEDS[8 * batch:8 * batch + 8]:
        rects = ff.sweep_rects(seed)
        dump = _oracle(ff.sweep_frame(seed, w))
        qk = {q["key"] for q in dump["quads"]}
        for key, count, box in ff.cluster_boxes(dump):
            i = ff.rect_of_box(box, rects, w, ff.LADDER_H)
            assert i is not None, (seed, count, box)
            if rects[i][5] == ff.D:
                (kept if key in qk else lost)[ff.size_class(count)] += 1
    return kept, lost


@pytest.mark.parametrize("batch", range(3))
@pytest.mark.parametrize("w", ff.LADDER_WIDTHS)
def test_sweep_batches_hold_both_kinds_in_every_class(built, w, batch):
    kept, lost = _sweep_batch(w, batch)
    assert (kept[1:] >= 1).all() and (lost[1:] >= 1).all(), (kept, lost)


@pytest.mark.parametrize("w", ff.LADDER_WIDTHS)
def test_sweep_condition_on_the_oracle(built, w):
    """Over the 24 frames, in each of the five k_fit_quads classes: at least 8 dark-on-light clusters that end in a quad and at least 5
    that do not.  As generated: kept 65, 10, 11, 10, 22; given up 7, 10, 9, 22, 26 (the one-wave class counts the two small rectangles
    without a ripple, 48 of its 65)."""
    kept = sum(_sweep_batch(w, b)[0] for b in range(3))
    lost = sum(_sweep_batch(w, b)[1] for b in range(3))
    assert (kept[1:] >= 8).all() and (lost[1:] >= 5).all(), (kept, lost)
    assert kept.tolist() == [48, 65, 10, 11, 10, 22] and lost.tolist() == [24, 7, 10, 9, 22, 26]


# ---- (c) giants ---------------------------------------------------------------------------------------------------------------------------
GIANT_COUNTS = {"1080p_lds_unpadded": 17936, "1080p_above_the_cap": None, "2048sq_global_split_a1": 17032, "2048sq_global_split_a2": 21644,
                "2800_global_general": 17456}


@pytest.mark.parametrize("name", sorted(ff.GIANTS))
def test_giants_on_the_oracle(built, name):
    w, h, _, _, _, _, _, (lo, hi), quad = ff.GIANTS[name]
    dump = _oracle(ff.giant(name))
    kept, dropped = ff.census_oracle(dump, ff.sort_cap(w, h))
    if not quad:
        assert dump["clusters"] == [] and kept == [] and ff.handle(w, h)[0] == 18000
        return
    n = GIANT_COUNTS[name]
    assert lo <= n <= hi and hi <= ff.handle(w, h)[0]
    assert kept == [(n, 5, "lds_unpadded" if name.startswith("1080p") else "global")] and dropped == []
    assert ff.handle(w, h)[1] == (0 if name.startswith("2800") else 1)


# ---- the two wrong builds of tests/test_fit_classes_gpu.py ----------------------------------------------------------------------------------
def test_wrong_builds_are_in_the_mutant_list():
    from isaac_ros_apriltag_amd import build
    root = os.path.dirname(lp.HERE)
    hooks = open(os.path.join(root, "isaac_ros_apriltag_amd", "csrc", "tools_hooks.h")).read()
    for n in (7, 8):
        assert n in build.MUTANTS and build.lib_mutant(n).endswith("libapriltag_amd_mut%d.so" % n)
        assert "AMDAT_MUTATE == %d" % n in hooks
    # what the product build compiles: the limit and the totals themselves
    assert "#define FQ_GROUP_TEST_MSE(NT, mse) (mse)\n" in hooks and "#define FQ_CARRY_LAST_WAVE(t) (t)\n" in hooks
