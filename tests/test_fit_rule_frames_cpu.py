"""The frames of tests/fit_rule_frames.py on the oracle alone: every condition tests/test_fit_rules_gpu.py relies on -- this cluster
leaves at the box test, that one by the winding term alone, a third is kept with a Heron area between 0.95 w^2 and w^2 or with its
weakest corner at rank exactly 10 -- holds for the reference, read from its per-cluster fit log, before the library sees a frame.  The
cluster sizes and exit reasons are written out per frame: a later edit of a frame cannot hollow a case out unnoticed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

from oracle import pyoracle as po  # noqa: E402
import fit_frames as ff  # noqa: E402
import fit_rule_frames as fr  # noqa: E402

# frame -> sorted (points, exit reason as ato_stats numbers it: pyoracle.FIT_REASONS) of every cluster that enters the fit
EXPECT = {
    "area_dec2": [(40, 10), (56, 10), (56, 10), (56, 10)],
    "area_tag16h5_above": [(56, 8), (56, 8), (56, 10)],
    "area_tag16h5_window": [(48, 10), (48, 10), (56, 8), (56, 8)],
    "area_tag25h9_above": [(56, 10), (64, 8), (72, 8)],
    "area_tag25h9_window": [(64, 8), (64, 10), (72, 8), (76, 10)],
    "area_tag36h11_above": [(64, 8), (80, 8), (84, 10)],
    "area_tag36h11_window": [(64, 8), (64, 10), (80, 8), (88, 10)],
    "border_reversed_only": [(208, 1), (208, 10), (232, 10), (240, 1), (712, 1)],
    "border_tag36h11": [(208, 1), (208, 10), (232, 1), (240, 10), (712, 10)],
    # (the 17 small clusters: pixels the seeded noise flips in the band along the rhombus' sides)
    "cut_lds": [(24, 1), (24, 3), (31, 1), (31, 1), (31, 1), (31, 1), (31, 1), (31, 8), (31, 8), (31, 8), (32, 8), (32, 8), (32, 8), (32, 8),
                (32, 8), (32, 8), (38, 1), (6278, 10)],
    "cut_lds_wide": [(24, 1), (24, 3), (31, 1), (31, 1), (31, 1), (31, 1), (31, 1), (31, 8), (31, 8), (31, 8), (32, 8), (32, 8), (32, 8),
                     (32, 8), (32, 8), (32, 8), (38, 1), (6278, 10)],
    "cut_regs": [(2750, 10)],
    "cut_regs_wide": [(2750, 10)],
    "cut_small": [(102, 10)],
    "cut_wave": [(752, 10)],
    "cuttwin_lds": [(30, 1), (30, 1), (30, 1), (31, 1), (31, 1), (32, 8), (32, 8), (32, 8), (33, 1), (41, 8), (45, 1), (6278, 10)],
    "cuttwin_lds_wide": [(30, 1), (30, 1), (30, 1), (31, 1), (31, 1), (32, 8), (32, 8), (32, 8), (33, 1), (41, 8), (45, 1), (6278, 10)],
    "cuttwin_regs": [(2510, 10)],
    "cuttwin_regs_wide": [(2510, 10)],
    "cuttwin_small": [(126, 10)],
    "exits_darts": [(543, 9), (543, 9), (543, 9), (543, 9)],
    "exits_edges": [(64, 4), (72, 3), (84, 7), (88, 3), (208, 4), (444, 0)],
    "exits_kites_dropped": [(800, 9), (812, 9), (828, 9), (836, 9), (844, 9)],
    "exits_kites_kept": [(852, 10), (860, 10), (868, 10), (884, 10)],
    "exits_rhombi_a": [(720, 9), (728, 4), (736, 4), (752, 4), (752, 9)],
    "exits_rhombi_b": [(760, 10), (760, 10), (768, 10), (776, 10), (784, 10)],
    "exits_shallow_3": [(856, 9)],
    "exits_shallow_5": [(835, 9)],
    "exits_shallow_7": [(860, 10)],
}
MIN_TAG_WIDTH = {"tag36h11": 8, "tag25h9": 7, "tag16h5": 6}


def _kinds(name, w=8):
    return [fr.kinds(r, w) for r in fr.census(name)[1]]


def _count(name, kind, w=8):
    return sum(kind in k for k in _kinds(name, w))


def test_every_frame_has_its_census(built):
    assert sorted(EXPECT) == sorted(fr.FRAMES)
    got = {n: fr.census(n)[0] for n in fr.FRAMES}
    assert got == EXPECT, "\n" + fr.table()
    for n in fr.RULE_FRAMES:
        assert max(fr.frame(n).shape) <= 224, n


def test_the_log_changes_no_result(built):
    """The dump with the log on and off, byte for byte, on every frame."""
    for n in sorted(fr.FRAMES):
        fam, dec, _ = fr.FRAMES[n]
        dets, plain = po.detect(fr.frame(n), families=(fr.oracle_family(fam),), params=po.default_params(decimate=dec), want_dump=True)
        logged, _ = fr.oracle_run(n)
        assert sorted(plain) == sorted(logged)
        for k in plain:
            if k == "quads":
                assert [(q["key"], q["reversed_border"], q["p"].tobytes()) for q in plain[k]] == \
                       [(q["key"], q["reversed_border"], q["p"].tobytes()) for q in logged[k]], n
            elif isinstance(plain[k], np.ndarray):
                assert plain[k].tobytes() == logged[k].tobytes(), (n, k)
            else:
                assert plain[k] == logged[k], (n, k)


def test_the_log_agrees_with_the_counters(built):
    """One record per cluster and reason, as ato_stats counts them; on sigma-1 noise, where most exits occur."""
    import ctypes as C
    img = ff.render(320, 240, [(100, 120, 60, 40, 0.2, ff.D, 2, 23), (250, 100, 20, 20, 0.1, ff.D, 0, 9)], sigma=1.0)
    stats = (C.c_longlong * 32).in_dll(po.lib(), "ato_stats")
    before = list(stats)
    _, dump, log = po.detect(img, want_dump=True, want_fit_log=True)
    by = np.bincount(log["reason"], minlength=11)
    assert [stats[r] - before[r] for r in range(11)] == by.tolist() and len(log) == len(dump["clusters"]) > 50
    assert [int(k) for k in log["key"]] == [c[0] for c in dump["clusters"]] and [int(c) for c in log["points_in"]] == [c[2] for c in dump["clusters"]]
    assert sorted(int(k) for k in log["key"][log["reason"] == 10]) == [q["key"] for q in dump["quads"]]


def test_exits_atlas(built):
    _, log = fr.census("exits_edges")
    by = {int(r["points_in"]): r for r in log}
    assert by[444]["reason"] == 0                                                    # the straight edge: box
    assert by[84]["reason"] == 7 and by[84]["min_abs_det"] < 0.001                   # the square cut by the frame's corner
    assert by[72]["reason"] == 3 and by[72]["nmaxima"] == 2 and by[88]["reason"] == 3   # fewer than four maxima
    assert by[64]["reason"] == 4 and by[64]["nmaxima"] == 4 and by[208]["nmaxima"] == 13   # four maxima and more, no admissible choice
    # darts at four turns: the winding term alone, |cos| well inside the limit
    assert _count("exits_darts", "winding_alone") == 4
    assert all(r["winding_fails"] == 1 and r["max_abs_cos"] < 0.9 for r in fr.census("exits_darts")[1])
    # rhombi of 6 .. 14 degrees: every one of 10.5 and more is kept with |cos| above 0.95; the sharper ones leave at the corner search
    # or with BOTH angle tests failed (the two angles of a rhombus add up to 180 degrees), the 9-degree one with the winding term too
    assert _count("exits_rhombi_b", "kept_cos_above_0.95") == 5 and _count("exits_rhombi_a", "kept") == 0
    assert _count("exits_rhombi_a", "cos_both") == 1 and _count("exits_rhombi_a", "cos_below_alone") == 0
    # kites: the tip alone is sharp.  6 .. 9.5 degrees leave by cos < -cos_critical alone, 10.5 .. 13 are kept above 0.95
    assert _count("exits_kites_dropped", "cos_below_alone") == len(fr.KITE_DROPPED_DEG) == 5
    assert _count("exits_kites_kept", "kept_cos_above_0.95") == len(fr.KITE_KEPT_DEG) == 4
    # shallow vertices: cos > +cos_critical alone at 3 and 5 pixels, kept at 7
    assert _count("exits_shallow_3", "cos_above_alone") == 1 and _count("exits_shallow_5", "cos_above_alone") == 1
    assert _count("exits_shallow_7", "kept_cos_above_0.95") == 1
    # the steps of the angle scan
    assert max(np.diff(sorted(set(fr.RHOMBUS_DEG) | {10.5} | set(fr.KITE_DROPPED_DEG) | set(fr.KITE_KEPT_DEG)))) <= 1.0


@pytest.mark.parametrize("fam", sorted(fr.AREA))
def test_area_atlas(built, fam):
    w = fr.AREA[fam][0]
    assert w == MIN_TAG_WIDTH[fam]
    win, above = "area_%s_window" % fam, "area_%s_above" % fam
    assert _count(win, "kept_under_w2", w) == 2 and _count(win, "dropped_by_area", w) == 2 and _count(win, "kept", w) == 2
    assert _count(above, "kept_under_w2", w) == 0 and _count(above, "kept", w) == 1 and _count(above, "dropped_by_area", w) == 2
    for r in fr.census(above)[1]:
        assert r["reason"] != 10 or r["area"] >= w * w
    for n in (win, above):
        for r in fr.census(n)[1]:
            assert (r["reason"] == 8) == (r["area"] < 0.95 * w * w) and abs(r["area"] - w * w) < 0.1 * w * w


def test_area_rule_cannot_be_met_from_below_at_decimate_2(built):
    cen, log = fr.census("area_dec2")
    assert all(r == 10 for _, r in cen) and log["area"].min() == 25.0 > 0.95 * 4 * 4   # min_tag_width 4; the 10-pixel square's cluster


def test_border_atlas(built):
    """The same frame goes one way on a handle whose only family has a reversed border and the other way under tag36h11."""
    (_, rev), (_, nor) = fr.census("border_reversed_only"), fr.census("border_tag36h11")
    assert [int(k) for k in rev["key"]] == [int(k) for k in nor["key"]]
    assert all((a == 1) != (b == 1) and {int(a), int(b)} == {1, 10} for a, b in zip(rev["reason"], nor["reason"]))
    assert sorted(int(r["points_in"]) for r in rev if r["reason"] == 10) == [208, 232]          # the two light rectangles in the dark field
    assert sorted(int(r["points_in"]) for r in nor if r["reason"] == 10) == [208, 240, 712]


# the cut's site per frame (csrc/kernels_quad.h, kernels_quad_small.h): maxima of the rhombus' cluster -> one per lane up to 64, FQ_SEL_REGS
# = 8 per lane up to 512, the removal rounds in LDS above
CUT_SITE = {"cut_small": (11, 64), "cut_wave": (11, 64), "cut_regs": (65, 512), "cut_regs_wide": (65, 512), "cut_lds": (513, 1 << 20),
            "cut_lds_wide": (513, 1 << 20)}


@pytest.mark.parametrize("name", fr.CUT_FRAMES)
def test_cut_atlas(built, name):
    """One cluster with more than max_nmaxima maxima, kept, the weakest corner of its quad at rank exactly 10 of them: the cut decides."""
    _, log = fr.census(name)
    over = [r for r in log if r["nmaxima"] > 10]
    assert len(over) == 1
    r = over[0]
    lo, hi = CUT_SITE[name]
    assert r["reason"] == 10 and r["weakest_rank"] == 10 and r["nkept"] == 10 and r["nties"] == 1 and lo <= r["nmaxima"] <= hi
    assert "kept_on_rank_10" in fr.kinds(r)
    h, w = fr.frame(name).shape
    if name == "cut_small":
        assert r["points_in"] <= ff.FIT_SMALL_HI and ff.has_fit_small(w, h, "throughput")     # k_fit_small on the throughput set
    if name.startswith("cut_regs"):
        assert r["points_in"] >= 769 and h <= 400 and w in (400, fr.WIDE)
    if name.startswith("cut_lds"):
        assert h <= 900 and w in (900, fr.WIDE)
    if name.endswith("_wide"):
        assert not ff.handle(w, h)[1]                                                         # the 128-bit sweep: k_fit_quads<NT, false>
        a = fr.census(name[:-5])[1]
        a = a[a["nmaxima"] > 10][0]
        assert all(a[f] == r[f] or (a[f] != a[f] and r[f] != r[f]) for f in a.dtype.names if f != "key")


# the twins: (points, maxima, rank of the kept quad's weakest corner) of the one cluster with more than max_nmaxima maxima
CUT_TWIN = {"cuttwin_small": (126, 12, 9), "cuttwin_regs": (2510, 289, 5), "cuttwin_lds": (6278, 765, 9)}
CUT_TWIN_SITE = {"cuttwin_small": (11, 64), "cuttwin_regs": (65, 512), "cuttwin_lds": (513, 1 << 20)}


@pytest.mark.parametrize("name", sorted(CUT_TWIN))
def test_cut_twins(built, name):
    """Where the cut decides the other way, once per site: a kept quad that is NOT the one the search over all maxima chooses -- that
    one has a corner at rank 11 or beyond, which the cut took away (the log repeats the search uncut; fit_rule_frames.uncut_record lifts
    its cap of 48 maxima).  A cut that kept one maximum too many could give that corner back."""
    r = fr.uncut_record(name)
    lo, hi = CUT_TWIN_SITE[name]
    assert (int(r["points_in"]), int(r["nmaxima"]), int(r["weakest_rank"])) == CUT_TWIN[name] and lo <= r["nmaxima"] <= hi
    assert r["reason"] == 10 and r["nkept"] == 10 and r["cut_changes"] == 1 and r["dot_changes"] == 0
    h, w = fr.frame(name).shape
    assert (w, h) == {"cuttwin_small": (80, 80), "cuttwin_regs": (400, 400), "cuttwin_lds": (900, 900)}[name]
    if name != "cuttwin_small":   # 2049 wide: the same record, on the 128-bit sweep
        a, b = [x[x["nmaxima"] > 10][0] for x in (fr.census(name)[1], fr.census(name + "_wide")[1])]
        assert all(a[f] == b[f] or (a[f] != a[f] and b[f] != b[f]) for f in a.dtype.names if f != "key")
        assert not ff.handle(fr.WIDE, h)[1] and [len([x for x in fr.census(n)[1] if x["nmaxima"] > 10]) for n in (name, name + "_wide")] == [1, 1]
    else:
        assert r["points_in"] <= ff.FIT_SMALL_HI


def test_cut_decides_in_the_rank_10_frames_too(built):
    """cut_small's quad is the uncut search's (the cut kept the corner at rank 10); cut_wave's and cut_regs' are not: beside their corner
    at rank 10 the uncut search would take one further down.  So is the 11-degree rhombus of the exits atlas (42 maxima)."""
    assert [int(fr.uncut_record(n)["cut_changes"]) for n in ("cut_small", "cut_wave", "cut_regs")] == [0, 1, 1]
    assert _count("exits_rhombi_b", "kept_cut_decided") == 1


def test_what_the_frames_do_not_reach(built):
    """Over all frames: no cluster loses a point to duplicate removal (gradient_points cannot emit one location twice for one pair of
    components: a pixel's (-1, 1) point is skipped exactly when its left neighbour's (1, 1) point exists), so reason 2 cannot fire; the
    final line mse (6) repeats fits the search already admitted; the total error (5) was not found; no cut meets two maxima at the
    threshold value.  One kept quad is decided by the dot test."""
    logs = np.concatenate([fr.census(n)[1] for n in sorted(fr.FRAMES)])
    by = np.bincount(logs["reason"], minlength=11)
    assert by[6] == 0 and by[2] == 0 and by[5] == 0
    entered = logs[logs["points"] >= 0]
    assert (entered["points"] == entered["points_in"]).all() and len(entered) > 60
    assert logs["nties"].max() == 1
    assert by[[0, 1, 3, 4, 7, 8, 9, 10]].min() >= 1
    # cut_wave's kept quad is decided by the dot test: without it another choice wins (wrong build 45).  With the test as dot >
    # cos_critical_rad, without fabs, no kept quad of any frame changes
    assert _count("cut_wave", "kept_dot_decided") == 1
    assert [int(r["dot_changes"]) for n in ("cut_small", "cut_regs", "cut_lds") for r in fr.census(n)[1] if r["nmaxima"] > 10] == [0, 0, 0]
    assert not (logs["dot_sign_changes"][logs["reason"] == 10] == 1).any()


def test_wrong_builds_37_to_45_are_registered():
    from isaac_ros_apriltag_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hooks = open(os.path.join(root, "isaac_ros_apriltag_amd", "csrc", "tools_hooks.h")).read()
    for n in range(37, 41):
        assert n in build.MUTANTS and "AMDAT_MUTATE == %d" % n in hooks
    assert all(n in build.MUTANTS for n in range(41, 45)) and "AMDAT_MUTATE >= 41 && AMDAT_MUTATE <= 44" in hooks
    assert 45 in build.MUTANTS and "AMDAT_MUTATE == 45" in hooks
    assert build.MUTANT_JOBS <= 16
