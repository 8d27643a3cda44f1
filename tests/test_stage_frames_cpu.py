"""The frames of tests/stage_frames.py on the oracle alone: every condition tests/test_integer_stages_gpu.py relies on -- a motif
hangs on the one link it was built for, a component has exactly 24 or 25 pixels over the tiles it was split over, a cluster exactly 23,
24 or 25 points, a tile a dilated range of exactly 4 or 5 -- holds for the reference before the library sees a frame.  No tolerance
anywhere: a later edit of a frame cannot hollow a case out unnoticed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

from oracle import pyoracle as po  # noqa: E402
import stage_frames as sf  # noqa: E402


def _dump(img, **params):
    return po.detect(img, params=po.default_params(**params), want_dump=True)[1]


# ---- (a) --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sf.LINK_SHAPES, ids=lambda s: "%dx%d" % s)
def test_link_atlas_every_motif_hangs_on_its_link(built, shape):
    img, motifs, want = sf.link_atlas(*shape)
    thr = po.threshold(img)
    assert np.array_equal(thr[want != 1], want[want != 1])            # the threshold returns the drawn pattern wherever a motif was drawn
    label, _ = po.connected_components(thr)
    lab = sf.components(thr)
    assert np.array_equal(lab[thr != 127], label[thr != 127])        # the census' union-find IS the oracle's link set
    n = {"essential": 0, "apart": 0, "joined": 0}
    for m in motifs:
        both = sf.joined(label, m["a"], m["b"])
        assert thr[m["a"][1], m["a"][0]] == m["cls"] and thr[m["b"][1], m["b"][0]] == m["cls"], m["name"]
        if m["expect"] == "essential":
            assert both and not sf.joined(sf.components(thr, without=m["link"]), m["a"], m["b"]), m["name"]
        elif m["expect"] == "joined":
            assert both, m["name"]
        else:
            assert not both, m["name"]
            if "gap" in m:
                assert thr[m["gap"][1], m["gap"][0]] == 127, m["name"]
        n[m["expect"]] += 1
    where = {m["where"] for m in motifs if m["expect"] == "essential"}
    assert where >= {"interior", "row", "col", "corner", "x1", "x1row", "xW-2", "xW-2row"}, where
    assert n["essential"] >= 20 and n["apart"] >= 7 and n["joined"] >= 3, n
    # both classes on the links both have, white on the diagonals
    for kind in sf.LINKS:
        classes = {m["cls"] for m in motifs if m["expect"] == "essential" and m["link"][2] == kind}
        assert classes == ({0, 255} if kind in ("left", "up") else {255}), (kind, classes)


def test_link_atlas_interior_twin(built):
    """40 x 130: the tile-interior motifs alone; no tile-top row, and no black / white edge that reaches x = 1."""
    img, motifs, want = sf.link_atlas(*sf.LINK_INTERIOR_SHAPE)
    d = _dump(img)
    assert np.array_equal(d["thr"][want != 1], want[want != 1]) and {m["where"] for m in motifs} == {"interior"}
    for m in motifs:
        assert sf.joined(d["label"], m["a"], m["b"]) == (m["expect"] != "apart"), m["name"]
    assert sf.emission_census(d["thr"], d["label"], d["csize"])["x1_kept"] == 0


# ---- (b) --------------------------------------------------------------------------------------------------------------------------------
def test_merge_atlas_sizes_and_spreads(built):
    img, recs, want = sf.merge_atlas(0)
    d = _dump(img)
    assert np.array_equal(d["thr"][want != 1], want[want != 1])
    partners = sf.cluster_partners([c[0] for c in d["clusters"]])
    for r in recs:
        rep = int(d["label"][r["pixel"][1], r["pixel"][0]])
        assert int(d["csize"].reshape(-1)[rep]) == r["size"], r["name"]
        tiles = {(y // sf.CC_T, x // sf.CC_T) for y, x in np.argwhere(d["label"] == rep)}
        assert len(tiles) == r["spread"], r["name"]
        if r["spread"] > 1:   # no tile holds 25 of its pixels: only the pass over the merged roots can call it large
            assert max(int((d["label"][ty * 64:ty * 64 + 64, tx * 64:tx * 64 + 64] == rep).sum()) for ty, tx in tiles) <= 13
        assert (rep in partners) == (r["size"] == sf.MIN_COMPONENT), r["name"]   # the 25s bound a kept cluster, the 24s none
    cen = sf.component_census(d["thr"], d["label"], d["csize"])
    for size in (24, 25):
        for spread in (1, 2, 4):
            assert cen.get((size, spread), 0) >= 1, cen


def test_merge_atlas_one_tile_twin(built):
    """Frame 2: the 24s and 25s inside one tile; no component of exactly 25 pixels lies in more than one tile (nor in frame 1)."""
    img, recs, _ = sf.merge_atlas(2)
    d = _dump(img)
    cen = sf.component_census(d["thr"], d["label"], d["csize"])
    assert cen.get((24, 1), 0) >= 2 and cen.get((25, 1), 0) >= 2 and not [k for k in cen if k[0] == 25 and k[1] > 1], cen
    d1 = _dump(sf.merge_atlas(1)[0])
    assert not [k for k in sf.component_census(d1["thr"], d1["label"], d1["csize"]) if k[0] == 25 and k[1] > 1]


def test_merge_atlas_serpentines_and_comb(built):
    img, recs, want = sf.merge_atlas(1)
    d = _dump(img)
    assert np.array_equal(d["thr"][want != 1], want[want != 1])
    assert {r["cls"] for r in recs if "serpentine" in r["name"]} == {0, 255}
    for r in recs:
        rep = int(d["label"][r["a"][1], r["a"][0]])
        assert sf.joined(d["label"], r["a"], r["b"]) and int(d["csize"].reshape(-1)[rep]) == r["size"], r["name"]
        ys, xs = np.nonzero(d["label"] == rep)
        tiles = {(y // sf.CC_T, x // sf.CC_T) for y, x in zip(ys, xs)}
        assert len(tiles) >= 2 and r["crossings"] >= 6, r["name"]
    comb = recs[-1]
    rep = int(d["label"][comb["a"][1], comb["a"][0]])
    upper = d["label"][:64] == rep   # above y = 64 the teeth are 24 pixels each and apart
    assert int(upper.sum()) == 24 * comb["crossings"] and not upper[:, 81::2][:, :5].any()


# ---- (c) --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sf.LIMIT_FRAMES))
def test_limit_frames_cluster_counts(built, name):
    img = sf.limit_frame(sf.LIMIT_FRAMES[name])
    default, loose = sf.LIMIT_COUNTS[name]
    d = _dump(img)
    assert sorted(c[2] for c in d["clusters"]) == default
    assert sorted(c[2] for c in _dump(img, min_cluster_points=1)["clusters"]) == loose
    if name.startswith("24_across"):
        (_, start, n), = d["clusters"]
        tiles = sf.point_tiles(d["points"][start:start + n])
        assert len(tiles) == 2 and ({t[0] for t in tiles} == {0, 1} if name.endswith("x64") else {t[1] for t in tiles} == {1, 2}), tiles


def test_limit_frames_hold_23_24_and_25(built):
    default = [n for v in sf.LIMIT_COUNTS.values() for n in v[0]]
    loose = [n for v in sf.LIMIT_COUNTS.values() for n in v[1]]
    assert 24 in default and 25 in default and 23 not in default and 23 in loose
    assert 24 not in sf.LIMIT_COUNTS["25_25"][1]   # the twin: nothing at the limit


# ---- (d) --------------------------------------------------------------------------------------------------------------------------------
def test_emission_atlas_meets_every_position_class(built):
    d = _dump(sf.emission_atlas())
    cen = sf.emission_census(d["thr"], d["label"], d["csize"])
    assert all(v >= 1 for v in cen.values()), cen
    assert len(d["clusters"]) >= 6


# ---- (e) --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sf.THRESHOLD_FRAMES))
def test_threshold_atlas_census(built, name):
    h, w, ts = sf.THRESHOLD_FRAMES[name]
    g = sf.threshold_atlas(name)
    assert g.shape == (h, w)
    thr, cen = sf.threshold_ref(g, ts)
    assert np.array_equal(po.threshold(g, ts), thr)
    need = ["tiles_range_4", "tiles_range_5", "tiles_range_even", "tiles_range_odd", "px_at_thresh_in_tiles", "px_at_thresh+1_in_tiles"]
    if h % ts or w % ts:
        need += ["px_at_thresh_in_strips", "px_at_thresh+1_in_strips", "flat_strip_px"]
    if name == "70x1100":
        need += ["halo_essential_x", "halo_essential_y"]
    assert all(cen[k] >= 1 for k in need), cen
    assert cen["corner_tiles_live"] == 4 and cen["flat_strip_px_not_0"] == 0, cen
    # the other two ways in: decimate 2 of the pixel-doubled frame is the frame; three equal channels give the same gray value
    assert np.array_equal(po.decimate(sf.decimate2_input(g), 2), g)
    b = sf.bgr8_input(g).astype(np.int64)
    assert np.array_equal((4899 * b[..., 2] + 9617 * b[..., 1] + 1868 * b[..., 0] + 8192) >> 14, g)


def test_wrong_builds_31_to_36_are_registered():
    from isaac_ros_apriltag_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hooks = open(os.path.join(root, "isaac_ros_apriltag_amd", "csrc", "tools_hooks.h")).read()
    for n in range(31, 37):
        assert n in build.MUTANTS and "AMDAT_MUTATE == %d" % n in hooks
