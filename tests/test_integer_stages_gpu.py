"""The integer stages -- threshold, connected components, boundary points, cluster selection -- on the frames of tests/stage_frames.py:
every rule of kernels_threshold.h, kernels_cc.h and kernels_cluster.h that shows only at x = 1 or x = W - 2, on a tile border, at a
dilated range of exactly 5, at a component of exactly 25 pixels or at a cluster of exactly 24 points is met here by construction.
Every frame goes through parity_util's comparison -- all stages bit for bit, on both launch sets, alone and in one submission with the
other frames of its size -- and then the census of tests/test_stage_frames_cpu.py is repeated on the library's own debug buffers.
Wrong builds 31 .. 36 (csrc/tools_hooks.h) show that each case fails where its rule is broken."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from isaac_ros_apriltag_amd import capi, synth  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402
import parity_util as pu  # noqa: E402
import stage_frames as sf  # noqa: E402

PATHS = ("latency", "throughput")
FAM = ("tag36h11",)


def _submit(frames, path, tile=4, mode="mono8"):
    """One submission of the equally sized working frames `frames` on launch set `path`: as they stand, pixel-doubled at decimate 2, or
    as bgr8 with three equal channels.  Every stage and record of every frame against the oracle; returns the library's buffers per
    frame (thr, label, csize, clusters, points)."""
    inputs = [sf.decimate2_input(f) for f in frames] if mode == "dec2" else list(frames)
    dec = 2 if mode == "dec2" else 1
    h, w = inputs[0].shape
    K = synth.default_K(w, h)
    det = AprilTagDetector(w, h, families=FAM, decimate=dec, tile_size=tile, intrinsics=(K[0, 0], K[1, 1], K[0, 2], K[1, 2]),
                           max_batch=len(frames))
    try:
        det.set_submission_path(path)
        if mode == "bgr8":
            g = det.detect_batch_ex(torch.from_numpy(np.stack([sf.bgr8_input(f) for f in frames])).cuda(), max_dets=64, encoding="bgr8")
        else:
            g = det.detect_batch_ex(torch.from_numpy(np.stack(inputs)).cuda(), max_dets=64)
        errs, out = [], []
        for i, img in enumerate(inputs):
            e, odets = pu.compare_stages(det, i, img, FAM, K, dec, tile_size=tile)
            e += pu.compare_detections(g[i], odets)
            errs += ["frame %d: %s" % (i, x) for x in e]
            fh, fw = frames[i].shape
            out.append({"thr": det.debug(i, capi.DBG_THRESH).reshape(fh, fw), "label": det.debug(i, capi.DBG_LABEL).reshape(fh, fw),
                        "csize": det.debug(i, capi.DBG_CSIZE).reshape(fh, fw), "clusters": det.debug(i, capi.DBG_CLUSTERS),
                        "points": det.debug(i, capi.DBG_POINTS)})
    finally:
        det.close()
    assert not errs, errs[:4]
    return out


# ---- the census of tests/test_stage_frames_cpu.py, on the library's buffers ---------------------------------------------------------------
def _check_link_atlas(shape, b):
    _, motifs, want = sf.link_atlas(*shape)
    assert np.array_equal(b["thr"][want != 1], want[want != 1])
    for m in motifs:
        both = sf.joined(b["label"], m["a"], m["b"])
        assert both == (m["expect"] != "apart"), m["name"]
        if m["expect"] == "essential":   # on the library's threshold image the pair hangs on that link alone
            assert not sf.joined(sf.components(b["thr"], without=m["link"]), m["a"], m["b"]), m["name"]


def _check_merge_atlas(k, b):
    _, recs, want = sf.merge_atlas(k)
    assert np.array_equal(b["thr"][want != 1], want[want != 1])
    size_at = lambda p: int(b["csize"].reshape(-1)[int(b["label"][p[1], p[0]])])
    if k == 1:
        for r in recs:
            assert sf.joined(b["label"], r["a"], r["b"]) and size_at(r["a"]) == r["size"], r["name"]
        return
    partners = sf.cluster_partners(b["clusters"]["key"])
    for r in recs:
        assert size_at(r["pixel"]) == r["size"], r["name"]
        assert (int(b["label"][r["pixel"][1], r["pixel"][0]]) in partners) == (r["size"] == sf.MIN_COMPONENT), r["name"]
    cen = sf.component_census(b["thr"], b["label"], b["csize"])
    assert all(cen.get((size, spread), 0) >= 1 for size in (24, 25) for spread in ((1, 2, 4) if k == 0 else (1,))), cen


def _check_limit_frame(name, b):
    assert sorted(int(n) for n in b["clusters"]["count"]) == sf.LIMIT_COUNTS[name][0]
    if name.startswith("24_across"):
        c = b["clusters"][0]
        tiles = sf.point_tiles(b["points"][int(c["start"]):int(c["start"]) + int(c["count"])])
        assert len(tiles) == 2 and ({t[0] for t in tiles} == {0, 1} if name.endswith("x64") else {t[1] for t in tiles} == {1, 2}), tiles


def _check_threshold_atlas(name, b):
    h, w, ts = sf.THRESHOLD_FRAMES[name]
    thr, cen = sf.threshold_ref(sf.threshold_atlas(name), ts)
    assert np.array_equal(b["thr"], thr)
    assert cen["tiles_range_4"] >= 1 and cen["tiles_range_5"] >= 1 and cen["px_at_thresh_in_tiles"] >= 1 and cen["px_at_thresh+1_in_tiles"] >= 1
    assert (h % ts == 0 and w % ts == 0) or (cen["px_at_thresh_in_strips"] >= 1 and cen["flat_strip_px"] >= 1)
    assert name != "70x1100" or (cen["halo_essential_x"] >= 1 and cen["halo_essential_y"] >= 1)


# ---- (a) the link atlas --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("shape", sf.LINK_SHAPES + (sf.LINK_INTERIOR_SHAPE,), ids=lambda s: "%dx%d" % s)
def test_link_atlas(built, shape, path):
    """Pairs of blobs joined by one link -- left, up, up-left, up-right -- inside a tile, on a tile-top row, on a tile-left column, at a
    four-tile corner and at x = 1 and x = W - 2 on and off a tile-top row, with the negative twin beside each; 130 x 130, and with the
    last row / column a tile of its own.  40 x 130 holds the tile-interior motifs alone."""
    _check_link_atlas(shape, _submit([sf.link_atlas(*shape)[0]], path)[0])


# ---- (b) the merge atlas, and the 130 x 130 frames of (a) and (b) in one submission -------------------------------------------------------------
_MERGE = {"split": 0, "chains": 1, "one_tile": 2}


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which", sorted(_MERGE))
def test_merge_atlas(built, which, path):
    """split: components of exactly 24 and 25 pixels inside one tile and over two and four -- the 25s bound a kept cluster, the 24s
    none.  chains: serpentines across seven tile borders in sequence and a comb joined in the last row of the tile below.  one_tile: the
    24s and 25s that lie inside one tile, alone."""
    _check_merge_atlas(_MERGE[which], _submit([sf.merge_atlas(_MERGE[which])[0]], path)[0])


@pytest.mark.parametrize("path", PATHS)
def test_130x130_frames_in_one_submission(built, path):
    res = _submit([sf.link_atlas(130, 130)[0]] + [sf.merge_atlas(k)[0] for k in (0, 1, 2)], path)
    _check_link_atlas((130, 130), res[0])
    for k in (0, 1, 2):
        _check_merge_atlas(k, res[1 + k])


# ---- (c) the cluster-limit frames ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("name", sorted(sf.LIMIT_FRAMES))
def test_limit_frames(built, name, path):
    """72 x 40, dark rectangles in the frame's corners: clusters of exactly 24 and 25 points (23 is dropped), one of 24 points across
    k_points' tile border x = 64 and one across y = 32; 25_25 holds nothing at the limit."""
    _check_limit_frame(name, _submit([sf.limit_frame(sf.LIMIT_FRAMES[name])], path)[0])


@pytest.mark.parametrize("path", PATHS)
def test_limit_frames_in_one_submission(built, path):
    names = sorted(sf.LIMIT_FRAMES)
    for name, b in zip(names, _submit([sf.limit_frame(sf.LIMIT_FRAMES[n]) for n in names], path)):
        _check_limit_frame(name, b)


# ---- (d) the emission atlas ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_emission_atlas(built, path):
    """200 x 50: the suppressed (-1, 1) emission on x % 64 == 0 in interior and edge tiles of k_points, at x = 2, in rows 1 and H - 2;
    kept at x = 1 (column 0 is no source) and beside a left neighbour without a class."""
    b = _submit([sf.emission_atlas()], path)[0]
    cen = sf.emission_census(b["thr"], b["label"], b["csize"])
    assert all(v >= 1 for v in cen.values()), cen


# ---- (e) the threshold atlas ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("mode", ("mono8", "dec2", "bgr8"))
@pytest.mark.parametrize("name", sorted(sf.THRESHOLD_FRAMES))
def test_threshold_atlas(built, name, mode, path):
    """Dilated ranges of exactly 4 and 5, pixels at thresh and thresh + 1, ranges that reach 5 only through the halo across x = 1024 and
    y = 32, clamped corners, flat and probing ragged strips; also as the decimation of the pixel-doubled frame and as bgr8 with equal
    channels (the same working image, so the same truth).  The tile-8 frame takes the two-pass kernels."""
    h, w, ts = sf.THRESHOLD_FRAMES[name]
    _check_threshold_atlas(name, _submit([sf.threshold_atlas(name)], path, tile=ts, mode=mode)[0])


# ---- six wrong builds -----------------------------------------------------------------------------------------------------------------------------
_WRONG_BUILDS = {
    # 31: the one-pass threshold's low-contrast rule with <=; the tile-8 frame takes other kernels
    31: {"select": "test_threshold_atlas and mono8", "stage": "thresh",
         "must_fail": ("test_threshold_atlas[36x68-", "test_threshold_atlas[37x70-", "test_threshold_atlas[70x1100-mono8-"),
         "must_pass": ("test_threshold_atlas[70x1100_tile8-",)},
    # 32: k_threshold_leftover with >=; 36 x 68 has no strips
    32: {"select": "test_threshold_atlas and (37x70 or 36x68)", "stage": "thresh",
         "must_fail": ("test_threshold_atlas[37x70-mono8-", "test_threshold_atlas[37x70-dec2-", "test_threshold_atlas[37x70-bgr8-"),
         "must_pass": ("test_threshold_atlas[36x68-mono8-", "test_threshold_atlas[36x68-dec2-", "test_threshold_atlas[36x68-bgr8-")},
    # 33: the up link's skip rule of cc_row_requests without left_src; 40 x 130 has no tile-top row
    33: {"select": "test_link_atlas", "stage": "label",
         "must_fail": ("test_link_atlas[130x130-", "test_link_atlas[129x130-", "test_link_atlas[130x129-"),
         "must_pass": ("test_link_atlas[40x130-",)},
    # 34: k_cc_resolve with >; the one-tile 25s have their bit from k_cc_local
    34: {"select": "test_merge_atlas", "stage": "clusters",
         "must_fail": ("test_merge_atlas[split-",), "must_pass": ("test_merge_atlas[one_tile-", "test_merge_atlas[chains-")},
    # 35: k_points' general form with column 0 taken for a source; 40 x 130 has no edge that reaches x = 1
    35: {"select": "test_emission_atlas or (test_link_atlas and 40x130)", "stage": "clusters",
         "must_fail": ("test_emission_atlas[",), "must_pass": ("test_link_atlas[40x130-",)},
    # 36: k_cluster_select with >; 25_25 has no cluster of 24
    36: {"select": "test_limit_frames and not submission", "stage": "clusters",
         "must_fail": ("test_limit_frames[23_24_25-", "test_limit_frames[24_24_24_25-", "test_limit_frames[24_across_x64-",
                       "test_limit_frames[24_across_y32-"),
         "must_pass": ("test_limit_frames[25_25-",)},
}


@pytest.mark.parametrize("mutant", sorted(_WRONG_BUILDS))
def test_integer_stage_tests_fail_on_the_wrong_builds(built, mutant):
    """libapriltag_amd_mut31.so .. _mut36.so (csrc/tools_hooks.h, AMDAT_MUTATE): a narrow selection of this file's cases, in a process of
    its own, must FAIL on the wrong build where its error lives -- with the stage that differs named -- and pass on the twin where it
    cannot show; all of it passes on the product library."""
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
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", os.path.basename(__file__)),
                              "-m", "gpu", "-q", "-rA", "-p", "no:cacheprovider", "-k", spec["select"]],
                             capture_output=True, text=True, timeout=600, cwd=root, env=env)
        ids = lambda word: sorted(l.split("::", 1)[1].split(" ")[0] for l in out.stdout.splitlines() if l.startswith(word + " ") and "::" in l)
        return out, ids("PASSED"), ids("FAILED")
    out, passed, failed = run("mut%d" % mutant)
    assert out.returncode == 1, (out.stdout[-1500:], out.stderr[-1500:])
    for want in spec["must_fail"]:
        assert any(t.startswith(want) for t in failed), (want, failed, passed)
    for want in spec["must_pass"]:
        assert any(t.startswith(want) for t in passed) and not any(t.startswith(want) for t in failed), (want, failed, passed)
    assert "%s: " % spec["stage"] in out.stdout   # the stage that differs
    out_ok, passed_ok, failed_ok = run(None)
    assert out_ok.returncode == 0 and not failed_ok and sorted(passed_ok) == sorted(passed + failed), (out_ok.stdout[-1500:], failed_ok)
