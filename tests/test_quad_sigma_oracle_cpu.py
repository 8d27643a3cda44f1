"""quad_sigma in the oracle (oracle/apriltag_oracle.c: ato_quad_sigma, ato_detect) against the numpy restatement
(tests/quad_sigma_ref.py), all exact: the filtered working image at every decimate and every tap width, the decimate-1 path against
the oracle run on the filtered frame (the method the GPU tests rested on before the oracle had the parameter), and at decimate > 1
the stages through the quads against the oracle on J -- whose records are NOT the detector's, which is why the oracle states
quad_sigma itself (refinement and decode read the untouched full-resolution frame)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import parity_util as pu  # noqa: E402
import quad_sigma_ref as qs  # noqa: E402

from isaac_ros_apriltag_amd import synth  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

STAGES = ("gray", "thr", "label", "csize", "points")


def _oracle(img, K, decimate, sigma=0.0, families=("tag36h11",)):
    return po.detect(np.ascontiguousarray(img), families=families, params=pu.oracle_params(K, decimate, quad_sigma=float(sigma)),
                     want_dump=True)


def _stage_diffs(a, b, stages=STAGES):
    bad = [k for k in stages if not np.array_equal(a[k], b[k])]
    if a["clusters"] != b["clusters"]:
        bad.append("clusters")
    if len(a["quads"]) != len(b["quads"]) or any(
            x["key"] != y["key"] or x["reversed_border"] != y["reversed_border"] or not np.array_equal(x["p"], y["p"])
            for x, y in zip(a["quads"], b["quads"])):
        bad.append("quads")
    return bad


def test_one_sigma_per_half_width():
    for h, s in qs.SIGMA_OF_H.items():
        assert len(qs.taps(s)) == 2 * h + 1 and qs.taps(-s) == qs.taps(s)
    assert len(qs.taps(0.5)) == 3 and len(qs.taps(-4.0)) == 17
    assert sorted({len(qs.taps(s)) // 2 for s in qs.ALL_SIGMAS}) == list(range(1, 9))


def test_filter_function_equals_the_restatement(built):
    """ato_quad_sigma alone (no tile-size floor): every sigma, sizes around ksz on either axis and 1-pixel-wide images."""
    rng = np.random.default_rng(7)
    for s in qs.ALL_SIGMAS + (0.0, 0.3, -0.49):
        ksz = max(len(qs.taps(s)), 1)
        for h, w in ((1, 1), (1, 40), (40, 1), (ksz, ksz), (ksz, ksz + 1), (ksz + 1, ksz), (ksz + 1, ksz + 1), (ksz - 1 or 1, 50),
                     (50, ksz - 1 or 1), (ksz + 2, 2 * ksz + 3), (45, 67)):
            img = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
            assert np.array_equal(po.quad_sigma(img, s), qs.filter_image(img, s)), (s, h, w)
    flat = np.full((30, 30), 255, dtype=np.uint8)   # the largest sums (sum of taps <= 255)
    for s in qs.ALL_SIGMAS:
        assert np.array_equal(po.quad_sigma(flat, s), qs.filter_image(flat, s)), s


@pytest.mark.parametrize("decimate", [1, 2, 3, 4])
def test_oracle_gray_is_the_filtered_working_image(built, decimate):
    """dump["gray"] == filter_image(decimate(img, d), sigma) on ragged noise frames whose WORKING image is ksz, ksz + 1 or below ksz
    wide / high (never below the 4-pixel tile, which the oracle refuses), for one sigma per h = 1 .. 8, both signs, and +-0.5, +-4."""
    rng = np.random.default_rng(100 + decimate)
    n = 0
    for s in qs.ALL_SIGMAS:
        ksz = len(qs.taps(s))
        work = {(max(ksz, 4), 23), (29, max(ksz, 4)), (ksz + 1, ksz + 1), (max(ksz - 1, 4), 41), (37, max(ksz - 2, 4)), (ksz + 1, 58),
                (61, 47)}
        for wk, hk in sorted(work):
            # a full-resolution size whose decimation is wk x hk, ragged: (wk - 1) d + 1 .. wk d
            w = (wk - 1) * decimate + 1 + int(rng.integers(0, decimate))
            h = (hk - 1) * decimate + 1 + int(rng.integers(0, decimate))
            img = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
            _, dump = _oracle(img, synth.default_K(w, h), decimate, s)
            want = qs.filter_image(qs.decimate(img, decimate), s)
            assert dump["gray"].shape == (hk, wk) and np.array_equal(dump["gray"], want), (s, w, h)
            n += 1
    assert n >= 5 * len(qs.ALL_SIGMAS)


def test_identity_values_leave_every_byte(built):
    img, K, _ = synth.scene_c1()
    for d in (1, 2):
        d0, p0 = _oracle(img, K, d)
        for s in (0.0, 0.3, -0.49, 0.4999):
            d1, p1 = _oracle(img, K, d, s)
            assert not _stage_diffs(p0, p1) and not pu.compare_detections(d1, d0, exact=True), (d, s)
    with pytest.raises(RuntimeError):
        _oracle(img, K, 1, float("nan"))


@pytest.mark.parametrize("name", ["c1", "noise", "c2", "c5"])
def test_decimate1_equals_the_oracle_on_the_filtered_frame(built, name):
    """oracle(img, quad_sigma) == oracle(filter_image(img, sigma)) in every stage and every record: the new path agrees with the
    method every decimate-1 test of the filter rests on."""
    fams = ("tag36h11",)
    if name == "c1":
        img, K, _ = synth.scene_c1()
        sigmas = qs.ALL_SIGMAS
    elif name == "noise":
        img = np.random.default_rng(3).integers(0, 256, size=(203, 301), dtype=np.uint8)
        K = synth.default_K(301, 203)
        sigmas = qs.ALL_SIGMAS
    elif name == "c2":
        img, K, _ = synth.scene_c2()
        sigmas = (0.8, 2.7, -1.7)
    else:
        img, K, _ = synth.scene_c5()
        fams = ("tag36h11", "tag25h9")
        sigmas = (1.2, -3.7)
    ndet = 0
    for s in sigmas:
        da, pa = _oracle(img, K, 1, s, fams)
        db, pb = _oracle(qs.filter_image(img, s), K, 1, 0.0, fams)
        assert not _stage_diffs(pa, pb), (s, _stage_diffs(pa, pb))
        assert not pu.compare_detections(da, db, exact=True), s
        ndet += len(da)
    assert ndet > 0 or name == "noise"


@pytest.mark.parametrize("decimate", [2, 3, 4])
def test_decimated_stages_equal_the_oracle_on_J(built, decimate):
    """Decimate > 1: gray and every stage through the quads equal the oracle on J (the frame whose decimation is the filtered working
    image), for every sigma on the 640 x 480 scene and on a noise frame."""
    img1, K1, _ = synth.scene_c1()
    img2 = np.random.default_rng(30 + decimate).integers(0, 256, size=(211, 317), dtype=np.uint8)
    nq = 0
    for img, K in ((img1, K1), (img2, synth.default_K(317, 211))):
        for s in qs.ALL_SIGMAS:
            _, pa = _oracle(img, K, decimate, s)
            J = qs.embed_decimated(img, qs.filter_image(qs.decimate(img, decimate), s), decimate)
            _, pb = _oracle(J, K, decimate)
            assert not _stage_diffs(pa, pb), (s, _stage_diffs(pa, pb))
            nq += len(pa["quads"])
    assert nq > 0


def test_J_cannot_stand_in_for_the_records(built):
    """scene_c2 at decimate 2, sigma 0.8: the oracle on J finds the same ten ids from the same quads, but its corners are not the
    detector's -- J carries filtered samples at every second pixel of every second row, and edge refinement and decode read the
    untouched frame.  The distance is far above rounding (1e-9 px would be): the planes differ.  This is why
    the oracle states quad_sigma itself and the GPU tests compare records against it, not against J."""
    img, K, truth = synth.scene_c2()
    for s in (0.8, -0.8):
        da, pa = _oracle(img, K, 2, s)
        J = qs.embed_decimated(img, qs.filter_image(qs.decimate(img, 2), s), 2)
        db, pb = _oracle(J, K, 2)
        assert not _stage_diffs(pa, pb)
        assert [d["id"] for d in da] == [d["id"] for d in db] and {d["id"] for d in da} == {int(t["id"]) for t in truth}
        assert pu.compare_detections(da, db, exact=True)
        dist = max(float(np.abs(a["p"] - b["p"]).max()) for a, b in zip(da, db))
        print("sigma %r: corners of oracle(J) up to %.3f px from the oracle's" % (s, dist))
        assert dist > 0.01, (s, dist)
    # ... and refinement does move the corners at this setting: switching it off (what the wrong build AMDAT_MUTATE=5 does on the
    # device) changes the records, so a test that compares them sees it
    d0, p0 = po.detect(img, params=pu.oracle_params(K, 2, quad_sigma=0.8, refine_edges=0), want_dump=True)
    d1, _ = _oracle(img, K, 2, 0.8)
    assert [d["id"] for d in d0] == [d["id"] for d in d1] and pu.compare_detections(d0, d1, exact=True)


# (scene, decimate) -> the sigmas at which every tag of the scene is found: the conditions that keep the GPU tests' record comparison
# at decimate > 1 from being vacuous (tests/test_quad_sigma_gpu.py asserts the same counts on the device)
FULL_COUNT = {
    ("c2", 2): (0.8, 1.5, 2.0, 2.7, 3.2, 3.7, 4.0, -0.8, -1.5, -4.0),
    ("c1", 3): (0.8, 1.5, 2.0, 2.7, 3.2, 3.7, -0.8, -1.5, -4.0),
    ("c2", 4): (0.8, 1.5, -0.8, -1.5, -4.0),
}


@pytest.mark.parametrize("name,decimate", sorted(FULL_COUNT))
def test_every_tag_is_found_with_the_filter_on(built, name, decimate):
    img, K, truth = synth.scene_c2() if name == "c2" else synth.scene_c1()
    ids = sorted(int(t["id"]) for t in truth)
    for s in FULL_COUNT[(name, decimate)]:
        dets, _ = _oracle(img, K, decimate, s)
        assert sorted(d["id"] for d in dets) == ids, (s, [d["id"] for d in dets])
