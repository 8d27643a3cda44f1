"""Raw formats without a GPU: the reference tests/raw_formats_ref.py stated twice, the properties of the
statement (one pattern shifted, constants, saturation, byte order), the preconditions of the GPU tests on the CPU oracle (every
detection case holds its record; the full-size scene keeps its tags and its corner accuracy through a mosaic), and what the build
left: the C ABI's symbols, the name table, the resources of the new kernels."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

from isaac_ros_apriltag_amd import build as bld, capi, synth  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
import parity_util as pu  # noqa: E402
import raw_formats_cases as cases  # noqa: E402
import raw_formats_ref as rf  # noqa: E402
import rectify_cases as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((2, 2), (3, 2), (7, 5), (16, 9))   # (w, h)


def _noise(w, h, encoding, seed=0):
    rng = np.random.default_rng(100 * w + h + seed)
    return rng.integers(0, 1 << 16, size=(h, w), dtype=np.uint16) if rf.is16(encoding) else rng.integers(0, 256, size=(h, w), dtype=np.uint8)


# ---- the reference, stated twice ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding", rf.ENCODINGS)
def test_two_statements_of_the_reference(encoding):
    for w, h in SHAPES:
        raw = _noise(w, h, encoding)
        for shift in ((0, 3, 4, 8) if rf.is16(encoding) else (8,)):
            a, b = rf.convert(raw, encoding, shift), rf.convert_pixelwise(raw, encoding, shift)
            assert a.dtype == np.uint8 and a.shape == (h, w) and np.array_equal(a, b), (encoding, w, h, shift)


def test_the_four_patterns_are_one_pattern_shifted():
    """ref(raw, rggb) on a frame, against the grbg demosaic of the frame without its first column and the gbrg demosaic of the frame
    without its first row (and bggr without both): equal on the matching pixels, but for the crop's new edge, where the reflect rule
    reads across it."""
    raw = _noise(16, 9, "bayer_rggb8", seed=5)
    full = rf.demosaic_gray(raw, "rggb")
    assert np.array_equal(rf.demosaic_gray(raw[:, 1:], "grbg")[:, 1:], full[:, 2:])
    assert np.array_equal(rf.demosaic_gray(raw[1:, :], "gbrg")[1:, :], full[2:, :])
    assert np.array_equal(rf.demosaic_gray(raw[1:, 1:], "bggr")[1:, 1:], full[2:, 2:])
    # and the crop's own edge does differ somewhere on noise: the exclusion is needed
    assert not np.array_equal(rf.demosaic_gray(raw[:, 1:], "grbg")[:, 0], full[:, 1])
    # a pattern and its mosaic: the sites of a colour carry that colour
    rgb = np.stack([np.full((4, 6), 10), np.full((4, 6), 20), np.full((4, 6), 30)], axis=-1).astype(np.uint8)
    assert rf.mosaic(rgb, "rggb")[:2, :2].tolist() == [[10, 20], [20, 30]] and rf.mosaic(rgb, "grbg")[:2, :2].tolist() == [[20, 10], [30, 20]]
    assert rf.mosaic(rgb, "gbrg")[:2, :2].tolist() == [[20, 30], [10, 20]] and rf.mosaic(rgb, "bggr")[:2, :2].tolist() == [[30, 20], [20, 10]]


def test_constants_saturation_and_byte_order():
    for encoding in rf.ENCODINGS:
        for c in (0, 1, 127, 254, 255):
            if rf.is16(encoding):
                for shift in (0, 4, 8):
                    raw = np.full((5, 7), c << shift, dtype=np.uint16)
                    assert (rf.convert(raw, encoding, shift) == c).all(), (encoding, c, shift)
            else:
                assert (rf.convert(np.full((5, 7), c, dtype=np.uint8), encoding) == c).all(), (encoding, c)
    # saturation: exactly from s = 256 << shift on
    for shift in range(8):   # (at shift 8 no uint16 saturates)
        edge = 256 << shift
        s = np.array([[edge - (1 << shift) - 1, edge - 1, edge, edge + 1, 65535]], dtype=np.uint16)
        assert rf.sample(s, "mono16", shift)[0].tolist() == [254, 255, 255, 255, 255], shift
    assert rf.sample(np.array([[0xFFFF, 0xFEFF]], dtype=np.uint16), "mono16", 8)[0].tolist() == [255, 254]
    assert rf.sample(np.array([[0x0234]], dtype=np.uint16), "mono16", 4)[0, 0] == 0x23
    assert rf.sample(np.array([[0x1234]], dtype=np.uint16), "mono16", 4)[0, 0] == 255   # 0x123 saturates
    # byte order: the low byte comes first
    rows = np.array([[0x34, 0x02, 0xFF, 0x00]], dtype=np.uint8)
    assert rf.samples_from_bytes(rows).tolist() == [[0x0234, 0x00FF]]
    assert rf.convert(rf.samples_from_bytes(rows), "mono16", 8).tolist() == [[0x02, 0x00]]
    assert rf.convert(rf.samples_from_bytes(rows), "mono16", 0).tolist() == [[255, 255]]
    le = np.array([[0x0234, 0x00FF]], dtype="<u2")
    assert np.array_equal(le.view(np.uint8), rows)


# ---- the detection cases hold their record on the oracle ------------------------------------------------------------------------------
def _oracle(img, K, **more):
    return po.detect(np.ascontiguousarray(img), families=cases.FAMILIES, params=pu.oracle_params(K, **more))[0]


@pytest.mark.parametrize("size", range(len(cases.SIZES)))
def test_detection_cases_hold_their_record(built, size):
    w, h = cases.SIZES[size][:2]
    K = cases.K_of(w, h)
    for encoding in rf.ENCODINGS:
        g = cases.tag_ref(size, encoding)
        assert g.shape == (h, w)
        for more in ({}, {"decimate": 2}, {"tile_size": 8}, {"quad_sigma": 0.8}):
            dets = _oracle(g, K, **more)
            assert [(d["id"], d["hamming"]) for d in dets] == [(cases.TAG_ID, 0)], (encoding, size, more, dets)
        if size == 2:   # the composition cases of the GPU tests: resized to 97 x 75, rectified with a mild plumb_bob model, and both
            r = po.rectify_mono8(np.ascontiguousarray(g), *rc.model_a(w, h))
            for img in (po.resize_mono8(np.ascontiguousarray(g), 97, 75), r, po.resize_mono8(r, 97, 75)):
                dets = _oracle(img, cases.K_of(img.shape[1], img.shape[0]))
                assert [(d["id"], d["hamming"]) for d in dets] == [(cases.TAG_ID, 0)], (encoding, img.shape)
    # the patterns see different frames: the planes differ from one another and from the untinted gray
    planes = [cases.tag_ref(size, "bayer_%s8" % p).tobytes() for p in rf.PATTERNS] + [cases.tag_gray(size).tobytes()]
    assert len(set(planes)) == 5


# ---- the full-size scene ----------------------------------------------------------------------------------------------------------------
TINTS = ((100, 85, 60), (100, 100, 100), (60, 85, 100))


@pytest.mark.parametrize("sigma", (0.0, 2.0))
def test_full_size_scene_through_a_mosaic(built, sigma):
    """synth.scene_c2, tinted and mosaiced in the four patterns: the oracle on ref(raw) finds all ten tags, and the median corner
    error against the renderer's truth stays within 0.1 px (measured: see DESIGN.md section 7k; the directly converted colour frame
    gives 0.045 .. 0.062 px)."""
    img, K, truth = synth.scene_c2(sigma=sigma)
    want = {t["id"]: np.asarray(t["p"]) for t in truth}
    for per_cent in TINTS:
        rgb = cases.tint(img, per_cent)
        for pat in rf.PATTERNS:
            g = rf.convert(rf.mosaic(rgb, pat), "bayer_%s8" % pat)
            dets = _oracle(g, K)
            assert sorted(d["id"] for d in dets) == list(range(10)), (per_cent, pat, [d["id"] for d in dets])
            err = np.concatenate([np.linalg.norm(np.asarray(d["p"]) - want[d["id"]], axis=1) for d in dets])
            print("sigma %g tint %s %s: median corner error %.4f px, worst %.3f px" % (sigma, per_cent, pat, np.median(err), err.max()))
            assert np.median(err) <= 0.1, (per_cent, pat, float(np.median(err)))


# ---- what the build left -----------------------------------------------------------------------------------------------------------------
def test_abi_symbols_and_name_table():
    hdr = open(os.path.join(ROOT, "include", "apriltag_amd.h")).read()
    dbg = open(os.path.join(ROOT, "include", "apriltag_amd_debug.h")).read()
    for name, value in capi.ENCODINGS.items():
        assert re.search(r"AMDAT_ENC_%s = %d\b" % (name.upper(), value), hdr), name
    assert [capi.ENCODINGS[e] for e in rf.ENCODINGS] == list(range(5, 14))
    assert re.search(r"AMDAT_DBG_RAW_GRAY = 12\b", dbg) and capi.DBG_RAW_GRAY == 12
    for sym in ("amdAprilTagsConvertRawToMono8", "amdAprilTagsSetRawShift"):
        assert sym in capi.EXPORTS and re.search(r"\b%s\s*\(" % sym, hdr)
    if not os.path.exists(capi.LIB_PATH):
        bld.build_amd()
    L = capi.lib()
    for name, value in capi.ENCODINGS.items():
        assert L.amdAprilTagsEncodingFromName(name.encode()) == value
    for name in ("yuv422", "yuv422_yuy2", "nv12", "mono16 ", "MONO16", "bayer_rggb", "bayer_rggb12", "16UC1", ""):
        assert L.amdAprilTagsEncodingFromName(name.encode()) == -1, name
    assert L.amdAprilTagsSetRawShift(None, 4) == 1   # AMDAT_INVALID_ARGUMENT, before any device call
    assert capi.ENC_SAMPLE_BYTES["mono16"] == 2 and capi.ENC_SAMPLE_BYTES["bayer_grbg8"] == 1 and capi.ENC_CHANNELS["bayer_bggr16"] == 1


def test_raw_kernels_have_no_scratch():
    assert os.path.exists(bld.RESOURCES_AMD), "%s is missing: written by isaac_ros_apriltag_amd.build.build_amd()" % bld.RESOURCES_AMD
    rows = bld.parse_resources(open(bld.RESOURCES_AMD).read())
    raw = {n: r for n, r in rows.items() if n.startswith("k_raw_")}
    assert sorted(raw) == sorted("%s<%d>" % (k, i) for k in ("k_raw_to_mono8", "k_raw_to_mono8_frames") for i in (1, 2, 3)), sorted(raw)
    for n, r in raw.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0 and r["LDS Size"] == 0, (n, r)
    assert set(bld.MUTANTS) >= {49, 50, 51, 52}
