"""quad_sigma on the host: the library's taps against the restatement, the setter's argument checks (no device needed for any of
them), and hand-checked vectors of the restatement itself (tests/quad_sigma_ref.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import quad_sigma_ref as qs  # noqa: E402

from isaac_ros_apriltag_amd import capi  # noqa: E402


def _need_lib():
    if not os.path.exists(capi.LIB_PATH):
        pytest.skip("libapriltag_amd.so not built")


def _sigmas():
    grid = [np.float32(i / 256.0) for i in range(-1024, 1025)]
    edges = []
    for m in range(0, 9):
        v = np.float32(m * 0.5)
        for s in (np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))):
            if abs(s) <= 4:
                edges += [s, -s]
    return grid + edges


def test_library_taps_equal_the_restatement():
    _need_lib()
    for s in _sigmas():
        assert capi.quad_sigma_taps(float(s)) == qs.taps(s), float(s)


def test_documented_taps():
    assert qs.taps(0.5) == [27, 200, 27]
    assert qs.taps(0.8) == [60, 133, 60]
    assert qs.taps(1.0) == [13, 62, 102, 62, 13]
    assert qs.taps(2.0) == [7, 16, 31, 45, 52, 45, 31, 16, 7]
    assert len(qs.taps(4.0)) == 17 and sum(qs.taps(4.0)) == 246
    assert qs.taps(0.0) == [] and qs.taps(0.49) == [] and qs.taps(-0.3) == []
    assert qs.taps(-0.8) == qs.taps(0.8)


def test_setter_and_taps_argument_checks_without_a_device():
    _need_lib()
    L = capi.lib()
    assert L.amdAprilTagsSetQuadSigma(None, 0.8) == 1
    assert L.amdAprilTagsSetQuadSigma(None, 0.0) == 1
    ksz = C.c_uint32()
    taps = (C.c_uint8 * 17)()
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert L.amdAprilTagsDebugQuadSigmaTaps(bad, taps, 17, C.byref(ksz)) == 1
    assert L.amdAprilTagsDebugQuadSigmaTaps(4.01, taps, 17, C.byref(ksz)) == 2
    assert L.amdAprilTagsDebugQuadSigmaTaps(-4.5, taps, 17, C.byref(ksz)) == 2
    assert L.amdAprilTagsDebugQuadSigmaTaps(0.8, taps, 17, None) == 1
    assert L.amdAprilTagsDebugQuadSigmaTaps(2.0, taps, 8, C.byref(ksz)) == 1      # 9 taps do not fit
    assert L.amdAprilTagsDebugQuadSigmaTaps(0.3, None, 0, C.byref(ksz)) == 0 and ksz.value == 1
    assert L.amdAprilTagsDebugQuadSigmaTaps(4.0, taps, 17, C.byref(ksz)) == 0 and ksz.value == 17


def test_row_vector_at_0_8():
    row = np.array([30, 60, 90, 120, 150, 180, 210], dtype=np.uint8)
    assert qs.pass_1d(row, qs.taps(0.8)).tolist() == [30, 59, 88, 118, 148, 180, 210]


def test_flat_frame_at_0_8():
    f = qs.filter_image(np.full((12, 10), 255, dtype=np.uint8), 0.8)
    # one sample on the left / top and two on the right / bottom are copied by each pass
    inner_r, inner_c = slice(1, 12 - 2), slice(1, 10 - 2)
    assert (f[inner_r, inner_c] == 249).all()
    row_copied = np.zeros((12, 10), dtype=bool)
    row_copied[:, [0, 8, 9]] = True
    col_copied = np.zeros((12, 10), dtype=bool)
    col_copied[[0, 10, 11], :] = True
    assert (f[row_copied & ~col_copied] == 252).all()
    assert (f[~row_copied & col_copied] == 252).all()
    assert (f[row_copied & col_copied] == 255).all()


def test_sharpen_clamps():
    img = np.zeros((9, 9), dtype=np.uint8)
    img[4, 4] = 255
    img[2, 2] = 10
    img[3, 2] = 200
    f = qs.filter_image(img, -1.0)
    assert f[4, 4] == 255                       # 2 * 255 - B > 255
    assert f[4, 3] == 0 and f[3, 3] == 0        # 2 * 0 - B < 0
    g = img.astype(np.int32)
    b = qs.filter_image(img, 1.0).astype(np.int32)
    assert np.array_equal(f, np.clip(2 * g - b, 0, 255))


def test_short_sequences_are_the_identity():
    k = qs.taps(2.0)                            # ksz 9
    x = np.arange(9, dtype=np.uint8) * 20
    assert np.array_equal(qs.pass_1d(x, k), x)
    img = np.random.default_rng(1).integers(0, 256, size=(9, 40), dtype=np.uint8)
    f = qs.filter_image(img, 2.0)               # the column pass (n = 9) copies, the row pass filters
    assert np.array_equal(f, qs.pass_1d(img, k))
    assert np.array_equal(qs.filter_image(img[:, :9], 2.0), img[:, :9])
