"""Resize inside the submission (amdAprilTagsSetResize), the parts that need no GPU: the preconditions the GPU comparisons of
tests/test_resize_submission_gpu.py stand on, restated with the oracle alone; the ABI and its binding; the wrong builds the GPU
suite ships."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

from isaac_ros_apriltag_amd import build  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
import rectify_cases as rc  # noqa: E402
import resize_cases as zc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _records_differ(a, b):
    return len(a) != len(b) or any(not np.array_equal(x["p"], y["p"]) for x, y in zip(a, b))


# ---- 1. the oracle's preconditions -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", zc.TARGETS, ids=lambda t: "%dx%d" % t)
def test_resized_scene_has_ten_detections(built, target):
    """scene_c2 resized to each target: ten detections at decimate 1 and 2 -- a GPU comparison cannot pass on empty lists."""
    for decimate in (1, 2):
        dets = zc.oracle_detections(*target, setting=(decimate, 4, 0.0))
        assert len(dets) == 10 and sorted(d["id"] for d in dets) == list(range(10)), (target, decimate, len(dets))


@pytest.mark.parametrize("setting", rc.SETTINGS)
def test_resized_rectified_scene_has_ten_detections(built, setting):
    """resize(rectified("a")) to 1280 x 720: ten detections at each of the six settings, and records other than those of the
    unrectified resize -- so the fused form cannot pass without rectifying."""
    dets = zc.oracle_detections(1280, 720, setting, "a")
    plain = zc.oracle_detections(1280, 720, setting)
    assert len(dets) == 10 and len(plain) == 10 and _records_differ(dets, plain)
    assert not np.array_equal(zc.resized(1280, 720, "a"), zc.resized(1280, 720))


@pytest.mark.parametrize("rectify", (False, True), ids=("plain", "rectified"))
def test_batch_case_has_records(built, rectify):
    """The batch of the GPU test: 58 records over its eight slots in both modes, the identity slots 3 and 4 equal to their gray plane,
    and slots of the two sizes that differ."""
    case = zc.batch_case(rectify)
    counts = [len(c[3]) for c in case]
    assert sum(counts) == 58, counts
    frames = zc.batch_frames()
    for i, (model, k4, S, dets) in enumerate(case):
        assert S.shape == zc.BATCH_SIZES[i % 2][::-1]
    if not rectify:
        for i in (3, 4):
            assert np.array_equal(case[i][2], rc.bt601(frames[i][..., ::-1]))
    else:
        for i in (3, 4):
            assert np.array_equal(case[i][2], po.rectify_mono8(rc.bt601(frames[i][..., ::-1]), *case[i][0]))
    assert case[0][2].shape != case[5][2].shape   # the same frame at both sizes: a build that takes sizes[0] everywhere differs


def test_identity_property():
    """sw == dw and sh == dh: wx = wy = 0 everywhere and the statement is the identity."""
    rng = np.random.default_rng(7)
    for h, w in ((203, 301), (1, 1), (3, 2), (64, 64), (720, 1280)):
        img = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        assert np.array_equal(po.resize_mono8(img, w, h), img)
    # and anything else is not
    img = rng.integers(0, 256, size=(203, 301), dtype=np.uint8)
    assert not np.array_equal(po.resize_mono8(img, 301, 202)[:202], img[:202])


def test_scaled_camera():
    K = zc.scaled_k(rc.knew_a(1920, 1080), 1920, 1080, 1280, 720)
    assert K[2].tolist() == [0, 0, 1] and K[0, 0] == 970.0 * 1280.0 / 1920.0 and K[1, 2] == 535.75 * 720.0 / 1080.0
    assert np.array_equal(zc.scaled_k(rc.camera(301, 203), 301, 203, 301, 203), rc.camera(301, 203))


# ---- 2. the C ABI and its binding -----------------------------------------------------------------------------------------------------
def test_abi_is_declared_and_bound():
    from isaac_ros_apriltag_amd import capi
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "apriltag_amd.h")).read()
    assert "typedef struct { uint32_t width, height; } amdAprilTagsSize_t;" in hdr
    assert re.search(r"int amdAprilTagsSetResize\(amdAprilTagsHandle handle, uint32_t nsizes, const amdAprilTagsSize_t\* sizes\);", hdr)
    dbg = open(os.path.join(ROOT, "include", "apriltag_amd_debug.h")).read()
    assert re.search(r"AMDAT_DBG_RESIZED = 10\b", dbg) and capi.DBG_RESIZED == 10
    assert re.search(r"AMDAT_DBG_RECTIFIED = 9\b", dbg) and capi.DBG_RECTIFIED == 9
    assert "amdAprilTagsSetResize" in capi.EXPORTS
    assert C.sizeof(capi.Size) == 8
    arr = capi.sizes([(1280, 720), (1000, 600)])
    assert len(arr) == 2 and (arr[1].width, arr[1].height) == (1000, 600)
    assert capi.sizes(None) is None and capi.sizes([]) is None


def test_version_and_layout_are_unchanged():
    """The setter is an addition: no structure of the ABI changed, so the layout version stays."""
    from isaac_ros_apriltag_amd import capi
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "apriltag_amd.h")).read()
    assert re.search(r"#define AMDAT_CONFIG_LAYOUT_VERSION 3\b", hdr)
    assert C.sizeof(capi.ImageInput) == 24 and C.sizeof(capi.CameraModel) == 23 * 8 and C.sizeof(capi.Intrinsics) == 16
    assert capi.NUM_STAGES == 12


def test_node_shell_header_carries_the_options():
    hdr = open(os.path.join(ROOT, "include", "apriltag_node_shell.hpp")).read()
    assert re.search(r"uint32_t resize_width = 0, resize_height = 0;", hdr)
    comp = open(os.path.join(ROOT, "ros2", "isaac_ros_apriltag", "src", "apriltag_node_component.cpp")).read()
    assert '"resize_width"' in comp and '"resize_height"' in comp


# ---- 3. the wrong builds ---------------------------------------------------------------------------------------------------------------
def test_wrong_builds_are_registered():
    assert 11 in build.MUTANTS and 12 in build.MUTANTS
    assert build.lib_mutant(11).endswith("libapriltag_amd_mut11.so") and build.lib_mutant(12).endswith("libapriltag_amd_mut12.so")
    hooks = open(os.path.join(ROOT, "isaac_ros_apriltag_amd", "csrc", "tools_hooks.h")).read()
    assert "AMDAT_MUTATE == 11" in hooks and "AMDAT_MUTATE == 12" in hooks
