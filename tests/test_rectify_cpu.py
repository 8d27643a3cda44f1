"""Rectification inside the submission (amdAprilTagsSetRectification), the parts that need no GPU: the preconditions the GPU
comparisons of tests/test_rectify_submission_gpu.py stand on, restated with the oracle alone; the node shell's handling of the camera
model; the wrong builds the GPU suite ships."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

from isaac_ros_apriltag_amd import build  # noqa: E402
import rectify_cases as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _records_differ(a, b):
    return len(a) != len(b) or any(not np.array_equal(x["p"], y["p"]) for x, y in zip(a, b))


# ---- 1. the oracle's preconditions -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", rc.SETTINGS)
def test_rectified_scene_has_ten_detections(built, setting):
    """Da, Knew_a: ten detections on the rectified frame at each of the six settings, and records other than those of the unrectified
    frame -- so a GPU comparison can neither pass on empty lists nor pass without rectifying."""
    dets = rc.oracle_detections("a", setting)
    assert len(dets) == 10 and sorted(d["id"] for d in dets) == list(range(10))
    plain = rc.oracle_detections("a", setting, rectify=False)
    assert len(plain) == 10 and _records_differ(dets, plain)
    assert all(not np.array_equal(x["p"], y["p"]) for x, y in zip(dets, plain))   # every tag moved


def test_pincushion_model_leaves_a_zero_filled_region(built):
    """Dz, Knew_z: about 9 * 10^5 destination pixels map outside the source and stay 0 (the scene itself has no 0 pixel there: its
    background is 150 with noise of sigma 2), and the ten tags are still detected."""
    R = rc.rectified("z")
    zeros = int((R == 0).sum())
    assert 8.0e5 < zeros < 1.0e6, zeros
    assert (R[:, 0] == 0).all() and (R[0, :] == 0).all() and R[540, 960] != 0   # the border is out of range, the centre is not
    assert int((rc.scene()[0] == 0).sum()) < 1000
    dets = rc.oracle_detections("z")
    assert len(dets) == 10 and _records_differ(dets, rc.oracle_detections("z", rectify=False))
    # Da, Knew_a shrink the image about its centre: its out-of-range region is a thin border
    Ra = rc.rectified("a")
    assert 0 < int((Ra == 0).sum()) < zeros


def test_models_are_as_stated():
    K, D, Kn = rc.model_a()
    assert K.tolist() == [[1000.0, 0, 960.0], [0, 1000.0, 540.0], [0, 0, 1]] and D == [-0.08, 0.01, 0.0005, -0.0007, 0.0]
    assert Kn.tolist() == [[970.0, 0, 966.5], [0, 970.0, 535.75], [0, 0, 1]]
    K, D, Kn = rc.model_z()
    assert D == [0.12, -0.03, 0.0, 0.0, 0.0] and Kn.tolist() == [[800.0, 0, 960.0], [0, 800.0, 540.0], [0, 0, 1]]


# ---- 2. the node shell's option handling (host code only: no detector library is loaded) ----------------------------------------------
def test_node_shell_camera_model():
    from isaac_ros_apriltag_amd import node
    build.build_node()
    K = [1000.0, 0.5, 960.0, 0.0, 1001.0, 540.0, 0.0, 0.0, 1.0]
    P = [970.0, 0.25, 966.5, 0.0, 0.0, 971.0, 535.75, 0.0, 0.0, 0.0, 1.0, 0.0]
    # Knew is the left 3x3 of P when p[0] != 0 ...
    k, d, kn = node.camera_model(K, rc.DA, "plumb_bob", P)
    assert k == K and d == rc.DA and kn == [970.0, 0.25, 966.5, 0.0, 971.0, 535.75, 0.0, 0.0, 1.0]
    # ... and K otherwise (an all-zero P, or none)
    assert node.camera_model(K, rc.DA, "plumb_bob", [0.0] * 12)[2] == K
    assert node.camera_model(K, rc.DA, "plumb_bob")[2] == K
    # up to five coefficients, zero-padded; an empty model name is taken as plumb_bob
    assert node.camera_model(K, [0.12, -0.03], "")[1] == [0.12, -0.03, 0.0, 0.0, 0.0]
    assert node.camera_model(K, [], "plumb_bob")[1] == [0.0] * 5
    assert node.camera_model(K)[1] == [0.0] * 5
    # anything else throws with a clear text
    for model in ("equidistant", "rational_polynomial", "Plumb_Bob"):
        with pytest.raises(RuntimeError, match="plumb_bob"):
            node.camera_model(K, rc.DA, model)
    with pytest.raises(RuntimeError, match="five coefficients"):
        node.camera_model(K, [0.1] * 8, "plumb_bob")


def test_node_shell_header_carries_the_fields():
    hdr = open(os.path.join(ROOT, "include", "apriltag_node_shell.hpp")).read()
    info = hdr[hdr.index("struct CameraInfo {"):]
    info = info[:info.index("\n};")]
    assert "std::vector<double> d;" in info and "std::string distortion_model;" in info and "std::array<double, 12> p{};" in info
    assert re.search(r"bool rectify = false;", hdr)


# ---- 3. the C ABI and its binding -----------------------------------------------------------------------------------------------------
def test_abi_is_declared_and_bound():
    from isaac_ros_apriltag_amd import capi
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "apriltag_amd.h")).read()
    assert "typedef struct { double K[9]; double D[5]; double Knew[9]; } amdAprilTagsCameraModel_t;" in hdr
    assert re.search(r"int amdAprilTagsSetRectification\(amdAprilTagsHandle handle, uint32_t ncams, const amdAprilTagsCameraModel_t\* cams\);", hdr)
    dbg = open(os.path.join(ROOT, "include", "apriltag_amd_debug.h")).read()
    assert re.search(r"AMDAT_DBG_RECTIFIED = 9\b", dbg) and capi.DBG_RECTIFIED == 9
    assert "amdAprilTagsSetRectification" in capi.EXPORTS
    assert C.sizeof(capi.CameraModel) == 23 * 8
    arr = capi.camera_models([rc.model_a(), (rc.camera(8, 4), [0.12, -0.03], rc.knew_z(8, 4))])
    assert len(arr) == 2 and list(arr[0].D) == rc.DA and list(arr[1].D) == [0.12, -0.03, 0.0, 0.0, 0.0]
    assert list(arr[0].Knew) == [970.0, 0, 966.5, 0, 970.0, 535.75, 0, 0, 1]
    assert capi.camera_models(None) is None and capi.camera_models([]) is None


# ---- 4. the wrong builds ---------------------------------------------------------------------------------------------------------------
def test_wrong_builds_are_registered():
    assert 9 in build.MUTANTS and 10 in build.MUTANTS
    assert build.lib_mutant(9).endswith("libapriltag_amd_mut9.so") and build.lib_mutant(10).endswith("libapriltag_amd_mut10.so")
    hooks = open(os.path.join(ROOT, "isaac_ros_apriltag_amd", "csrc", "tools_hooks.h")).read()
    assert "AMDAT_MUTATE == 9" in hooks and "AMDAT_MUTATE == 10" in hooks
