"""The general rectification without a GPU: tests/camera_models_ref.py against the oracle where the two overlap (plumb_bob and
rational_polynomial with zero k4 .. k6, R = I), atan_s against libm, csrc/camera_models.h compiled by a host compiler against the
reference bit for bit, the oracle-side preconditions of tests/test_camera_models_gpu.py, and the host side of the options."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

from oracle import pyoracle as po  # noqa: E402
import camera_models_ref as cm  # noqa: E402
import parity_util as pu  # noqa: E402
import rectify_cases as rc  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- 1. the reference is the oracle where they overlap -------------------------------------------------------------------------------
def _gray(name):
    return rc.scene()[0] if name == "scene_c2" else rc.bt601(cm.noise(name))


@pytest.mark.parametrize("name", ("noise301", "8x4", "scene_c2"))
def test_reference_equals_the_oracle_with_identity_rotation(built, name):
    gray = _gray(name)
    h, w = gray.shape
    for label, (K, D, Kn) in (("Da", rc.model_a(w, h)), ("Dz", rc.model_z(w, h)), ("identity", rc.model_identity(w, h))):
        want = po.rectify_mono8(gray, K, D, Kn)
        for kind, R in (("plumb_bob", None), ("rational_polynomial", None), ("plumb_bob", np.eye(3)), ("rational_polynomial", np.eye(3))):
            got = cm.rectify(gray, K, D, Kn, kind, R)
            assert np.array_equal(got, want), (name, label, kind, int((got != want).sum()))
        if label == "identity":
            assert np.array_equal(want, gray)


# ---- 2. atan_s ------------------------------------------------------------------------------------------------------------------------
def test_atan_s_against_libm():
    args = np.concatenate([np.linspace(0.0, 3.0, 200001), np.logspace(-12, 3, 100001), [0.0, 1.0, 0.41421356237309503, 1000.0],
                           np.nextafter(1.0, [0.0, 2.0]), np.nextafter(0.41421356237309503, [0.0, 1.0]), 1.0 / np.linspace(0.3, 0.5, 2001)])
    got = cm.atan_s(args)
    want = np.array([math.atan(float(a)) for a in args])
    err = float(np.abs(got - want).max())
    print("atan_s: largest distance from math.atan over %d arguments in [0, 1e3]: %.3g" % (args.size, err))
    assert err <= 1e-13
    assert cm.atan_s(np.array([0.0]))[0] == 0.0


# ---- 3. the header's lines under a host compiler --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("camera_models") / "camera_models_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", os.path.join(HERE, "aux_c", "camera_models_driver.cpp"), "-o", exe])
    return exe


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("name", cm.CAMERA_NAMES + ("behind",))
def test_header_under_a_host_compiler(driver, name):
    """u, v of every seventh pixel of a 301 x 203 image, bit for bit.  "behind": a rotation by 100 degrees about y, for which part of
    the image looks away from the camera (W <= 0)."""
    w, h, step = 301, 203, 7
    if name == "behind":
        K, D, Kn, kind, R = cm.cameras(w, h)["rational"]
        R = cm.rot(0.0, math.radians(100.0), 0.0)
    else:
        K, D, Kn, kind, R = cm.cameras(w, h)[name]
    Rm = np.eye(3) if R is None else R
    d8 = list(D) + [0.0] * (8 - len(D))
    args = [w, h, step, cm.KINDS[kind]] + [float(v).hex() for v in list(rc.k4(K)) + d8 + list(Rm.reshape(-1)) + list(rc.k4(Kn))]
    out = subprocess.run([driver] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout.split("\n")
    u, v, ok = cm.project(w, h, K, D, Kn, kind, R)
    ubits, vbits = _bits(u), _bits(v)
    n = same = 0
    for line in out:
        if not line:
            continue
        x, y, k, ub, vb = line.split()
        x, y = int(x), int(y)
        n += 1
        assert int(k) == int(ok[y, x]), (x, y)
        if ok[y, x]:
            assert int(ub, 16) == int(ubits[y, x]) and int(vb, 16) == int(vbits[y, x]), (x, y, ub, u[y, x])
            same += 1
    assert n == len(range(0, w, step)) * len(range(0, h, step))
    assert same == n if name != "behind" else 0 < same < n


def test_atan_s_under_a_host_compiler(driver):
    args = np.concatenate([np.linspace(0.0, 3.0, 701), np.logspace(-12, 3, 300)])
    out = subprocess.run([driver, "0"] + [float(a).hex() for a in args], capture_output=True, text=True, check=True).stdout.split()
    assert [int(t, 16) for t in out] == [int(b) for b in _bits(cm.atan_s(args))]


# ---- 4. what the GPU tests rest on ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cm.CAMERA_NAMES[1:])
def test_ten_detections_at_every_setting(built, name):
    for setting in rc.SETTINGS:
        assert len(cm.oracle_detections(name, setting)) == 10, (name, setting)


def test_each_feature_changes_the_plane(built):
    """On 301 x 203 noise (seed 301, drawn as a gray plane) under Knew_a: what k4 .. k6, R and the fisheye's k4 change."""
    gray = np.random.default_rng(301).integers(0, 256, size=(203, 301), dtype=np.uint8)
    C = cm.cameras(301, 203)
    K, D, Kn, kind, _ = C["rational"]
    rational = cm.rectify(gray, K, D, Kn, kind)
    assert int((rational != cm.rectify(gray, K, D[:5], Kn, "plumb_bob")).sum()) == 60187          # k4 .. k6
    assert int((rational != cm.rectify(gray, *C["rational+R"])).sum()) == 60584                     # R
    D = cm.D_FISHEYE
    assert int((cm.rectify(gray, K, D, Kn, "equidistant") != cm.rectify(gray, K, D[:3] + [0.0], Kn, "equidistant")).sum()) == 870   # the fisheye k4
    assert gray.size == 61103
    # and on the plane cases of the GPU tests, every camera's plane is its own
    gray = rc.bt601(cm.noise("noise301"))
    planes = [cm.rectify(gray, *C[n]) for n in cm.CAMERA_NAMES]
    for i in range(6):
        for j in range(i):
            assert int((planes[i] != planes[j]).sum()) > 30000, (i, j)


# ---- 5. options, host only ---------------------------------------------------------------------------------------------------------------
def test_distortion_from_name():
    from isaac_ros_apriltag_amd import capi
    L = capi.lib()
    assert [L.amdAprilTagsDistortionFromName(n) for n in (b"plumb_bob", b"rational_polynomial", b"equidistant")] == [0, 1, 2]
    assert capi.DISTORTIONS == {"plumb_bob": 0, "rational_polynomial": 1, "equidistant": 2}
    for bad in (b"", b"fisheye", b"Plumb_Bob", b"plumb_bob ", None):
        assert L.amdAprilTagsDistortionFromName(bad) == -1


def test_python_camera_models():
    from isaac_ros_apriltag_amd import capi
    K, Kn, R = rc.camera(640, 480), rc.knew_a(640, 480), cm.rot()
    arr = capi.camera_models_ex([(K, rc.DA, Kn), (K, cm.D_FISHEYE, Kn, "equidistant", R), (K, cm.D_RATIONAL[:6], Kn, "rational_polynomial", None)])
    assert [m.kind for m in arr] == [0, 2, 1]
    assert list(arr[0].R) == [1, 0, 0, 0, 1, 0, 0, 0, 1] == list(arr[2].R) and list(arr[1].R) == list(R.reshape(-1))
    assert list(arr[0].D) == rc.DA + [0.0] * 3 and list(arr[1].D) == cm.D_FISHEYE + [0.0] * 4 and list(arr[2].D) == cm.D_RATIONAL[:6] + [0.0] * 2
    assert list(arr[1].K) == list(K.reshape(-1)) and list(arr[1].Knew) == list(Kn.reshape(-1))
    for bad in ((K, [0.0] * 5, Kn, "equidistant", None), (K, [0.0] * 6, Kn, "plumb_bob", None), (K, [0.0] * 9, Kn, "rational_polynomial", None),
                (K, rc.DA, Kn, "fisheye", None), (K, rc.DA, Kn, "plumb_bob", np.eye(2)), (K, rc.DA, Kn, "plumb_bob")):
        with pytest.raises(ValueError):
            capi.camera_models_ex([bad])


def test_node_shell_options():
    """RectificationModelEx: the three models with their coefficient counts, r all zero -> the identity, Knew from P; NodeOptions::rectify
    without rectify_full keeps its own exceptions."""
    from isaac_ros_apriltag_amd import build as b
    from isaac_ros_apriltag_amd import node
    b.build_node()
    K = [float(v) for v in rc.camera(640, 480).reshape(-1)]
    Kn = rc.knew_a(640, 480)
    P = [Kn[0, 0], 0.0, Kn[0, 2], 0.0, 0.0, Kn[1, 1], Kn[1, 2], 0.0, 0.0, 0.0, 1.0, 0.0]
    eye = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
    R = cm.rot()
    for name, kind, nmax in (("plumb_bob", 0, 5), ("rational_polynomial", 1, 8), ("equidistant", 2, 4), ("", 0, 5), (None, 0, 5)):
        for nd in (0, 1, nmax):
            D = [0.01 * (i + 1) for i in range(nd)]
            got = node.camera_model_ex(K, D, name, P, R)
            assert got == (kind, K, D + [0.0] * (8 - nd), [float(v) for v in R.reshape(-1)], [float(v) for v in Kn.reshape(-1)])
        with pytest.raises(RuntimeError, match="has %d coefficients, camera_info carries %d" % (nmax, nmax + 1)):
            node.camera_model_ex(K, [0.0] * (nmax + 1), name, P, R)
    assert node.camera_model_ex(K, cm.D_FISHEYE, "equidistant", P, None)[3] == eye            # r never filled in
    assert node.camera_model_ex(K, cm.D_FISHEYE, "equidistant", P, np.zeros((3, 3)))[3] == eye
    assert node.camera_model_ex(K, cm.D_FISHEYE, "equidistant", None, R)[4] == K                # no P: Knew = K
    for bad in ("fisheye", "Plumb_Bob", "rational"):
        with pytest.raises(RuntimeError, match="'plumb_bob', 'rational_polynomial' and 'equidistant', not '%s'" % bad):
            node.camera_model_ex(K, [], bad, P, R)
    # `rectify` alone: what it always took and refused
    assert node.camera_model(K, rc.DA, "plumb_bob", P) == (K, rc.DA, [float(v) for v in Kn.reshape(-1)])
    with pytest.raises(RuntimeError, match="'plumb_bob' only"):
        node.camera_model(K, cm.D_FISHEYE, "equidistant", P)
    with pytest.raises(RuntimeError, match="five coefficients"):
        node.camera_model(K, cm.D_RATIONAL, "plumb_bob", P)
    with pytest.raises(ValueError):
        node.AprilTagNode(rectify="all")
