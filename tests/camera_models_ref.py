"""The numpy statement of the general rectification: the three distortion models of sensor_msgs/CameraInfo
behind a rectification rotation R.  Vectorised float64, one ufunc per operator in the order of the definition, so that every value is
the IEEE result of the same operation on the same operands as in the kernels; atan_s is stated here as well, because libm's atan and
the device library's do not agree bit for bit.  Written from the definition, not from the kernels.  Shared by
tests/test_camera_models_cpu.py and tests/test_camera_models_gpu.py; results are cached per process and never changed."""
import math

import numpy as np

KINDS = {"plumb_bob": 0, "rational_polynomial": 1, "equidistant": 2}
NCOEF = {"plumb_bob": 5, "rational_polynomial": 8, "equidistant": 4}
_ATAN_C = [(-1.0 if n & 1 else 1.0) / float(2 * n + 1) for n in range(23)]
_TAN_PI_8 = 0.41421356237309503


def atan_s(r):
    """The library's arctangent for r >= 0 (array in, array out)."""
    r = np.asarray(r, dtype=np.float64)
    with np.errstate(divide="ignore"):
        a = np.where(r > 1.0, 1.0 / r, r)
    red = a > _TAN_PI_8
    t = np.where(red, (a - 1.0) / (a + 1.0), a)
    z = t * t
    p = np.full_like(z, _ATAN_C[22])
    for n in range(21, -1, -1):
        p = _ATAN_C[n] + z * p
    s = t * p
    s = np.where(red, math.pi / 4 + s, s)
    return np.where(r > 1.0, math.pi / 2 - s, s)


def rot(rx=0.01, ry=-0.015, rz=0.004):
    """Rz(rz) . Ry(ry) . Rx(rx)."""
    cx, sx, cy, sy, cz, sz = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    Rx = np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]])
    return Rz @ Ry @ Rx


def project(w, h, K, D, Knew, kind="plumb_bob", R=None):
    """(u, v, ok): the source position of every destination pixel of a w x h image, [h, w] float64 each, and where the ray points
    towards the camera (W > 0).  u, v are NaN-free only where ok."""
    K, Knew = np.asarray(K, dtype=np.float64).reshape(3, 3), np.asarray(Knew, dtype=np.float64).reshape(3, 3)
    D = [float(v) for v in D] + [0.0] * (8 - len(D))
    assert len(D) == 8 and all(v == 0.0 for v in D[NCOEF[kind]:])
    Ri = (np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3)).T.reshape(-1)
    x = np.arange(w, dtype=np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    xp = (x - Knew[0, 2]) / Knew[0, 0]
    yp = (y - Knew[1, 2]) / Knew[1, 1]
    X = (Ri[0] * xp + Ri[1] * yp) + Ri[2]
    Y = (Ri[3] * xp + Ri[4] * yp) + Ri[5]
    W = (Ri[6] * xp + Ri[7] * yp) + Ri[8]
    ok = W > 0.0
    with np.errstate(all="ignore"):
        xn = X / W
        yn = Y / W
        r2 = xn * xn + yn * yn
        if kind == "equidistant":
            k1, k2, k3, k4 = D[:4]
            r = np.sqrt(r2)
            th = atan_s(np.where(ok, r, 0.0))
            t2 = th * th
            thd = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
            s = np.where(r > 1e-8, thd / r, 1.0)
            xd = xn * s
            yd = yn * s
        else:
            k1, k2, p1, p2, k3, k4, k5, k6 = D
            radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
            if kind == "rational_polynomial":
                radial = radial / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)))
            xd = xn * radial + (2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn))
            yd = yn * radial + (p1 * (r2 + 2.0 * yn * yn) + 2.0 * p2 * xn * yn)
        u = K[0, 0] * xd + K[0, 2]
        v = K[1, 1] * yd + K[1, 2]
    return u, v, ok


def rectify(gray, K, D, Knew, kind="plumb_bob", R=None):
    """The rectified plane of an [h, w] uint8 image: bounds test, 1/32-pixel position, clamps and integer blend of section 7b."""
    gray = np.asarray(gray)
    h, w = gray.shape
    u, v, ok = project(w, h, K, D, Knew, kind, R)
    with np.errstate(invalid="ignore"):
        ok = ok & (u >= 0.0) & (v >= 0.0) & (u <= float(w - 1)) & (v <= float(h - 1))
    fu = (np.where(ok, u, 0.0) * 32.0 + 0.5).astype(np.int64)
    fv = (np.where(ok, v, 0.0) * 32.0 + 0.5).astype(np.int64)
    x0, y0, wx, wy = fu >> 5, fv >> 5, fu & 31, fv & 31
    cx, cy = x0 >= w - 1, y0 >= h - 1
    x0, wx = np.where(cx, w - 1, x0), np.where(cx, 0, wx)
    y0, wy = np.where(cy, h - 1, y0), np.where(cy, 0, wy)
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    g = gray.astype(np.int64)
    top = g[y0, x0] * (32 - wx) + g[y0, x1] * wx
    bot = g[y1, x0] * (32 - wx) + g[y1, x1] * wx
    out = (top * (32 - wy) + bot * wy + 512) >> 10
    return np.where(ok, out, 0).astype(np.uint8)


# ---- the cameras of the tests (scene_c2's camera scaled to w x h, as tests/rectify_cases.py does) ------------------------------------
D_RATIONAL = [0.35, -0.12, 0.0005, -0.0007, 0.02, 0.42, -0.05, 0.01]
D_FISHEYE = [-0.03, 0.004, -0.0006, 0.0001]


def knew_fisheye(w, h):
    """rc.camera with both focal lengths x 0.7 and the principal point moved by (+6.5, -4.25) (of the 1080p image; scaled with the size)."""
    import rectify_cases as rc
    K = rc.camera(w, h)
    K[0, 0] *= 0.7
    K[1, 1] *= 0.7
    K[0, 2] += 6.5 * w / 1920.0
    K[1, 2] -= 4.25 * h / 1080.0
    return K


def cameras(w=1920, h=1080):
    """name -> (K, D, Knew, kind, R): each kind with and without the rotation."""
    import rectify_cases as rc
    K, R = rc.camera(w, h), rot()
    return {
        "plumb_bob": (K, rc.DA, rc.knew_a(w, h), "plumb_bob", None),
        "plumb_bob+R": (K, rc.DA, rc.knew_a(w, h), "plumb_bob", R),
        "rational": (K, D_RATIONAL, rc.knew_a(w, h), "rational_polynomial", None),
        "rational+R": (K, D_RATIONAL, rc.knew_a(w, h), "rational_polynomial", R),
        "equidistant": (K, D_FISHEYE, knew_fisheye(w, h), "equidistant", None),
        "equidistant+R": (K, D_FISHEYE, knew_fisheye(w, h), "equidistant", R),
    }


CAMERA_NAMES = ("plumb_bob", "plumb_bob+R", "rational", "rational+R", "equidistant", "equidistant+R")
_cache = {}


def noise(name):
    """[H, W, 3] RGB noise of the plane cases: 301 x 203 (seed 301) and 8 x 4 (seed 84), as tests/test_rectify_submission_gpu.py has them."""
    if name not in _cache:
        if name == "noise301":
            _cache[name] = np.random.default_rng(301).integers(0, 256, size=(203, 301, 3), dtype=np.uint8)
        else:
            _cache[name] = np.random.default_rng(84).integers(0, 256, size=(4, 8, 3), dtype=np.uint8)
    return _cache[name]


def rectified_scene(name):
    """scene_c2 rectified by this file under cameras()[name]."""
    import rectify_cases as rc
    if ("scene", name) not in _cache:
        _cache[("scene", name)] = rectify(rc.scene()[0], *cameras()[name])
    return _cache[("scene", name)]


def oracle_detections(name, setting):
    """The oracle's records on rectified_scene(name) at (decimate, tile_size, quad_sigma), posed with the camera's Knew."""
    import parity_util as pu
    import rectify_cases as rc
    from oracle import pyoracle as po
    key = ("dets", name, setting)
    if key not in _cache:
        decimate, tile, sigma = setting
        more = {"quad_sigma": sigma} if sigma else {}
        _cache[key] = po.detect(rectified_scene(name), families=rc.FAM, params=pu.oracle_params(cameras()[name][2], decimate, tile_size=tile, **more))[0]
    return _cache[key]
