"""The corner undistortion of raw-frame mode, DESIGN.md section 7h: the numpy statement of csrc/undistort.h -- vectorised float64, one
ufunc per operator in the order of the definition, so that every value is the IEEE result of the same operation on the same operands
as in k_undistort_records -- and the undistorted record of a kept record in Python floats (the four-point homography through
bundle_ref.eliminate, the pose through the oracle's pose_from_homography).  Written from the definition, not from the kernel.  Shared by
tests/test_corner_undistortion_cpu.py and tests/test_corner_undistortion_gpu.py; results are never changed."""
import numpy as np

import bundle_ref as br
import camera_models_ref as cm
from oracle import pyoracle as po

ITERATIONS = 20
GATE_PX = 2.0 ** -20
OK, INVALID = 0, 1
INT32_MAX = 0x7FFFFFFF
POSE_DEGENERATE = 2


def _d8(D):
    D = [float(v) for v in D] + [0.0] * (8 - len(D))
    assert len(D) == 8
    return D


def distort(x, y, D, kind):
    """Section 7b's forward distortion of normalised points (arrays)."""
    D = _d8(D)
    r2 = x * x + y * y
    if kind == "equidistant":
        k1, k2, k3, k4 = D[:4]
        rr = np.sqrt(r2)
        th = cm.atan_s(rr)
        t2 = th * th
        thd = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
        s = np.where(rr > 1e-8, thd / rr, 1.0)
        return x * s, y * s
    k1, k2, p1, p2, k3, k4, k5, k6 = D
    radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    if kind == "rational_polynomial":
        radial = radial / (1.0 + r2 * (k4 + r2 * (k5 + r2 * k6)))
    xd = x * radial + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))
    yd = y * radial + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)
    return xd, yd


def _newton_poly(xd, yd, x, y, D, kind):
    k1, k2, p1, p2, k3, k4, k5, k6 = _d8(D)
    r2 = x * x + y * y
    radial = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    drad = k1 + r2 * (2.0 * k2 + r2 * (3.0 * k3))
    if kind == "rational_polynomial":
        den = 1.0 + r2 * (k4 + r2 * (k5 + r2 * k6))
        dden = k4 + r2 * (2.0 * k5 + r2 * (3.0 * k6))
        radial = radial / den
        drad = (drad - radial * dden) / den
    ex = (x * radial + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))) - xd
    ey = (y * radial + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)) - yd
    cross = 2.0 * p1 * x + 2.0 * p2 * y
    J00 = (radial + 2.0 * (x * x) * drad) + (2.0 * p1 * y + 6.0 * p2 * x)
    J01 = 2.0 * (x * y) * drad + cross
    J10 = J01
    J11 = (radial + 2.0 * (y * y) * drad) + (6.0 * p1 * y + 2.0 * p2 * x)
    det = J00 * J11 - J01 * J10
    return x - (J11 * ex - J01 * ey) / det, y - (J00 * ey - J10 * ex) / det


def _newton_fisheye(thd, r, D):
    k1, k2, k3, k4 = _d8(D)[:4]
    # (atan_s is stated for r >= 0; an iterate that leaves that range takes the same operations, as in the header)
    th = cm.atan_s(r)
    t2 = th * th
    g = th * (1.0 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4)))) - thd
    dg = (1.0 + t2 * (3.0 * k1 + t2 * (5.0 * k2 + t2 * (7.0 * k3 + t2 * (9.0 * k4))))) / (1.0 + r * r)
    return r - g / dg


def _finite(v):
    return (v - v) == 0.0


def undistort(u, v, K, D, Knew, kind="plumb_bob", R=None, iterations=ITERATIONS, rotation=True):
    """(uo, vo, ok) of raw pixels (arrays of one shape): the ideal pixel, zero where ok is false.  rotation=False: R taken as the
    identity (tests of the tests)."""
    K, Knew = np.asarray(K, dtype=np.float64).reshape(3, 3), np.asarray(Knew, dtype=np.float64).reshape(3, 3)
    Rm = (np.eye(3) if R is None or not rotation else np.asarray(R, dtype=np.float64).reshape(3, 3)).reshape(-1)
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    with np.errstate(all="ignore"):
        xd = (u - K[0, 2]) / K[0, 0]
        yd = (v - K[1, 2]) / K[1, 1]
        if kind == "equidistant":
            thd = np.sqrt(xd * xd + yd * yd)
            r = thd.copy()
            for _ in range(iterations):
                r = _newton_fisheye(thd, r, D)
            s = r / thd
            far = thd > 1e-8
            x = np.where(far, xd * s, xd)
            y = np.where(far, yd * s, yd)
        else:
            x, y = xd.copy(), yd.copy()
            for _ in range(iterations):
                x, y = _newton_poly(xd, yd, x, y, D, kind)
        xf, yf = distort(x, y, D, kind)
        gx = K[0, 0] * (xf - xd)
        gy = K[1, 1] * (yf - yd)
        ok = _finite(x) & _finite(y) & _finite(gx) & _finite(gy)
        ok = ok & (np.abs(gx) <= GATE_PX) & (np.abs(gy) <= GATE_PX)
        X = (Rm[0] * x + Rm[1] * y) + Rm[2]
        Y = (Rm[3] * x + Rm[4] * y) + Rm[5]
        W = (Rm[6] * x + Rm[7] * y) + Rm[8]
        ok = ok & (W > 0.0)
        uu = Knew[0, 0] * (X / W) + Knew[0, 2]
        vv = Knew[1, 1] * (Y / W) + Knew[1, 2]
        ok = ok & _finite(uu) & _finite(vv)
    return np.where(ok, uu, 0.0), np.where(ok, vv, 0.0), ok


# ---- the undistorted record ---------------------------------------------------------------------------------------------------------------
def homography4(p):
    """The exact homography with H(c_k) = p[k]: the 8 x 9 rows of the detector, eliminated as bundle_ref.eliminate does.  None: singular."""
    rows = []
    for k in range(4):
        x, y = br.CORNERS[k]
        u, v = float(p[k][0]), float(p[k][1])
        rows.append([x, y, 1.0, 0.0, 0.0, 0.0, -x * u, -y * u, u])
        rows.append([0.0, 0.0, 0.0, x, y, 1.0, -x * v, -y * v, v])
    return br.eliminate(rows)


def project_h(H, x, y):
    xx = H[0] * x + H[1] * y + H[2]
    yy = H[3] * x + H[4] * y + H[5]
    zz = H[6] * x + H[7] * y + H[8]
    return xx / zz, yy / zz


def record(rec, camera, intrinsics, tag_size, skew=0.0, rotation=True):
    """The undistorted twin of one kept record (a dict with "p", as pyoracle.detect returns it) under camera = (K, D, Knew, kind, R) and
    the frame's pose intrinsics (fx, fy, cx, cy) and skew as the C ABI carries them (f32).  A copy of `rec` with "status" and the geometric
    fields replaced; an invalid record has them all zero and "hamming_dev" (the hamming of the device twin) INT32_MAX."""
    K, D, Knew, kind, R = camera
    p = np.asarray(rec["p"], dtype=np.float64)
    uo, vo, ok = undistort(p[:, 0], p[:, 1], K, D, Knew, kind, R, rotation=rotation)
    out = dict(rec)
    zero = dict(status=INVALID, H=np.zeros((3, 3)), center=np.zeros(2), p=np.zeros((4, 2)), R=np.zeros((3, 3)), t=np.zeros(3), hamming_dev=INT32_MAX)
    if not bool(ok.all()):
        out.update(zero)
        return out
    pu = [[float(uo[k]), float(vo[k])] for k in range(4)]
    H = homography4(pu)
    if H is None:
        out.update(zero)
        return out
    fx, fy, cx, cy = (br.f32(v) for v in intrinsics)
    with np.errstate(all="ignore"):
        c = project_h([np.float64(h) for h in H], np.float64(0.0), np.float64(0.0))
        Rp, tp = po.pose_from_homography(H, fx, fy, cx, cy, br.f32(tag_size), br.f32(skew))
    vals = np.concatenate([np.asarray(H), np.asarray(c, dtype=np.float64), Rp.reshape(-1), tp])
    if not bool(np.isfinite(vals).all()):
        out.update(zero)
        return out
    out.update(status=OK, H=np.array(H).reshape(3, 3), center=np.array([float(c[0]), float(c[1])]), p=np.array(pu), R=Rp, t=tp,
               hamming_dev=int(rec["hamming"]))
    return out


def records(recs, camera, intrinsics, tag_size, skew=0.0, rotation=True):
    return [record(r, camera, intrinsics, tag_size, skew, rotation) for r in recs]


def for_consumers(urecs):
    """What the bundle references are fed: the twins as the device holds them (hamming INT32_MAX where invalid, so every gate skips them)."""
    return [dict(r, hamming=r["hamming_dev"]) for r in urecs]


def compare(got, want):
    """Mismatch strings between a library record (detector.undistorted_detections) and record()'s; empty: equal, bit for bit."""
    errs = []
    if int(got["status"]) != int(want["status"]):
        errs.append("status %r, the reference has %r" % (got["status"], want["status"]))
    for k in ("H", "center", "p", "R", "t"):
        a, b = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        if a.shape != b.shape or not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
            errs.append("%s differ by %.3e" % (k, float(np.abs(a - b).max()) if a.shape == b.shape else float("nan")))
    return errs


# ---- what the consumers give for the twins (section 7h: the rule for an invalid twin, stated here once) ----------------------------------------
def refined(urecs, intrinsics, skew, tag_size, iterations, **kw):
    """The refined records of a frame's twins: pose_refine_ref's for a valid twin; for an invalid one DEGENERATE with every other field zero."""
    import pose_refine_ref as pr
    zero = {"status": POSE_DEGENERATE, "chosen": 0, "R": np.zeros((3, 3)), "t": np.zeros(3), "err": 0.0, "R_alt": np.zeros((3, 3)),
            "t_alt": np.zeros(3), "err_alt": 0.0, "err_homography": 0.0}
    return [pr.refine(r["p"], intrinsics, skew, tag_size, r["R"], r["t"], iterations, **kw) if r["status"] == OK else dict(zero) for r in urecs]


def covariances(urecs, intrinsics, skew, tag_size, refined_recs, sigma):
    """The covariance records beside refined(): pose_cov_ref's for a valid twin; for an invalid one all zero, valid = 0."""
    import pose_cov_ref as pv
    return [pv.tag_record(r["p"], intrinsics, skew, tag_size, o, sigma) if r["status"] == OK else dict(pv.ZERO) for r, o in zip(urecs, refined_recs)]
