"""The orthogonal-iteration tag pose with both minima, DESIGN.md section 7e, in pure Python floats: one IEEE double operation per
operator, in the order the section gives them, every sum over the four corners in the form (x0 + x1) + (x2 + x3).  The library
(csrc/pose_refine.h, on the host and -- through csrc/kernels_pose.h -- on the device) states the same; tests compare bit for bit.

refine(p, intrinsics, skew, tag_size, R_h, t_h, iterations) takes a record's corners p[k] = (u, v), the frame's camera and the handle's
tag_size as the C ABI carries them (f32), and the record's homography pose, and returns the record of amdAprilTagsGetRefinedPoses as a
dict."""
import math

import numpy as np

REFINED, REFINED_NO_ALT, DEGENERATE = 0, 1, 2
CORNERS = ((-1.0, 1.0), (1.0, 1.0), (1.0, -1.0), (-1.0, -1.0))   # c_k: p[k] = H(c_k)
NPTS = 4.0
NAN = float("nan")


def f32(v):
    return float(np.float32(v))


def sqrt(x):
    """The correctly rounded square root; NaN below zero (as the C library's and the device's)."""
    if x != x or x < 0.0:
        return NAN
    return math.sqrt(x) if x != math.inf else math.inf


def div(a, b):
    """IEEE division: Python raises where C gives an infinity or a NaN."""
    if b == 0.0:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def finite(x):
    return x - x == 0.0


def sum4(x):
    return (x[0] + x[1]) + (x[2] + x[3])


def setup(p, intr, skew, s):
    """The points [(F00, F01, F02, F11, F12, F22, px, py)] and the six distinct entries of G^-1."""
    fx, fy, cx, cy = intr
    pts = []
    for k in range(4):
        px = s * CORNERS[k][0]
        py = s * CORNERS[k][1]
        vn = div(float(p[k][1]) - cy, fy)
        un = div((float(p[k][0]) - cx) - skew * vn, fx)
        nn = (un * un + vn * vn) + 1.0
        pts.append((div(un * un, nn), div(un * vn, nn), div(un, nn), div(vn * vn, nn), div(vn, nn), div(1.0, nn), px, py))
    S = [sum4([pt[e] for pt in pts]) for e in range(6)]
    G00 = 1.0 - S[0] / NPTS
    G01 = -(S[1] / NPTS)
    G02 = -(S[2] / NPTS)
    G11 = 1.0 - S[3] / NPTS
    G12 = -(S[4] / NPTS)
    G22 = 1.0 - S[5] / NPTS
    c00 = G11 * G22 - G12 * G12
    c01 = G12 * G02 - G01 * G22
    c02 = G01 * G12 - G11 * G02
    c11 = G00 * G22 - G02 * G02
    c12 = G01 * G02 - G00 * G12
    c22 = G00 * G11 - G01 * G01
    det = (G00 * c00 + G01 * c01) + G02 * c02
    return pts, (div(c00, det), div(c01, det), div(c02, det), div(c11, det), div(c12, det), div(c22, det))


def translation(pts, Gi, R):
    a0, a1, a2 = [], [], []
    for (F00, F01, F02, F11, F12, F22, px, py) in pts:
        w0 = R[0] * px + R[1] * py
        w1 = R[3] * px + R[4] * py
        w2 = R[6] * px + R[7] * py
        a0.append(((F00 * w0 + F01 * w1) + F02 * w2) - w0)
        a1.append(((F01 * w0 + F11 * w1) + F12 * w2) - w1)
        a2.append(((F02 * w0 + F12 * w1) + F22 * w2) - w2)
    b0 = sum4(a0) / NPTS
    b1 = sum4(a1) / NPTS
    b2 = sum4(a2) / NPTS
    return [(Gi[0] * b0 + Gi[1] * b1) + Gi[2] * b2, (Gi[1] * b0 + Gi[3] * b1) + Gi[4] * b2, (Gi[2] * b0 + Gi[4] * b1) + Gi[5] * b2]


def error(pts, R, t):
    e = []
    for (F00, F01, F02, F11, F12, F22, px, py) in pts:
        x0 = (R[0] * px + R[1] * py) + t[0]
        x1 = (R[3] * px + R[4] * py) + t[1]
        x2 = (R[6] * px + R[7] * py) + t[2]
        e0 = x0 - ((F00 * x0 + F01 * x1) + F02 * x2)
        e1 = x1 - ((F01 * x0 + F11 * x1) + F12 * x2)
        e2 = x2 - ((F02 * x0 + F12 * x1) + F22 * x2)
        e.append((e0 * e0 + e1 * e1) + e2 * e2)
    return sum4(e)


def rotation(pts, R, t):
    """(the next R, whether det S > 0)."""
    q0, q1, q2 = [], [], []
    for (F00, F01, F02, F11, F12, F22, px, py) in pts:
        x0 = (R[0] * px + R[1] * py) + t[0]
        x1 = (R[3] * px + R[4] * py) + t[1]
        x2 = (R[6] * px + R[7] * py) + t[2]
        q0.append((F00 * x0 + F01 * x1) + F02 * x2)
        q1.append((F01 * x0 + F11 * x1) + F12 * x2)
        q2.append((F02 * x0 + F12 * x1) + F22 * x2)
    qb0 = sum4(q0) / NPTS
    qb1 = sum4(q1) / NPTS
    qb2 = sum4(q2) / NPTS
    q0 = [v - qb0 for v in q0]
    q1 = [v - qb1 for v in q1]
    q2 = [v - qb2 for v in q2]
    px = [pt[6] for pt in pts]
    py = [pt[7] for pt in pts]
    A00 = sum4([q0[k] * px[k] for k in range(4)])
    A01 = sum4([q0[k] * py[k] for k in range(4)])
    A10 = sum4([q1[k] * px[k] for k in range(4)])
    A11 = sum4([q1[k] * py[k] for k in range(4)])
    A20 = sum4([q2[k] * px[k] for k in range(4)])
    A21 = sum4([q2[k] * py[k] for k in range(4)])
    S00 = (A00 * A00 + A10 * A10) + A20 * A20
    S01 = (A00 * A01 + A10 * A11) + A20 * A21
    S11 = (A01 * A01 + A11 * A11) + A21 * A21
    d = S00 * S11 - S01 * S01
    r = sqrt(d)
    tau = sqrt((S00 + S11) + 2.0 * r)
    T00 = div(S00 + r, tau)
    T01 = div(S01, tau)
    T11 = div(S11 + r, tau)
    dt = T00 * T11 - T01 * T01
    I00 = div(T11, dt)
    I01 = div(-T01, dt)
    I11 = div(T00, dt)
    Q00 = A00 * I00 + A01 * I01
    Q01 = A00 * I01 + A01 * I11
    Q10 = A10 * I00 + A11 * I01
    Q11 = A10 * I01 + A11 * I11
    Q20 = A20 * I00 + A21 * I01
    Q21 = A20 * I01 + A21 * I11
    Rn = [Q00, Q01, Q10 * Q21 - Q20 * Q11,
          Q10, Q11, Q20 * Q01 - Q00 * Q21,
          Q20, Q21, Q00 * Q11 - Q10 * Q01]
    return Rn, d > 0.0


def pose_finite(R, t):
    return all(finite(v) for v in R) and all(finite(v) for v in t)


def mirror_start(Rh, th):
    """(2 c c^T - I) R_h diag(-1, -1, 1), c = t_h / |t_h|."""
    n = sqrt((th[0] * th[0] + th[1] * th[1]) + th[2] * th[2])
    c = [div(th[0], n), div(th[1], n), div(th[2], n)]
    R1 = [0.0] * 9
    for i in range(3):
        m0 = 2.0 * (c[i] * c[0]) - (1.0 if i == 0 else 0.0)
        m1 = 2.0 * (c[i] * c[1]) - (1.0 if i == 1 else 0.0)
        m2 = 2.0 * (c[i] * c[2]) - (1.0 if i == 2 else 0.0)
        R1[3 * i + 0] = -((m0 * Rh[0] + m1 * Rh[3]) + m2 * Rh[6])
        R1[3 * i + 1] = -((m0 * Rh[1] + m1 * Rh[4]) + m2 * Rh[7])
        R1[3 * i + 2] = (m0 * Rh[2] + m1 * Rh[5]) + m2 * Rh[8]
    return R1


def chain(pts, Gi, Rstart, iterations, t_follows_step=lambda it, n: True):
    """(ok, R, t, E) of one chain."""
    R = list(Rstart)
    t = translation(pts, Gi, R)
    ok = pose_finite(R, t)
    for it in range(iterations):
        R, pos = rotation(pts, R, t)
        if t_follows_step(it, iterations):
            t = translation(pts, Gi, R)
        ok = ok and pos and pose_finite(R, t)
    E = error(pts, R, t)
    return ok and finite(E), R, t, E


def refine(p, intrinsics, skew, tag_size, R_h, t_h, iterations, mirrored=True, t_follows_step=lambda it, n: True):
    """The refined record.  mirrored, t_follows_step: the definition's (tests of the tests pass the wrong builds' forms)."""
    intr = tuple(f32(v) for v in intrinsics)
    skew = f32(skew)
    Rh = [float(v) for v in np.asarray(R_h, dtype=np.float64).reshape(-1)]
    th = [float(v) for v in np.asarray(t_h, dtype=np.float64).reshape(-1)]
    pts, Gi = setup(p, intr, skew, f32(tag_size) / 2.0)
    Eh = error(pts, Rh, th)
    Rs1 = mirror_start(Rh, th) if mirrored else list(Rh)
    ok0, R0, t0, E0 = chain(pts, Gi, Rh, iterations, t_follows_step)
    ok1, R1, t1, E1 = chain(pts, Gi, Rs1, iterations, t_follows_step)
    second = ok0 and ok1 and E1 < E0
    alt = ok0 and ok1
    zero9, zero3 = [0.0] * 9, [0.0] * 3
    out = {"status": DEGENERATE if not ok0 else REFINED_NO_ALT if not ok1 else REFINED, "chosen": 1 if second else 0,
           "R": Rh if not ok0 else R1 if second else R0, "t": th if not ok0 else t1 if second else t0,
           "err": Eh if not ok0 else E1 if second else E0,
           "R_alt": zero9 if not alt else R0 if second else R1, "t_alt": zero3 if not alt else t0 if second else t1,
           "err_alt": 0.0 if not alt else E0 if second else E1, "err_homography": Eh}
    for k in ("R", "R_alt"):
        out[k] = np.array(out[k], dtype=np.float64).reshape(3, 3)
    for k in ("t", "t_alt"):
        out[k] = np.array(out[k], dtype=np.float64)
    return out


def refine_records(records, intrinsics, skew, tag_size, iterations, **kw):
    """The refined records of a frame's detection records (pyoracle.detect: "p", "R", "t")."""
    return [refine(r["p"], intrinsics, skew, tag_size, r["R"], r["t"], iterations, **kw) for r in records]


FIELDS = ("R", "t", "err", "R_alt", "t_alt", "err_alt", "err_homography")


def bits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64)).reshape(-1).view(np.uint64)


def compare(got, want, label=""):
    """Mismatch strings between a library record (detector.refined_poses) and refine()'s; empty: every field equal, bit for bit."""
    errs = []
    for k in ("status", "chosen"):
        if int(got[k]) != int(want[k]):
            errs.append("%s%s %r, the reference has %r: they differ" % (label, k, got[k], want[k]))
    for k in FIELDS:
        if not np.array_equal(bits(got[k]), bits(want[k])):
            errs.append("%s%s differ by %.3e" % (label, k, float(np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(want[k], dtype=np.float64)).max())))
    return errs


def compare_frames(got, want, label=""):
    errs = []
    if len(got) != len(want):
        return ["%s%d refined records, the reference has %d: they differ" % (label, len(got), len(want))]
    for i, (g, w) in enumerate(zip(got, want)):
        errs += compare(g, w, "%srecord %d: " % (label, i))
    return errs


def rot_angle_deg(Ra, Rb):
    """The angle of Ra^T Rb in degrees."""
    M = np.asarray(Ra).reshape(3, 3).T @ np.asarray(Rb).reshape(3, 3)
    return math.degrees(math.atan2(math.sqrt((M[2, 1] - M[1, 2]) ** 2 + (M[0, 2] - M[2, 0]) ** 2 + (M[1, 0] - M[0, 1]) ** 2),
                                   M[0, 0] + M[1, 1] + M[2, 2] - 1.0))
