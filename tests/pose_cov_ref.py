"""The first-order pose covariance, DESIGN.md section 7g, in pure Python floats: one IEEE double operation per operator, in the order
the section gives them, every sum over the points through the caller's `sum` (pose_refine_ref.sum4 for a tag's four corners,
tree_sum(ntags) for a rigid bundle's 64 slots of four).  The library (csrc/pose_covariance.h, on the host and -- through
csrc/kernels_pose.h and csrc/kernels_rigid.h -- on the device) states the same; tests compare bit for bit.

The parameters are ROS' PoseWithCovariance's in the camera optical frame, x = (dt_x, dt_y, dt_z, dtheta_x, dtheta_y, dtheta_z), with
t' = t + dt and R' = Exp(dtheta) R."""
import numpy as np

import pose_refine_ref as pr

NAN = float("nan")


def ix(i, j):
    """Entry (i, j), i >= j, among the 21 distinct entries kept row by row."""
    return i * (i + 1) // 2 + j


def tree_sum(ntags):
    """rigid_pose.h's RgSumTree: slot s < ntags gives (x0 + x1) + (x2 + x3), an unused slot +0.0, then the balanced tree over 64."""
    def f(x):
        v = [(x[4 * s] + x[4 * s + 1]) + (x[4 * s + 2] + x[4 * s + 3]) if s < ntags else 0.0 for s in range(64)]
        n = 32
        while n >= 1:
            v = [v[2 * s] + v[2 * s + 1] for s in range(n)]
            n //= 2
        return v[0]
    return f


def jacobian_rows(P, R, t, cam, skew_in_ju=True):
    """(J_u, J_v, u, v) of one object point P at the pose (R row-major 9, t) under cam = (fx, fy, cx, cy, skew)."""
    fx, fy, cx, cy, skew = cam
    W0 = (R[0] * P[0] + R[1] * P[1]) + R[2] * P[2]
    W1 = (R[3] * P[0] + R[4] * P[1]) + R[5] * P[2]
    W2 = (R[6] * P[0] + R[7] * P[1]) + R[8] * P[2]
    X0 = W0 + t[0]
    X1 = W1 + t[1]
    X2 = W2 + t[2]
    iz = pr.div(1.0, X2)
    g = fx * X0 + skew * X1
    h = fy * X1
    a = fx * iz
    b = skew * iz
    c = fy * iz
    d = -((g * iz) * iz)
    e = -((h * iz) * iz)
    bu = b if skew_in_ju else 0.0
    Ju = [a, bu, d, d * W1 - bu * W2, a * W2 - d * W0, bu * W0 - a * W1]
    Jv = [0.0, c, e, e * W1 - c * W2, -(e * W0), c * W0]
    return Ju, Jv, pr.div(g, X2) + cx, pr.div(h, X2) + cy


def normal(points, pix, R, t, cam, sum_, skew_in_ju=True):
    """(the 21 distinct entries of N, the squared pixel residual sum) over the points."""
    rows = [jacobian_rows(P, R, t, cam, skew_in_ju) for P in points]
    m = []
    for (_, _, u, v), q in zip(rows, pix):
        du = u - float(q[0])
        dv = v - float(q[1])
        m.append(du * du + dv * dv)
    sq = sum_(m)
    N = [0.0] * 21
    for r in range(6):
        for s in range(r + 1):
            N[ix(r, s)] = sum_([Ju[r] * Ju[s] + Jv[r] * Jv[s] for (Ju, Jv, _, _) in rows])
    return N, sq


def invert(N, sigma2):
    """(ok, cov 6 x 6): cov = sigma2 * N^-1 through the Cholesky factor; (False, zeros) on a refused pivot or a non-finite entry."""
    zeros = np.zeros((6, 6))
    L = [0.0] * 21
    for j in range(6):
        pivot = N[ix(j, j)]
        if j > 0:
            acc = L[ix(j, 0)] * L[ix(j, 0)]
            for k in range(1, j):
                acc = acc + L[ix(j, k)] * L[ix(j, k)]
            pivot = pivot - acc
        if not (pivot > 0.0 and pr.finite(pivot)):
            return False, zeros
        ljj = pr.sqrt(pivot)
        L[ix(j, j)] = ljj
        for i in range(j + 1, 6):
            v = N[ix(i, j)]
            if j > 0:
                acc = L[ix(i, 0)] * L[ix(j, 0)]
                for k in range(1, j):
                    acc = acc + L[ix(i, k)] * L[ix(j, k)]
                v = v - acc
            L[ix(i, j)] = pr.div(v, ljj)
    M = [0.0] * 21
    for j in range(6):
        M[ix(j, j)] = pr.div(1.0, L[ix(j, j)])
        for i in range(j + 1, 6):
            acc = L[ix(i, j)] * M[ix(j, j)]
            for k in range(j + 1, i):
                acc = acc + L[ix(i, k)] * M[ix(k, j)]
            M[ix(i, j)] = pr.div(-acc, L[ix(i, i)])
    cov = np.zeros((6, 6))
    for r in range(6):
        for s in range(r + 1):
            acc = M[ix(r, r)] * M[ix(r, s)]
            for k in range(r + 1, 6):
                acc = acc + M[ix(k, r)] * M[ix(k, s)]
            c = sigma2 * acc
            if not pr.finite(c):
                return False, zeros
            cov[r, s] = c
            cov[s, r] = c
    return True, cov


def _flat(R):
    return [float(v) for v in np.asarray(R, dtype=np.float64).reshape(-1)]


def record(points, pix, cam, pose, pose_alt, sigma, sum_, residuals=True, skew_in_ju=True):
    """The covariance record: pose = (R, t), pose_alt = (R_alt, t_alt) or None."""
    sigma2 = float(sigma) * float(sigma)
    N, sq = normal(points, pix, _flat(pose[0]), _flat(pose[1]), cam, sum_, skew_in_ju)
    ok, cov = invert(N, sigma2)
    out = {"cov": cov, "cov_alt": np.zeros((6, 6)), "sq_err_sum": sq if residuals else 0.0, "sq_err_sum_alt": 0.0, "valid": 1 if ok else 0}
    if pose_alt is not None:
        N, sq = normal(points, pix, _flat(pose_alt[0]), _flat(pose_alt[1]), cam, sum_, skew_in_ju)
        ok, cov = invert(N, sigma2)
        out["cov_alt"] = cov
        out["sq_err_sum_alt"] = sq if residuals else 0.0
        out["valid"] |= 2 if ok else 0
    return out


def tag_points(tag_size):
    s = pr.f32(tag_size) / 2.0
    return [(s * c[0], s * c[1], 0.0) for c in pr.CORNERS]


def tag_record(p, intrinsics, skew, tag_size, refined, sigma, **kw):
    """The covariance record of one tag from its corners p, the camera as the C ABI carries it (f32) and its refined record."""
    cam = tuple(pr.f32(v) for v in intrinsics) + (pr.f32(skew),)
    alt = (refined["R_alt"], refined["t_alt"]) if refined["status"] == pr.REFINED else None
    return record(tag_points(tag_size), p, cam, (refined["R"], refined["t"]), alt, sigma, pr.sum4, **kw)


def tag_records(records, intrinsics, skew, tag_size, refined, sigma, **kw):
    return [tag_record(r["p"], intrinsics, skew, tag_size, o, sigma, **kw) for r, o in zip(records, refined)]


ZERO = {"cov": np.zeros((6, 6)), "cov_alt": np.zeros((6, 6)), "sq_err_sum": 0.0, "sq_err_sum_alt": 0.0, "valid": 0}
TOO_FEW_TAGS = 1


def bundle_record(pix, obj, intrinsics, skew, solved, sigma, centred=False):
    """The covariance record of one rigid bundle: pix[s][k], obj[s][k] the pixels and object points of the used slots in slot order
    (rigid_bundle_ref.inputs), solved its pose record (rigid_bundle_ref.solve).  centred: the wrong build's P - mean P."""
    if solved["status"] == TOO_FEW_TAGS:
        return dict(ZERO)
    ntags = len(pix)
    cam = tuple(pr.f32(v) for v in intrinsics) + (pr.f32(skew),)
    sum_ = tree_sum(ntags)
    pts = [tuple(float(v) for v in P) for slot in obj for P in slot]
    px = [tuple(float(v) for v in q) for slot in pix for q in slot]
    if centred:
        npts = 4.0 * float(ntags)
        mean = [sum_([P[e] for P in pts]) / npts for e in range(3)]
        pts = [(P[0] - mean[0], P[1] - mean[1], P[2] - mean[2]) for P in pts]
    alt = (solved["R_alt"], solved["t_alt"]) if np.asarray(solved["R_alt"]).any() else None
    return record(pts, px, cam, (solved["R"], solved["t"]), alt, sigma, sum_, residuals=False)


def bundle_record_of(records, bundle, families, intrinsics, skew, solved, sigma, **kw):
    """bundle_record on a frame's detection records: the used slots are rigid_bundle_ref.inputs'."""
    import rigid_bundle_ref as rr
    _, _, pix, obj, _, _ = rr.inputs(records, bundle, families, intrinsics, skew)
    return bundle_record(pix, obj, intrinsics, skew, solved, sigma, **kw)


def compare(got, want, label=""):
    """Mismatch strings between a library record (a numpy record of capi.POSE_COV_DTYPE, or a dict) and a reference record; empty:
    every field equal, bit for bit."""
    errs = []
    if int(got["valid"]) != int(want["valid"]):
        errs.append("%svalid %r, the reference has %r: they differ" % (label, int(got["valid"]), int(want["valid"])))
    for k in ("cov", "cov_alt", "sq_err_sum", "sq_err_sum_alt"):
        g, w = np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64)
        if not np.array_equal(pr.bits(g), pr.bits(w)):
            with np.errstate(all="ignore"):
                errs.append("%s%s differ by %.3e (relative %.3e)" % (label, k, float(np.abs(g - w).max()),
                                                                   float(np.abs(g - w).max() / max(np.abs(w).max(), 1e-300))))
    return errs


def compare_frames(got, want, label=""):
    if len(got) != len(want):
        return ["%s%d covariance records, the reference has %d: they differ" % (label, len(got), len(want))]
    errs = []
    for i, (g, w) in enumerate(zip(got, want)):
        errs += compare(g, w, "%srecord %d: " % (label, i))
    return errs
