"""The pose of a rigid 3-D tag bundle, DESIGN.md section 7f, in pure Python floats: one IEEE double operation per operator, in the order
the section gives them.  Every sum over the points adds a tag's four values as (x0 + x1) + (x2 + x3) and then the 64 tag slots as a
balanced binary tree, an unused slot contributing +0.0.  The library (csrc/rigid_layout.h and csrc/rigid_pose.h on the host, and --
through csrc/kernels_rigid.h -- on the device) states the same; tests compare bit for bit.  Classification, gates and the duplicate
rule are bundle_ref.classify's; the seed's homography pose is the oracle's pose_from_homography with the member's size.

A rigid bundle is {"name", "iterations", "members": [(family_index, id, R (3 x 3), t (3), size)], "max_hamming", "min_decision_margin",
"min_tags"}; a record is what pyoracle.detect returns."""
import numpy as np

from oracle import pyoracle as po
import bundle_ref as br
from pose_refine_ref import CORNERS, div, f32, finite, mirror_start, pose_finite, sqrt  # noqa: F401

SOLVED, TOO_FEW_TAGS, DEGENERATE = 0, 1, 3
SLOTS = 64
SWEEPS = 5
ITERATIONS = 50


def member_corners(member, use_rotation=True):
    """The four bundle-frame corners of a member (rigid_layout.h: rigid_member_corner)."""
    _, _, R, t, size = member
    R = [float(v) for v in np.asarray(R, dtype=np.float64).reshape(-1)]
    if not use_rotation:
        R = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    t = [float(v) for v in np.asarray(t, dtype=np.float64).reshape(-1)]
    hs = float(size) / 2.0
    out = []
    for k in range(4):
        ax = hs * CORNERS[k][0]
        ay = hs * CORNERS[k][1]
        out.append([(R[3 * i] * ax + R[3 * i + 1] * ay) + t[i] for i in range(3)])
    return out


def is_rotation(R):
    R = [float(v) for v in np.asarray(R, dtype=np.float64).reshape(-1)]
    for i in range(3):
        for j in range(3):
            d = ((R[3 * i] * R[3 * j] + R[3 * i + 1] * R[3 * j + 1]) + R[3 * i + 2] * R[3 * j + 2]) - (1.0 if i == j else 0.0)
            if not abs(d) <= 1e-6:
                return False
    det = (R[0] * (R[4] * R[8] - R[5] * R[7]) + R[1] * (R[5] * R[6] - R[3] * R[8])) + R[2] * (R[3] * R[7] - R[4] * R[6])
    return det > 0.0


def tree_sum(tags):
    """tags: per used slot its four values.  (x0 + x1) + (x2 + x3) per slot, +0.0 for the unused, then the balanced tree over 64 slots."""
    v = [(x[0] + x[1]) + (x[2] + x[3]) for x in tags] + [0.0] * (SLOTS - len(tags))
    n = SLOTS // 2
    while n >= 1:
        v = [v[2 * s] + v[2 * s + 1] for s in range(n)]
        n //= 2
    return v[0]


def setup(pix, obj, intr, skew, npts):
    """pix, obj: per used slot four (u, v) and four (X, Y, Z).  The points, per slot four of [F00, F01, F02, F11, F12, F22, px, py, pz,
    cx, cy, cz], and the six distinct entries of G^-1."""
    fx, fy, cx, cy = intr
    pts = []
    for tp, to in zip(pix, obj):
        tag = []
        for k in range(4):
            vn = div(float(tp[k][1]) - cy, fy)
            un = div((float(tp[k][0]) - cx) - skew * vn, fx)
            nn = (un * un + vn * vn) + 1.0
            tag.append([div(un * un, nn), div(un * vn, nn), div(un, nn), div(vn * vn, nn), div(vn, nn), div(1.0, nn),
                        float(to[k][0]), float(to[k][1]), float(to[k][2]), 0.0, 0.0, 0.0])
        pts.append(tag)
    col = lambda e: tree_sum([[pt[e] for pt in tag] for tag in pts])
    mx = col(6) / npts
    my = col(7) / npts
    mz = col(8) / npts
    for tag in pts:
        for pt in tag:
            pt[9] = pt[6] - mx
            pt[10] = pt[7] - my
            pt[11] = pt[8] - mz
    G00 = 1.0 - col(0) / npts
    G01 = -(col(1) / npts)
    G02 = -(col(2) / npts)
    G11 = 1.0 - col(3) / npts
    G12 = -(col(4) / npts)
    G22 = 1.0 - col(5) / npts
    c00 = G11 * G22 - G12 * G12
    c01 = G12 * G02 - G01 * G22
    c02 = G01 * G12 - G11 * G02
    c11 = G00 * G22 - G02 * G02
    c12 = G01 * G02 - G00 * G12
    c22 = G00 * G11 - G01 * G01
    det = (G00 * c00 + G01 * c01) + G02 * c02
    return pts, (div(c00, det), div(c01, det), div(c02, det), div(c11, det), div(c12, det), div(c22, det))


def _rp(R, pt):
    return ((R[0] * pt[6] + R[1] * pt[7]) + R[2] * pt[8], (R[3] * pt[6] + R[4] * pt[7]) + R[5] * pt[8],
            (R[6] * pt[6] + R[7] * pt[7]) + R[8] * pt[8])


def translation(pts, Gi, R, npts):
    a0, a1, a2 = [], [], []
    for tag in pts:
        r0, r1, r2 = [], [], []
        for pt in tag:
            F00, F01, F02, F11, F12, F22 = pt[:6]
            w0, w1, w2 = _rp(R, pt)
            r0.append(((F00 * w0 + F01 * w1) + F02 * w2) - w0)
            r1.append(((F01 * w0 + F11 * w1) + F12 * w2) - w1)
            r2.append(((F02 * w0 + F12 * w1) + F22 * w2) - w2)
        a0.append(r0)
        a1.append(r1)
        a2.append(r2)
    b0 = tree_sum(a0) / npts
    b1 = tree_sum(a1) / npts
    b2 = tree_sum(a2) / npts
    return [(Gi[0] * b0 + Gi[1] * b1) + Gi[2] * b2, (Gi[1] * b0 + Gi[3] * b1) + Gi[4] * b2, (Gi[2] * b0 + Gi[4] * b1) + Gi[5] * b2]


def error(pts, R, t):
    e = []
    for tag in pts:
        r = []
        for pt in tag:
            F00, F01, F02, F11, F12, F22 = pt[:6]
            w0, w1, w2 = _rp(R, pt)
            x0 = w0 + t[0]
            x1 = w1 + t[1]
            x2 = w2 + t[2]
            e0 = x0 - ((F00 * x0 + F01 * x1) + F02 * x2)
            e1 = x1 - ((F01 * x0 + F11 * x1) + F12 * x2)
            e2 = x2 - ((F02 * x0 + F12 * x1) + F22 * x2)
            r.append((e0 * e0 + e1 * e1) + e2 * e2)
        e.append(r)
    return tree_sum(e)


def jacobi(S, V, p, q, k):
    apq, app, aqq = S[3 * p + q], S[3 * p + p], S[3 * q + q]
    theta = div(aqq - app, 2.0 * apq)
    at = -theta if theta < 0.0 else theta
    tm = div(1.0, at + sqrt(theta * theta + 1.0))
    ts = -tm if theta < 0.0 else tm
    tt = 0.0 if apq == 0.0 else ts
    c = div(1.0, sqrt(tt * tt + 1.0))
    s = tt * c
    S[3 * p + p] = app - tt * apq
    S[3 * q + q] = aqq + tt * apq
    S[3 * p + q] = 0.0
    S[3 * q + p] = 0.0
    akp, akq = S[3 * k + p], S[3 * k + q]
    nkp = c * akp - s * akq
    nkq = s * akp + c * akq
    S[3 * k + p] = nkp
    S[3 * p + k] = nkp
    S[3 * k + q] = nkq
    S[3 * q + k] = nkq
    for r in range(3):
        vp, vq = V[3 * r + p], V[3 * r + q]
        V[3 * r + p] = c * vp - s * vq
        V[3 * r + q] = s * vp + c * vq


def polar(M, sweeps=SWEEPS):
    """(the rotation maximising tr(R^T M) with determinant +1, whether |M v1| > 0)."""
    S = [0.0] * 9
    V = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    for i in range(3):
        for j in range(3):
            S[3 * i + j] = (M[i] * M[j] + M[3 + i] * M[3 + j]) + M[6 + i] * M[6 + j]
    for _ in range(sweeps):
        jacobi(S, V, 0, 1, 2)
        jacobi(S, V, 0, 2, 1)
        jacobi(S, V, 1, 2, 0)
    l = (S[0], S[4], S[8])
    b1 = l[1] > l[0]
    b2 = l[2] > (l[1] if b1 else l[0])
    i1 = 2 if b2 else (1 if b1 else 0)
    ia = 1 if i1 == 0 else 0
    ib = 1 if i1 == 2 else 2
    i2 = ib if l[ib] > l[ia] else ia
    v1 = [V[3 * k + i1] for k in range(3)]
    v2 = [V[3 * k + i2] for k in range(3)]
    w = [(M[3 * i] * v1[0] + M[3 * i + 1] * v1[1]) + M[3 * i + 2] * v1[2] for i in range(3)]
    n1 = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    u1 = [div(w[i], n1) for i in range(3)]
    w = [(M[3 * i] * v2[0] + M[3 * i + 1] * v2[1]) + M[3 * i + 2] * v2[2] for i in range(3)]
    d = (u1[0] * w[0] + u1[1] * w[1]) + u1[2] * w[2]
    w = [w[i] - d * u1[i] for i in range(3)]
    n2 = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    u2 = [div(w[i], n2) for i in range(3)]
    u3 = [u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]]
    v3 = [v1[1] * v2[2] - v1[2] * v2[1], v1[2] * v2[0] - v1[0] * v2[2], v1[0] * v2[1] - v1[1] * v2[0]]
    Rn = [(u1[i] * v1[j] + u2[i] * v2[j]) + u3[i] * v3[j] for i in range(3) for j in range(3)]
    return Rn, n1 > 0.0


def moment_matrix(pts, R, t, npts):
    """M = sum (q_j - mean q)(P_j - mean P)^T, row-major."""
    q = []
    for tag in pts:
        r = []
        for pt in tag:
            F00, F01, F02, F11, F12, F22 = pt[:6]
            w0, w1, w2 = _rp(R, pt)
            x0 = w0 + t[0]
            x1 = w1 + t[1]
            x2 = w2 + t[2]
            r.append([(F00 * x0 + F01 * x1) + F02 * x2, (F01 * x0 + F11 * x1) + F12 * x2, (F02 * x0 + F12 * x1) + F22 * x2])
        q.append(r)
    qb = [tree_sum([[c[i] for c in tag] for tag in q]) / npts for i in range(3)]
    q = [[[c[i] - qb[i] for i in range(3)] for c in tag] for tag in q]
    return [tree_sum([[q[s][k][i] * pts[s][k][9 + j] for k in range(4)] for s in range(len(pts))]) for i in range(3) for j in range(3)]


def chain(pts, Gi, Rstart, iterations, npts, sweeps=SWEEPS, moments=None):
    """(ok, R, t, E) of one chain; moments: a list that collects every M the chain forms."""
    R = list(Rstart)
    t = translation(pts, Gi, R, npts)
    ok = pose_finite(R, t)
    for _ in range(iterations):
        M = moment_matrix(pts, R, t, npts)
        if moments is not None:
            moments.append(M)
        R, pos = polar(M, sweeps)
        t = translation(pts, Gi, R, npts)
        ok = ok and pos and pose_finite(R, t)
    E = error(pts, R, t)
    return ok and finite(E), R, t, E


def area2(p):
    a = ((float(p[0][0]) * float(p[1][1]) - float(p[1][0]) * float(p[0][1])) + (float(p[1][0]) * float(p[2][1]) - float(p[2][0]) * float(p[1][1]))) + \
        ((float(p[2][0]) * float(p[3][1]) - float(p[3][0]) * float(p[2][1])) + (float(p[3][0]) * float(p[0][1]) - float(p[0][0]) * float(p[3][1])))
    return -a if a < 0.0 else a


def compose_start(Rc, tc, Rm, tm):
    Rs = [(Rc[3 * i] * Rm[3 * j] + Rc[3 * i + 1] * Rm[3 * j + 1]) + Rc[3 * i + 2] * Rm[3 * j + 2] for i in range(3) for j in range(3)]
    ts = None if tc is None else [tc[i] - ((Rs[3 * i] * tm[0] + Rs[3 * i + 1] * tm[1]) + Rs[3 * i + 2] * tm[2]) for i in range(3)]
    return Rs, ts


def reprojection(tp, to, R, t, intr, skew):
    fx, fy, cx, cy = intr
    e = []
    for k in range(4):
        xc = ((R[0] * to[k][0] + R[1] * to[k][1]) + R[2] * to[k][2]) + t[0]
        yc = ((R[3] * to[k][0] + R[4] * to[k][1]) + R[5] * to[k][2]) + t[1]
        zc = ((R[6] * to[k][0] + R[7] * to[k][1]) + R[8] * to[k][2]) + t[2]
        xn = div(xc, zc)
        yn = div(yc, zc)
        u = (fx * xn + skew * yn) + cx
        v = fy * yn + cy
        du = u - float(tp[k][0])
        dv = v - float(tp[k][1])
        e.append(du * du + dv * dv)
    return ((e[0] + e[1]) + e[2]) + e[3]


def planar_bundle(bundle):
    """The bundle with members (family_index, id) alone, for bundle_ref.classify."""
    return dict(bundle, members=[(m[0], m[1]) for m in bundle["members"]])


def used_slots(records, bundle, families):
    """([(record index, member)] of the used records in the canonical order, nskipped)."""
    by_key = {(int(m[0]), int(m[1])): m for m in bundle["members"]}
    cls = br.classify(records, planar_bundle(bundle), families)
    used = [(i, by_key[(int(c[0][0]), int(c[0][1]))]) for i, c in enumerate(cls) if c is not None and c[1]]
    return used, sum(1 for c in cls if c is not None and not c[1])


def zero_record(bundle_index, ntags, nskipped):
    return {"bundle": bundle_index, "status": TOO_FEW_TAGS, "ntags": ntags, "nskipped": nskipped, "seed": 0, "chosen": 0,
            "R": np.zeros((3, 3)), "t": np.zeros(3), "err": 0.0, "sq_err_sum": 0.0,
            "R_alt": np.zeros((3, 3)), "t_alt": np.zeros(3), "err_alt": 0.0, "sq_err_sum_alt": 0.0}


def inputs(records, bundle, families, intrinsics, skew, member_rotation=True):
    """What the solve of one frame reads: (used, nskipped, pix, obj, homography poses [(Rh, th)], member poses [(Rm, tm)])."""
    intr = tuple(f32(v) for v in intrinsics)
    skew = f32(skew)
    used, nskipped = used_slots(records, bundle, families)
    pix = [[(float(records[i]["p"][k][0]), float(records[i]["p"][k][1])) for k in range(4)] for i, _ in used]
    obj = [member_corners(m, member_rotation) for _, m in used]
    hom, mem = [], []
    for i, m in used:
        Rh, th = po.pose_from_homography(records[i]["H"], intr[0], intr[1], intr[2], intr[3], float(m[4]), skew)
        hom.append(([float(v) for v in Rh.reshape(-1)], [float(v) for v in th]))
        mem.append(([float(v) for v in np.asarray(m[2], dtype=np.float64).reshape(-1)], [float(v) for v in np.asarray(m[3], dtype=np.float64).reshape(-1)]))
    return used, nskipped, pix, obj, hom, mem


def solve(records, bundle, families, intrinsics, skew=0.0, bundle_index=0, member_rotation=True, npts_of=lambda n: n, sweeps=SWEEPS,
          moments=None):
    """The rigid bundle record of one frame.  member_rotation, npts_of: the definition's (tests of the tests pass the wrong builds'
    forms: False, and lambda n: 4.0)."""
    intr = tuple(f32(v) for v in intrinsics)
    skew = f32(skew)
    used, nskipped, pix, obj, hom, mem = inputs(records, bundle, families, intrinsics, skew, member_rotation)
    ntags = len(used)
    out = zero_record(bundle_index, ntags, nskipped)
    if ntags < int(bundle.get("min_tags", 1)):
        return out
    seed, best = 0, -1.0
    for s in range(ntags):
        a = area2(pix[s])
        if a > best:
            best, seed = a, s
    (Rh, th), (Rm, tm) = hom[seed], mem[seed]
    Rs0, ts0 = compose_start(Rh, th, Rm, tm)
    Rs1, _ = compose_start(mirror_start(Rh, th), None, Rm, tm)
    npts = npts_of(4.0 * float(ntags))
    iterations = int(bundle.get("iterations", ITERATIONS))
    pts, Gi = setup(pix, obj, intr, skew, npts)
    Es = error(pts, Rs0, ts0)
    ok0, R0, t0, E0 = chain(pts, Gi, Rs0, iterations, npts, sweeps, moments)
    ok1, R1, t1, E1 = chain(pts, Gi, Rs1, iterations, npts, sweeps, moments)
    sq0, sq1 = 0.0, 0.0
    for s in range(ntags):
        sq0 = sq0 + reprojection(pix[s], obj[s], R0, t0, intr, skew)
        sq1 = sq1 + reprojection(pix[s], obj[s], R1, t1, intr, skew)
    none = not ok0 and not ok1
    alt = ok0 and ok1
    second = ok1 and (not ok0 or E1 < E0)
    zero9, zero3 = [0.0] * 9, [0.0] * 3
    out.update(status=DEGENERATE if none else SOLVED, seed=used[seed][0], chosen=1 if second else 0,
               R=Rs0 if none else R1 if second else R0, t=ts0 if none else t1 if second else t0,
               err=Es if none else E1 if second else E0, sq_err_sum=0.0 if none else sq1 if second else sq0,
               R_alt=zero9 if not alt else R0 if second else R1, t_alt=zero3 if not alt else t0 if second else t1,
               err_alt=0.0 if not alt else E0 if second else E1, sq_err_sum_alt=0.0 if not alt else sq0 if second else sq1)
    for k in ("R", "R_alt"):
        out[k] = np.array(out[k], dtype=np.float64).reshape(3, 3)
    for k in ("t", "t_alt"):
        out[k] = np.array(out[k], dtype=np.float64)
    return out


FIELDS = ("R", "t", "err", "sq_err_sum", "R_alt", "t_alt", "err_alt", "sq_err_sum_alt")


def bits(v):
    return np.ascontiguousarray(np.asarray(v, dtype=np.float64)).reshape(-1).view(np.uint64)


def compare(got, want, label=""):
    """Mismatch strings between a library record (detector.bundle_poses_ex) and solve()'s; empty: every field equal, bit for bit."""
    errs = []
    for k in ("bundle", "status", "ntags", "nskipped", "seed", "chosen"):
        if int(got[k]) != int(want[k]):
            errs.append("%sbundle %d: %s %r, the reference has %r: they differ" % (label, want["bundle"], k, got[k], want[k]))
    for k in FIELDS:
        if not np.array_equal(bits(got[k]), bits(want[k])):
            errs.append("%sbundle %d: %s differ by %.3e" % (label, want["bundle"], k, float(np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(want[k], dtype=np.float64)).max())))
    return errs
