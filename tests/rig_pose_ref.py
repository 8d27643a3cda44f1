"""The pose of a rigid 3-D tag bundle in the frame of a camera rig, DESIGN.md section 7j, in pure Python floats: one IEEE double
operation per operator, in the order the section gives them.  The library (csrc/rig_pose.h on the host and -- through
csrc/kernels_rig.h -- on the device) states the same; tests compare bit for bit.  The sums, the polar rotation, the seed area, the
start composition and the outcome rule are rigid_bundle_ref's, as rig_pose.h takes rigid_pose.h's; classification, gates and the
per-frame duplicate rule are bundle_ref.classify's.

A group is a list of frames in ascending batch-slot order, each {"slot", "records" (what pyoracle.detect returns), "intrinsics"
(fx, fy, cx, cy), "skew", "camera": (Rc (3 x 3), tc (3))}: the rig frame in the camera frame, X_cam = Rc X_rig + tc."""
import numpy as np

from oracle import pyoracle as po
import rigid_bundle_ref as rr
from rigid_bundle_ref import SOLVED, TOO_FEW_TAGS, DEGENERATE, div, f32, finite, mirror_start, pose_finite  # noqa: F401

SLOTS = 64
INT_FIELDS = ("group", "bundle", "status", "nobs", "nskipped", "ndropped", "ncams", "seed_frame", "seed", "chosen")
FIELDS = rr.FIELDS


def _flat(v):
    return [float(x) for x in np.asarray(v, dtype=np.float64).reshape(-1)]


def gather(group, bundle, families, slot_cut=SLOTS):
    """(observations [(frame of the group, record index, member)] that fill the slots, nskipped, ndropped, ncams)."""
    obs, nskipped, total, ncams = [], 0, 0, 0
    for fr in group:
        used, skipped = rr.used_slots(fr["records"], bundle, families)
        nskipped += skipped
        if used and total < slot_cut:
            ncams += 1
        for i, m in used:
            if total < slot_cut:
                obs.append((fr, i, m))
            total += 1
    return obs, nskipped, total - len(obs), ncams


def camera_of(fr):
    """(fx, fy, cx, cy, skew, Rc (9), tc (3)) as the library holds them: intrinsics and skew rounded to float."""
    Rc, tc = fr["camera"]
    return tuple(f32(v) for v in fr["intrinsics"]) + (f32(fr.get("skew", 0.0)), _flat(Rc), _flat(tc))


def setup(pix, obj, cams, npts, ray_transpose=True):
    """pix, obj, cams: per slot four (u, v), four (X, Y, Z) and the camera.  The points, per slot four of [F00, F01, F02, F11, F12,
    F22, px, py, pz, cx, cy, cz, ox, oy, oz], and the six distinct entries of G^-1."""
    pts = []
    for tp, to, (fx, fy, cx, cy, skew, Rc, tc) in zip(pix, obj, cams):
        rt = (lambda i, k: Rc[3 * k + i]) if ray_transpose else (lambda i, k: Rc[3 * i + k])
        e0 = 0.0 - tc[0]
        e1 = 0.0 - tc[1]
        e2 = 0.0 - tc[2]
        o = [(Rc[i] * e0 + Rc[3 + i] * e1) + Rc[6 + i] * e2 for i in range(3)]
        tag = []
        for k in range(4):
            vn = div(float(tp[k][1]) - cy, fy)
            un = div((float(tp[k][0]) - cx) - skew * vn, fx)
            d0 = (rt(0, 0) * un + rt(0, 1) * vn) + rt(0, 2)
            d1 = (rt(1, 0) * un + rt(1, 1) * vn) + rt(1, 2)
            d2 = (rt(2, 0) * un + rt(2, 1) * vn) + rt(2, 2)
            nn = (d0 * d0 + d1 * d1) + d2 * d2
            tag.append([div(d0 * d0, nn), div(d0 * d1, nn), div(d0 * d2, nn), div(d1 * d1, nn), div(d1 * d2, nn), div(d2 * d2, nn),
                        float(to[k][0]), float(to[k][1]), float(to[k][2]), 0.0, 0.0, 0.0, o[0], o[1], o[2]])
        pts.append(tag)
    col = lambda e: rr.tree_sum([[pt[e] for pt in tag] for tag in pts])
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


def translation(pts, Gi, R, npts, origin=True):
    a0, a1, a2 = [], [], []
    for tag in pts:
        r0, r1, r2 = [], [], []
        for pt in tag:
            F00, F01, F02, F11, F12, F22 = pt[:6]
            p0, p1, p2 = rr._rp(R, pt)
            w0 = p0 - (pt[12] if origin else 0.0)
            w1 = p1 - (pt[13] if origin else 0.0)
            w2 = p2 - (pt[14] if origin else 0.0)
            r0.append(((F00 * w0 + F01 * w1) + F02 * w2) - w0)
            r1.append(((F01 * w0 + F11 * w1) + F12 * w2) - w1)
            r2.append(((F02 * w0 + F12 * w1) + F22 * w2) - w2)
        a0.append(r0)
        a1.append(r1)
        a2.append(r2)
    b0 = rr.tree_sum(a0) / npts
    b1 = rr.tree_sum(a1) / npts
    b2 = rr.tree_sum(a2) / npts
    return [(Gi[0] * b0 + Gi[1] * b1) + Gi[2] * b2, (Gi[1] * b0 + Gi[3] * b1) + Gi[4] * b2, (Gi[2] * b0 + Gi[4] * b1) + Gi[5] * b2]


def _x(R, t, pt):
    w0, w1, w2 = rr._rp(R, pt)
    return (w0 + t[0]) - pt[12], (w1 + t[1]) - pt[13], (w2 + t[2]) - pt[14]


def error(pts, R, t):
    e = []
    for tag in pts:
        r = []
        for pt in tag:
            F00, F01, F02, F11, F12, F22 = pt[:6]
            x0, x1, x2 = _x(R, t, pt)
            e0 = x0 - ((F00 * x0 + F01 * x1) + F02 * x2)
            e1 = x1 - ((F01 * x0 + F11 * x1) + F12 * x2)
            e2 = x2 - ((F02 * x0 + F12 * x1) + F22 * x2)
            r.append((e0 * e0 + e1 * e1) + e2 * e2)
        e.append(r)
    return rr.tree_sum(e)


def moment_matrix(pts, R, t, npts):
    q = []
    for tag in pts:
        r = []
        for pt in tag:
            F00, F01, F02, F11, F12, F22 = pt[:6]
            x0, x1, x2 = _x(R, t, pt)
            r.append([pt[12] + ((F00 * x0 + F01 * x1) + F02 * x2), pt[13] + ((F01 * x0 + F11 * x1) + F12 * x2),
                      pt[14] + ((F02 * x0 + F12 * x1) + F22 * x2)])
        q.append(r)
    qb = [rr.tree_sum([[c[i] for c in tag] for tag in q]) / npts for i in range(3)]
    q = [[[c[i] - qb[i] for i in range(3)] for c in tag] for tag in q]
    return [rr.tree_sum([[q[s][k][i] * pts[s][k][9 + j] for k in range(4)] for s in range(len(pts))]) for i in range(3) for j in range(3)]


def chain(pts, Gi, Rstart, iterations, npts, origin=True):
    """(ok, R, t, E) of one chain."""
    R = list(Rstart)
    t = translation(pts, Gi, R, npts, origin)
    ok = pose_finite(R, t)
    for _ in range(iterations):
        R, pos = rr.polar(moment_matrix(pts, R, t, npts))
        t = translation(pts, Gi, R, npts, origin)
        ok = ok and pos and pose_finite(R, t)
    E = error(pts, R, t)
    return ok and finite(E), R, t, E


def from_camera(Rc, tc, Rb, tb):
    """A bundle pose in a camera's frame moved into the rig frame: Rc^T Rb, Rc^T (tb - tc)."""
    Rr = [(Rc[i] * Rb[j] + Rc[3 + i] * Rb[3 + j]) + Rc[6 + i] * Rb[6 + j] for i in range(3) for j in range(3)]
    if tb is None:
        return Rr, None
    e0 = tb[0] - tc[0]
    e1 = tb[1] - tc[1]
    e2 = tb[2] - tc[2]
    return Rr, [(Rc[i] * e0 + Rc[3 + i] * e1) + Rc[6 + i] * e2 for i in range(3)]


def reprojection(tp, to, R, t, cam):
    fx, fy, cx, cy, skew, Rc, tc = cam
    e = []
    for k in range(4):
        X0 = ((R[0] * to[k][0] + R[1] * to[k][1]) + R[2] * to[k][2]) + t[0]
        X1 = ((R[3] * to[k][0] + R[4] * to[k][1]) + R[5] * to[k][2]) + t[1]
        X2 = ((R[6] * to[k][0] + R[7] * to[k][1]) + R[8] * to[k][2]) + t[2]
        xc = ((Rc[0] * X0 + Rc[1] * X1) + Rc[2] * X2) + tc[0]
        yc = ((Rc[3] * X0 + Rc[4] * X1) + Rc[5] * X2) + tc[1]
        zc = ((Rc[6] * X0 + Rc[7] * X1) + Rc[8] * X2) + tc[2]
        xn = div(xc, zc)
        yn = div(yc, zc)
        u = (fx * xn + skew * yn) + cx
        v = fy * yn + cy
        du = u - float(tp[k][0])
        dv = v - float(tp[k][1])
        e.append(du * du + dv * dv)
    return ((e[0] + e[1]) + e[2]) + e[3]


def zero_record(group_index, bundle_index, nobs=0, nskipped=0, ndropped=0, ncams=0):
    return {"group": group_index, "bundle": bundle_index, "status": TOO_FEW_TAGS, "nobs": nobs, "nskipped": nskipped, "ndropped": ndropped,
            "ncams": ncams, "seed_frame": 0, "seed": 0, "chosen": 0, "R": np.zeros((3, 3)), "t": np.zeros(3), "err": 0.0, "sq_err_sum": 0.0,
            "R_alt": np.zeros((3, 3)), "t_alt": np.zeros(3), "err_alt": 0.0, "sq_err_sum_alt": 0.0}


def inputs(group, bundle, families, slot_cut=SLOTS):
    """What the solve of one (group, bundle) reads: (obs, nskipped, ndropped, ncams, pix, obj, cams, homography poses, member poses)."""
    obs, nskipped, ndropped, ncams = gather(group, bundle, families, slot_cut)
    pix = [[(float(fr["records"][i]["p"][k][0]), float(fr["records"][i]["p"][k][1])) for k in range(4)] for fr, i, _ in obs]
    obj = [rr.member_corners(m) for _, _, m in obs]
    cams = [camera_of(fr) for fr, _, _ in obs]
    hom, mem = [], []
    for (fr, i, m), cam in zip(obs, cams):
        Rh, th = po.pose_from_homography(fr["records"][i]["H"], cam[0], cam[1], cam[2], cam[3], float(m[4]), cam[4])
        hom.append((_flat(Rh), _flat(th)))
        mem.append((_flat(m[2]), _flat(m[3])))
    return obs, nskipped, ndropped, ncams, pix, obj, cams, hom, mem


def solve_slots(pix, obj, cams, hom, mem, iterations, origin=True, ray_transpose=True):
    """The pose fields of the record from the filled slots (rig_pose.h: rig_solve_host); "seed" is the seed's SLOT."""
    nobs = len(pix)
    seed, best = 0, -1.0
    for s in range(nobs):
        a = rr.area2(pix[s])
        if a > best:
            best, seed = a, s
    (Rh, th), (Rm, tm) = hom[seed], mem[seed]
    Rc, tc = cams[seed][5], cams[seed][6]
    Rb0, tb0 = rr.compose_start(Rh, th, Rm, tm)
    Rb1, _ = rr.compose_start(mirror_start(Rh, th), None, Rm, tm)
    Rs0, ts0 = from_camera(Rc, tc, Rb0, tb0)
    Rs1, _ = from_camera(Rc, tc, Rb1, None)
    npts = 4.0 * float(nobs)
    pts, Gi = setup(pix, obj, cams, npts, ray_transpose)
    Es = error(pts, Rs0, ts0)
    ok0, R0, t0, E0 = chain(pts, Gi, Rs0, iterations, npts, origin)
    ok1, R1, t1, E1 = chain(pts, Gi, Rs1, iterations, npts, origin)
    sq0, sq1 = 0.0, 0.0
    for s in range(nobs):
        sq0 = sq0 + reprojection(pix[s], obj[s], R0, t0, cams[s])
        sq1 = sq1 + reprojection(pix[s], obj[s], R1, t1, cams[s])
    none = not ok0 and not ok1
    alt = ok0 and ok1
    second = ok1 and (not ok0 or E1 < E0)
    zero9, zero3 = [0.0] * 9, [0.0] * 3
    out = dict(status=DEGENERATE if none else SOLVED, seed=seed, chosen=1 if second else 0,
               R=Rs0 if none else R1 if second else R0, t=ts0 if none else t1 if second else t0,
               err=Es if none else E1 if second else E0, sq_err_sum=0.0 if none else sq1 if second else sq0,
               R_alt=zero9 if not alt else R0 if second else R1, t_alt=zero3 if not alt else t0 if second else t1,
               err_alt=0.0 if not alt else E0 if second else E1, sq_err_sum_alt=0.0 if not alt else sq0 if second else sq1)
    for k in ("R", "R_alt"):
        out[k] = np.array(out[k], dtype=np.float64).reshape(3, 3)
    for k in ("t", "t_alt"):
        out[k] = np.array(out[k], dtype=np.float64)
    return out


def solve(group, bundle, families, group_index=0, bundle_index=0, origin=True, ray_transpose=True, slot_cut=SLOTS):
    """The rig record of one (group, bundle).  origin, ray_transpose, slot_cut: the definition's (tests of the tests pass the wrong
    builds' forms: False, False, 63)."""
    obs, nskipped, ndropped, ncams, pix, obj, cams, hom, mem = inputs(group, bundle, families, slot_cut)
    out = zero_record(group_index, bundle_index, len(obs), nskipped, ndropped, ncams)
    if len(obs) < int(bundle.get("min_tags", 1)) or not obs:
        return out
    out.update(solve_slots(pix, obj, cams, hom, mem, int(bundle.get("iterations", rr.ITERATIONS)), origin, ray_transpose))
    fr, i, _ = obs[out["seed"]]
    out["seed_frame"], out["seed"] = int(fr["slot"]), i
    return out


def solve_submission(frames, slots, bundles, families, **forms):
    """Every record of a submission, [group][bundle]: frames is the list of all its frames by batch slot ({"records", "intrinsics",
    "skew"}), slots[i] = (group, camera index or None), cameras come with the frames' "camera" entries."""
    out = []
    for g in range(len(frames)):
        group = [dict(frames[i], slot=i) for i in range(len(frames)) if slots[i][0] == g and slots[i][1] is not None]
        out.append([solve(group, b, families, g, bi, **forms) for bi, b in enumerate(bundles)])
    return out


def compare(got, want, label=""):
    """Mismatch strings between a library record (detector.rig_bundle_poses) and solve()'s; empty: every field equal, bit for bit."""
    errs = []
    for k in INT_FIELDS:
        if int(got[k]) != int(want[k]):
            errs.append("%sgroup %d bundle %d: %s %r, the reference has %r: they differ" % (label, want["group"], want["bundle"], k, got[k], want[k]))
    for k in FIELDS:
        if not np.array_equal(rr.bits(got[k]), rr.bits(want[k])):
            errs.append("%sgroup %d bundle %d: %s differ by %.3e" % (label, want["group"], want["bundle"], k, float(
                np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(want[k], dtype=np.float64)).max())))
    return errs
