"""The board pose of a tag bundle, DESIGN.md section 7d, in pure Python floats: one IEEE double operation per operator, in the order the
section gives them, every sum starting from +0.0.  The pose step is the oracle's pose_from_homography (pyoracle), unchanged.  The library
(csrc/bundle_layout.h on the host, csrc/kernels_bundle.h on the device) states the same; tests compare with numpy.array_equal.

A bundle is {"name", "members": [(family_index, id, x, y, size)], "max_hamming", "min_decision_margin", "min_tags"}; a record is what
pyoracle.detect returns ("family" a name: `families` maps it to its index, "id", "hamming", "decision_margin", "p")."""
import math

import numpy as np

from oracle import pyoracle as po

SOLVED, TOO_FEW_TAGS, SINGULAR = 0, 1, 2
CORNERS = ((-1.0, 1.0), (1.0, 1.0), (1.0, -1.0), (-1.0, -1.0))   # c_k: p[k] = H(c_k)


def f32(v):
    return float(np.float32(v))


def normalisation(members):
    """(mx, my, sc) of a bundle's members: the sequential means of the centres, and the largest extent from them out to a border."""
    sx, sy = 0.0, 0.0
    for (_, _, x, y, _) in members:
        sx = sx + x
        sy = sy + y
    mx = sx / float(len(members))
    my = sy / float(len(members))
    sc = 0.0
    for (_, _, x, y, size) in members:
        ax = abs(x - mx)
        ay = abs(y - my)
        e = (ax if ax > ay else ay) + size / 2.0
        if e > sc:
            sc = e
    return mx, my, sc


def classify(records, bundle, families):
    """Per record of the frame, in the canonical order: None (no member of the bundle), or (member, used)."""
    lookup = {(int(m[0]), int(m[1])): m for m in bundle["members"]}
    keys = [(families.index(r["family"]), int(r["id"])) for r in records]
    out = []
    for i, r in enumerate(records):
        m = lookup.get(keys[i])
        if m is None:
            out.append(None)
            continue
        dup = (i > 0 and keys[i - 1] == keys[i]) or (i + 1 < len(records) and keys[i + 1] == keys[i])
        gates = int(r["hamming"]) <= int(bundle.get("max_hamming", 2)) and \
            f32(r["decision_margin"]) >= f32(bundle.get("min_decision_margin", 0.0))
        out.append((m, gates and not dup))
    return out


def rows_of(member, p, norm, intr, skew):
    """The eight rows r (nine entries each) of one used record: corner 0 r0, corner 0 r1, corner 1 r0, ..."""
    mx, my, sc = norm
    fx, fy, cx, cy = intr
    _, _, x, y, size = member
    hs = size / 2.0
    rows = []
    for k in range(4):
        xb = x + hs * CORNERS[k][0]
        yb = y + hs * CORNERS[k][1]
        X = (xb - mx) / sc
        Y = (yb - my) / sc
        u, v = float(p[k][0]), float(p[k][1])
        vn = (v - cy) / fy
        un = ((u - cx) - skew * vn) / fx
        rows.append([X, Y, 1.0, 0.0, 0.0, 0.0, -X * un, -Y * un, un])
        rows.append([0.0, 0.0, 0.0, X, Y, 1.0, -X * vn, -Y * vn, vn])
    return rows


def normal_equations(used, norm, intr, skew):
    """[M | b] as 8 rows of 9: per used record the sum of r^T r | r^T rhs over its eight rows, then the records in order."""
    M = [[0.0] * 9 for _ in range(8)]
    for member, p in used:
        Md = [[0.0] * 9 for _ in range(8)]
        for r in rows_of(member, p, norm, intr, skew):
            for i in range(8):
                for j in range(i, 9):
                    Md[i][j] = Md[i][j] + r[i] * r[j]
        for i in range(8):
            for j in range(i, 9):
                M[i][j] = M[i][j] + Md[i][j]
    for i in range(8):
        for j in range(i):
            M[i][j] = M[j][i]
    return M


def eliminate(A):
    """homography_compute2's pivoted Gaussian elimination and back-substitution on the 8 x 9 system; None where it refuses."""
    A = [row[:] for row in A]
    for col in range(8):
        max_val, max_idx = 0.0, -1
        for row in range(col, 8):
            val = abs(A[row][col])
            if val > max_val:
                max_val, max_idx = val, row
        if max_val < 1e-10:
            return None
        if max_idx != col:
            A[col], A[max_idx] = A[max_idx], A[col]
        for i in range(col + 1, 8):
            f = A[i][col] / A[col][col]
            A[i][col] = 0.0
            for j in range(col + 1, 9):
                A[i][j] = A[i][j] - f * A[col][j]
    for col in range(7, -1, -1):
        s = 0.0
        for i in range(col + 1, 8):
            s = s + A[col][i] * A[i][8]
        A[col][8] = (A[col][8] - s) / A[col][col]
    return [A[i][8] for i in range(8)] + [1.0]


def sq_err(used, R, t, intr, skew):
    fx, fy, cx, cy = intr
    total = 0.0
    for member, p in used:
        _, _, x, y, size = member
        hs = size / 2.0
        e = []
        for k in range(4):
            xb = x + hs * CORNERS[k][0]
            yb = y + hs * CORNERS[k][1]
            xc = (R[0] * xb + R[1] * yb) + t[0]
            yc = (R[3] * xb + R[4] * yb) + t[1]
            zc = (R[6] * xb + R[7] * yb) + t[2]
            xn = xc / zc
            yn = yc / zc
            u = (fx * xn + skew * yn) + cx
            v = fy * yn + cy
            du = u - float(p[k][0])
            dv = v - float(p[k][1])
            e.append(du * du + dv * dv)
        total = total + (((e[0] + e[1]) + e[2]) + e[3])
    return total


def solve(records, bundle, families, intrinsics, skew=0.0, bundle_index=0, corner_of=lambda k: k):
    """The bundle record of one frame.  intrinsics (fx, fy, cx, cy) and skew as the C ABI carries them (f32); corner_of: which record
    corner is board corner k (the identity; tests of the tests pass another)."""
    intr = tuple(f32(v) for v in intrinsics)
    skew = f32(skew)
    norm = normalisation(bundle["members"])
    cls = classify(records, bundle, families)
    used = [(c[0], [records[i]["p"][corner_of(k)] for k in range(4)]) for i, c in enumerate(cls) if c is not None and c[1]]
    out = {"bundle": bundle_index, "status": SOLVED, "ntags": len(used), "nskipped": sum(1 for c in cls if c is not None and not c[1]),
           "R": np.zeros((3, 3)), "t": np.zeros(3), "sq_err_sum": 0.0, "h": None}
    if len(used) < int(bundle.get("min_tags", 1)):
        out["status"] = TOO_FEW_TAGS
        return out
    h = eliminate(normal_equations(used, norm, intr, skew))
    if h is None:
        out["status"] = SINGULAR
        return out
    mx, my, sc = norm
    R, tc = po.pose_from_homography(h, 1.0, 1.0, 0.0, 0.0, 2.0 * sc)
    R = [float(v) for v in R.reshape(-1)]
    t = [float(tc[i]) - (R[3 * i] * mx + R[3 * i + 1] * my) for i in range(3)]
    out.update(R=np.array(R).reshape(3, 3), t=np.array(t), sq_err_sum=sq_err(used, R, t, intr, skew), h=h)
    return out


def compare(got, want):
    """Mismatch strings between a library record (detector.bundle_poses) and solve()'s; empty: equal, bit for bit."""
    errs = []
    for k in ("bundle", "status", "ntags", "nskipped"):
        if got[k] != want[k]:
            errs.append("bundle %d: %s %r, the reference has %r: they differ" % (want["bundle"], k, got[k], want[k]))
    for k in ("R", "t"):
        if not np.array_equal(got[k], want[k]):
            errs.append("bundle %d: %s differ by %.3e" % (want["bundle"], k, float(np.abs(got[k] - want[k]).max())))
    if not np.array_equal(np.float64(got["sq_err_sum"]), np.float64(want["sq_err_sum"])):
        errs.append("bundle %d: sq_err_sum %r, the reference has %r: they differ" % (want["bundle"], got["sq_err_sum"], want["sq_err_sum"]))
    return errs


def rot_err(R, R_true):
    return float(np.abs(np.asarray(R) - np.asarray(R_true)).max())


def rms(rec):
    return math.sqrt(rec["sq_err_sum"] / (4.0 * rec["ntags"])) if rec["ntags"] else 0.0
