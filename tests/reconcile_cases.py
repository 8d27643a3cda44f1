"""Shared by tests/test_reconcile_cpu.py and tests/test_reconcile_gpu.py: records handed to the reconcile step on its own
(ato_reconcile, amdAprilTagsDebugReconcile, tests/reconcile_ref.py).  Crafted cases carry small integer coordinates, so every product
and difference of the overlap rule is exact, and each names what it reaches and writes its outcome out; random cases are seeded.
Everything is built once per process and never changed."""
import numpy as np

from oracle import pyoracle as po
import reconcile_ref as ref

DTYPE = po.RECORD_DTYPE
MAX_DETECTIONS = 256            # the GPU handle's capacity; the largest random case fills it
INTRINSICS = (600.0, 610.0, 320.0, 240.0)   # fx, fy, cx, cy of the handle and of ato_reconcile's parameters
TAG_SIZE = 0.16


def sq(x0, y0, s):
    """Axis-parallel square [x0, x0 + s] x [y0, y0 + s] in the records' corner order (y down: H(-1,1), H(1,1), H(1,-1), H(-1,-1))."""
    return [(x0, y0 + s), (x0 + s, y0 + s), (x0 + s, y0), (x0, y0)]


def rect(x0, y0, x1, y1):
    return [(x0, y1), (x1, y1), (x1, y0), (x0, y0)]


def diamond(cx, cy, r):
    return [(cx - r, cy), (cx, cy + r), (cx + r, cy), (cx, cy - r)]


def record(family, tid, hamming, margin, quad):
    """One decoded record: H is a mild projective map about the quad's centre (reconcile reads it only for the pose), R and t zero."""
    r = np.zeros((), dtype=DTYPE)
    q = np.asarray(quad, dtype=np.float64)
    cx, cy = q[:, 0].mean(), q[:, 1].mean()
    half = 0.5 * max(np.ptp(q[:, 0]), np.ptp(q[:, 1]), 1.0)
    r["family"], r["id"], r["hamming"], r["decision_margin"] = family, tid, hamming, margin
    r["H"] = [half, 0.25, cx, -0.5, half, cy, 0.0005, 0.001, 1.0]
    r["c"] = [cx, cy]
    r["p"] = q
    return r


def _records(rows):
    return np.array([record(*row) for row in rows], dtype=DTYPE) if rows else np.zeros(0, dtype=DTYPE)


# name -> (rows (family, id, hamming, margin, quad) in INPUT order, indices of the kept records in OUTPUT order)
_PLUS_A, _PLUS_B = rect(0, 10, 40, 20), rect(15, 0, 25, 30)   # a plus sign: four proper crossings, no corner of one inside the other
CRAFTED = {
    "disjoint_both_kept": ([(0, 1, 0, 80.0, sq(10, 10, 20)), (0, 1, 0, 70.0, sq(50, 10, 20))], [0, 1]),
    "crossing_edges": ([(0, 1, 0, 80.0, _PLUS_A), (0, 1, 0, 70.0, _PLUS_B)], [0]),
    # containment alone: no side meets a side, no two sides share a line; the preferred record is the outer one, then the inner one
    "b_strictly_inside_a": ([(0, 1, 0, 80.0, sq(0, 0, 40)), (0, 1, 0, 70.0, sq(13, 11, 10))], [0]),
    "a_strictly_inside_b": ([(0, 1, 0, 50.0, sq(100, 200, 40)), (0, 1, 0, 90.0, sq(117, 209, 10))], [1]),
    "touching_in_one_corner": ([(0, 1, 0, 80.0, sq(0, 0, 10)), (0, 1, 0, 70.0, sq(10, 10, 10))], [0]),
    "corner_on_an_edge": ([(0, 1, 0, 80.0, sq(0, 0, 10)), (0, 1, 0, 70.0, diamond(15, 5, 5))], [0]),
    "shared_collinear_edge_piece": ([(0, 1, 0, 80.0, sq(0, 0, 10)), (0, 1, 0, 70.0, rect(10, 5, 20, 15))], [0]),
    "collinear_edges_that_do_not_meet": ([(0, 1, 0, 80.0, sq(0, 0, 10)), (0, 1, 0, 70.0, sq(10, 20, 10))], [0, 1]),
    "crossing_under_another_id": ([(0, 2, 0, 70.0, _PLUS_B), (0, 1, 0, 80.0, _PLUS_A)], [1, 0]),
    "crossing_under_another_family": ([(1, 1, 0, 80.0, _PLUS_A), (0, 1, 0, 70.0, _PLUS_B)], [1, 0]),
    # A overlaps B, B overlaps C, A and C are apart; preference A, B, C: B goes, so C has nothing kept to overlap
    "chain_c_survives": ([(0, 1, 0, 90.0, sq(0, 0, 10)), (0, 1, 0, 80.0, sq(8, 1, 10)), (0, 1, 0, 70.0, sq(16, 2, 10))], [0, 2]),
    # three (family, id) runs: the last record of run one is removed; the first record of run two lies on a kept record of run one and
    # stays, as does run three's, which lies on kept records of both earlier runs; run two's second record is apart
    "runs_do_not_see_each_other": ([(0, 1, 0, 90.0, sq(0, 0, 10)), (0, 1, 0, 80.0, sq(5, 5, 10)), (0, 2, 0, 90.0, sq(2, 2, 10)),
                                    (0, 2, 0, 80.0, sq(100, 0, 10)), (0, 3, 0, 90.0, sq(4, 4, 10))], [0, 2, 3, 4]),
    # the order keys, one pair each, the other keys arranged to point the wrong way (input order, margin, corners)
    "lower_hamming_beats_higher_margin": ([(0, 1, 1, 90.0, sq(0, 0, 10)), (0, 1, 0, 10.0, sq(5, 5, 10))], [1]),
    "higher_margin_wins": ([(0, 1, 0, 30.0, sq(0, 0, 10)), (0, 1, 0, 60.0, sq(5, 5, 10))], [1]),
    "equal_margin_first_differing_corner": ([(0, 1, 0, 40.0, sq(10, 12, 10)), (0, 1, 0, 40.0, sq(10, 8, 10))], [1]),
    "exact_duplicate_leaves_one": ([(0, 1, 0, 40.0, sq(3, 4, 10)), (0, 1, 0, 40.0, sq(3, 4, 10))], [0]),
}

RANDOM_COUNTS = (0, 1, 2, 63, 64, 65, 130, MAX_DETECTIONS)
MARGINS = (12.5, 31.0, 31.25, 77.0)
_cache = {}


def crafted(name):
    if name not in _cache:
        rows, kept = CRAFTED[name]
        _cache[name] = (_records(rows), list(kept))
        _cache[name][0].setflags(write=False)
    return _cache[name]


def _convex_quad(rng, cx, cy, r):
    """Four points on a circle of radius r at increasing angles (one per quadrant, jittered): convex, any orientation of its sides."""
    ang = rng.uniform(0, 2 * np.pi) + np.arange(4) * (np.pi / 2) + rng.uniform(-0.5, 0.5, 4)
    rad = r * rng.uniform(0.7, 1.0, 4)
    return np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1)


def random_case(n, seed=None):
    """n records: jittered copies (shifted by a few pixels, or shrunk about the centre so that they lie inside) of n // 20 + 1 random
    convex quads in a 1000 x 1000 area, families {0, 1}, ids {0 .. 3}, hamming {0, 1, 2}, margins from a set of four, and a few exact
    duplicates of records drawn before."""
    key = ("random", n, seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(20240611 + 7919 * n if seed is None else seed)
    nbase = n // 20 + 1
    bases = [_convex_quad(rng, rng.uniform(100, 900), rng.uniform(100, 900), rng.uniform(50, 90)) for _ in range(nbase)]
    rows = []
    for i in range(n):
        if i >= 4 and rng.uniform() < 0.06:
            rows.append(rows[int(rng.integers(0, i))])
            continue
        q = bases[int(rng.integers(0, nbase))]
        kind = rng.uniform()
        if kind < 0.5:
            q = q + rng.uniform(-3, 3, (1, 2)) + rng.uniform(-0.5, 0.5, (4, 2))
        else:
            c = q.mean(axis=0)
            q = c + (q - c) * rng.uniform(0.3, 0.8) + (rng.uniform(-3, 3, (1, 2)) if kind < 0.75 else 0.0)
        rows.append((int(rng.integers(0, 2)), int(rng.integers(0, 4)), int(rng.integers(0, 3)), MARGINS[int(rng.integers(0, 4))], q))
    rec = _records(rows)
    rec.setflags(write=False)
    _cache[key] = rec
    return rec


# ---- what both test files expect ------------------------------------------------------------------------------------------------------
def params():
    fx, fy, cx, cy = INTRINSICS
    return po.default_params(fx=fx, fy=fy, cx=cx, cy=cy, tag_size=float(np.float32(TAG_SIZE)))


def expected_records(records, prm=None):
    """The reference's kept records in order, with the pose the oracle's pose statement gives each (the reference states order and
    overlap; the pose has its own tests)."""
    prm = prm or params()
    out = records[ref.reconcile(records)].copy()
    for r in out:
        R, t = po.pose_from_homography(r["H"], prm.fx, prm.fy, prm.cx, prm.cy, prm.tag_size, prm.skew)
        r["R"], r["t"] = R.reshape(-1), t
    return out


def same_records(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
