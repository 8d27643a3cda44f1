"""The reconcile step on records the test chooses, without a GPU: tests/reconcile_ref.py (plain Python) and the oracle's ato_reconcile
agree on every case of tests/reconcile_cases.py -- kept set, order, every field -- each crafted case gives the outcome its entry
writes out, no two crafted cases are one case shifted, and the random cases remove and keep enough to mean something.
tests/test_reconcile_gpu.py runs the same cases through k_reconcile."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

from oracle import pyoracle as po  # noqa: E402
import reconcile_cases as rcs  # noqa: E402
import reconcile_ref as ref  # noqa: E402


params, expected_records, same_records = rcs.params, rcs.expected_records, rcs.same_records


@pytest.mark.parametrize("name", sorted(rcs.CRAFTED))
def test_crafted_case(built, name):
    records, kept = rcs.crafted(name)
    assert ref.reconcile(records) == kept or same_records(records[ref.reconcile(records)], records[kept])   # (a duplicate: either index)
    want = expected_records(records)
    assert len(want) == len(kept) and all(np.array_equal(want[f], records[kept][f]) for f in ("family", "id", "hamming", "decision_margin", "H", "c", "p"))
    got = po.reconcile(records, params())
    assert same_records(got, want), (name, got[["id", "decision_margin"]], want[["id", "decision_margin"]])
    assert np.isfinite(got["R"]).all() and np.isfinite(got["t"]).all() and (got["t"][:, 2] > 0).all()


def test_crafted_coordinates_are_small_integers():
    for name in rcs.CRAFTED:
        p = rcs.crafted(name)[0]["p"]
        assert np.array_equal(p, np.round(p)) and np.abs(p).max() < 1024, name


def test_no_two_crafted_cases_are_one_case_shifted():
    """Each case as (family, id, hamming, margin, corners relative to the case's smallest x and y), in input order, plus its outcome."""
    seen = {}
    for name in sorted(rcs.CRAFTED):
        records, kept = rcs.crafted(name)
        origin = records["p"].reshape(-1, 2).min(axis=0)
        key = (tuple((int(r["family"]), int(r["id"]), int(r["hamming"]), float(r["decision_margin"]), (r["p"] - origin).tobytes()) for r in records),
               tuple(kept))
        assert key not in seen, (name, seen.get(key))
        seen[key] = name
    assert len(seen) == len(rcs.CRAFTED) >= 16


def test_each_part_of_the_overlap_rule_decides_some_case():
    """The crafted geometry reaches what its name says: which part of the rule (crossing, touching, containment) fires."""
    def parts(name):
        rec = rcs.crafted(name)[0]
        first, second = sorted(range(2), key=lambda i: ref.order_key(rec[i]))   # the rule is asked (kept record, candidate)
        a, b = ref._quad(rec[first]), ref._quad(rec[second])
        cross = touch = False
        for i in range(4):
            for j in range(4):
                p1, p2, q1, q2 = a[i], a[(i + 1) % 4], b[j], b[(j + 1) % 4]
                d = [ref._side_of(q1, q2, p1), ref._side_of(q1, q2, p2), ref._side_of(p1, p2, q1), ref._side_of(p1, p2, q2)]
                proper = ref._opposite(d[0], d[1]) and ref._opposite(d[2], d[3])
                cross |= proper
                touch |= ref.sides_meet(p1, p2, q1, q2) and not proper
        return cross, touch, ref.corner_inside(a, b[0]), ref.corner_inside(b, a[0])
    assert parts("disjoint_both_kept") == (False, False, False, False)
    assert parts("crossing_edges") == (True, False, False, False)
    assert parts("b_strictly_inside_a") == (False, False, True, False)
    assert parts("a_strictly_inside_b") == (False, False, False, True)   # (the preferred record is the inner quad)
    for name in ("touching_in_one_corner", "corner_on_an_edge", "shared_collinear_edge_piece"):
        assert parts(name) == (False, True, False, False), name
    assert parts("collinear_edges_that_do_not_meet") == (False, False, False, False)
    # the containment cases are decided with room to spare: the inner quad is at least 9 pixels from every side of the outer one
    for name in ("b_strictly_inside_a", "a_strictly_inside_b"):
        p = rcs.crafted(name)[0]["p"]
        outer, inner = (0, 1) if np.ptp(p[0][:, 0]) > np.ptp(p[1][:, 0]) else (1, 0)
        assert (p[inner].min(axis=0) - p[outer].min(axis=0)).min() >= 9 and (p[outer].max(axis=0) - p[inner].max(axis=0)).min() >= 9


@pytest.mark.parametrize("n", rcs.RANDOM_COUNTS)
def test_random_case(built, n):
    records = rcs.random_case(n)
    assert len(records) == n
    kept = ref.reconcile(records)
    if n >= 63:
        print("n %d: kept %d, removed %d" % (n, len(kept), n - len(kept)))
        assert 4 * len(kept) >= n and 4 * (n - len(kept)) >= n, (n, len(kept))
        # ties in (family, id, hamming, margin) reach the corner keys, and a few records are exact duplicates
        head = [ref.order_key(r)[:4] for r in records]
        assert len(set(head)) < n and len({r.tobytes() for r in records}) < n
    want = expected_records(records)
    got = po.reconcile(records, params())
    assert same_records(got, want), (n, len(got), len(want))


def test_more_than_64_records_in_one_run(built):
    """The largest random case has runs of one (family, id) whose kept records alone are more than a handful, and 256 records need
    four trips of a 64-wide rank sort."""
    records = rcs.random_case(rcs.MAX_DETECTIONS)
    kept = records[ref.reconcile(records)]
    runs = {}
    for r in kept:
        runs[(int(r["family"]), int(r["id"]))] = runs.get((int(r["family"]), int(r["id"])), 0) + 1
    assert len(runs) == 8 and min(runs.values()) >= 4, runs
