"""Shared by tests/test_tag_table_cpu.py and tests/test_tag_table_gpu.py: the seeded tables of the header test, the tables of the GPU
cases, and the per-size references of their frames -- each reference run once per distinct size, record i taken from the run of its
own size (the kept order does not depend on the size), computed once per process and never changed afterwards."""
import math

import numpy as np

from isaac_ros_apriltag_amd import capi, synth
from oracle import pyoracle as po
import bundle_cases as bc
import parity_util as pu
import pose_cov_ref as pv
import pose_refine_cases as pc
import pose_refine_ref as pr
import tag_table_ref as tt

_cache = {}
ANY = tt.ID_ANY
SIGMA = 0.3

# ---- 1. tables of the header test: name -> (num_families, ncodes, entries in INPUT order, queries (family, id)) -------------------------
NCODES = (587, 35, 30, 65535)     # tag36h11, tag25h9, tag16h5, a registered family of the largest admitted size
DEFAULT = tt.f32(0.22)


def _all_queries(entries, extra=()):
    """Every entry's own key, its neighbours, id 0 and the last id of every family, ids that cannot be keys."""
    q = set(extra)
    for fi, tid, _ in entries:
        for d in (-1, 0, 1):
            if 0 <= tid + d < ANY:
                q.add((fi, tid + d))
    for fi in range(5):
        q |= {(fi, 0), (fi, 65534), (fi, ANY), (fi, 70000)}
    return sorted(q)


def _big():
    """4096 entries over four families, unsorted: all of tag36h11, all of tag25h9, all of tag16h5, the rest from the large family."""
    rng = np.random.default_rng(4096)
    rows = [(0, i, 0.05 + 0.001 * (i % 7)) for i in range(587)] + [(1, i, 0.1) for i in range(35)] + [(2, i, 0.0) for i in range(30)]
    ids3 = rng.choice(65535, size=4096 - len(rows) - 1, replace=False)
    ids3[0] = 65534
    rows += [(3, int(i), 0.02 + 0.0001 * int(i % 97)) for i in ids3] + [(3, ANY, 0.5)]
    order = rng.permutation(len(rows))
    return [rows[i] for i in order]


TABLES = {
    "empty": (4, NCODES, [], [(0, 0), (3, 65534), (4, 1)]),
    "one": (1, NCODES, [(0, 17, 0.16)], None),
    "first_and_last_key": (2, NCODES, [(0, 0, 0.05), (0, 9, 0.07), (1, 34, 0.11)], None),
    "absent_between_two": (1, NCODES, [(0, 10, 0.05), (0, 12, 0.07)], [(0, 9), (0, 10), (0, 11), (0, 12), (0, 13)]),
    "same_id_two_families": (2, NCODES, [(1, 3, 0.11), (0, 3, 0.05)], None),
    "family_3_and_id_65534": (4, NCODES, [(3, 65534, 0.3), (3, 0, 0.2), (0, 586, 0.1)], None),
    "wildcard_alone": (2, NCODES, [(1, ANY, 0.09)], None),
    "wildcard_beside_exact": (2, NCODES, [(0, ANY, 0.1), (0, 2, 0.05), (0, 5, 0.16), (1, 7, 0.2)], None),
    "size_zero": (2, NCODES, [(0, 4, 0.0), (1, ANY, 0.0), (1, 2, 0.12)], None),
    "unsorted": (3, NCODES, [(2, 29, 0.03), (0, 500, 0.05), (1, 0, 0.07), (0, 1, 0.09), (2, 0, 0.11), (0, 250, 0.13)], None),
    "full_4096": (4, NCODES, _big(), None),
}

# what tt_build refuses: name -> (num_families, ncodes, entries)
REFUSED = {
    "duplicate_key": (1, NCODES, [(0, 3, 0.05), (0, 7, 0.05), (0, 3, 0.07)]),
    "duplicate_wildcard": (2, NCODES, [(1, ANY, 0.05), (1, ANY, 0.05)]),
    "family_beyond_the_handle": (2, NCODES, [(0, 3, 0.05), (2, 0, 0.05)]),
    "family_4": (4, NCODES, [(4, 0, 0.05)]),
    "id_at_the_code_count": (1, NCODES, [(0, 587, 0.05)]),
    "id_beyond_the_wildcard": (4, NCODES, [(3, 0x10000, 0.05)]),
    "negative_size": (1, NCODES, [(0, 3, -0.05)]),
    "infinite_size": (1, NCODES, [(0, 3, math.inf)]),
    "nan_size": (1, NCODES, [(0, 3, math.nan)]),
    "one_entry_too_many": (4, NCODES, [(3, i, 0.05) for i in range(4097)]),
}


def queries(name):
    nf, ncodes, entries, q = TABLES[name]
    return q if q is not None else _all_queries(entries)


# ---- 2. the GPU cases' tables, as AprilTagDetector.set_tag_table takes them ---------------------------------------------------------------
# content frames (bundle_cases): ids 0 .. 5 on the board, LONE_ID 7 in non_member, a second id 1 in duplicate; the handle's size is SIZE1.
# "exact": two sizes on some ids, the rest at the default; its last key is the lone tag's, which only non_member looks up.
# "wild": a wildcard (the table's last key) beside exact entries and one size-0 entry.
CONTENT_TABLES = {
    "exact": [("tag36h11", 1, 0.05), ("tag36h11", 4, 0.05), ("tag36h11", 5, 0.16), ("tag36h11", bc.LONE_ID, 0.1)],
    "wild": [("tag36h11", "*", 0.1), ("tag36h11", 2, 0.05), ("tag36h11", 3, 0.0), ("tag36h11", 5, 0.16)],
}
# the 72-tag board: three sizes by id % 3
BOARD72_SIZES = (0.048, 0.03, 0.12)
BOARD72_TABLE = [("tag36h11", i, BOARD72_SIZES[i % 3]) for i in range(72)]
# listed-only on the content frames: the board's ids but 4, which painted_over lacks anyway and all_six has; not the lone tag
LISTED = [("tag36h11", (0, 3), 0.05), ("tag36h11", 5, 0.0)]


def table_of(tags, families):
    """{key: size} of a set_tag_table list (names, "*", ranges) for a handle of `families`."""
    rows = []
    for fam, tid, size in tags:
        fi = families.index(fam) if isinstance(fam, str) else int(fam)
        ids = [ANY] if tid == "*" else list(range(tid[0], tid[1] + 1)) if isinstance(tid, tuple) else [tid]
        rows += [(fi, i, size) for i in ids]
    ncodes = [len(capi.family_info(f)["codes"]) for f in families]
    table = tt.build(len(families), ncodes, rows)
    assert table is not None
    return table


def size_of(table, families, rec, default):
    return tt.lookup(table, families.index(rec["family"]), int(rec["id"]), tt.f32(default))[0]


def listed(table, families, rec):
    return tt.lookup(table, families.index(rec["family"]), int(rec["id"]), 0.0)[1]


def sized(key, img, intr, skew, default, table, families=bc.FAM, lookup=None):
    """(records, refined records, covariance records) of a frame under a table: the oracle, pose_refine_ref and pose_cov_ref run once
    per distinct size on the whole frame, record i taken from the run of its own size.  lookup: another form of size_of (the wrong
    builds' forms, for the preconditions)."""
    lookup = lookup or size_of
    k = ("sized", key)
    if k in _cache:
        return _cache[k]
    runs = {}

    def run(s):
        if s not in runs:
            recs = _oracle(img, intr, skew, s, families)
            ref = pr.refine_records(recs, intr, skew, s, pc.ITERATIONS)
            cov = pv.tag_records(recs, intr, skew, s, ref, SIGMA)
            runs[s] = (recs, ref, cov)
        return runs[s]
    base = run(tt.f32(default))[0]
    out = ([], [], [])
    for i, r in enumerate(base):
        got = run(lookup(table, list(families), r, default))
        assert len(got[0]) == len(base) and got[0][i]["id"] == r["id"] and np.array_equal(got[0][i]["p"], r["p"])   # the kept order does not depend on the size
        for o, g in zip(out, got):
            o.append(g[i])
    _cache[k] = out
    return out


def _oracle(img, intr, skew, size, families):
    k = ("oracle", id(img), tuple(intr), skew, size, tuple(families))
    if k not in _cache:
        if tuple(families) == tuple(bc.FAM):
            _cache[k] = bc.oracle_records(img, intr, skew, tag_size=size)
        else:
            K = np.array([[intr[0], 0, intr[2]], [0, intr[1], intr[3]], [0, 0, 1.0]])
            _cache[k] = po.detect(img, families=tuple(families), params=pu.oracle_params(K, tag_size=size))[0]
    return _cache[k]


def content_sized(name, which, lookup=None):
    """The references of a content frame under CONTENT_TABLES[which] (or LISTED: sizes only, the filter is the caller's)."""
    slot = bc.SLOTS[name][1]
    tags = LISTED if which == "listed" else CONTENT_TABLES[which]
    key = ("content", name, which, lookup.__name__ if lookup else "")
    return sized(key, bc.content_frame(name), bc.INTR1[slot], bc.SKEW1[slot], bc.SIZE1, table_of(tags, list(bc.FAM)), lookup=lookup)


def board72_sized():
    return sized("board72", bc.frame72(), bc.INTR2, 0.0, bc.SIZE2, table_of(BOARD72_TABLE, list(bc.FAM)))


# ---- 3. the two-family frame: tag36h11 id 3 and tag25h9 id 3 among others ------------------------------------------------------------------
FAMS2 = ("tag36h11", "tag25h9")
W3, H3 = 640, 480
INTR3 = (600.0, 600.0, 320.0, 240.0)
SIZE3 = 0.08
TWO_FAMILY_TAGS = (("tag36h11", 3, 150.0, 130.0), ("tag25h9", 3, 470.0, 130.0), ("tag36h11", 11, 150.0, 350.0), ("tag25h9", 8, 470.0, 350.0))
TWO_FAMILY_TABLES = {
    "exact": [("tag36h11", 3, 0.05), ("tag25h9", 3, 0.16)],
    "wild_on_family_1": [("tag36h11", 3, 0.05), (1, "*", 0.16)],
}


def two_family_frame():
    if "frame2" not in _cache:
        tags = [{"family": f, "id": i, "H": np.array([[40.0, 0, cx], [0, 40.0, cy], [0, 0, 1.0]])} for f, i, cx, cy in TWO_FAMILY_TAGS]
        _cache["frame2"] = np.ascontiguousarray(synth.render(W3, H3, tags, background=150, sigma=1.0, seed=53))
    return _cache["frame2"]


def two_family_sized(which):
    return sized(("two", which), two_family_frame(), INTR3, 0.0, SIZE3, table_of(TWO_FAMILY_TABLES[which], list(FAMS2)), families=FAMS2)


# ---- 4. the oblique frame of the node test: ids 3, 8, 21, 34 ------------------------------------------------------------------------------
NODE_TAGS = [(3, 0.05, "dock_left"), (21, 0.0, ""), (34, 0.2, "tote_34")]     # (id, size, frame); id 8 is not listed


def oblique_sized():
    table = table_of([("tag36h11", i, s) for i, s, _ in NODE_TAGS], list(bc.FAM))
    return sized("oblique", pc.oblique_frame(), pc.INTR_O, 0.0, pc.SIZE_O, table), table


# ---- 5. amdAprilTagsDebugReconcile on reconcile_cases' records (families 0, 1; ids 0 .. 3): entries (family_index, id, size) ------------
RECONCILE_ENTRIES = [(0, 0, 0.05), (0, 2, 0.0), (1, 1, 0.3), (1, 3, 0.16)]


# ---- 6. the forms of the wrong builds (tag_table_ref) as size_of's -----------------------------------------------------------------------
def size_without_last(table, families, rec, default):
    return tt.lookup_without_last(table, families.index(rec["family"]), int(rec["id"]), tt.f32(default))[0]


def size_wildcard_first(table, families, rec, default):
    return tt.lookup(table, families.index(rec["family"]), int(rec["id"]), tt.f32(default), wildcard_first=True)[0]
