"""The tag table without a GPU: csrc/tag_table.h compiled by a host compiler against tests/tag_table_ref.py --
sorted keys, sizes and every lookup, bit for bit -- on the tables of tests/tag_table_cases.py (and once under AddressSanitizer and
UBSan as a program of its own); every refusal of tt_build; the ABI; and, on the oracle, the preconditions of the GPU cases of
tests/test_tag_table_gpu.py, so that none of them is vacuous."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

from isaac_ros_apriltag_amd import capi  # noqa: E402
import bundle_cases as bc  # noqa: E402
import pose_refine_cases as pc  # noqa: E402
import pose_refine_ref as pr  # noqa: E402
import reconcile_cases as rcs  # noqa: E402
import tag_table_cases as tc  # noqa: E402
import tag_table_ref as tt  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DRIVER = os.path.join(HERE, "aux_c", "tag_table_driver.cpp")
INVALID_ARGUMENT = 1


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def _run(exe, tmp, name, num_families, ncodes, entries, queries, **kw):
    """(refused, keys, size bits, [(listed, size bits)]) as the driver wrote them."""
    src, dst = os.path.join(str(tmp), name + ".in"), os.path.join(str(tmp), name + ".out")
    words = [num_families] + list(ncodes) + list(struct.unpack("<II", struct.pack("<d", tc.DEFAULT))) + [len(entries), len(queries)]
    for fi, tid, size in entries:
        words += [fi, tid, struct.unpack("<I", np.float32(size).tobytes())[0]]
    for fam, tid in queries:
        words += [fam, tid]
    np.array(words, dtype="<u4").tofile(src)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120, **kw)
    assert r.returncode == 0 and not r.stderr and not r.stdout, (name, r.returncode, r.stderr[-3000:])
    out = np.fromfile(dst, dtype="<u8")
    if out[0]:
        assert out.size == 1
        return True, None, None, None
    n = int(out[1])
    assert out.size == 2 + 2 * n + 2 * len(queries)
    res = out[2 + 2 * n:].reshape(-1, 2)
    return False, out[2:2 + n].tolist(), out[2 + n:2 + 2 * n].tolist(), [(int(a), int(b)) for a, b in res]


def _check(exe, tmp, name, **kw):
    nf, ncodes, entries, _ = tc.TABLES[name]
    queries = tc.queries(name)
    refused, keys, sizes, res = _run(exe, tmp, name, nf, ncodes, entries, queries, **kw)
    table = tt.build(nf, ncodes, entries)
    assert not refused and table is not None
    assert keys == sorted(table) and sizes == [_bits(table[k]) for k in keys]     # sorted by key, the sizes beside them
    want = [tt.lookup(table, f, i, tc.DEFAULT) for f, i in queries]
    assert res == [(int(l), _bits(s)) for s, l in want], name
    return table, queries, want


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tag_table") / "tag_table_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", DRIVER, "-o", exe])
    return exe


# ---- 1. the header's lines under a host compiler ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(tc.TABLES))
def test_header_equals_the_reference(driver, tmp_path, name):
    _check(driver, tmp_path, name)


def test_the_tables_reach_what_they_are_for(driver, tmp_path):
    t = {n: _check(driver, tmp_path, n) for n in tc.TABLES}
    look = lambda n, f, i: t[n][2][t[n][1].index((f, i))]
    assert len(t["empty"][0]) == 0 and all(w == (tc.DEFAULT, False) for w in t["empty"][2])
    assert len(t["one"][0]) == 1 and len(t["full_4096"][0]) == tt.MAX_ENTRIES == 4096
    assert look("first_and_last_key", 0, 0) == (tt.f32(0.05), True) and look("first_and_last_key", 1, 34) == (tt.f32(0.11), True)
    assert look("absent_between_two", 0, 11) == (tc.DEFAULT, False) and look("absent_between_two", 0, 10)[1] and look("absent_between_two", 0, 12)[1]
    assert look("same_id_two_families", 0, 3) == (tt.f32(0.05), True) and look("same_id_two_families", 1, 3) == (tt.f32(0.11), True)
    assert look("family_3_and_id_65534", 3, 65534) == (tt.f32(0.3), True) and look("family_3_and_id_65534", 3, 65533) == (tc.DEFAULT, False)
    assert look("wildcard_alone", 1, 0) == (tt.f32(0.09), True) and look("wildcard_alone", 0, 0) == (tc.DEFAULT, False)
    assert look("wildcard_beside_exact", 0, 2) == (tt.f32(0.05), True) and look("wildcard_beside_exact", 0, 3) == (tt.f32(0.1), True)   # exact beats the wildcard
    assert look("wildcard_beside_exact", 1, 8) == (tc.DEFAULT, False)
    assert look("size_zero", 0, 4) == (tc.DEFAULT, True) and look("size_zero", 1, 3) == (tc.DEFAULT, True) and look("size_zero", 1, 2) == (tt.f32(0.12), True)
    # the wildcard itself, a family beyond the key and an id beyond it are no tags: never listed
    assert look("wildcard_alone", 1, tt.ID_ANY) == (tc.DEFAULT, False) and look("full_4096", 4, 0) == (tc.DEFAULT, False)
    assert look("full_4096", 3, 70000) == (tc.DEFAULT, False)
    ent = tc.TABLES["unsorted"][2]
    assert [tt.key(f, i) for f, i, _ in ent] != sorted(tt.key(f, i) for f, i, _ in ent)
    big = tc.TABLES["full_4096"][2]
    assert {f for f, _, _ in big} == {0, 1, 2, 3} and (3, 65534) in {(f, i) for f, i, _ in big}
    # sizes are the double of the float: 0.05 is not
    assert tt.f32(0.05) != 0.05 and look("first_and_last_key", 0, 0)[0] == float(np.float32(0.05))


@pytest.mark.parametrize("name", sorted(tc.REFUSED))
def test_build_refuses(driver, tmp_path, name):
    nf, ncodes, entries = tc.REFUSED[name]
    assert tt.build(nf, ncodes, entries) is None
    assert _run(driver, tmp_path, name, nf, ncodes, entries, [(0, 0)])[0]
    # and the same entries without the offending one are taken (the refusal is that entry's)
    if name != "one_entry_too_many":
        assert tt.build(nf, ncodes, entries[:-1]) is not None and not _run(driver, tmp_path, name + "_less", nf, ncodes, entries[:-1], [(0, 0)])[0]
    else:
        assert not _run(driver, tmp_path, name + "_less", nf, ncodes, entries[:-1], [(3, 4095), (3, 4096)])[0]


def test_header_under_asan_ubsan(tmp_path):
    """The same driver as a program of its own, built with -fsanitize=address,undefined and run here on every table and refusal: the
    key and size arrays have exactly as many slots as entries, so a search step or an insertion outside them is reported."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    exe = str(tmp_path / "tag_table_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra"] + san + [DRIVER, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name in sorted(tc.TABLES):
        _check(exe, tmp_path, name, env=env)
    for name, (nf, ncodes, entries) in sorted(tc.REFUSED.items()):
        assert _run(exe, tmp_path, name, nf, ncodes, entries, [(0, 0)], env=env)[0], name


@pytest.mark.parametrize("mutant,name,differs", [(53, "first_and_last_key", (1, 34)), (53, "wildcard_alone", (1, 0)), (54, "wildcard_beside_exact", (0, 2))])
def test_the_wrong_builds_forms_differ(tmp_path, mutant, name, differs):
    """The header with -DAMDAT_MUTATE=53 / 54 is the reference's wrong form, and differs from the right one on the named lookup only
    where stated: 53 where the table's last key is looked up, 54 where an exact entry sits beside its family's wildcard."""
    exe = str(tmp_path / ("tag_table_mut%d" % mutant))
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-DAMDAT_MUTATE=%d" % mutant, DRIVER, "-o", exe])
    for n in sorted(tc.TABLES):
        nf, ncodes, entries, _ = tc.TABLES[n]
        queries = tc.queries(n)
        table = tt.build(nf, ncodes, entries)
        res = _run(exe, tmp_path, n, nf, ncodes, entries, queries)[3]
        wrong = [tt.lookup_without_last(table, f, i, tc.DEFAULT) if mutant == 53 else tt.lookup(table, f, i, tc.DEFAULT, wildcard_first=True)
                 for f, i in queries]
        assert res == [(int(l), _bits(s)) for s, l in wrong], n
        right = [tt.lookup(table, f, i, tc.DEFAULT) for f, i in queries]
        where = {q for q, a, b in zip(queries, wrong, right) if a != b}
        if n == name:
            assert differs in where
        if mutant == 53:   # only lookups that the last key answers: the last entry's own, or (a wildcard last) its family's others
            last = max(table) if table else None
            assert all(tt.key(f, i) == last or (last & 0xFFFF) == tt.ID_ANY and (last >> 16) == f for f, i in where), (n, where)
        else:              # only exact entries beside a wildcard of their family
            assert all(tt.key(f, i) in table and tt.key(f, tt.ID_ANY) in table for f, i in where), (n, where)


# ---- 2. the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_struct_layout_and_exports(tmp_path):
    names = ("family_index", "id", "size", "reserved")
    lines = ['printf("%zu", sizeof(amdAprilTagsTagEntry_t));'] + ['printf(" %%zu", offsetof(amdAprilTagsTagEntry_t, %s));' % n for n in names]
    lines.append('printf(" %u %u", AMDAT_MAX_TAG_ENTRIES, AMDAT_TAG_ID_ANY);')
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "apriltag_amd.h"\nint main(void){ %s return 0; }\n' % " ".join(lines))
    exe = str(tmp_path / "s")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    row = [int(v) for v in subprocess.check_output([exe]).decode().split()]
    assert row == [C.sizeof(capi.TagEntry)] + [getattr(capi.TagEntry, n).offset for n in names] + [capi.MAX_TAG_ENTRIES, capi.TAG_ID_ANY]
    assert row[0] == 16 and (capi.MAX_TAG_ENTRIES, capi.TAG_ID_ANY) == (tt.MAX_ENTRIES, tt.ID_ANY) == (4096, 0xFFFF)
    assert "amdAprilTagsSetTagTable" in capi.EXPORTS


def test_library_exports_and_refuses_without_a_device(built):
    L = capi.lib()
    e = (capi.TagEntry * 1)()
    assert L.amdAprilTagsSetTagTable(None, 0, None, 0) == INVALID_ARGUMENT
    assert L.amdAprilTagsSetTagTable(None, 1, e, 0) == INVALID_ARGUMENT


def test_python_expands_names_wildcards_and_ranges():
    arr = capi.tag_entries([("tag25h9", (2, 4), 0.1), (0, "*", 0.0), ("tag36h11", 7, 0.05)], ["tag36h11", "tag25h9"])
    assert [(e.family_index, e.id, float(e.size), e.reserved) for e in arr] == \
        [(1, 2, tt.f32(0.1), 0), (1, 3, tt.f32(0.1), 0), (1, 4, tt.f32(0.1), 0), (0, 0xFFFF, 0.0, 0), (0, 7, tt.f32(0.05), 0)]
    assert capi.tag_entries(None, ["tag36h11"]) is None and capi.tag_entries([], ["tag36h11"]) is None
    with pytest.raises(ValueError):
        capi.tag_entries([("tag36h11", "all", 0.1)], ["tag36h11"])


# ---- 3. the preconditions of the GPU cases, on the oracle ---------------------------------------------------------------------------------
def _ids(recs):
    return [int(r["id"]) for r in recs]


def test_content_frames_hold_what_the_gpu_cases_claim():
    fams = list(bc.FAM)
    assert _ids(bc.content_records("all_six")) == [0, 1, 2, 3, 4, 5]
    assert _ids(bc.content_records("painted_over")) == [0, 1, 2, 3, 5]
    assert _ids(bc.content_records("non_member")) == [0, 1, 2, 3, 4, 5, bc.LONE_ID]
    assert sorted(_ids(bc.content_records("duplicate"))) == [0, 1, 1, 2, 3, 4, 5]
    assert any(r["hamming"] == 1 for r in bc.content_records("hamming")) and bc.content_records("no_tags") == []
    # the sizes tables: each gives at least three distinct sizes on all_six, the default among them; "exact" has the lone tag's key last
    for which in tc.CONTENT_TABLES:
        table = tc.table_of(tc.CONTENT_TABLES[which], fams)
        sizes = {tc.size_of(table, fams, r, bc.SIZE1) for r in bc.content_records("non_member")}
        assert len(sizes) >= 3 and tt.f32(bc.SIZE1) in sizes, (which, sizes)
    assert max(tc.table_of(tc.CONTENT_TABLES["exact"], fams)) == tt.key(0, bc.LONE_ID)
    wild = tc.table_of(tc.CONTENT_TABLES["wild"], fams)
    assert max(wild) == tt.key(0, tt.ID_ANY) and wild[tt.key(0, 3)] == 0.0
    # listed-only: non_member holds a record that is not listed (the lone tag) and listed ones; all_six loses id 4; the parent's cut
    # to three records would lose id 5, which the filtered list's first three hold
    listed = tc.table_of(tc.LISTED, fams)
    keep = lambda name: [r for r in bc.content_records(name) if tc.listed(listed, fams, r)]
    assert _ids(keep("non_member")) == [0, 1, 2, 3, 5] and _ids(keep("all_six")) == [0, 1, 2, 3, 5]
    assert sorted(_ids(keep("duplicate"))) == [0, 1, 1, 2, 3, 5] and len(keep("hamming")) == 5 and keep("no_tags") == []
    assert 5 not in _ids(bc.content_records("all_six")[:5]) and 5 in _ids(keep("all_six")[:5])


def test_two_sizes_differ_in_t_and_in_the_refined_record():
    recs, refined, covs = tc.content_sized("all_six", "exact")
    base = bc.content_records("all_six")
    base_ref = pc.content_refined("all_six")
    for i, r in enumerate(base):
        resized = int(r["id"]) in (1, 4, 5)
        assert np.array_equal(recs[i]["R"], r["R"]) and np.array_equal(recs[i]["p"], r["p"])       # the size scales t alone
        assert np.array_equal(recs[i]["t"], r["t"]) != resized
        assert (not pr.compare(refined[i], base_ref[i])) != resized
    assert any(not np.array_equal(c["cov"], d["cov"]) for c, d in zip(covs, tc.content_sized("all_six", "wild")[2]))


def test_board72_has_three_sizes_and_72_records():
    recs, refined, _ = tc.board72_sized()
    assert len(recs) == 72 == len(bc.records72()) and len(refined) == 72
    moved = [not np.array_equal(a["t"], b["t"]) for a, b in zip(recs, bc.records72())]
    assert [m for m in moved] == [int(r["id"]) % 3 != 0 for r in recs]     # id % 3 == 0 keeps the handle's size


def test_two_family_frame_decodes_id_3_in_both_families():
    for which in tc.TWO_FAMILY_TABLES:
        recs = tc.two_family_sized(which)[0]
        assert [(r["family"], int(r["id"])) for r in recs] == [("tag36h11", 3), ("tag36h11", 11), ("tag25h9", 3), ("tag25h9", 8)]
        t = {(r["family"], int(r["id"])): r["t"] for r in recs}
        # the same pixels size, 80 px: depth follows the tag's size, 0.05 and 0.16 for the two id 3
        assert abs(t[("tag36h11", 3)][2] / t[("tag25h9", 3)][2] - 0.05 / 0.16) < 0.01
    a, b = tc.two_family_sized("exact")[0], tc.two_family_sized("wild_on_family_1")[0]
    assert np.array_equal(a[2]["t"], b[2]["t"]) and not np.array_equal(a[3]["t"], b[3]["t"])     # tag25h9 id 8: default, then the wildcard's


def test_wrong_builds_forms_differ_on_the_named_gpu_cases():
    def differs(name, which, lookup):
        return [i for i, (a, b) in enumerate(zip(tc.content_sized(name, which)[0], tc.content_sized(name, which, lookup)[0]))
                if not np.array_equal(a["t"], b["t"])]
    # 53: under "exact" only the lone tag of non_member has the last key; under "wild" the wildcard is last, and every frame with tags has
    # a tag that only the wildcard lists
    assert differs("non_member", "exact", tc.size_without_last) == [6]
    assert all(not differs(n, "exact", tc.size_without_last) for n in bc.CONTENT if n != "non_member")
    assert all(differs(n, "wild", tc.size_without_last) for n in bc.CONTENT if n != "no_tags")
    # 54: never under "exact" (no wildcard); under "wild" the exact entries 2, 3 and 5, present in every frame with tags
    assert all(not differs(n, "exact", tc.size_wildcard_first) for n in bc.CONTENT)
    assert all(differs(n, "wild", tc.size_wildcard_first) for n in bc.CONTENT if n != "no_tags")
    # 55: a refined record at the handle's size differs from the one at the table's, the detection record does not enter it
    recs, refined, _ = tc.content_sized("all_six", "exact")
    assert any(pr.compare(a, b) for a, b in zip(refined, pc.content_refined("all_six")))


def test_reconcile_records_interleave_listed_and_unlisted_ids():
    rec = rcs.random_case(rcs.MAX_DETECTIONS)
    table = tt.build(2, (587, 35), tc.RECONCILE_ENTRIES)
    flags = [tt.lookup(table, int(r["family"]), int(r["id"]), 0.0)[1] for r in rec]
    assert 40 < sum(flags) < len(rec) - 40
    import reconcile_ref as ref
    kept = ref.reconcile(rec)
    kept_flags = [flags[i] for i in kept]
    assert True in kept_flags and False in kept_flags and len(kept) < len(rec)     # overlaps removed, both kinds kept
    assert sum(1 for a, b in zip(kept_flags, kept_flags[1:]) if a != b) >= 3           # runs of listed and unlisted ids alternate


def test_oblique_frame_for_the_nodes():
    (recs, refined, _), table = tc.oblique_sized()
    assert _ids(recs) == [3, 8, 21, 34] and [tc.listed(table, list(bc.FAM), r) for r in recs] == [True, False, True, True]
    base = pc.oblique_records()
    assert [not np.array_equal(a["t"], b["t"]) for a, b in zip(recs, base)] == [True, False, False, True]
