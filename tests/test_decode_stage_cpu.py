"""The preconditions of tests/test_decode_stage_gpu.py on the oracle alone: the frames of tests/decode_cases.py reach what they are
built for -- the border tags decode, the tag16h5 word resolves to the intended (id, hamming) at every turn, the nested duplicate
gives two raw records and one kept, the overflow frames hold more decodable tags than the small handle has room for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import decode_cases as dc  # noqa: E402


def _border_found(decimate, refine, sigma):
    out = {}
    for name, img in dc.border_cases(sigma, decimate):
        odets, dump = dc.oracle_on(("border", name, sigma), img, dc.FAM36, decimate, refine_edges=refine)
        out[name] = [d["id"] for d in odets] == [5] and len(dump["dets_raw"]) == 1
    return out


def test_the_oracle_finds_the_border_tags(built):
    """At least 90 % of the listed cases, and every case at a listed gap of 2 px or more at decimate 1.  Printed: per placement the
    smallest listed gap at which the oracle keeps the tag in every variant."""
    total, found, smallest = 0, 0, {}
    for decimate, refine in dc.BORDER_SETTINGS:
        for sigma in dc.SIGMAS:
            res = _border_found(decimate, refine, sigma)
            total += len(res)
            found += sum(res.values())
            for gname, pl, turned, gap in dc.border_geometries():
                ok = all(res["%s_px%d" % (gname, p0)] for p0 in dc.PIXEL0)
                if decimate == 1 and gap >= 2.0:
                    assert ok, (gname, decimate, refine, sigma)
                smallest.setdefault((decimate, pl, turned), {}).setdefault(gap, True)
                smallest[(decimate, pl, turned)][gap] &= ok
    for (decimate, pl, turned), gaps in sorted(smallest.items()):
        kept = [g for g in sorted(gaps) if all(gaps[h] for h in gaps if h >= g)]
        print("decimate %d %-12s %-6s smallest listed gap kept: %s" % (decimate, pl, "turned" if turned else "axis", kept[0] if kept else None))
    print("found %d of %d" % (found, total))
    assert total == 8 * 7 * 2 * 2 * 4 and 10 * found >= 9 * total, (found, total)


def test_gap_moves_are_small_and_listed():
    for (decimate, pl, turned, gap), used in dc.MOVED_GAPS.items():
        assert decimate == 2 and pl in dc.PLACEMENTS and gap in (dc.TURNED_GAPS if turned else dc.AXIS_GAPS) and 0 < used - gap <= 1.0


def test_border_tags_reach_the_frame_edge():
    """What makes these cases border cases: the quiet ring (one cell, 10 px) is cut by the frame edge in every one, and the gap is
    within the normal search of the refinement (decimate + 1 pixels either way, plus one for the gradient) in most."""
    ring = 2 * dc.HALF / 8
    for decimate in (1, 2):
        used = [dc.MOVED_GAPS.get((decimate, pl, turned, gap), gap) for _, pl, turned, gap in dc.border_geometries()]
        assert max(used) < ring / 2 and sum(g <= decimate + 2 for g in used) * 2 > len(used)


def test_the_large_border_tag(built):
    img = dc.large_frame()
    odets, dump = dc.oracle_on("large", img, dc.FAM36, 1)
    assert [d["id"] for d in odets] == [5]
    side = np.linalg.norm(odets[0]["p"][0] - odets[0]["p"][1])
    assert side > 136 * 2 and odets[0]["p"].min() < 4   # more than 2 x 17 refinement samples a side: a second chunk of 64


def test_tie_word_resolves_to_the_first_code(built):
    codes = dc.codes16()
    c0, c15 = codes[dc.TIE_IDS[0]], codes[dc.TIE_IDS[1]]
    assert bin(c0 ^ c15).count("1") == 6
    w = dc.tie_word()
    assert w is not None and bin(w ^ c0).count("1") == 3 and bin(w ^ c15).count("1") == 3
    assert min(bin(w ^ c).count("1") for c in codes) == 3   # no code nearer: a 3/3 tie decided by the order of the scan
    for turns in range(4):
        img = dc.word_frame(w, turns)
        odets, dump = dc.oracle_on(("tie", turns), img, dc.FAM16, 1, max_hamming=3)
        assert [(d["id"], d["hamming"]) for d in odets] == [(0, 3)], (turns, odets)
        none, _ = dc.oracle_on(("tie", turns), img, dc.FAM16, 1, max_hamming=2)
        assert none == []
    # the four turns give four different corner orders: the rotation the decoder found is in H
    firsts = {tuple(np.round(dc.oracle_on(("tie", t), dc.word_frame(w, t), dc.FAM16, 1, max_hamming=3)[0][0]["p"][0]).tolist()) for t in range(4)}
    assert len(firsts) == 4


def test_no_tag16h5_word_is_a_turned_code_near_another_code():
    """The search the rotation order would need: a word that is a code exactly after one to three quarter turns but within 3 bits of
    another code unturned.  tag16h5 has none (its generator keeps every rotation of a code at distance 5 or more from every other
    code), so no frame can show that rotation 0 is tried first with a DIFFERENT id; the tie word's four turns show the order itself."""
    assert dc.turned_exact_words() == []
    codes = dc.codes16()
    near = min(bin(dc.turn_word(c) ^ o).count("1") for i, c in enumerate(codes) for j, o in enumerate(codes) if i != j)
    assert near >= 5


@pytest.mark.parametrize("k", dc.NESTED_IDS)
def test_nested_duplicate(built, k):
    odets, dump = dc.oracle_on(("nested", k, k), dc.nested_frame(k, k), dc.FAM36, 1)
    raw = dump["dets_raw"]
    assert [int(i) for i in raw["id"]] == [k, k] and len(odets) == 1
    diag = np.linalg.norm(odets[0]["p"][0] - odets[0]["p"][2])
    assert 60 < diag < 75, diag   # the small tag survives
    odets2, dump2 = dc.oracle_on(("nested", k, k + 1), dc.nested_frame(k, k + 1), dc.FAM36, 1)
    assert sorted(d["id"] for d in odets2) == [k, k + 1] and len(dump2["dets_raw"]) == 2
    assert sorted(round(float(np.linalg.norm(d["p"][0] - d["p"][2]))) for d in odets2) == [68, 849]


def test_overflow_frames(built):
    f0, f1 = dc.overflow_frames()
    o0, d0 = dc.oracle_on("overflow0", f0, dc.FAM36, 1)
    o1, d1 = dc.oracle_on("overflow1", f1, dc.FAM36, 1)
    assert len(d0["dets_raw"]) >= 8 > dc.OVERFLOW_CAPACITY and sorted(d["id"] for d in o0) == list(range(10, 18))
    assert len(d1["dets_raw"]) == 2 and sorted(d["id"] for d in o1) == [20, 21]


def test_wrong_builds_21_to_24_are_declared():
    from isaac_ros_apriltag_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hooks = open(os.path.join(root, "isaac_ros_apriltag_amd", "csrc", "tools_hooks.h")).read()
    for n in (21, 22, 23, 24):
        assert n in build.MUTANTS and "AMDAT_MUTATE == %d" % n in hooks


def test_unsuffixed_oracle_symbols_keep_the_shorter_dump(built):
    """ato_dump_t grew by dets_raw; the library keeps ato_detect / ato_dump_free for a binding built with the struct that ends after
    `dets` (oracle/apriltag_oracle.h).  They fill the same stages as the suffixed entry and leave every byte beyond `dets` alone."""
    import ctypes as C
    from isaac_ros_apriltag_amd import synth
    from oracle import pyoracle as po
    img = np.ascontiguousarray(synth.scene_c1()[0])
    h, w = img.shape
    L, prm, fam = po.lib(), po.default_params(decimate=2), (po.Family * 1)(po.family("tag36h11"))
    short = po.Dump.ndet_raw.offset
    assert short == po.Dump.dets.offset + C.sizeof(C.c_void_p)
    guard = b"\xa5" * 64
    buf = C.create_string_buffer(b"\x5a" * short + guard, short + len(guard))
    out, out2, full = (po.Detection * 8)(), (po.Detection * 8)(), po.Dump()
    args = (C.byref(prm), fam, 1, img.ctypes.data, w, h, img.strides[0])
    L.ato_detect.argtypes = L.ato_detect_v2.argtypes[:-1] + [C.c_void_p]
    L.ato_dump_free.argtypes = [C.c_void_p]
    assert L.ato_detect(*args, out, 8, buf) == L.ato_detect_v2(*args, out2, 8, C.byref(full)) == 1
    assert bytes(out) == bytes(out2) and buf.raw[short:] == guard
    got = po.Dump.from_buffer_copy(buf.raw[:short] + bytes(C.sizeof(po.Dump) - short))
    for name in ("w", "h", "nclusters", "npoints", "nquads", "ndet"):
        assert getattr(got, name) == getattr(full, name) > 0, name
    assert bytes(got.dets[0]) == bytes(full.dets[0]) == bytes(out[0]) and full.ndet_raw == 1
    L.ato_dump_free(buf)
    L.ato_dump_free_v2(C.byref(full))
    assert buf.raw == bytes(short) + guard and bytes(full) == bytes(C.sizeof(po.Dump))
