"""What tests/test_decode_families_gpu.py rests on, on the oracle alone (no GPU, nothing compiled): on the frames of
tests/decode_family_cases.py the oracle finds every tag as a quad and answers, for every tag of every family at max_hamming 0 .. 3, what
the scan of tests/decode_lookup_cases.py answers for the word as first read; and a census, asserted, of what those frames reach in
k_decode_wave -- records at the limit of max_hamming, every rotation, ties inside one lane of the code scan and across lanes, a
64-bit word turned with data bit 63 white, border samples beyond index 63 that matter -- so that no GPU case is vacuous.  The three
wrong builds 56 - 58 (csrc/tools_hooks.h) are restated in Python and held against the right form on the cases they must fail and pass."""
import os
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

import decode_cases as dcs  # noqa: E402
import decode_family_cases as fc  # noqa: E402
import decode_lookup_ref as ref  # noqa: E402

CASES = [(n, mh) for n in fc.NAMES for mh in fc.MAX_HAMMINGS]
_IDS = ["%s-mh%d" % c for c in CASES]
# Where "at least 20 records at the limit" cannot hold: dense16 has 3 000 codes of 16 bits, 3 000 * (1 + 16 + 120) / 65 536 = 6.3 codes
# within two bits of any word, so next to no word has its nearest code three bits away.
NO_LIMIT_CENSUS = {("dense16", 3)}
# Where every result rotation can have 20 records: a family whose words have one answer at any max_hamming (std52, d8, d7); the dense
# families only while acceptance is sparse enough for the scan to get past rotation 0 -- d3 has 20 codes, so at max_hamming 0 at most
# 20 words per rotation exist at all, and from max_hamming 2 on (dense16: 1) nearly every word is accepted unturned.  d7's word list
# holds 82 words that are a code in some orientation (40 exact, 42 turned), 20 per rotation only if every one were drawn: from 1 on.
ROTATION_CENSUS = {"d3": (1,), "h5": (2, 3), "dense16": (0,), "std52": (0, 1, 2, 3), "d8": (0, 1, 2, 3), "d7": (1, 2, 3)}


def _tags(name, mh):
    """(tags, observed, first-read orientations, expected rows) of a family at max_hamming."""
    tg, ob = fc.tags(name), fc.oracle_observed(name, mh)
    orient = [fc.read_orientation(t, o["near"]) for t, o in zip(tg, ob)]
    return tg, ob, orient, fc.expected_rows(name, mh, orient)


def _read_word(name, tag, orientation, turns=0):
    f = fc.family(name)
    return ref.rotations(fc.words(name)[tag["word"]], f["rot_src"])[(orientation + turns) % 4]


# ---- the cases themselves ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.NAMES)
def test_selection_and_frames(name):
    """400 distinct words with every kind among them; at most 14 frames of 640 x 480; 30 tags a frame for d8 and 70 for d3; every tag
    inside its frame, 10 px from the next; d7 is the classic entry point's limit."""
    sel, kd, lay, tg, imgs = fc.selection(name), fc.kinds(name), fc.layout(name), fc.tags(name), fc.frames(name)
    assert len(sel) == fc.NWORDS == len(set(sel.tolist())) == len(tg)
    assert {kd[i] for i in sel} == {"exact", "flipped", "turned", "mid", "edge", "random"}
    assert len(imgs) <= 14 and all(img.shape == (fc.H, fc.W) and img.dtype == np.uint8 for img in imgs)
    per = lay["cols"] * lay["rows"]
    assert per == {"d3": 70, "d8": 30}.get(name, per) and len(imgs) == -(-fc.NWORDS // per)
    assert lay["x0"] >= 0 and lay["y0"] >= 0 and lay["x0"] + lay["cols"] * (lay["side"] + fc.GAP) - fc.GAP <= fc.W
    assert lay["y0"] + lay["rows"] * (lay["side"] + fc.GAP) - fc.GAP <= fc.H
    assert Counter(t["k"] for t in tg)[3] >= 90
    f = fc.family(name)
    assert 8 * f["width_at_border"] <= 80 and f["total_width"] ** 2 <= 144      # the kernel's LDS arrays
    if name == "d7":
        assert (f["nbits"], f["width_at_border"], f["total_width"], len(f["codes"])) == (49, 9, 11, 200)
    if name == "d8":
        assert (f["nbits"], f["width_at_border"], f["total_width"]) == (64, 10, 12)


@pytest.mark.parametrize("name,mh", CASES, ids=_IDS)
def test_the_oracle_answers_the_scan_on_every_tag(name, mh):
    """Every tag is a quad of the oracle; its record -- exactly one on the tag's border square where the scan accepts the word as first
    read, none where it rejects it -- carries the scan's id, hamming and rotation."""
    tg, ob, orient, exp = _tags(name, mh)
    bad = [(j, fc.row_of(o), tuple(e), len(o["records"])) for j, (o, e) in enumerate(zip(ob, exp))
           if fc.row_of(o) != tuple(e) or len(o["records"]) != e[0]]
    print("%s max_hamming %d: %d of %d tags found; %d records inside a tag's square; %d mismatches" %
          (name, mh, sum(e[0] for e in exp), len(tg), sum(o["inner"] for o in ob), len(bad)))
    assert not bad, bad[:5]
    if name in ("std52", "d8", "d7", "h5") or mh == 0:
        assert not any(o["inner"] for o in ob)      # only a dense family decodes a single data cell


def test_read_offset():
    """READ_OFFSET is the only offset between the fitted and the decoded quad's corner numbers under which the oracle's answers are the
    scan's, in each family whose words scan differently from their four orientations; every other offset misses at least 20 tags.  And
    what the exact words alone can say: orientation + rotation = 0 for each whose other orientations are no codes."""
    for name, mh in (("d3", 1), ("dense16", 1), ("h5", 3)):
        tg, ob = fc.tags(name), fc.oracle_observed(name, mh)
        misses = {}
        for off in range(4):
            exp = fc.expected_rows(name, mh, [fc.read_orientation(t, o["near"], off) for t, o in zip(tg, ob)])
            misses[off] = sum(fc.row_of(o, off) != tuple(e) for o, e in zip(ob, exp))
        print(name, "tags whose answer differs from the scan's, per offset:", misses)
        assert misses[fc.READ_OFFSET] == 0 and all(m >= 20 for off, m in misses.items() if off != fc.READ_OFFSET), (name, misses)
    for name in fc.NAMES:
        tg, ob, orient, exp = _tags(name, 0)
        kd, (dist, _) = fc.kinds(name), fc.nearest(name)
        rows = [(o, b) for t, o, b in zip(tg, ob, orient) if kd[t["word"]] == "exact" and (dist[t["word"]] == 0).sum() == 1]
        assert len(rows) >= 3 and all(o["found"] and (b + fc.row_of(o)[3]) % 4 == 0 for o, b in rows), name


# ---- census ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fc.NAMES)
def test_census_limit_and_rotations(name):
    """At least 20 records with hamming = max_hamming for each max_hamming >= 1; at least 20 records at each of the rotations 1, 2 and
    3 (ROTATION_CENSUS); at least 20 tags first read from each orientation."""
    for mh in fc.MAX_HAMMINGS:
        tg, ob, orient, exp = _tags(name, mh)
        at_limit = sum(1 for e in exp if e[0] and e[2] == mh)
        rot = Counter(e[3] for e in exp if e[0])
        print("%s max_hamming %d: %d records at the limit; rotations %s; orientations %s" % (name, mh, at_limit, sorted(rot.items()), sorted(Counter(orient).items())))
        if mh >= 1 and (name, mh) not in NO_LIMIT_CENSUS:
            assert at_limit >= 20
        if mh in ROTATION_CENSUS[name]:
            assert min(rot[r] for r in (1, 2, 3)) >= 20
        assert min(Counter(orient)[b] for b in range(4)) >= 20


def _accepted_ties(name, mh):
    """Per found tag (tied code indices at the accepted rotation, the right id, wrong build 56's id)."""
    tg, ob, orient, exp = _tags(name, mh)
    f = fc.family(name)
    codes = np.array(f["codes"], dtype=np.uint64)
    out = []
    for t, b, e in zip(tg, orient, exp):
        right = fc.kernel_scan(f, _read_word(name, t, b), mh)
        assert right == tuple(e)
        if e[0]:
            hd = ref._popcount_u64(codes ^ np.uint64(_read_word(name, t, b, e[3])))
            out.append((np.flatnonzero(hd == e[2]), e[1], fc.kernel_scan(f, _read_word(name, t, b), mh, lane_keeps_later=True)[1]))
    return out


@pytest.mark.parametrize("mh", (2, 3))
def test_census_dense16_ties(mh):
    """dense16 at max_hamming 2 and 3: at least 20 tags whose winning distance is shared by two codes of one lane (indices congruent
    mod 64) -- there the in-lane rule with <= gives another id -- and at least 20 where the first code's lane holds no second."""
    rows = _accepted_ties("dense16", mh)
    same = [r for r in rows if any(i != r[1] and i % 64 == r[1] % 64 for i in r[0])]
    across = [r for r in rows if len(r[0]) >= 2 and not any(i != r[1] and i % 64 == r[1] % 64 for i in r[0])]
    print("dense16 max_hamming %d: %d found, %d with a tie, %d inside the first code's lane, %d across lanes only" %
          (mh, len(rows), sum(len(r[0]) >= 2 for r in rows), len(same), len(across)))
    assert len(same) >= 20 and len(across) >= 20
    assert all(r[2] != r[1] for r in same) and all(r[2] == r[1] for r in across)


def test_census_d8_bit_63():
    """d8: at least 20 records found after a quarter turn whose first turn moves a white cell onto data bit 63, at every max_hamming."""
    for mh in fc.MAX_HAMMINGS:
        tg, ob, orient, exp = _tags("d8", mh)
        n = sum(1 for t, b, e in zip(tg, orient, exp) if e[0] and e[3] >= 1 and _read_word("d8", t, b, 1) & 1)
        print("d8 max_hamming %d: %d turned reads with data bit 63 white after the first turn" % (mh, n))
        assert n >= 20


_models = {}


def _gray_model_change(name):
    """Per tag (valid border samples at index 64 and above, largest change of a gray-model coefficient when they are dropped)."""
    if name not in _models:
        f, imgs, out = fc.family(name), fc.frames(name), []
        for t, o in zip(fc.tags(name), fc.oracle_observed(name, 0)):
            qd = np.roll(o["quad"], -fc.READ_OFFSET, axis=0)
            w_all, b_all, late = fc.gray_models(f, imgs[t["frame"]], qd)
            w_cut, b_cut, _ = fc.gray_models(f, imgs[t["frame"]], qd, first=64)
            out.append((late, max(np.abs(w_all - w_cut).max(), np.abs(b_all - b_cut).max())))
        _models[name] = out
    return _models[name]


@pytest.mark.parametrize("name", ("d8", "d7"))
def test_census_border_samples_beyond_63(name):
    """d8 and d7: every tag has all its 8 * width_at_border - 64 border samples from index 64 on inside the frame, and without them
    a gray-model coefficient moves by more than 0.01 gray levels -- a threshold that far off is a decision margin that differs in
    its leading digits, where a change in the last bits of a double (all that a frame of exactly two gray values gives) would vanish in
    the margin's float."""
    f = fc.family(name)
    rows = _gray_model_change(name)
    print("%s: smallest change of a coefficient %.4f, median %.4f" % (name, min(r[1] for r in rows), float(np.median([r[1] for r in rows]))))
    assert all(r[0] == 8 * f["width_at_border"] - 64 > 0 for r in rows)
    assert all(r[1] > 0.01 for r in rows)


# ---- the three wrong forms ---------------------------------------------------------------------------------------------------------------------
def test_wrong_form_56_lane_keeps_the_later_code():
    """Differs from the scan on dense16 at max_hamming 2 and 3 (on at least 20 tags); agrees on every h5 tag at every max_hamming
    (30 codes: one per lane) and on the tie word of tests/decode_cases.py."""
    for mh in (2, 3):
        assert sum(r[2] != r[1] for r in _accepted_ties("dense16", mh)) >= 20
    for mh in fc.MAX_HAMMINGS:
        assert all(r[2] == r[1] for r in _accepted_ties("h5", mh))
    h5 = fc.family("h5")
    for mh in (2, 3):
        assert fc.kernel_scan(h5, dcs.tie_word(), mh, lane_keeps_later=True) == fc.kernel_scan(h5, dcs.tie_word(), mh) == ((1, 0, 3, 0) if mh == 3 else ref.NOT_FOUND)


def test_wrong_form_57_turn_without_lane_63():
    """Differs from the scan on d8 (on at least 20 tags at every max_hamming); agrees on every tag of std52 and d7."""
    for name in ("d8", "std52", "d7"):
        f = fc.family(name)
        for mh in fc.MAX_HAMMINGS:
            tg, ob, orient, exp = _tags(name, mh)
            differ = sum(fc.kernel_scan(f, _read_word(name, t, b), mh, turn_drops_lane63=True) != tuple(e) for t, b, e in zip(tg, orient, exp))
            print("%s max_hamming %d: wrong form 57 differs on %d tags" % (name, mh, differ))
            assert differ >= 20 if name == "d8" else differ == 0


def test_wrong_form_58_late_border_samples_invalid():
    """Changes the gray models of every d8 and d7 tag (test_census_border_samples_beyond_63); std52 and dense16 have 48 border samples,
    none at index 64 or above."""
    for name in ("d8", "d7"):
        assert all(r[0] > 0 and r[1] > 0.01 for r in _gray_model_change(name))
    for name in ("std52", "dense16", "h5", "d3"):
        assert 8 * fc.family(name)["width_at_border"] <= 64


# ---- four families in one handle ---------------------------------------------------------------------------------------------------------------
def test_four_families_precondition():
    """h5 and dense16 share one layout: at least 20 quads of the eight frames give two records that differ only in the family, and
    reconcile keeps both; no frame has more records than the handle of the GPU case holds."""
    pairs = kept = 0
    for dets, dump in fc.four_oracle():
        raw = dump["dets_raw"]
        assert len(raw) < fc.FOUR_MAX_DETECTIONS
        by_quad = {}
        for r in raw:
            by_quad.setdefault(r["p"].tobytes(), set()).add(int(r["family"]))
        both = [k for k, fams in by_quad.items() if {0, 1} <= fams]
        pairs += len(both)
        final = {(d["family"], d["p"].tobytes()) for d in dets}
        kept += sum((fc.family("h5")["name"], k) in final and (fc.family("dense16")["name"], k) in final for k in both)
    print("four families: %d quads with a tag16h5 and a dense16 record, both kept on %d" % (pairs, kept))
    assert pairs >= 20 and kept >= 20
