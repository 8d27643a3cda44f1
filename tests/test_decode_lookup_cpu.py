"""The decode stage's code index without a GPU: csrc/code_index.h compiled by a host compiler against
tests/decode_lookup_ref.py -- shape, offsets and index lists byte for byte, lookup results field for field -- on every family of
tests/decode_lookup_cases.py at max_hamming 0 to 3 (and once under AddressSanitizer and UBSan as a program of its own); the reference's
indexed lookup against its own scan on all of it; what the families are there to reach; and the threshold's floor.  (The decode
kernel does not use the index yet: DESIGN.md section 7l.)"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))

from isaac_ros_apriltag_amd import capi  # noqa: E402
import decode_lookup_cases as dc  # noqa: E402
import decode_lookup_ref as ref  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DRIVER = os.path.join(HERE, "aux_c", "code_index_driver.cpp")
HEADER = os.path.join(ROOT, "isaac_ros_apriltag_amd", "csrc", "code_index.h")
CASES = [(n, mh) for n in dc.NAMES for mh in dc.MAX_HAMMINGS]
_cache = {}


def _reference_lookup(name, mh):
    """The reference's indexed lookup of every word of the family: rows of (found, id, hamming, rotation), once per process."""
    if (name, mh) not in _cache:
        f = dc.family(name)
        sh = ref.shape(f["nbits"], mh, len(f["codes"]))
        ix = dc.index_of(name, mh)
        rows = np.array([ref.lookup_index(ix, sh, f["codes"], w4, mh) for w4 in dc.words4(name)], dtype=np.int32).reshape(-1, 4)
        rows.setflags(write=False)
        _cache[(name, mh)] = rows
    return _cache[(name, mh)]


def _write_input(path, name, mh):
    f = dc.family(name)
    w4 = dc.words4(name)
    head = [f["nbits"], mh, len(f["codes"]), len(w4)]
    np.array(head + list(f["codes"]) + [w for ws in w4 for w in ws], dtype="<u8").tofile(path)


def _run_driver(exe, tmp, name, mh, **kw):
    """{"min_codes", "shape", "table", "results"} as the driver wrote them."""
    src, dst = os.path.join(str(tmp), "%s_%d.in" % (name, mh)), os.path.join(str(tmp), "%s_%d.out" % (name, mh))
    _write_input(src, name, mh)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120, **kw)
    assert r.returncode == 0 and not r.stderr and not r.stdout, (name, mh, r.returncode, r.stderr[-3000:])
    out = np.fromfile(dst, dtype="<u4")
    words = int(out[18])
    nw = len(dc.words(name))
    assert out.size == 19 + words + 4 * nw
    return {"min_codes": int(out[0]),
            "shape": {"K": int(out[1]), "lo": out[2:6].tolist(), "keybits": out[6:10].tolist(), "off": out[10:14].tolist(),
                      "ids": out[14:18].tolist(), "words": words},
            "table": out[19:19 + words], "results": out[19 + words:].reshape(nw, 4)}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("code_index") / "code_index_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", DRIVER, "-o", exe])
    return exe


# ---- 1. the header's lines under a host compiler ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mh", CASES)
def test_header_equals_the_reference(driver, tmp_path, name, mh):
    f = dc.family(name)
    got = _run_driver(driver, tmp_path, name, mh)
    assert got["shape"] == ref.shape(f["nbits"], mh, len(f["codes"]))
    assert got["table"].tobytes() == ref.flat_index(dc.index_of(name, mh)).tobytes()     # offsets and index lists, byte for byte
    want = _reference_lookup(name, mh)
    res = got["results"]
    none = res[:, 0] == 0xFFFFFFFF
    assert np.array_equal(~none, want[:, 0] == 1)
    assert np.array_equal(res[:, 3].astype(np.int32), want[:, 1]) and np.array_equal(res[:, 2].astype(np.int32), want[:, 2])
    assert np.array_equal(res[:, 1].astype(np.int32), want[:, 3])
    # the packed form orders candidates as (rotation, hamming, index)
    ok = ~none
    assert np.array_equal(res[ok, 0], (res[ok, 1] << 30) | (res[ok, 2] << 28) | res[ok, 3])


@pytest.mark.parametrize("name,mh", CASES)
def test_reference_index_equals_its_scan(name, mh):
    assert np.array_equal(_reference_lookup(name, mh), dc.expected(name, mh))


def test_vectorised_scan_is_the_plain_scan():
    """decode_lookup_cases.expected comes from numpy (nearest_many); the statement is ref.scan.  All of d3, and a sample of the others."""
    for name in dc.NAMES:
        f, w4 = dc.family(name), dc.words4(name)
        step = 1 if name == "d3" else max(1, len(w4) // (40 if len(f["codes"]) <= 5000 else 8))
        for mh in (dc.MAX_HAMMINGS if name == "d3" else (2,)):
            want = dc.expected(name, mh)
            for i in range(0, len(w4), step):
                assert ref.scan(f["codes"], w4[i], mh) == tuple(int(v) for v in want[i]), (name, mh, i)


def test_header_under_asan_ubsan(tmp_path):
    """The same driver as a program of its own, built with -fsanitize=address,undefined and run here on every family and max_hamming:
    the 64-bit family's shifts, the 16-bit key cap and every table access."""
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    exe = str(tmp_path / "code_index_san")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra"] + san + [DRIVER, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for name, mh in CASES:
        got = _run_driver(exe, tmp_path, name, mh, env=env)
        assert got["table"].tobytes() == ref.flat_index(dc.index_of(name, mh)).tobytes(), (name, mh)


def test_a_family_of_fewer_bits_than_chunks(driver, tmp_path):
    """nbits < K: the chunks without bits have one bucket that holds every code (2 bits at max_hamming 3: lengths 0, 1, 0, 1)."""
    codes, words4 = [0, 1, 2, 3, 1], [(w, w, w, w) for w in range(4)]
    src, dst = str(tmp_path / "tiny.in"), str(tmp_path / "tiny.out")
    np.array([2, 3, len(codes), len(words4)] + codes + [w for ws in words4 for w in ws], dtype="<u8").tofile(src)
    subprocess.check_call([driver, src, dst])
    out = np.fromfile(dst, dtype="<u4")
    sh = ref.shape(2, 3, len(codes))
    assert sh["keybits"] == [0, 1, 0, 1] and out[6:10].tolist() == sh["keybits"] and int(out[18]) == sh["words"]
    assert out[19:19 + sh["words"]].tobytes() == ref.flat_index(ref.build_index(codes, 2, 3)).tobytes()
    res = out[19 + sh["words"]:].reshape(4, 4)
    for i, w4 in enumerate(words4):
        want = ref.scan(codes, w4, 3)
        assert (1, int(res[i, 3]), int(res[i, 2]), int(res[i, 1])) == want == (1, i, 0, 0)


# ---- 2. what the families are there to reach ---------------------------------------------------------------------------------------------------
def test_families_reach_what_they_are_for():
    for name in dc.NAMES:
        f = dc.family(name)
        src = f["rot_src"]
        assert sorted(src) == list(range(f["nbits"])), name                         # closed under the quarter turn
        w = f["codes"][0]
        assert ref.rotate(ref.rotations(w, src)[3], src) == w, name                 # four turns are the identity
        assert 3000 <= len(dc.words(name)) <= 7000 or name == "d3", (name, len(dc.words(name)))
    assert ref.shape(9, 3, 20)["keybits"] == [2, 2, 2, 3]
    sh = ref.shape(52, 2, 20000)
    assert sh["keybits"] == [16, 16, 16, 0] and [sh["lo"][j] for j in range(3)] == [0, 17, 34]
    assert dc.family("d8")["nbits"] == 64 and ref.shape(64, 3, 5000)["lo"] == [0, 16, 32, 48]
    codes16 = dc.family("dense16")["codes"]
    assert len(set(codes16)) < len(codes16) == 3000                                  # duplicates kept
    # buckets beyond one wave's worth of candidates, at max_hamming 2 and 3
    for mh in (2, 3):
        sh = ref.shape(16, mh, 3000)
        ix = dc.index_of("dense16", mh)
        assert max(ref.candidates(ix, sh, w) for w in dc.words("dense16")[::5]) > 64
    # every rotation and every distance up to max_hamming is some word's answer, and some words are not found
    for name in ("h5", "std52", "d8"):
        e = dc.expected(name, 3)
        found = e[e[:, 0] == 1]
        assert set(found[:, 3].tolist()) == {0, 1, 2, 3} and set(found[:, 2].tolist()) == {0, 1, 2, 3} and len(found) < len(e), name
    # ties: words equally near two or more codes at the scan's best distance, resolved to the lowest index -- a third of d3's words, half
    # of dense16's (duplicates among them)
    for name, share in (("d3", 3), ("dense16", 2)):
        codes = np.array(dc.family(name)["codes"], dtype=np.uint64)
        dist, _ = dc.nearest(name)
        ties = sum(1 for i, w4 in enumerate(dc.words4(name)) if int((ref._popcount_u64(codes ^ np.uint64(w4[0])) == dist[i, 0]).sum()) > 1)
        assert share * ties > len(dist), (name, ties, len(dist))


# ---- 3. the threshold ------------------------------------------------------------------------------------------------------------------------
def test_threshold_is_above_every_built_in_table(driver, tmp_path):
    got = _run_driver(driver, tmp_path, "d3", 0)
    text = open(HEADER).read()
    m = re.search(r"^#define AMDAT_INDEX_MIN_CODES (\d+)u?\s*$", text, flags=re.M)
    assert m and int(m.group(1)) == got["min_codes"] >= 588
    for fam in ("tag36h11", "tag25h9", "tag16h5"):
        assert len(capi.family_info(fam)["codes"]) < got["min_codes"]
