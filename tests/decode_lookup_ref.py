"""The decode stage's code lookup in plain Python integers (csrc/code_index.h states the same in C++): the index
build, the indexed lookup and the brute-force scan it must equal.

A family is a list of code words of `nbits` bits.  A word is looked up as its four rotations words4 = [w, turn(w), turn(turn(w)), ...]
(rotations(): bit i, counted from the MSB, takes the value of bit rot_src[i]).  Every lookup returns (found, id, hamming, rotation),
(0, 0, 0, 0) where nothing lies within max_hamming.

scan():         rotations 0 .. 3 in turn; per rotation the lowest index at the smallest distance, accepted within max_hamming.
build_index():  K = max_hamming + 1 chunks; chunk j covers bits [j * nbits // K, (j + 1) * nbits // K) from the LSB; its key is the low
                min(length, 16) bits of the chunk; per chunk offsets[2^keybits + 1] and the code indices grouped by key, ascending
                inside a bucket.
lookup_index(): the candidates of the K buckets at the word's keys, for each rotation; the smallest (rotation, hamming, index) among
                those within max_hamming.
nearest_many(): the scan's (distance, index) of many words at once in numpy, for the tests' large families; scan_from_nearest() turns
                it into scan()'s answer (tests/test_decode_lookup_cpu.py holds the two against each other).
"""
import numpy as np

MAX_KEY_BITS = 16
MAX_CHUNKS = 4
NOT_FOUND = (0, 0, 0, 0)


def popcount(x):
    return bin(x).count("1")


def rotate(word, rot_src):
    n, out = len(rot_src), 0
    for i in range(n):
        if (word >> (n - 1 - rot_src[i])) & 1:
            out |= 1 << (n - 1 - i)
    return out


def rotations(word, rot_src):
    out = [word]
    for _ in range(3):
        out.append(rotate(out[-1], rot_src))
    return out


def unrotate(word, rot_src, turns):
    """The word that becomes `word` after `turns` rotations."""
    inv = [0] * len(rot_src)
    for i, s in enumerate(rot_src):
        inv[s] = i
    for _ in range(turns):
        word = rotate(word, inv)
    return word


def scan(codes, words4, max_hamming):
    for r, w in enumerate(words4):
        best, bid = 1 << 30, 1 << 30
        for i, c in enumerate(codes):
            hd = popcount(w ^ c)
            if hd < best:
                best, bid = hd, i
        if best <= max_hamming:
            return (1, bid, best, r)
    return NOT_FOUND


def shape(nbits, max_hamming, ncodes):
    """The chunks and where their tables lie in the index's array of 32-bit words (CodeIndexShape)."""
    K = max_hamming + 1
    lo, keybits, off, ids = [0] * MAX_CHUNKS, [0] * MAX_CHUNKS, [0] * MAX_CHUNKS, [0] * MAX_CHUNKS
    at = 0
    for j in range(K):
        a, b = j * nbits // K, (j + 1) * nbits // K
        lo[j], keybits[j] = a, min(b - a, MAX_KEY_BITS)
        off[j] = at
        ids[j] = at + (1 << keybits[j]) + 1
        at = ids[j] + ncodes
    return {"K": K, "lo": lo, "keybits": keybits, "off": off, "ids": ids, "words": at}


def key(word, lo, keybits):
    return (word >> lo) & ((1 << keybits) - 1)


def build_index(codes, nbits, max_hamming):
    """[(offsets, ids)] per chunk."""
    sh = shape(nbits, max_hamming, len(codes))
    out = []
    for j in range(sh["K"]):
        buckets = {}
        for i, c in enumerate(codes):
            buckets.setdefault(key(c, sh["lo"][j], sh["keybits"][j]), []).append(i)
        offsets, ids = [0], []
        for k in range(1 << sh["keybits"][j]):
            ids += buckets.get(k, [])
            offsets.append(len(ids))
        out.append((offsets, ids))
    return out


def flat_index(index):
    """The index as the one array of 32-bit words the library uploads: per chunk its offsets, then its indices."""
    words = []
    for offsets, ids in index:
        words += offsets + ids
    return np.array(words, dtype="<u4")


def lookup_index(index, sh, codes, words4, max_hamming):
    best = None
    for r, w in enumerate(words4):
        for j, (offsets, ids) in enumerate(index):
            k = key(w, sh["lo"][j], sh["keybits"][j])
            for i in ids[offsets[k]:offsets[k + 1]]:
                hd = popcount(w ^ codes[i])
                if hd <= max_hamming and (best is None or (r, hd, i) < best):
                    best = (r, hd, i)
    return NOT_FOUND if best is None else (1, best[2], best[1], best[0])


def candidates(index, sh, word):
    """How many candidates one word has (with repeats: a code near the word sits in several of its buckets)."""
    return sum(offsets[key(word, sh["lo"][j], sh["keybits"][j]) + 1] - offsets[key(word, sh["lo"][j], sh["keybits"][j])]
               for j, (offsets, _) in enumerate(index))


# ---- the scan of many words at once ----------------------------------------------------------------------------------------------------
def _popcount_u64(a):
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(a).astype(np.int64)
    table = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)
    return table[a.view(np.uint8).reshape(a.shape + (8,))].sum(axis=-1)


def nearest_many(codes, words):
    """(distance, index) of the scan's choice for every word: the lowest index at the smallest distance."""
    c = np.array(codes, dtype=np.uint64)
    dist, idx = np.empty(len(words), dtype=np.int64), np.empty(len(words), dtype=np.int64)
    for i, w in enumerate(words):
        hd = _popcount_u64(c ^ np.uint64(w))
        idx[i] = int(np.argmin(hd))       # (argmin returns the first minimum)
        dist[i] = hd[idx[i]]
    return dist, idx


def scan_from_nearest(dist4, idx4, max_hamming):
    """scan()'s answer from the (distance, index) of the four rotations."""
    for r in range(4):
        if dist4[r] <= max_hamming:
            return (1, int(idx4[r]), int(dist4[r]), r)
    return NOT_FOUND
