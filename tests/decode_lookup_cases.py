"""The seeded families and words of the code-lookup tests (tests/test_decode_lookup_cpu.py)
(DESIGN.md section 7l).  Layouts come from tests/family_layouts.py and are closed under the quarter turn.  Families, words and the
expected results are computed once per process and never changed.

  d3       classic 3 x 3, 9 bits, 20 random codes          chunks of 2, 2, 2, 3 bits at max_hamming 3; a third of the words tie
  h5       tag16h5's own table, 30 codes                   a built-in family under a forced index
  dense16  classic 4 x 4, 16 bits, 3 000 random codes      duplicates kept; buckets beyond 64 candidates; half of the words tie
  std52    standard_layout(10, 6), 52 bits, 20 000 codes   keys capped at 16 bits (chunks of 17 / 17 / 18 bits at max_hamming 2)
  d8       classic_spiral_layout(8), 64 bits, 5 000 codes  nbits = 64: shifts and masks at the word's edge
"""
import numpy as np

from isaac_ros_apriltag_amd import synth
import family_layouts as fl
import decode_lookup_ref as ref

NAMES = ("d3", "h5", "dense16", "std52", "d8")
MAX_HAMMINGS = (0, 1, 2, 3)
SLOTS = {"d3": 4, "dense16": 5, "std52": 6, "d8": 7}   # registrable slots (capi.SLOT_CUSTOM0 ..); h5 is the built-in tag16h5
_SPEC = {   # name: (layout, width_at_border, total_width, codes, seed)
    "d3": (lambda: fl.classic_spiral_layout(3), 5, 7, 20, 301),
    "dense16": (lambda: fl.classic_spiral_layout(4), 6, 8, 3000, 302),
    "std52": (lambda: fl.standard_layout(10, 6), 6, 10, 20000, 303),
    "d8": (lambda: fl.classic_spiral_layout(8), 10, 12, 5000, 304),
}
_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _random_word(rng, nbits):
    return (int(rng.integers(0, 1 << 32)) | (int(rng.integers(0, 1 << 32)) << 32)) & ((1 << nbits) - 1)


def family(name):
    """{"name" (as registered), "builtin", "bit_x", "bit_y", "width_at_border", "total_width", "nbits", "codes", "rot_src"}."""
    def make():
        if name == "h5":
            codes, d = synth.family_codes("tag16h5")
            bx, by = [1 + i % d for i in range(d * d)], [1 + i // d for i in range(d * d)]
            wb, tw, codes, builtin = d + 2, d + 4, [int(c) for c in codes], True
        else:
            layout, wb, tw, count, seed = _SPEC[name]
            bx, by = layout()
            rng = np.random.default_rng(seed)
            codes, builtin = [_random_word(rng, len(bx)) for _ in range(count)], False
        return {"name": "tag16h5" if builtin else "lookup_" + name, "builtin": builtin, "bit_x": list(bx), "bit_y": list(by),
                "width_at_border": wb, "total_width": tw, "nbits": len(bx), "codes": codes, "rot_src": fl.rot_source(bx, by, wb)}
    return _cached(("family", name), make)


def register_args(name):
    f = family(name)
    return (SLOTS[name], f["name"], f["bit_x"], f["bit_y"], f["width_at_border"], f["total_width"], False, f["codes"])


def _flip(word, bits):
    for b in bits:
        word ^= 1 << int(b)
    return word


def words(name):
    """The family's test words: every 5th code exact; a sample of those with 1 to 4 flipped bits (max_hamming + 1 for every
    max_hamming); the same words carried through 1, 2 and 3 inverse quarter turns, so that the answer's rotation is 1, 2 or 3;
    midpoints between two codes at equal distance; 0 and all-ones; random words, about 4 000 words in all."""
    return _cached(("words+kinds", name), lambda: make_words(family(name), 1000 + NAMES.index(name)))[0]


def kinds(name):
    """Per word of words(name) the list it came from (make_words)."""
    return _cached(("words+kinds", name), lambda: make_words(family(name), 1000 + NAMES.index(name)))[1]


def make_words(f, seed):
    """(words, kinds) of a family dict as family() returns it: the words as words() describes them and, per word, the list it came
    from ("exact", "flipped", "turned", "mid", "edge" for 0 and all-ones, "random")."""
    n, codes, src = f["nbits"], f["codes"], f["rot_src"]
    rng = np.random.default_rng(seed)
    exact = [codes[i] for i in range(0, len(codes), 5)]
    step = max(1, len(exact) // 150)
    flipped = [_flip(c, rng.choice(n, size=k, replace=False)) for c in exact[::step] for k in (1, 2, 3, 4)]
    turned = [ref.unrotate(w, src, t) for t in (1, 2, 3) for w in (exact[::step] + flipped)[::3]]
    mid = []
    for i in range(0, len(codes), max(1, len(codes) // 200)):
        others = [int(j) for j in rng.integers(0, len(codes), size=64)]
        even = [(ref.popcount(codes[i] ^ codes[j]), j) for j in others if ref.popcount(codes[i] ^ codes[j]) % 2 == 0 and codes[j] != codes[i]]
        if even:
            d, j = min(even)
            diff = [b for b in range(n) if ((codes[i] ^ codes[j]) >> b) & 1]
            mid.append(_flip(codes[i], rng.choice(diff, size=d // 2, replace=False)))
    crafted = exact + flipped + turned + mid + [0, (1 << n) - 1]
    # random words fill up to about 4 000 (at least 500); a family of up to 12 bits gets every word there is
    rand = list(range(1 << n)) if n <= 12 else [_random_word(rng, n) for _ in range(max(500, 4000 - len(crafted)))]
    kinds = ["exact"] * len(exact) + ["flipped"] * len(flipped) + ["turned"] * len(turned) + ["mid"] * len(mid) + ["edge"] * 2 + ["random"] * len(rand)
    return tuple(crafted + rand), tuple(kinds)


def words4(name):
    f = family(name)
    return _cached(("words4", name), lambda: tuple(tuple(ref.rotations(w, f["rot_src"])) for w in words(name)))


def nearest(name):
    """Per word and rotation the scan's (distance, index): arrays of shape (nwords, 4)."""
    def make():
        f, w4 = family(name), words4(name)
        flat = [w for ws in w4 for w in ws]
        dist, idx = ref.nearest_many(f["codes"], flat)
        dist.setflags(write=False), idx.setflags(write=False)
        return dist.reshape(-1, 4), idx.reshape(-1, 4)
    return _cached(("nearest", name), make)


def expected(name, max_hamming):
    """The scan's (found, id, hamming, rotation) of every word as four int32 arrays."""
    def make():
        dist, idx = nearest(name)
        rows = np.array([ref.scan_from_nearest(dist[i], idx[i], max_hamming) for i in range(len(dist))], dtype=np.int32).reshape(-1, 4)
        rows.setflags(write=False)
        return rows
    return _cached(("expected", name, max_hamming), make)


def index_of(name, max_hamming):
    f = family(name)
    return _cached(("index", name, max_hamming), lambda: ref.build_index(f["codes"], f["nbits"], max_hamming))
