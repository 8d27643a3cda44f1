"""Shared by tests/test_decode_stage_cpu.py and tests/test_decode_stage_gpu.py: frames that reach the edges of the decode stage --
tags within a few pixels of the frame border, tag16h5 words equally near two codes, a duplicate nested inside a tag of its own id,
and a frame with more decodable tags than the handle holds records for.  Frames and the oracle's results on them are computed
once per process and never changed."""
import itertools
import math

import numpy as np

from isaac_ros_apriltag_amd import synth
from oracle import pyoracle as po
import parity_util as pu

W, H = 320, 240
_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _frozen(img):
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


def tag_H(cx, cy, half, theta=0.0):
    c, s = math.cos(theta), math.sin(theta)
    return np.array([[half * c, -half * s, cx], [half * s, half * c, cy], [0, 0, 1.0]])


# ---- border tags ------------------------------------------------------------------------------------------------------------------------
FAM36 = ("tag36h11",)
HALF = 40.0
TURN = 0.3
PLACEMENTS = ("top_left", "top", "top_right", "right", "bottom_right", "bottom", "bottom_left", "left")
AXIS_GAPS = (1.5, 2.0, 3.0, 4.0)      # pixels between the black border's outer edge and the frame edge
TURNED_GAPS = (0.5, 1.0, 2.0)         # the same for the bounding box of the border of a tag turned by TURN
# Where the oracle loses the tag at the listed gap at decimate 2 -- in any of the eight variants (refine_edges, sigma, pixel (0, 0)) -- the
# gap of that geometry is moved up at decimate 2 by the smallest of 0.5 and 1 px at which the oracle keeps it in all eight; the listed
# gap stays the case's name.  (decimate, placement, turned, listed gap) -> gap used.  Seven axis-parallel geometries are still lost one
# pixel further out and stay where they are listed: top_left 1.5, top_right 1.5 and 2, right 1.5 and 2, bottom_right 1.5 and 2.  Decimate
# 1 loses one geometry (top_left, axis-parallel, 1.5 px, under noise with pixel (0, 0) at 255); it stays as listed.
MOVED_GAPS = {(2, "top_left", False, 2.0): 3.0, (2, "top", False, 1.5): 2.5, (2, "top", False, 2.0): 2.5, (2, "top_right", False, 3.0): 4.0,
              (2, "right", False, 3.0): 4.0, (2, "bottom_right", False, 3.0): 3.5, (2, "bottom_right", True, 0.5): 1.5,
              (2, "bottom_right", True, 1.0): 1.5, (2, "bottom_left", False, 1.5): 2.0, (2, "bottom_left", True, 0.5): 1.5,
              (2, "bottom_left", True, 1.0): 1.5, (2, "left", False, 1.5): 2.5, (2, "left", False, 2.0): 2.5}
BORDER_SETTINGS = [(d, r) for d in (1, 2) for r in (1, 0)]   # (decimate, refine_edges)
SIGMAS = (0, 1)
PIXEL0 = (0, 255)
PITCH_PAD = 19


def border_geometries():
    """(name, placement, turned, listed gap) of the 56 border geometries."""
    out = []
    for pl in PLACEMENTS:
        out += [("%s_axis_gap%g" % (pl, g), pl, False, g) for g in AXIS_GAPS]
        out += [("%s_turned_gap%g" % (pl, g), pl, True, g) for g in TURNED_GAPS]
    return out


def border_centre(placement, turned, gap, w=W, h=H, half=HALF):
    ext = half * (math.cos(TURN) + math.sin(TURN)) if turned else half   # half the bounding box of the border square
    lo, hx, hy = gap + ext, w - gap - ext, h - gap - ext
    cx = lo if "left" in placement else hx if "right" in placement else w / 2.0
    cy = lo if "top" in placement else hy if "bottom" in placement else h / 2.0
    return cx, cy


def border_frame(placement, turned, gap, sigma, pixel0, decimate=1, tag_id=5, w=W, h=H, half=HALF):
    """One tag36h11 at `gap` pixels (MOVED_GAPS for `decimate`) from the frame edge(s) of `placement`, noise sigma, pixel (0, 0) forced to
    `pixel0`."""
    g = MOVED_GAPS.get((decimate, placement, turned, gap), gap)

    def make():
        cx, cy = border_centre(placement, turned, g, w, h, half)
        img = synth.render(w, h, [{"family": FAM36[0], "id": tag_id, "H": tag_H(cx, cy, half, TURN if turned else 0.0)}],
                           background=150, sigma=float(sigma), seed=1000 + int(10 * gap) + 100 * PLACEMENTS.index(placement)).copy()
        if pixel0 is not None:
            img[0, 0] = pixel0
        return _frozen(img)
    return _cached(("border", placement, turned, gap, g, sigma, pixel0, tag_id, w, h, half), make)


def border_cases(sigma, decimate):
    """[(name, image)] of one noise level at one decimate: every geometry with pixel (0, 0) forced to 0 and to 255."""
    return [("%s_px%d" % (name, p0), border_frame(pl, turned, gap, sigma, p0, decimate))
            for name, pl, turned, gap in border_geometries() for p0 in PIXEL0]


LARGE = dict(w=640, h=480, half=150.0, gap=2.0, sigma=1)   # sides of 300 px: above 136 px the refinement samples in a second chunk


def large_frame():
    return border_frame("top_left", False, LARGE["gap"], LARGE["sigma"], None, w=LARGE["w"], h=LARGE["h"], half=LARGE["half"])


def K_of(w, h):
    return synth.default_K(w, h)


def oracle_on(key, img, families, decimate=1, **more):
    """(detections, dump) of the oracle on a frame, once per (key, settings)."""
    h, w = img.shape
    return _cached(("oracle", key, tuple(families), decimate, tuple(sorted(more.items()))),
                   lambda: po.detect(img, families=families, params=pu.oracle_params(K_of(w, h), decimate, **more), want_dump=True))


# ---- ties: tag16h5 at max_hamming 3 -----------------------------------------------------------------------------------------------------
FAM16 = ("tag16h5",)
TIE_IDS = (0, 15)


def codes16():
    return _cached("codes16", lambda: po.family_codes("tag16h5")[0])


def turn_word(word, d=4):
    """The word the decoder forms for its next rotation: data cell (x, y) takes the value of cell (d - 1 - y, x); cell i = y * d + x is
    bit d * d - 1 - i."""
    n, out = d * d, 0
    for i in range(n):
        x, y = i % d, i // d
        j = x * d + (d - 1 - y)
        if (word >> (n - 1 - j)) & 1:
            out |= 1 << (n - 1 - i)
    return out


def scan(word, max_hamming, codes=None):
    """The code scan as DESIGN states it: rotations 0 .. 3 in turn, per rotation the FIRST code at the smallest distance, accepted
    if within max_hamming.  (id, hamming, rotation) or None."""
    codes = codes or codes16()
    for r in range(4):
        dist = [bin(word ^ c).count("1") for c in codes]
        best = min(dist)
        if best <= max_hamming:
            return dist.index(best), best, r
        word = turn_word(word)
    return None


def tie_word():
    """A word three flips from code 0 and three from code 15 (the two are six bits apart) that the scan resolves to (0, 3) whichever
    way the tag is turned: of the twenty ways to split the six bits, the first for which the word read from each of the four
    physical turns gives id 0 with three errors."""
    def find():
        c0, c15 = codes16()[TIE_IDS[0]], codes16()[TIE_IDS[1]]
        bits = [b for b in range(16) if ((c0 ^ c15) >> b) & 1]
        assert len(bits) == 6
        for trio in itertools.combinations(bits, 3):
            w = c0
            for b in trio:
                w ^= 1 << b
            reads, ok = w, True
            for _ in range(4):   # the word as read when the tag is turned by a further quarter: a rotation of w
                got = scan(reads, 3)
                ok = ok and got is not None and got[:2] == (TIE_IDS[0], 3)
                reads = turn_word(turn_word(turn_word(reads)))
            if ok and scan(w, 2) is None:
                return w
        return None
    return _cached("tie_word", find)


def turned_exact_words():
    """Words that are some code exactly after one, two or three quarter turns of the decoder but lie within 3 bits of another code
    unturned: [(word, unturned id, its hamming, the exact code's id, its rotation)].  The scan takes rotation 0 first, so the
    unturned id must win."""
    def find():
        out = []
        for j, c in enumerate(codes16()):
            w = c
            for k in (3, 2, 1):   # w turns into c after k more turns
                w = turn_word(w)
                got = scan(w, 3)
                if got is not None and got[2] == 0 and got[0] != j:
                    out.append((w, got[0], got[1], j, k))
        return out
    return _cached("turned_exact", find)


def word_frame(word, quarter_turns, half=40.0):
    """A 320 x 240 frame with one tag16h5-shaped tag carrying `word`, turned by quarter_turns * 90 degrees about the frame centre."""
    return _cached(("word", word, quarter_turns, half), lambda: _frozen(synth.render(
        W, H, [{"family": FAM16[0], "id": 0, "code": int(word), "H": tag_H(W / 2.0, H / 2.0, half, quarter_turns * math.pi / 2)}],
        background=150, sigma=0.0, seed=3)))


# ---- a duplicate nested inside a tag of its own id -----------------------------------------------------------------------------------------
NW, NH = 960, 720
NESTED_IDS = (0, 3, 7)


def white_cell_centre(tag_id, half=300.0):
    """Pixel centre of the first (row-major) white data cell of tag36h11 id tag_id drawn with half-side `half` at the frame centre."""
    code = po.family_codes("tag36h11")[0][tag_id]
    i = next(i for i in range(36) if (code >> (35 - i)) & 1)
    cell = 2.0 / 8
    return NW / 2.0 + half * (-1 + (1 + i % 6 + 0.5) * cell), NH / 2.0 + half * (-1 + (1 + i // 6 + 0.5) * cell)


def nested_frame(tag_id, inner_id):
    def make():
        cx, cy = white_cell_centre(tag_id)
        tags = [{"family": FAM36[0], "id": tag_id, "H": tag_H(NW / 2.0, NH / 2.0, 300.0)},
                {"family": FAM36[0], "id": inner_id, "H": tag_H(cx, cy, 24.0)}]
        return _frozen(synth.render(NW, NH, tags, background=150, sigma=0.0, seed=5))
    return _cached(("nested", tag_id, inner_id), make)


# ---- more decodable tags than the handle holds records for ------------------------------------------------------------------------------
OVERFLOW_CAPACITY = 4


def overflow_frames():
    """Frame 0: eight tag36h11 tags (ids 10 .. 17) on a 4 x 2 grid; frame 1: two (ids 20, 21)."""
    def make():
        def grid(ids, cols, rows, half):
            return [{"family": FAM36[0], "id": t, "H": tag_H((k % cols + 0.5) * W / cols, (k // cols + 0.5) * H / rows, half, 0.1 * k)}
                    for k, t in enumerate(ids)]
        f0 = synth.render(W, H, grid(range(10, 18), 4, 2, 22.0), background=150, sigma=1.0, seed=11)
        f1 = synth.render(W, H, grid((20, 21), 2, 1, 40.0), background=150, sigma=1.0, seed=12)
        return _frozen(f0), _frozen(f1)
    return _cached("overflow", make)
