"""Frames for the integer stages -- threshold, connected components, boundary points, cluster selection -- that put every rule of
those stages on its edge by construction, and the census that says which edges a frame really meets.

The stages in front of the quad fit are compared with the oracle bit for bit on noise and on content, but a rule that only shows at
x = 1, on a tile border, at a count of exactly 24 or at a range of exactly 5 is met there by the luck of a seed or not at all.  The
frames here are small and deterministic (the tests/fit_frames.py idiom: no file I/O, numpy only):

  (a) link_atlas        two blobs joined by exactly ONE link of the oracle's link set, at every position class of the 64 x 64 CC tiles
  (b) merge_atlas       components of exactly 24 / 25 pixels inside one tile and split over two and four; serpentines; a comb
  (c) LIMIT_FRAMES      72 x 40 frames of edge-hugging rectangles with clusters of exactly 23, 24 and 25 points (frozen search winners)
  (d) emission_atlas    the "left neighbour emitted its (1,1) point" rule of the boundary points across k_points' 64 x 16 tiles
  (e) threshold_atlas   gray frames with dilated tile ranges of exactly 4 and 5 and pixels at thresh / thresh + 1, halo-essential
  (f) the census        on an oracle dump or on the library's debug buffers (the same arrays)

tests/test_stage_frames_cpu.py holds every census condition on the oracle alone; tests/test_integer_stages_gpu.py puts the same
frames through the library.  A plain helper module: nothing here touches a GPU."""
import functools

import numpy as np

CC_T = 64                  # tile edge of k_cc_local
PT_TW, PT_TH = 64, 16      # tile of k_points
MIN_COMPONENT, MIN_CLUSTER, MIN_DIFF = 25, 24, 5   # the parameters' defaults (oracle: ato_default_params)

# ---- the oracle's link set (ato_connected_components): a SOURCE pixel (x, y), 1 <= x <= W - 2, of class v != 127 is joined with
# its left neighbour, its upper neighbour and -- white only -- its upper-left and upper-right neighbour, where that has class v.
# Columns 0 and W - 1 are never a source: they join others only as a partner. -----------------------------------------------------------
LINKS = {"left": (-1, 0), "up": (0, -1), "upleft": (-1, -1), "upright": (1, -1)}


def components(thr, without=None):
    """Min-index labels of the partition the link set gives on `thr` (equal to the oracle's `label` where thr != 127; 127 pixels keep
    their own index).  without = (x, y, kind): that one link is left out."""
    h, w = thr.shape
    idx = np.arange(w * h, dtype=np.int64).reshape(h, w)
    src, dst = [], []
    for kind, (dx, dy) in LINKS.items():
        ys, xs = slice(max(0, -dy), h), slice(1, w - 1)
        a = thr[ys, xs]
        b = thr[max(0, -dy) + dy:h + dy, 1 + dx:w - 1 + dx]
        m = (a == b) & (a != 127) & ((a == 255) | (kind in ("left", "up")))
        if without is not None and without[2] == kind:
            m = m.copy()
            m[without[1] - max(0, -dy), without[0] - 1] = False
        src.append(idx[ys, xs][m])
        dst.append(idx[max(0, -dy) + dy:h + dy, 1 + dx:w - 1 + dx][m])
    src, dst = np.concatenate(src), np.concatenate(dst)
    lab = idx.reshape(-1).copy()
    while True:
        new = lab.copy()
        np.minimum.at(new, src, lab[dst])
        np.minimum.at(new, dst, lab[src])
        new = new[new]
        if np.array_equal(new, lab):
            return lab.reshape(h, w)
        lab = new


def joined(lab, a, b):
    return bool(lab[a[1], a[0]] == lab[b[1], b[0]])


# ---- drawing ---------------------------------------------------------------------------------------------------------------------------
class Canvas:
    """A 0 / 255 frame under construction: two-pixel vertical stripes as the ground (every 4 x 4 tile holds both values, so the
    threshold returns the frame itself), and shapes that bring a one-pixel ring of the other class with them.  `drawn` marks what a
    shape set; two shapes may not touch each other's pixels."""

    def __init__(self, h, w):
        self.h, self.w = h, w
        self.img = np.tile(np.where((np.arange(w) // 2) % 2 == 0, 0, 255).astype(np.uint8), (h, 1))
        self.drawn = np.zeros((h, w), bool)
        self.flat = np.zeros((h, w), bool)

    def shape(self, cls, *pixel_sets):
        px = {(x, y) for s in pixel_sets for (x, y) in s}
        assert all(0 <= x < self.w and 0 <= y < self.h for x, y in px), sorted(px)[:3]
        ring = {(x + dx, y + dy) for x, y in px for dx in (-1, 0, 1) for dy in (-1, 0, 1)} - px
        ring = {(x, y) for x, y in ring if 0 <= x < self.w and 0 <= y < self.h}
        for x, y in px | ring:
            assert not self.drawn[y, x], ("shapes overlap at", x, y)
            self.drawn[y, x] = True
            self.img[y, x] = cls if (x, y) in px else 255 - cls

    def flat_band(self, x0, y0, y1):
        """Rows y0 .. y1 - 1 (multiples of 4): white columns x0 .. x0 + 3 and x0 + 16 .. x0 + 19 around a flat band of 200, twelve wide.
        Between its first and last tile row the band's outer tile columns see 200 and 255 and come out BLACK, its middle one sees 200
        alone and comes out 127: two black blobs with a strip without a class between them (the band's ends see the stripes: white)."""
        assert not self.drawn[y0:y1, x0:x0 + 20].any() and x0 % 4 == 0 and y0 % 4 == 0 and y1 % 4 == 0
        self.img[y0:y1, x0:x0 + 20] = 255
        self.img[y0:y1, x0 + 4:x0 + 16] = 200
        self.drawn[y0 + 4:y1 - 4, x0:x0 + 20] = True
        self.flat[y0 + 4:y1 - 4, x0 + 4:x0 + 16] = True

    @property
    def want(self):
        """The threshold image the frame is drawn for, where a shape was drawn; 1 elsewhere."""
        t = np.where(self.img > 127, 255, 0).astype(np.uint8)
        t[self.flat & (self.img == 200)] = 0
        f = np.argwhere(self.flat)
        if len(f):   # (one band per canvas)
            t[f[:, 0].min():f[:, 0].max() + 1, f[:, 1].min() + 4:f[:, 1].min() + 8] = 127
        t[~self.drawn] = 1
        return t


def arm_block(x, y, ax, ay, shift=0):
    """A 28-pixel blob: three pixels from (x, y) in direction (ax, ay), then a 5 x 5 block, moved `shift` across the direction."""
    px = [(x + ax * i, y + ay * i) for i in range(3)]
    cx, cy = x + ax * 5 + (shift if ax == 0 else 0), y + ay * 5 + (shift if ay == 0 else 0)
    return px + [(cx + i, cy + j) for i in range(-2, 3) for j in range(-2, 3)]


def run_below(x, y, step, n=24):
    """(x, y) and n pixels of the row below it, away from x in direction `step`: a 25-pixel blob two rows high."""
    return [(x, y)] + [(x + step * i, y + 1) for i in range(n)]


def run_row(x, y, step, n=25):
    return [(x + step * i, y) for i in range(n)]


# ---- (a) the link atlas ----------------------------------------------------------------------------------------------------------------
LINK_SHAPES = ((130, 130), (129, 130), (130, 129))   # (H, W): 3 x 3 tiles; the last row / the last column a tile of its own
LINK_INTERIOR_SHAPE = (40, 130)   # the twin: the tile-interior motifs alone, in a frame without a tile-top row and with nothing at x = 1


def _link_motif(c, out, name, kind, x, y, cls, S, T, expect="essential", where=""):
    """Blob S holds the source (x, y), blob T its partner: `essential` -- they are joined, and not without that link; `apart` -- the
    negative twin, nothing joins them; `joined` -- a premise of a skip rule, several links join them."""
    dx, dy = LINKS[kind]
    c.shape(cls, S, T)
    out.append({"name": name, "link": (x, y, kind), "a": (x, y), "b": (x + dx, y + dy), "cls": cls, "expect": expect, "where": where})


def _pair(c, out, name, kind, x, y, cls, expect="essential", where="", down=None):
    """The standard motif of a link at source (x, y): S hangs below / right of the source, T above / left of the partner.  down: S
    where there is no room for a block below (a tile-top row that is one of the frame's last two rows)."""
    W = c.w
    dx, dy = LINKS[kind]
    edge = 2 if x <= 3 else (-2 if x >= W - 4 else 0)   # blocks move inward at the frame's left / right edge
    if kind == "left":
        S, T = arm_block(x, y, 1, 0), arm_block(x - 1, y, -1, 0)
    else:
        sS = {"up": edge, "upleft": 2, "upright": -2}[kind]
        sT = {"up": edge, "upleft": -2, "upright": 2}[kind]
        S = down if down is not None else arm_block(x, y, 0, 1, sS)
        T = arm_block(x + dx, y + dy, 0, -1, sT)
    _link_motif(c, out, name, kind, x, y, cls, S, T, expect, where)


def _interior_motifs(c, m):
    B, Wh = 0, 255
    # tile interiors (tiles (0, 0) and (1, 0))
    _pair(c, m, "interior up black", "up", 12, 12, B, where="interior")
    _pair(c, m, "interior up white", "up", 22, 12, Wh, where="interior")
    _pair(c, m, "interior upleft white", "upleft", 36, 12, Wh, where="interior")
    _pair(c, m, "interior upleft black twin", "upleft", 50, 12, B, "apart", "interior")
    _pair(c, m, "interior upright white", "upright", 74, 12, Wh, where="interior")
    _pair(c, m, "interior upright black twin", "upright", 88, 12, B, "apart", "interior")
    _pair(c, m, "interior left black", "left", 110, 6, B, where="interior")
    _pair(c, m, "interior left white", "left", 110, 14, Wh, where="interior")


@functools.lru_cache(maxsize=None)
def link_atlas(h, w):
    """(frame, motifs, want) of one link-atlas shape; want: the threshold image wherever a motif was drawn, 1 elsewhere.  Where a blob
    would lie in column 0 or W - 1 it is the partner pixel alone: such a pixel is joined to others only by the one link that names it,
    so nothing else can be added to it."""
    c, m = Canvas(h, w), []
    B, Wh = 0, 255
    if (h, w) == LINK_INTERIOR_SHAPE:
        _interior_motifs(c, m)
        return c.img, m, c.want
    _interior_motifs(c, m)
    # x = 1 and x = W - 2 off a tile-top row
    _link_motif(c, m, "x=1 upleft white off-row", "upleft", 1, 12, Wh, arm_block(1, 12, 0, 1, 2), [(0, 11)], where="x1")
    _pair(c, m, "x=1 up black off-row", "up", 1, 34, B, where="x1")
    _link_motif(c, m, "x=W-2 upright white off-row", "upright", w - 2, 12, Wh, arm_block(w - 2, 12, 0, 1, -2), [(w - 1, 11)], where="xW-2")
    _pair(c, m, "x=W-2 up white off-row", "up", w - 2, 112, Wh, where="xW-2")
    # the tile-top row y = 64
    y = CC_T
    _pair(c, m, "row64 up black", "up", 12, y, B, where="row")
    _pair(c, m, "row64 up white", "up", 22, y, Wh, where="row")
    _pair(c, m, "row64 upleft white", "upleft", 36, y, Wh, where="row")
    _pair(c, m, "row64 upleft black twin", "upleft", 50, y, B, "apart", "row")
    if (h, w) == (130, 130):   # the four-tile corner, one diagonal per frame
        _pair(c, m, "corner upleft white (64,64)->(63,63)", "upleft", CC_T, y, Wh, where="corner")
    else:
        _pair(c, m, "corner upright white (63,64)->(64,63)", "upright", CC_T - 1, y, Wh, where="corner")
    _pair(c, m, "row64 upright white", "upright", 80, y, Wh, where="row")
    _pair(c, m, "row64 upright black twin", "upright", 94, y, B, "apart", "row")
    # x = 1 on the tile-top row: the bar two pixels wide in columns 0..1 (black: its halves hang on the up link of (1, 64) alone;
    # column 0 is no source) -- the same-class 2 x 2 block across the border whose LEFT neighbour is no source ...
    bar = lambda x0, y0, step: [(x0 + i, y0 + step * j) for i in (0, 1) for j in range(13)]
    _link_motif(c, m, "x=1 row64 bar two wide black", "up", 1, y, B, bar(0, y, 1), bar(0, y - 1, -1), where="x1row")
    # ... and with a source as the left neighbour: two up links, the rule keeps the first (a premise: joined, neither link essential)
    _link_motif(c, m, "row64 bar two wide black", "up", 104, y, B, bar(103, y, 1), bar(103, y - 1, -1), "joined", "row")
    _link_motif(c, m, "row64 bar two wide white", "up", 108, y, Wh, bar(107, y, 1), bar(107, y - 1, -1), "joined", "row")
    # the up-right link with the pixel above white (bc) where the right neighbour IS a source: the rule skips it, up + left carry it
    _link_motif(c, m, "row64 upright white, bc white", "upright", 115, y, Wh, arm_block(115, y, 0, 1, -2) + [(115, y - 1)],
                arm_block(116, y - 1, 0, -1, 2), "joined", "row")
    # x = W - 2 on the tile-top row: the same with right_src false -- (W - 1, 63) hangs on the up-right link of (W - 2, 64) alone
    _link_motif(c, m, "x=W-2 row64 upright white, bc white", "upright", w - 2, y, Wh, arm_block(w - 2, y, 0, 1, -2) + [(w - 2, y - 1)],
                [(w - 1, y - 1)], where="xW-2row")
    # tile-left columns
    _pair(c, m, "col64 left black", "left", CC_T, 28, B, where="col")
    _pair(c, m, "col64 left white", "left", CC_T, 36, Wh, where="col")
    _pair(c, m, "col64 upleft white", "upleft", CC_T, 90, Wh, where="col")
    _pair(c, m, "col64 upright white (63,y)->(64,y-1)", "upright", CC_T - 1, 108, Wh, where="col")
    x = 2 * CC_T
    if x <= w - 2:   # 130 wide: x = 128 is a source, its left link crosses the border (black: a white blob right of it has no room)
        _link_motif(c, m, "col128 left black", "left", x, 24, B, [(x, 24 + j) for j in range(25)], arm_block(x - 1, 24, -1, 0), where="col")
    else:            # 129 wide: x = 128 = W - 1 is no source, the same black pair is NOT joined
        _link_motif(c, m, "col128 = W-1 left black twin", "left", x, 24, B, [(x, 24 + j) for j in range(25)], arm_block(x - 1, 24, -1, 0),
                    "apart", "col")
    # a vertical run in column 0 and in column W - 1 alone: no pixel of it is a source, nothing joins it
    c.shape(B, [(0, 100 + j) for j in range(26)])
    m.append({"name": "column 0 run", "link": None, "a": (0, 100), "b": (0, 101), "cls": B, "expect": "apart", "where": "x0"})
    c.shape(Wh, [(w - 1, 76 + j) for j in range(26)])
    m.append({"name": "column W-1 run", "link": None, "a": (w - 1, 76), "b": (w - 1, 77), "cls": Wh, "expect": "apart", "where": "xW-1"})
    # the tile-top row y = 128: two rows (130 high) or one (129 high) below it
    y = 2 * CC_T
    if h - y >= 2:
        _pair(c, m, "row128 up black", "up", 6, y, B, where="row", down=run_below(6, y, 1))
        _pair(c, m, "row128 up white", "up", 36, y, Wh, where="row", down=run_below(36, y, 1))
        _pair(c, m, "row128 upleft white", "upleft", 70, y, Wh, where="row", down=run_below(70, y, 1))
        # the up-right link with the right neighbour white (tr) and a source: the rule skips it, the neighbour's up link carries it ...
        _pair(c, m, "row128 upright white, tr white", "upright", 96, y, Wh, "joined", "row", down=run_below(96, y, 1, 7) + [(97, y)])
        # ... and at x = W - 2, right_src false: (W - 1, 127) hangs on the up-right link of (W - 2, 128) alone
        _link_motif(c, m, "x=W-2 row128 upright white, tr white", "upright", w - 2, y, Wh, run_below(w - 2, y, -1, 23) + [(w - 1, y)],
                    [(w - 1, y - 1)], where="xW-2row")
    else:
        _link_motif(c, m, "x=W-2 row128 upright white, tr white", "upright", w - 2, y, Wh, run_row(w - 2, y, -1, 20) + [(w - 1, y)],
                    [(w - 1, y - 1)], where="xW-2row")
        _pair(c, m, "row128 up black", "up", 6, y, B, where="row", down=run_row(6, y, 1))
        _pair(c, m, "row128 upleft white", "upleft", 40, y, Wh, where="row", down=run_row(40, y, 1))
        _pair(c, m, "row128 upright white", "upright", 100, y, Wh, where="row", down=run_row(100, y, -1))
    # the same bridge through a 127 pixel: black, no class (four pixels of it), black side by side in a row -- the left link of
    # (32, y) meets a pixel without a class
    c.flat_band(20, 80, 100)
    m.append({"name": "127 bridge", "link": None, "a": (32, 90), "b": (27, 90), "cls": B, "expect": "apart", "where": "interior", "gap": (28, 90)})
    return c.img, m, c.want


# ---- (b) the merge atlas ---------------------------------------------------------------------------------------------------------------
def _line(x, y, n, dx=1, dy=0):
    return [(x + dx * i, y + dy * i) for i in range(n)]


@functools.lru_cache(maxsize=None)
def merge_atlas(k):
    """130 x 130.  k = 0: components of exactly 24 and 25 pixels, inside one tile and split over two and four tiles (12 + 12, 12 + 13,
    6 + 6 + 6 + 6, 6 + 6 + 6 + 7): no tile-local root is large, only k_cc_resolve can set the size bit.  k = 1: serpentines one pixel
    wide that cross a tile border seven times in sequence, and a comb whose teeth meet only in the last row of the tile below.
    Returns (frame, records, want); a record names a pixel of the shape and what the census must find there."""
    c, r = Canvas(130, 130), []
    B, Wh = 0, 255
    if k in (0, 2):   # (2: the one-tile components alone -- the twin in which k_cc_local sets every size bit)
        def comp(name, cls, px, spread):
            if k == 2 and spread > 1:
                return
            c.shape(cls, px)
            r.append({"name": name, "pixel": px[0], "cls": cls, "size": len(px), "spread": spread})
        for cls, y0 in ((B, 10), (Wh, 20)):
            comp("one tile 25", cls, _line(10, y0, 25), 1)
            comp("one tile 24", cls, _line(10, y0 + 4, 24), 1)
        for cls, y0 in ((B, 30), (Wh, 40)):
            comp("two tiles 12+13 across x=64", cls, _line(52, y0, 25), 2)
            comp("two tiles 12+12 across x=64", cls, _line(52, y0 + 4, 24), 2)
        for cls, x0 in ((B, 10), (Wh, 20)):
            comp("two tiles 12+13 across y=64", cls, _line(x0, 52, 25, 0, 1), 2)
            comp("two tiles 12+12 across y=64", cls, _line(x0 + 4, 52, 24, 0, 1), 2)
        comp("four tiles 6+6+6+7 at (64,64)", B, _line(58, 63, 12) + _line(63, 64, 6, 0, 1) + _line(64, 64, 7, 0, 1), 4)
        comp("four tiles 6+6+6+6 at (64,128)", B, _line(58, 127, 12) + [(63, 128)] + _line(63, 129, 5, -1, 0) + [(64, 128)] + _line(64, 129, 5), 4)
    else:
        def serpentine(name, cls, x0, x1, y0, rows):
            px = []
            for i in range(rows):
                px += _line(x0, y0 + 2 * i, x1 - x0 + 1)
                if i + 1 < rows:
                    px.append((x1 if i % 2 == 0 else x0, y0 + 2 * i + 1))
            c.shape(cls, px)
            r.append({"name": name, "a": (x0, y0), "b": (x1 if rows % 2 else x0, y0 + 2 * (rows - 1)), "cls": cls, "size": len(px),
                      "crossings": rows})
        serpentine("serpentine black across x=64 and y=64", B, 60, 68, 58, 7)
        serpentine("serpentine white across x=64", Wh, 60, 68, 20, 7)
        teeth = list(range(80, 92, 2))
        px = [p for x in teeth for p in _line(x, 40, 87, 0, 1)] + _line(80, 127, 11)
        c.shape(B, px)
        r.append({"name": "comb black, spine in row 127", "a": (teeth[0], 40), "b": (teeth[-1], 40), "cls": B, "size": len(set(px)),
                  "crossings": len(teeth)})
    return c.img, r, c.want


# ---- (c) cluster-limit frames: 72 x 40, dark rectangles on a light ground, drawn in order.  Winners of a search on the oracle
# (min_cluster_points = 1; seeded random rectangles, then every rectangle of 2 .. 15 pixels a side in every corner and on every edge)
# for clusters of exactly 23, 24 and 25 points, frozen here as rectangle lists (x0, y0, x1, y1, value), x1 / y1 exclusive. ---------------------------------------------------------------------------------------------------------------------
LIMIT_W, LIMIT_H = 72, 40
LIMIT_GROUND = 215


def limit_frame(rects):
    img = np.full((LIMIT_H, LIMIT_W), LIMIT_GROUND, np.uint8)
    for x0, y0, x1, y1, v in rects:
        img[y0:y1, x0:x1] = v
    return img


# What the search showed: two components of 25 or more pixels that meet away from the frame's edges share 26 points or more, so a
# cluster of 23 .. 25 points is a dark rectangle in a CORNER of the frame (columns 0 and W - 1, rows 0 and H - 1 are no sources): w + h
# = 14 gives 24 points in three corners and 25 in the bottom-left one, w + h = 13 gives 23 there.  For the same reason no 24-point cluster
# can have points on both sides of x = 64 AND of y = 16 in a 72 x 40 frame (the nearest corner is 8 columns and 16 rows away; the smallest
# cluster found across that point has 35 points): the frames below cross the k_points tile borders x = 64 and y = 32 one at a time.
D = 35
LIMIT_FRAMES = {
    "24_24_24_25": ((0, 0, 5, 9, D), (0, 31, 5, 40, D), (67, 0, 72, 9, D), (67, 31, 72, 40, D)),   # default: 24, 24, 24, 25
    "23_24_25": ((0, 31, 4, 40, D), (0, 0, 4, 10, D), (20, 0, 25, 5, D)),                          # min_cluster_points 1: 23, 24, 25
    "25_25": ((0, 30, 4, 40, D), (20, 0, 25, 5, D)),                                               # no 24: the twin of the frames above
    "24_across_x64": ((63, 35, 72, 40, D),),                                                       # k_points tiles (0, 2) and (1, 2)
    "24_across_y32": ((68, 30, 72, 40, D),),                                                       # k_points tiles (1, 1) and (1, 2)
}
LIMIT_COUNTS = {"24_24_24_25": ([24, 24, 24, 25], [24, 24, 24, 25]), "23_24_25": ([24, 25], [23, 24, 25]), "25_25": ([25, 25], [25, 25]),
                "24_across_x64": ([24], [24]), "24_across_y32": ([24], [24])}   # (default parameters, min_cluster_points = 1)


# ---- (d) the emission atlas --------------------------------------------------------------------------------------------------------------
EMISSION_H, EMISSION_W = 50, 200
_BANDS = ((0, 2, 255), (2, 10, 0), (10, 20, 255), (20, 28, 0), (28, 36, 255), (36, 44, 0), (44, 49, 255), (49, 50, 0))


@functools.lru_cache(maxsize=None)
def emission_atlas():
    """200 x 50: 4 x 4 tiles of k_points, the middle 2 x 2 interior.  Horizontal black / white edges from column 0 to column W - 1 -- in
    rows 1 and H - 2, inside edge tiles and inside interior tiles --, two wedges with diagonal sides across x = 128, and a flat patch
    whose middle tile comes out 127 beside a white and above a black one (a left neighbour without a class)."""
    img = np.zeros((EMISSION_H, EMISSION_W), np.uint8)
    for y0, y1, v in _BANDS:
        img[y0:y1] = v
    for x in range(72, 104):   # a white wedge into the black band above row 28: sides of slope 1/2
        img[28 - min(x - 72, 103 - x) // 2 - 1:28, x] = 255
    for x in range(120, 134):  # a black wedge into the white band above row 36: sides of slope 1, across x = 128
        img[36 - min(x - 120, 133 - x) - 1:36, x] = 0
    img[8:32, 148:172] = 100
    img[8:32, 164:172] = 0
    img[24:32, 148:164] = 255
    return img


def emission_census(thr, label, csize, min_component=MIN_COMPONENT):
    """Where the (-1, 1) emission of a source pixel meets the rule "the left neighbour emitted its (1, 1) point", by position class.
    thr, label, csize: the oracle's dump or the library's debug buffers (label: representative per pixel)."""
    h, w = thr.shape
    lab = np.where(thr == 127, 0, label).astype(np.int64)
    big = (thr != 127) & (csize.reshape(-1)[lab] >= min_component)
    t = thr.astype(np.int32)

    def opp(ay, ax, by, bx):   # slices of equal shape
        return big[ay, ax] & big[by, bx] & (t[ay, ax] + t[by, bx] == 255)
    ys, xs = slice(1, h - 1), slice(1, w - 1)
    yd = slice(2, h)
    cand = opp(ys, xs, yd, slice(0, w - 2))                       # (x, y) against (x - 1, y + 1)
    left = opp(ys, slice(0, w - 2), yd, xs)                      # (x - 1, y) against (x, y + 1)
    left_weak = (thr[ys, slice(0, w - 2)] == 127) | ~big[ys, slice(0, w - 2)]
    X, Y = np.meshgrid(np.arange(1, w - 1), np.arange(1, h - 1))
    bx, by = X // PT_TW, Y // PT_TH
    interior = (bx >= 1) & (by >= 1) & (bx * PT_TW + PT_TW + 1 <= w) & (by * PT_TH + PT_TH + 1 <= h)
    both = cand & left
    n = lambda m: int(m.sum())
    return {"tile_edge_interior": n(both & (X % PT_TW == 0) & interior), "tile_edge_outer": n(both & (X % PT_TW == 0) & ~interior),
            "x1_kept": n(both & (X == 1)), "x2_suppressed": n(both & (X == 2)), "row_1": n(both & (Y == 1)), "row_H-2": n(both & (Y == h - 2)),
            "into_last_row": n(cand & (Y == h - 2)), "into_last_column": n(opp(ys, slice(w - 2, w - 1), yd, slice(w - 1, w))),
            "left_127_or_small": n(cand & ~left & left_weak & (X >= 2)), "suppressed": n(both & (X >= 2))}


# ---- (e) the threshold atlas -------------------------------------------------------------------------------------------------------------
TH_BASE = 100
TH_BLOCK = (256, 8)   # tiles of one k_threshold block (tile size 4): 1024 x 32 pixels
THRESHOLD_FRAMES = {"70x1100": (70, 1100, 4), "37x70": (37, 70, 4), "36x68": (36, 68, 4), "70x1100_tile8": (70, 1100, 8)}


@functools.lru_cache(maxsize=None)
def threshold_atlas(name):
    """A gray frame of TH_BASE with single pixels a few levels above it, three tiles apart or more so that no two features share a tile's
    3 x 3 neighbourhood.  A `peak` of +4 gives its nine tiles a dilated range of exactly 4 (below min_white_black_diff: 127), +5 and +6
    of exactly 5 and 6 with thresh = base + 2 and + 3; `probes` at thresh and thresh + 1 sit in the peak's tile or in the tile named.
    Pairs across x = 1024 and y = 32 (tile size 4) put the peak into the next kernel block: the probe's tile has its range from the halo
    alone.  Corner tiles see a peak diagonally inside (clamped neighbourhoods); the ragged strips hold a probe beside a peak and are flat
    elsewhere."""
    h, w, ts = THRESHOLD_FRAMES[name]
    tw, th = w // ts, h // ts
    img = np.full((h, w), TH_BASE, np.uint8)

    def feature(peak_tile, up, probe_tile=None, probe_px=None):
        (px, py), (qx, qy) = peak_tile, probe_tile or peak_tile
        if not (0 <= px < tw and 0 <= py < th and 0 <= qx < tw and 0 <= qy < th):
            return
        img[py * ts + 1, px * ts + 1] = TH_BASE + up
        t = TH_BASE + up // 2
        if probe_px is None:
            probe_px = (qx * ts + 2, qy * ts + 2)
        img[probe_px[1], probe_px[0]] = t          # the probes: one pixel at thresh, the next (right of it, or below it) at thresh + 1
        x2, y2 = (probe_px[0] + 1, probe_px[1]) if probe_px[0] + 1 < w else (probe_px[0], probe_px[1] + 1)
        img[y2, x2] = t + 1
    feature((5, 3), 4)
    feature((9, 3), 5)
    feature((12, 3), 6)
    if ts == 4:
        bxt, byt = TH_BLOCK
        feature((bxt, 3), 5, (bxt - 1, 3))
        feature((bxt - 1, 11), 5, (bxt, 11))
        feature((4, byt), 5, (4, byt - 1))
        feature((12, byt - 1), 5, (12, byt))
    feature((1, 1), 5, (0, 0))
    feature((tw - 2, 1), 5, (tw - 1, 0))
    feature((1, th - 2), 5, (0, th - 1))
    feature((tw - 2, th - 2), 5, (tw - 1, th - 1))
    if h > th * ts:
        feature((8, th - 1), 5, (8, th - 1), (8 * ts + 1, th * ts))
    if w > tw * ts:
        feature((tw - 1, 4), 5, (tw - 1, 4), (tw * ts, 4 * ts + 1))
    return img


def threshold_ref(gray, tile=4, min_diff=MIN_DIFF):
    """The threshold statement in numpy, and the census of its edges.  Returns (thr, census)."""
    h, w = gray.shape
    tw, th = w // tile, h // tile
    g = gray[:th * tile, :tw * tile].reshape(th, tile, tw, tile).astype(np.int32)
    tmin, tmax = g.min(axis=(1, 3)), g.max(axis=(1, 3))

    def dilate(a, f, pad, keep=None):
        p = np.pad(a, 1, constant_values=pad)
        views = [p[1 + dy:1 + dy + th, 1 + dx:1 + dx + tw] for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
        if keep is not None:
            views = [np.where(k, v, pad) for v, k in zip(views, keep)]
        return functools.reduce(f, views)
    dmin, dmax = dilate(tmin, np.minimum, 255), dilate(tmax, np.maximum, 0)
    rng = dmax - dmin
    thresh = dmin + rng // 2
    ty = np.minimum(np.arange(h) // tile, th - 1)[:, None]
    tx = np.minimum(np.arange(w) // tile, tw - 1)[None, :]
    in_tiles = (np.arange(h)[:, None] < th * tile) & (np.arange(w)[None, :] < tw * tile)
    gi = gray.astype(np.int32)
    thr = np.where(gi > thresh[ty, tx], 255, 0).astype(np.uint8)
    thr[in_tiles & (rng[ty, tx] < min_diff)] = 127
    live = rng[ty, tx] >= min_diff
    cen = {"tiles_range_4": int((rng == min_diff - 1).sum()), "tiles_range_5": int((rng == min_diff).sum()),
           "tiles_range_even": int(((rng >= min_diff) & (rng % 2 == 0)).sum()), "tiles_range_odd": int(((rng >= min_diff) & (rng % 2 == 1)).sum()),
           "px_at_thresh_in_tiles": int((in_tiles & live & (gi == thresh[ty, tx])).sum()),
           "px_at_thresh+1_in_tiles": int((in_tiles & live & (gi == thresh[ty, tx] + 1)).sum()),
           "px_at_thresh_in_strips": int((~in_tiles & live & (gi == thresh[ty, tx])).sum()),
           "px_at_thresh+1_in_strips": int((~in_tiles & live & (gi == thresh[ty, tx] + 1)).sum()),
           "flat_strip_px": int((~in_tiles & ~live).sum()), "flat_strip_px_not_0": int((~in_tiles & ~live & (thr != 0)).sum()),
           "corner_tiles_live": int(sum(rng[a, b] >= min_diff for a in (0, th - 1) for b in (0, tw - 1)))}
    if tile == 4:   # tiles whose range reaches min_diff only through a tile of the neighbouring kernel block
        TY, TX = np.meshgrid(np.arange(th), np.arange(tw), indexing="ij")
        for key, blk in (("halo_essential_x", TX // TH_BLOCK[0]), ("halo_essential_y", TY // TH_BLOCK[1])):
            pb = np.pad(blk, 1, constant_values=-1)
            keep = [pb[1 + dy:1 + dy + th, 1 + dx:1 + dx + tw] == blk for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
            own = dilate(tmax, np.maximum, 0, keep) - dilate(tmin, np.minimum, 255, keep)
            cen[key] = int(((rng >= min_diff) & (own < min_diff)).sum())
    return thr, cen


def decimate2_input(gray):
    """The frame whose point-sampled decimation by 2 is `gray`."""
    return np.ascontiguousarray(np.repeat(np.repeat(gray, 2, axis=0), 2, axis=1))


def bgr8_input(gray):
    """Three equal channels: Y = (16384 v + 8192) >> 14 = v."""
    return np.ascontiguousarray(np.repeat(gray[:, :, None], 3, axis=2))


# ---- (f) the census of components and clusters --------------------------------------------------------------------------------------------
def component_census(thr, label, csize):
    """{(size, tile spread): count} of the components of exactly 24 and 25 pixels (spread: CC tiles the component touches)."""
    h, w = thr.shape
    out = {}
    for n in (MIN_COMPONENT - 1, MIN_COMPONENT):
        for rep in np.flatnonzero(csize.reshape(-1) == n):
            if thr.reshape(-1)[rep] == 127 or label.reshape(-1)[rep] != rep:
                continue
            ys, xs = np.nonzero((label == rep) & (thr != 127))
            key = (n, len(set(zip((ys // CC_T).tolist(), (xs // CC_T).tolist()))))
            out[key] = out.get(key, 0) + 1
    return out


def cluster_partners(cluster_keys):
    """The representatives that are one side of a kept cluster."""
    k = np.asarray(cluster_keys, dtype=np.uint64)
    return set((k >> np.uint64(32)).tolist()) | set((k & np.uint64(0xFFFFFFFF)).tolist())


def point_tiles(points):
    """The k_points tiles (bx, by) of a cluster's packed points (x << 18 | y << 4 | ..., half-pixel units; the source pixel of a point
    lies at most one pixel from it)."""
    p = np.asarray(points, dtype=np.uint32)
    x, y = (p >> 18) // 2, ((p >> 4) & 0x3FFF) // 2
    return set(zip((x // PT_TW).tolist(), (y // PT_TH).tolist()))
