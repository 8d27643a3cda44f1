"""Frames that meet the quad fit's floating-point rules by design, and the census that says which rule each frame reaches.

tests/fit_frames.py shows that every size class and sort form ends in a quad the oracle keeps; it does not show WHY a cluster lives or
dies.  The frames here are small shapes built for one statement each -- the box and border-direction tests (csrc/fit_statements.h), the
cut to max_nmaxima corners (k_fit_small, three forms in k_fit_quads), the tests of the corner search, and the determinant, area, angle
and winding tests of k_quad_finish -- each with a twin on the other side of the rule.  `census` reads the oracle's per-cluster fit log
(oracle/apriltag_oracle.c: ato_fit_rec_t) beside its dump; tests/test_fit_rule_frames_cpu.py holds every condition on the oracle alone,
tests/test_fit_rules_gpu.py puts the same frames through the library.  A plain helper module: nothing here touches a GPU."""
import functools

import numpy as np

import fit_frames as ff

D, L = ff.D, ff.L
COS_CRITICAL = float(np.float32(np.cos(np.radians(10.0))))   # cos_critical_rad as the float parameter field holds it


# ---- painting ---------------------------------------------------------------------------------------------------------------------------
def ground(w, h):
    return np.full((h, w), L, dtype=np.uint8)


def fill(img, verts, val=D):
    """Even-odd fill of the polygon `verts` ((x, y) pairs) on pixel centres."""
    v = np.asarray(verts, dtype=np.float64)
    h, w = img.shape
    x0, x1 = max(0, int(v[:, 0].min()) - 1), min(w, int(v[:, 0].max()) + 2)
    y0, y1 = max(0, int(v[:, 1].min()) - 1), min(h, int(v[:, 1].max()) + 2)
    yy, xx = np.mgrid[y0:y1, x0:x1].astype(np.float64)
    inside = np.zeros(xx.shape, dtype=bool)
    for i in range(len(v)):
        (ax, ay), (bx, by) = v[i], v[(i + 1) % len(v)]
        if ay != by:
            inside ^= ((ay > yy) != (by > yy)) & (xx < (bx - ax) * (yy - ay) / (by - ay) + ax)
    img[y0:y1, x0:x1][inside] = val


def turned(verts, angle, centre):
    v = np.asarray(verts, dtype=np.float64)
    c, s = np.cos(angle), np.sin(angle)
    return np.stack([centre[0] + v[:, 0] * c - v[:, 1] * s, centre[1] + v[:, 0] * s + v[:, 1] * c], 1)


def rhombus(hl, acute_deg):
    """Half length hl along x, acute angle at both ends: the obtuse corners turn by the acute angle, the acute ones by 180 - it, so
    cos_dtheta is +cos(acute) at two corners and -cos(acute) at the other two."""
    hs = hl * np.tan(np.radians(acute_deg) / 2)
    return [(-hl, 0.0), (0.0, -hs), (hl, 0.0), (0.0, hs)]


def kite(lh, x1, x2, tip_deg):
    """A tip of tip_deg at (-lh, 0), the widest point at x1, a blunt end at x2: only the tip's angle is extreme."""
    hh = (x1 + lh) * np.tan(np.radians(tip_deg) / 2)
    return [(-lh, 0.0), (x1, -hh), (x2, 0.0), (x1, hh)]


DART = [(-30.0, -30.0), (30.0, 0.0), (-30.0, 30.0), (-10.0, 0.0)]   # one reflex vertex


def shallow(b):
    """A triangle with a fourth vertex pushed b pixels out of its base: that vertex turns by 2 atan(b / 60)."""
    return [(0.0, -50.0), (60.0, 40.0), (0.0, 40.0 + b), (-60.0, 40.0)]


def _cells(w, h, cell, rects):
    """Rectangles (s, aspect, ox, oy, angle): sides s * aspect and s / aspect about the centre of its cell plus (ox, oy), cells in
    row order."""
    per_row = w // cell
    out = []
    for i, (s, asp, ox, oy, ang) in enumerate(rects):
        out.append((cell * (i % per_row) + cell / 2 + ox, cell * (i // per_row) + cell / 2 + oy, s * asp / 2, s / asp / 2, ang, D, 0, 9))
    return ff.render(w, h, out)


# ---- the exits atlas (tag36h11, decimate 1) -----------------------------------------------------------------------------------------------
RHOMBUS_DEG = (6, 7, 8, 9, 10, 11, 12, 13, 14)
KITE_DROPPED_DEG = (6, 7, 8, 9, 9.5)
KITE_KEPT_DEG = (10.5, 11, 12, 13)


def _rows(shapes, angle=0.05, w=224, pitch=44):
    assert pitch * len(shapes) + 4 <= 224
    img = ground(w, 224)
    for i, s in enumerate(shapes):
        fill(img, turned(s, angle, (w / 2, pitch * i + pitch / 2 + 2)))
    return img


def _exits_edges():
    """A straight edge across the frame (every point of its cluster on one row: the box exit), a square cut by the frame's corner,
    bars of two pixels' width (2 x 16 and 2 x 20: two maxima; 2 x 14: four maxima and no admissible choice; 2 x 50: 13 maxima, none
    admissible)."""
    img = ground(224, 224)
    img[190:, :] = D
    img[:20, :24] = D
    img[60:62, 20:36] = D
    img[80:82, 20:34] = D
    img[100:102, 20:40] = D
    img[120:122, 20:70] = D
    return img


def _exits_darts():
    img = ground(224, 224)
    for t in range(4):
        fill(img, turned(DART, t * np.pi / 2 + 0.1, (56 + 112 * (t % 2), 56 + 112 * (t // 2))))
    return img


def _exits_shallow(b, angle):
    img = ground(160, 160)
    fill(img, turned(shallow(b), angle, (80, 80)))
    return img


# ---- the area atlas: rectangles of _cells, 40-pixel cells ---------------------------------------------------------------------------------------
# per family (min_tag_width w): "window" = two kept with a Heron area in [0.95 w^2, w^2) and two dropped by area; "above" = one kept at
# or above w^2 beside the two dropped ones
AREA = {
    "tag36h11": (8, [(7.125, 1.0, 0.0, 0.0, 0.785), (7.125, 1.0, 0.5, 0.5, 0.0), (7.75, 1.25, 0.0, 0.0, 0.3), (7.25, 1.25, 0.5, 0.5, 0.0)],
                 [(8.125, 1.25, 0.3, 0.6, 0.3), (7.75, 1.25, 0.0, 0.0, 0.3), (7.25, 1.25, 0.5, 0.5, 0.0)]),
    "tag25h9": (7, [(6.75, 1.0, 0.3, 0.6, 0.3), (6.75, 1.25, 0.3, 0.6, 0.785), (7.0, 1.25, 0.0, 0.0, 0.3), (6.75, 1.25, 0.5, 0.5, 0.3)],
                [(6.125, 1.0, 0.0, 0.0, 0.0), (7.0, 1.25, 0.0, 0.0, 0.3), (6.75, 1.25, 0.5, 0.5, 0.3)]),
    "tag16h5": (6, [(5.125, 1.25, 0.0, 0.0, 0.0), (5.125, 1.0, 0.5, 0.5, 0.0), (5.625, 1.25, 0.5, 0.5, 0.3), (5.625, 1.0, 0.0, 0.0, 0.3)],
                [(6.0, 1.25, 0.3, 0.6, 0.3), (5.625, 1.25, 0.5, 0.5, 0.3), (5.625, 1.0, 0.0, 0.0, 0.3)]),
}


def _area_dec2():
    """Decimate 2 (min_tag_width 4): squares of 10 to 16 pixels; the smallest cluster the working image can hold is already kept."""
    return ff.render(80, 80, [(20, 20, 5, 5, 0, D, 0, 9), (60, 20, 6, 6, 0.3, D, 0, 9), (20, 60, 7, 7, 0.2, D, 0, 9), (60, 60, 8, 8, 0, D, 0, 9)])


# ---- the border atlas --------------------------------------------------------------------------------------------------------------------------
REVERSED = "standard41h12"   # the reversed-border layout of tests/family_layouts.py (9 x 9 grid, border square of 5): the handle's only family


@functools.lru_cache(maxsize=None)
def reversed_family_args():
    """(slot, name, bit_x, bit_y, width_at_border, total_width, reversed_border, codes) as tests/test_gpu_parity.py registers it."""
    import family_layouts as fl
    bx, by = fl.standard_layout(9, 5)
    return (7, REVERSED, bx, by, 5, 9, True, fl.toy_codes(41, 5, seed=11, min_dist=12, layout=(bx, by, 5)))


def _border():
    """Two dark rectangles in the light ground (normal borders) and two light ones inside a dark field (reversed)."""
    img = ff.render(160, 120, [(30, 30, 12, 10, 0.2, D, 0, 9), (30, 85, 9, 14, -0.4, D, 0, 9), (110, 60, 40, 50, 0.0, D, 0, 9),
                               (100, 40, 13, 10, 0.3, L, 0, 9), (118, 85, 10, 12, -0.2, L, 0, 9)])
    return img


# ---- the cut atlas: thin rhombi, whose two obtuse corners are weak maxima among those of the sides' staircase -----------------------------------
# name -> (w, h, half length, acute angle, turn, sigma, seed); the census finds the rhombus' cluster kept with its weakest corner at
# rank exactly max_nmaxima = 10 among all maxima: one rank lower and the cut takes a corner of the quad away
CUT = {
    "cut_small": (80, 80, 12.0, 27.0, 1.09, 0.0, 0),                       # 102 points, 12 maxima: k_fit_small / k_fit_quads<64>, one per lane
    "cut_wave": (224, 120, 90.0, 10.0, 0.05, 0.0, 0),                      # 752 points, 41 maxima: one per lane
    "cut_regs": (400, 400, 250.0, 11.0, 0.8, 0.0, 0),                      # 2750 points, 322 maxima: FQ_SEL_REGS per lane
    "cut_lds": (900, 900, 560.0, 11.5, np.pi / 4 + 0.02, 1.0, 1),          # 6278 points, 727 maxima: the removal rounds in LDS
    # the twin: 126 points, 12 maxima, kept -- but with another quad than the search over all 12 maxima would choose: the cut took a
    # corner of that one away (cut_wave's cluster, the 11-degree rhombus and two of the sharper ones of the exits atlas are of this kind too)
    "cuttwin_small": (80, 80, 13.0, 24.0, 2.65, 0.0, 0),
    "cuttwin_regs": (400, 400, 230.0, 12.0, 0.6, 0.0, 0),                  # 2510 points, 289 maxima, weakest corner at rank 5
    "cuttwin_lds": (900, 900, 560.0, 10.25, np.pi / 4 + 0.02, 1.0, 2),     # 6278 points, 765 maxima, weakest corner at rank 9
}
WIDE = 2049   # the multi-wave cases again in a canvas of this width: k_fit_quads<NT, false>


NOISE_BAND = 4   # seeded noise reaches this far from the shape's boundary: it moves the points' weights and leaves the ground flat


def _near_boundary(dark, r):
    """Pixels within r (Chebyshev) of a dark / light transition."""
    def spread(m):
        out = m.copy()
        for axis in (0, 1):
            acc = out.copy()
            for s in range(1, r + 1):
                acc |= np.roll(out, s, axis) | np.roll(out, -s, axis)
            out = acc
        return out
    return spread(dark) & spread(~dark)


@functools.lru_cache(maxsize=None)
def _cut(name):
    w, h, hl, a, ang, sigma, seed = CUT[name]
    img = ground(w, h)
    fill(img, turned(rhombus(hl, a), ang, (w / 2, h / 2)))
    if sigma > 0:   # the noise ff.finish would add to the whole frame, kept near the boundary only: no noise clusters beside the shape's
        noise = np.random.default_rng(seed).normal(0, sigma, img.shape)
        img = ff.finish(img + np.where(_near_boundary(img == D, NOISE_BAND), noise, 0.0))
    img.setflags(write=False)
    return img


def _cut_wide(name):
    img = ground(WIDE, CUT[name][1])
    img[:, :CUT[name][0]] = _cut(name)
    return img


# ---- every frame: name -> (family, decimate, builder) ------------------------------------------------------------------------------------------
FRAMES = {
    "exits_edges": ("tag36h11", 1, _exits_edges),
    "exits_darts": ("tag36h11", 1, _exits_darts),
    "exits_rhombi_a": ("tag36h11", 1, lambda: _rows([rhombus(90, a) for a in RHOMBUS_DEG[:5]])),
    "exits_rhombi_b": ("tag36h11", 1, lambda: _rows([rhombus(90, a) for a in RHOMBUS_DEG[5:]] + [rhombus(90, 10.5)])),
    "exits_kites_dropped": ("tag36h11", 1, lambda: _rows([kite(100, 60, 85, a) for a in KITE_DROPPED_DEG])),
    "exits_kites_kept": ("tag36h11", 1, lambda: _rows([kite(100, 60, 85, a) for a in KITE_KEPT_DEG], pitch=52)),
    "exits_shallow_3": ("tag36h11", 1, lambda: _exits_shallow(3, 0.1)),
    "exits_shallow_5": ("tag36h11", 1, lambda: _exits_shallow(5, 0.9)),
    "exits_shallow_7": ("tag36h11", 1, lambda: _exits_shallow(7, 0.1)),
    "area_dec2": ("tag36h11", 2, _area_dec2),
    "border_reversed_only": (REVERSED, 1, _border),
    "border_tag36h11": ("tag36h11", 1, _border),
    "cut_small": ("tag36h11", 1, lambda: _cut("cut_small")),
    "cuttwin_small": ("tag36h11", 1, lambda: _cut("cuttwin_small")),
    "cuttwin_regs": ("tag36h11", 1, lambda: _cut("cuttwin_regs")),
    "cuttwin_lds": ("tag36h11", 1, lambda: _cut("cuttwin_lds")),
    "cuttwin_regs_wide": ("tag36h11", 1, lambda: _cut_wide("cuttwin_regs")),
    "cuttwin_lds_wide": ("tag36h11", 1, lambda: _cut_wide("cuttwin_lds")),
    "cut_wave": ("tag36h11", 1, lambda: _cut("cut_wave")),
    "cut_regs": ("tag36h11", 1, lambda: _cut("cut_regs")),
    "cut_lds": ("tag36h11", 1, lambda: _cut("cut_lds")),
    "cut_regs_wide": ("tag36h11", 1, lambda: _cut_wide("cut_regs")),
    "cut_lds_wide": ("tag36h11", 1, lambda: _cut_wide("cut_lds")),
}
for _fam, (_w, _win, _above) in AREA.items():
    FRAMES["area_%s_window" % _fam] = (_fam, 1, functools.partial(_cells, 80, 80, 40, _win))
    FRAMES["area_%s_above" % _fam] = (_fam, 1, functools.partial(_cells, 80, 80, 40, _above))
RULE_FRAMES = tuple(sorted(n for n in FRAMES if not n.startswith("cut")))   # at most 224 x 224
CUT_FRAMES = tuple(sorted(n for n in FRAMES if n.startswith("cut_")))        # a kept quad on rank exactly 10
CUT_TWINS = tuple(sorted(n for n in FRAMES if n.startswith("cuttwin_")))     # a kept quad that is not the uncut search's


@functools.lru_cache(maxsize=None)
def frame(name):
    """Frame `name` as submitted (mono8).  Read-only: shared by the tests."""
    img = np.ascontiguousarray(FRAMES[name][2]())
    img.setflags(write=False)
    return img


def groups():
    """The frames that can share one submission: {(family, decimate, h, w): names}."""
    out = {}
    for n in sorted(FRAMES):
        out.setdefault((FRAMES[n][0], FRAMES[n][1]) + frame(n).shape, []).append(n)
    return out


# ---- census ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_family(name):
    from oracle import pyoracle as po
    if name != REVERSED:
        return name
    a = reversed_family_args()
    return po.custom_family(*a[1:])


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """(dump, fit log) of frame `name` under its family and decimate, every other parameter at its default."""
    from oracle import pyoracle as po
    fam, dec, _ = FRAMES[name]
    _, dump, log = po.detect(frame(name), families=(oracle_family(fam),), params=po.default_params(decimate=dec), want_dump=True,
                             want_fit_log=True)
    return dump, log


@functools.lru_cache(maxsize=None)
def uncut_record(name):
    """The log record of the one cluster of cut frame `name` with more than max_nmaxima maxima, with the log's search over ALL maxima
    run whatever their number (cut_changes; a few seconds at 700 maxima, so only where a test asks for it)."""
    from oracle import pyoracle as po
    fam, dec, _ = FRAMES[name]
    _, _, log = po.detect(frame(name), families=(oracle_family(fam),), params=po.default_params(decimate=dec), want_dump=True,
                          want_fit_log=True, fit_log_uncut_max=1 << 20)
    (r,) = log[log["nmaxima"] > 10]
    return r


def census(name):
    """The fit log of frame `name` as a sorted list of (points_in, reason) -- what the CPU test writes out per frame -- and the log."""
    dump, log = oracle_run(name)
    assert len(log) == len(dump["clusters"]) and sorted(int(k) for k in log["key"][log["reason"] == 10]) == [q["key"] for q in dump["quads"]]
    return sorted((int(r["points_in"]), int(r["reason"])) for r in log), log


def kinds(rec, w=8):
    """The rule-level labels of one log record (w: min_tag_width): what a wrong build of one statement would change."""
    out = set()
    r = int(rec["reason"])
    if r == 10:
        out.add("kept")
        if 0.95 * w * w <= rec["area"] < w * w:
            out.add("kept_under_w2")
        if rec["max_abs_cos"] > 0.95:
            out.add("kept_cos_above_0.95")
        if rec["weakest_rank"] == 10 and rec["nmaxima"] > 10:
            out.add("kept_on_rank_10")
        if rec["dot_changes"] == 1:
            out.add("kept_dot_decided")
        if rec["cut_changes"] == 1:
            out.add("kept_cut_decided")
    if r == 8:
        out.add("dropped_by_area")
    if r == 9:
        below, above = rec["min_cos"] < -COS_CRITICAL, rec["max_cos"] > COS_CRITICAL
        if rec["winding_only"] == 1:
            out.add("winding_alone")
        if below and not above and rec["winding_fails"] == 0:
            out.add("cos_below_alone")
        if above and not below and rec["winding_fails"] == 0:
            out.add("cos_above_alone")
        if above and below:
            out.add("cos_both")
    return out


def expectation(name):
    """(keys of the clusters the oracle keeps, keys of those it drops) of frame `name`: what the GPU test looks up in the library's lists."""
    _, log = oracle_run(name)
    return {int(k) for k in log["key"][log["reason"] == 10]}, {int(k) for k in log["key"][log["reason"] != 10]}


def table():
    """Reason by frame, for a failure message."""
    from oracle import pyoracle as po
    lines = []
    for n in sorted(FRAMES):
        _, log = oracle_run(n)
        by = np.bincount(log["reason"], minlength=11)
        lines.append("%-28s %s" % (n, "  ".join("%s: %d" % (po.FIT_REASONS[r], by[r]) for r in range(11) if by[r])))
    return "\n".join(lines)
