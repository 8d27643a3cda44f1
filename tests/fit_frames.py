"""Frames for the quad fit's size classes and sort forms, and the census that says which of them a frame really reaches.

A bit-exact comparison of quads only bites where the oracle KEEPS a quad: a cluster both sides drop passes however wrong the fit
behind it is.  So the frames here are built from rectangles whose boundary clusters have chosen sizes, and `census` maps every
quad (the oracle's or the library's) back to its cluster's point count, hence to the kernel instance and the sort form that
produced it.  tests/test_fit_frames_cpu.py holds every census condition on the oracle alone; tests/test_fit_classes_gpu.py puts the
same frames through the library.  A plain helper module: nothing here touches a GPU."""
import functools

import numpy as np

D, L = 35, 215   # dark and light paint; the ground is light

# ---- the launch plan's size classes, as literals (isaac_ros_apriltag_amd/csrc/launch_plan.h: plan_classes).  tests/test_fit_frames_cpu.py
# compares them with the class table the header produces, so a change there breaks a host test and not this census silently. ----------
CLASS_HI = (128, 768, 2048, 4096, 8192)      # class c takes CLASS_HI[c - 1] < count <= CLASS_HI[c]; class 5 everything above 8192
CLASS_NT = (64, 64, 128, 256, 512, 1024)     # threads of k_fit_quads for the class (class 0: k_fit_small<2> where the plan has one)
NCLASSES = 6
FIT_SMALL_HI = 128                           # k_fit_small<2> takes clusters up to here: throughput set of a split-moments handle only
SORT_CAP = 16384                             # LDS key array of the 1024-thread class ...
SORT_CAP_RAISED_MAX = 18432                  # ... raised to the handle's largest cluster (rounded up to 64) where that is at most this
REG_FORMS = ("reg1", "reg2", "reg4")         # one-wave class: keys in registers, 1 / 2 / 4 per lane (up to 64 / 128 / 256 keys)
ONE_WAVE_FORMS = REG_FORMS + ("lds_padded", "lds_unpadded")   # ... 257-512 in LDS padded to 512, 513-768 unpadded (the array holds 768)


def handle(w, h):
    """max_cluster_points and split_moments of a w x h working image (amdCreateAprilTagsDetectorEx)."""
    mcp = 3 * (2 * w + 2 * h)
    return mcp, int(w <= 2048 and h <= 2048 and mcp < 32768)


def sort_cap(w, h):
    mcp = handle(w, h)[0]
    return (mcp + 63) & ~63 if SORT_CAP < mcp <= SORT_CAP_RAISED_MAX else SORT_CAP


def has_fit_small(w, h, path):
    """The plan launches k_fit_small<2> for clusters up to 128 points: throughput set, two-double moments."""
    return path == "throughput" and bool(handle(w, h)[1])


def size_class(count):
    return int(np.searchsorted(np.asarray(CLASS_HI), count, side="left"))


def sort_form(count, cap=SORT_CAP, fit_small=False):
    """How the keys of a cluster of `count` points are sorted (kernels_quad.h: k_fit_quads, slope keys + sort)."""
    if count <= FIT_SMALL_HI and fit_small:
        return "fit_small"
    if count <= 64:
        return "reg1"
    if count <= 128:
        return "reg2"
    if count <= 256:
        return "reg4"
    if count <= 512:
        return "lds_padded"
    if count <= 768:
        return "lds_unpadded"
    if count <= SORT_CAP:          # 128 .. 512 threads: the array holds the class's power of two; 1024 threads: up to 16 384
        return "lds_padded"
    return "lds_unpadded" if count <= cap else "global"


def census(clusters, quads, cap=SORT_CAP, fit_small=False):
    """clusters: (keys, counts); quads: keys of the quads.  Returns (kept, dropped): kept = one (count, class, form) per quad, sorted;
    dropped = the sorted counts of the clusters that ended without a quad."""
    ckeys, ccounts = clusters
    by_key = {int(k): int(c) for k, c in zip(ckeys, ccounts)}
    qkeys = [int(k) for k in quads]
    assert len(by_key) == len(ckeys) and len(set(qkeys)) == len(qkeys) and all(k in by_key for k in qkeys)
    kept = sorted((by_key[k], size_class(by_key[k]), sort_form(by_key[k], cap, fit_small)) for k in qkeys)
    dropped = sorted(c for k, c in by_key.items() if k not in set(qkeys))
    return kept, dropped


def census_oracle(dump, cap=SORT_CAP, fit_small=False):
    return census(([c[0] for c in dump["clusters"]], [c[2] for c in dump["clusters"]]), [q["key"] for q in dump["quads"]], cap, fit_small)


def census_gpu(cl, q, cap=SORT_CAP, fit_small=False):
    """cl, q: the library's DBG_CLUSTERS and DBG_QUADS records of a frame."""
    return census((cl["key"], cl["count"]), q["key"], cap, fit_small)


def classes_of(kept):
    return {c for _, c, _ in kept}


def forms_of(kept, cls=None):
    return {f for _, c, f in kept if cls is None or c == cls}


# ---- renderer ------------------------------------------------------------------------------------------------------------------------
def rect_extent(r):
    """Half extents (x, y) of the axis-aligned box that holds rectangle r = (cx, cy, hw, hh, angle, value, amp, period), ripple included."""
    cx, cy, hw, hh, ang, val, amp, per = r
    c, s = abs(np.cos(ang)), abs(np.sin(ang))
    return c * (hw + abs(amp)) + s * (hh + abs(amp)), s * (hw + abs(amp)) + c * (hh + abs(amp))


def paint(w, h, rects, checker=None):
    """Rectangles (cx, cy, hw, hh, angle, value, amp, period) painted in list order on a light ground, as float64.  In the rectangle's
    frame (u, v) a pixel is inside if |u| < hw + amp sin(2 pi v / period) and |v| < hh + amp sin(2 pi u / period + 1): sides that ripple
    with amplitude amp.  checker = (x0, y0, cell, size): a size x size patch of a checkerboard of cell-pixel squares, dark first (the
    last row and column of cells are cut where cell does not divide size).  Every rectangle is evaluated inside its bounding box only
    (a third of the time of whole-frame arithmetic on a 2-megapixel frame)."""
    img = np.full((h, w), float(L))
    for r in rects:
        cx, cy, hw, hh, ang, val, amp, per = r
        ex, ey = rect_extent(r)
        x0, x1 = max(0, int(np.floor(cx - ex)) - 1), min(w, int(np.ceil(cx + ex)) + 2)
        y0, y1 = max(0, int(np.floor(cy - ey)) - 1), min(h, int(np.ceil(cy + ey)) + 2)
        if x0 >= x1 or y0 >= y1:
            continue
        yy, xx = np.mgrid[y0:y1, x0:x1].astype(np.float64)
        c, s = np.cos(ang), np.sin(ang)
        u, v = (xx - cx) * c + (yy - cy) * s, -(xx - cx) * s + (yy - cy) * c
        ru = hw + amp * np.sin(2 * np.pi * v / per)
        rv = hh + amp * np.sin(2 * np.pi * u / per + 1.0)
        img[y0:y1, x0:x1][(np.abs(u) < ru) & (np.abs(v) < rv)] = val
    if checker is not None:
        x0, y0, cell, size = checker
        yy, xx = np.mgrid[0:size, 0:size]
        img[y0:y0 + size, x0:x0 + size] = np.where(((xx // cell) + (yy // cell)) % 2 == 0, float(D), float(L))
    return img


def finish(img, sigma=0.0, seed=606):
    """The mono8 frame of a painted image: sigma > 0 adds Gaussian noise from default_rng(seed) of the frame's shape; rounded, clipped."""
    if sigma > 0:
        img = img + np.random.default_rng(seed).normal(0, sigma, img.shape)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def render(w, h, rects, sigma=0.0, seed=606, checker=None):
    return finish(paint(w, h, rects, checker), sigma, seed)


# ---- the ladder: three large nested rectangles and a row of small ones, so that one frame has a quad in every class ------------------
LADDER_H = 1000
# an 88 x 88 patch of 9-pixel cells in free ground: quads from clusters of 68 - 71 points (whole cells) and of 62 (the 9 x 7 cells of the
# cut last row and column) -- the register sorts with two keys and with one key per lane
LADDER_CHECKER = (1850, 235, 9, 88)


def ladder_rects(a):
    return [(700, 500, 680, 480, 0.01, D, a, 37), (700, 500, 600, 420, 0.0, L, 0, 37), (700, 500, 520, 360, -0.04, D, a, 41),
            (700, 500, 440, 300, 0.0, L, 0, 37), (700, 500, 200, 160, 0.2, D, a, 29), (1600, 150, 90, 80, -0.3, D, 0, 37),
            (1850, 150, 30, 25, 0.5, D, 0, 37), (1960, 150, 20, 18, 0.4, D, 0, 37), (1500, 400, 12, 10, 0.3, D, 0, 37),
            (1600, 400, 7, 6, 0.2, D, 0, 37), (1700, 400, 5, 5, 0.6, D, 0, 37), (1800, 400, 3.2, 3.2, 0.1, D, 0, 37),
            (1700, 750, 230, 200, 0.7, D, a, 31)]


LADDER_WIDTHS = (2048, 2049)   # the same content: the one column more takes the handle off the two-double moments (and k_fit_small)


@functools.lru_cache(maxsize=None)
def _ladder_painted(a):
    img = paint(max(LADDER_WIDTHS), LADDER_H, ladder_rects(a), LADDER_CHECKER)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def ladder(w, a=0.0, sigma=0.0, seed=606):
    """The ladder frame, w wide (nothing is painted beyond column 2047, so both widths cut one painting).  Read-only: shared by the tests."""
    assert w in LADDER_WIDTHS
    img = finish(_ladder_painted(a)[:, :w], sigma, seed)
    img.setflags(write=False)
    return img


LADDER_CONTENT = {"clean": (0.0, 0.0), "noise": (0.0, 1.0), "ripple": (3.0, 0.0)}   # name -> (a, sigma)


# ---- the near-limit sweep: the nested layout with seeded ripples, so that every class sees quads that only just pass and shapes that
# only just fail ---------------------------------------------------------------------------------------------------------------------
SWEEP_SEEDS = tuple(range(9000, 9024))


def sweep_rects(seed):
    rng = np.random.default_rng(seed)
    rects = ladder_rects(0.0)
    # (index in the ladder, angle jitter, amplitude range, scale of amplitude and period)
    for i, jit, amax, scale in ((0, 0.01, 4.5, 1.0), (2, 0.04, 4.5, 1.0), (4, 0.4, 6.0, 1.0), (12, 0.7, 4.5, 1.0), (5, 0.7, 6.0, 1.0),
                                (6, 0.7, 6.0, 0.5)):
        cx, cy, hw, hh, ang, val, _, _ = rects[i]
        amp, per, dang = rng.uniform(1.5, amax), rng.uniform(23.0, 45.0), rng.uniform(-jit, jit)
        rects[i] = (cx, cy, hw, hh, ang + dang, val, amp * scale, per * scale)
    return rects


@functools.lru_cache(maxsize=None)
def _sweep_painted(seed):
    img = finish(paint(max(LADDER_WIDTHS), LADDER_H, sweep_rects(seed)))
    img.setflags(write=False)
    return img


def sweep_frame(seed, w):
    """Sweep frame `seed`, w wide.  Read-only: shared by the tests."""
    assert w in LADDER_WIDTHS
    img = np.ascontiguousarray(_sweep_painted(seed)[:, :w])
    img.setflags(write=False)
    return img


def rect_of_box(box, rects, w, h, tol=4.0):
    """Index of the rectangle of `rects` whose boundary a cluster is, from the box (xmin, xmax, ymin, ymax) of the cluster's points in
    pixels: every side of the box lies where the rectangle's own box (cut by the frame) has it, to the ripple and `tol` pixels.  None
    if no rectangle fits."""
    for i, r in enumerate(rects):
        ex, ey = rect_extent(r)
        want = (max(r[0] - ex, 0.0), min(r[0] + ex, w - 1.0), max(r[1] - ey, 0.0), min(r[1] + ey, h - 1.0))
        if all(abs(g - t) <= tol + 2 * abs(r[6]) for g, t in zip(box, want)):
            return i
    return None


def cluster_boxes(dump):
    """Per cluster of an oracle dump: (key, count, (xmin, xmax, ymin, ymax) in pixels)."""
    out = []
    pts = dump["points"]
    for key, start, count in dump["clusters"]:
        p = pts[start:start + count]
        x, y = (p >> 18).astype(np.float64) * 0.5, ((p >> 4) & 0x3FFF).astype(np.float64) * 0.5
        out.append((key, count, (x.min(), x.max(), y.min(), y.max())))
    return out


# ---- giants: one rectangle a frame, boundaries beyond the 16 384-key LDS array of the 1024-thread class -----------------------------
# name -> (w, h, hw, hh, angle, amp, period, (count range), quad expected)
GIANTS = {
    "1080p_lds_unpadded": (1920, 1080, 930, 510, 0.0, 2.0, 12.0, (16385, 18000), True),     # raised sort_cap 18 048: LDS, unpadded
    "1080p_above_the_cap": (1920, 1080, 930, 510, 0.0, 2.0, 10.0, (0, 0), False),            # above 18 000 points: no cluster on either side
    "2048sq_global_split_a1": (2048, 2048, 1000, 1000, 0.0, 1.0, 31.0, (16385, 24576), True),   # global-scratch sort, two-double sweep
    "2048sq_global_split_a2": (2048, 2048, 1000, 1000, 0.0, 2.0, 17.0, (16385, 24576), True),
    "2800_global_general": (2800, 1800, 1330, 830, 0.01, 0.0, 37.0, (16385, 27600), True),   # global-scratch sort, 128-bit sweep
}


def giant(name):
    w, h, hw, hh, ang, amp, per, _, _ = GIANTS[name]
    return render(w, h, [(w / 2, h / 2, hw, hh, ang, D, amp, per)])
