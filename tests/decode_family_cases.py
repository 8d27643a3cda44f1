"""Shared by tests/test_decode_families_cpu.py and tests/test_decode_families_gpu.py: the families, words and expected scan results of
tests/decode_lookup_cases.py (taken from there, not copied) drawn as tags, so that the decode KERNEL's scan meets them -- code tables
of several codes per lane with ties (dense16), a 64-bit word (d8), border squares of 9 and 10 cells (d7, d8) -- plus one family:

  d7   classic row-major 7 x 7, 49 bits, 200 seeded random codes, registered through amdAprilTagsRegisterFamily at its limit d = 7
       (width_at_border 9, total_width 11: 72 border samples); its words are built by decode_lookup_cases.make_words like the others'

Frames.  A tag is its cell grid -- total_width cells and one more white ring around them, the data cells from the word -- turned by
k mod 4 quarter turns for the k-th tag of its frame (np.rot90), every cell 6 x 6 pixels of 25 or 230, on a 640 x 480 ground of 150,
10 px between tags: 30 tags a frame for d8, 70 for d3.  No warping, no supersampling.  On top of that every pixel carries the grain
GRAIN (below).  400 words per family, drawn with a fixed seed from the family's word list with a quota per kind of word, are one
submission of at most 14 frames.

Which way the detector reads a tag decides the answer wherever the scans of the four orientations differ.  read_orientation() takes it
from the oracle's own quad: the tag's corner, as drawn, that the decoded quad's corner 0 lies on, plus the tag's turn.  One constant is
left, READ_OFFSET, between the corner numbers of the quad as fitted and as decoded.  The exact code words cannot fix it: a record's
rotation is itself read off the quad's corners, and for an exact word orientation + rotation = 0 holds under every offset.  The words
whose four orientations scan differently can: tests/test_decode_families_cpu.py::test_read_offset asserts that READ_OFFSET is the only
offset under which the oracle's answers are the scan's, in every family that has such words.

Everything is computed once per process and never changed."""
import numpy as np

from oracle import pyoracle as po
import decode_lookup_cases as dl
import decode_lookup_ref as ref
import family_layouts as fl
import parity_util as pu
from isaac_ros_apriltag_amd import synth

NAMES = ("d3", "h5", "dense16", "std52", "d8", "d7")
MAX_HAMMINGS = dl.MAX_HAMMINGS
SLOTS = dict(dl.SLOTS, d7=8)      # d7 takes the remaining custom slot
W, H = 640, 480
CELL, GAP, BLACK, WHITE, GROUND = 6, 10, 25, 230, 150
NWORDS = 400
MAX_DETECTIONS = 256              # std52's outer-ring data cells give about 350 quads a frame; few of them decode
PITCH_PAD = 19
QUOTA = (("exact", 100), ("flipped", 100), ("turned", 120), ("mid", 30), ("edge", 2))   # the rest of the 400: random words
# The edge refinement renumbers a quad's corners: its corner i becomes the meeting point of the refined sides i and i + 1, which is the
# fitted quad's corner i + 1 (upstream's refine_edges does the same).  So the decoded quad's corner j is the fitted quad's corner
# j + READ_OFFSET.  tests/test_decode_families_cpu.py::test_read_offset holds the constant against the oracle's own answers.
READ_OFFSET = 1
CENTRED = 3.0                     # a record within half a cell of a tag's centre is "centred on" it
_cache = {}
_D7 = {"d": 7, "codes": 200, "seed": 305, "words_seed": 1005}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- families, words, the scan's answers -------------------------------------------------------------------------------------------------
def family(name):
    """decode_lookup_cases.family(name); for d7 the same dict."""
    if name != "d7":
        return dl.family(name)

    def make():
        d = _D7["d"]
        bx, by = [1 + i % d for i in range(d * d)], [1 + i // d for i in range(d * d)]
        rng = np.random.default_rng(_D7["seed"])
        codes = [dl._random_word(rng, d * d) for _ in range(_D7["codes"])]
        return {"name": "lookup_d7", "builtin": False, "classic_d": d, "bit_x": bx, "bit_y": by, "width_at_border": d + 2, "total_width": d + 4,
                "nbits": d * d, "codes": codes, "rot_src": fl.rot_source(bx, by, d + 2)}
    return _cached(("family", name), make)


def words(name):
    return dl.words(name) if name != "d7" else _cached(("words+kinds", name), lambda: dl.make_words(family(name), _D7["words_seed"]))[0]


def kinds(name):
    return dl.kinds(name) if name != "d7" else _cached(("words+kinds", name), lambda: dl.make_words(family(name), _D7["words_seed"]))[1]


def nearest(name):
    """Per word and rotation the scan's (distance, index): decode_lookup_cases.nearest."""
    if name != "d7":
        return dl.nearest(name)

    def make():
        f = family(name)
        flat = [w for word in words(name) for w in ref.rotations(word, f["rot_src"])]
        dist, idx = ref.nearest_many(f["codes"], flat)
        dist.setflags(write=False), idx.setflags(write=False)
        return dist.reshape(-1, 4), idx.reshape(-1, 4)
    return _cached(("nearest", name), make)


def register(name, capi):
    """Registers the family in its slot (nothing to do for the built-in h5); returns the name a handle takes."""
    f = family(name)
    if f["builtin"]:
        return f["name"]
    if "classic_d" in f:
        capi.register_family(SLOTS[name], f["name"], f["classic_d"], f["codes"])
    else:
        capi.register_family_ex(SLOTS[name], f["name"], f["bit_x"], f["bit_y"], f["width_at_border"], f["total_width"], False, f["codes"])
    return f["name"]


def unregister(name, capi):
    if not family(name)["builtin"]:
        capi.unregister_family(SLOTS[name])


def oracle_family(name):
    f = family(name)
    return f["name"] if f["builtin"] else _cached(("ofam", name), lambda: po.custom_family(
        f["name"], f["bit_x"], f["bit_y"], f["width_at_border"], f["total_width"], False, f["codes"]))


# ---- the selection and its frames ----------------------------------------------------------------------------------------------------------
LANE_TIES = {"dense16": 40}        # words per family drawn for a tie inside one lane of the kernel's scan (below)
PRESUMED_CORNER = 2                # the drawn corner (bottom-right) the decoded quad's corner 0 is presumed to lie on when drawing those


def lane_tie(name, wi, orientation, max_hamming=2):
    """Whether the word, first read from `orientation`, is accepted unturned within max_hamming and its winning distance is shared by
    a second code in the first code's lane (index congruent mod 64)."""
    f = family(name)
    dist, idx = nearest(name)
    if dist[wi][orientation] > max_hamming:
        return False
    hd = ref._popcount_u64(np.array(f["codes"], dtype=np.uint64) ^ np.uint64(ref.rotations(words(name)[wi], f["rot_src"])[orientation]))
    tied = np.flatnonzero(hd == dist[wi][orientation])
    return bool((tied[1:] % 64 == tied[0] % 64).any())


def selection(name):
    """Indices into words(name) of the 400 words drawn: QUOTA per kind (all there are where a family has fewer), random words for the
    rest, in a drawn order (the order decides a tag's frame, place and turn).  In a family of LANE_TIES that many places of the order
    are filled afterwards, each with a drawn word that has a lane_tie() at the orientation its place would be read from if the
    detector's quads start where PRESUMED_CORNER says (the census of tests/test_decode_families_cpu.py counts what the oracle really
    reads)."""
    def make():
        rng = np.random.default_rng(7000 + NAMES.index(name))
        kd = np.array(kinds(name))
        nlane = LANE_TIES.get(name, 0)
        picked = []
        for kind, quota in QUOTA:
            at = np.flatnonzero(kd == kind)
            picked += [int(i) for i in rng.choice(at, size=min(quota, len(at)), replace=False)]
        at = np.flatnonzero(kd == "random")
        picked += [int(i) for i in rng.choice(at, size=NWORDS - nlane - len(picked), replace=False)]
        out = np.array(picked + [-1] * nlane, dtype=np.int64)[rng.permutation(NWORDS)]
        if nlane:
            per = layout(name)["cols"] * layout(name)["rows"]
            used = set(picked)
            pool = [int(i) for i in rng.permutation(len(kd)) if int(i) not in used]
            for j in np.flatnonzero(out < 0):
                b = (PRESUMED_CORNER + (j % per) % 4) % 4
                out[j] = next(i for i in pool if i not in used and lane_tie(name, i, b))
                used.add(int(out[j]))
        out.setflags(write=False)
        return out
    return _cached(("selection", name), make)


def cell_grid(f, word):
    """The tag's cells as gray values, (total_width + 2)^2: the border square's outer cells black, the ring around it white, data cells
    from the word (bit nbits - 1 - i is data cell i, 1 = white), everything else white."""
    wb, tw, n = f["width_at_border"], f["total_width"], f["nbits"]
    m = (wb - tw) // 2
    g = np.full((tw + 2, tw + 2), WHITE, dtype=np.uint8)
    o = 1 - m                                             # grid index of border coordinate 0
    g[o:o + wb, o:o + wb] = BLACK
    g[o + 1:o + wb - 1, o + 1:o + wb - 1] = WHITE
    for i in range(n):
        g[f["bit_y"][i] + o, f["bit_x"][i] + o] = WHITE if (word >> (n - 1 - i)) & 1 else BLACK
    return g


# The grain every frame carries on top of its cells: a seeded integer field in [-GRAIN, GRAIN], far below the thresholds' contrast
# limit against a black-to-white step of 205.  Without it every border sample of a tag is exactly 25 or exactly 230, both gray models
# are constants whichever samples enter them, and a decode that loses the border samples from index 64 on gives the same records.
GRAIN = 6


def layout(name):
    """{"side": pixels of a tag with its ring, "cols", "rows", "x0", "y0", "border0": offset of the border square inside the tag,
    "border": its side}."""
    f = family(name)
    side = (f["total_width"] + 2) * CELL
    cols, rows = (W + GAP) // (side + GAP), (H + GAP) // (side + GAP)
    return {"side": side, "cols": cols, "rows": rows, "x0": (W - cols * side - (cols - 1) * GAP) // 2, "y0": (H - rows * side - (rows - 1) * GAP) // 2,
            "border0": (1 + (f["total_width"] - f["width_at_border"]) // 2) * CELL, "border": f["width_at_border"] * CELL}


def tags(name):
    """The selection's tags in order: dicts {"word": index into words(name), "frame", "k": quarter turns, "x", "y": the tag's top-left
    pixel, "centre", "corners": the border square's corners as drawn, clockwise from the top-left one}."""
    def make():
        lay = layout(name)
        per = lay["cols"] * lay["rows"]
        out = []
        for j, wi in enumerate(selection(name)):
            slot = j % per
            x = lay["x0"] + (slot % lay["cols"]) * (lay["side"] + GAP)
            y = lay["y0"] + (slot // lay["cols"]) * (lay["side"] + GAP)
            a, b = lay["border0"], lay["border0"] + lay["border"]
            out.append({"word": int(wi), "frame": j // per, "k": slot % 4, "x": x, "y": y,
                        "centre": np.array([x + lay["side"] / 2.0, y + lay["side"] / 2.0]),
                        "corners": np.array([[x + a, y + a], [x + b, y + a], [x + b, y + b], [x + a, y + b]], dtype=np.float64)})
        return tuple(out)
    return _cached(("tags", name), make)


def frames(name):
    """The family's frames (uint8, read-only), at most 14."""
    def make():
        f, ws, tg = family(name), words(name), tags(name)
        imgs = [np.full((H, W), GROUND, dtype=np.int16) for _ in range(tg[-1]["frame"] + 1)]
        for t in tg:
            cells = np.rot90(cell_grid(f, ws[t["word"]]), t["k"])
            px = np.kron(cells, np.ones((CELL, CELL), dtype=np.uint8))
            imgs[t["frame"]][t["y"]:t["y"] + px.shape[0], t["x"]:t["x"] + px.shape[1]] = px
        out = []
        for i, img in enumerate(imgs):
            img = np.clip(img + _grain_of(name, i), 0, 255).astype(np.uint8)
            img.setflags(write=False)
            out.append(img)
        assert len(out) <= 14
        return tuple(out)
    return _cached(("frames", name), make)


def _grain_of(name, i):
    return np.random.default_rng(9000 + 100 * NAMES.index(name) + i).integers(-GRAIN, GRAIN + 1, size=(H, W)).astype(np.int16)


def K():
    return synth.default_K(W, H)


# ---- the oracle on the frames ---------------------------------------------------------------------------------------------------------------
def oracle_frames(key, imgs, ofams, max_hamming):
    """[(detections, dump)] of the oracle per frame.  The dumps are large: only the last key's are kept."""
    if _cache.get("oracle_key") != (key, max_hamming):
        _cache["oracle_val"] = [po.detect(img, families=ofams, params=pu.oracle_params(K(), 1, max_hamming=max_hamming), want_dump=True, max_det=4096)
                                for img in imgs]
        _cache["oracle_key"] = (key, max_hamming)
    return _cache["oracle_val"]


def oracle_on(name, max_hamming):
    return oracle_frames(name, frames(name), (oracle_family(name),), max_hamming)


def tag_quad(tag, quads):
    """The oracle's quad on the tag's border square -- normal border, every corner within 2.5 px of a corner of the square -- as
    (near, p): near[i] is the corner of the tag as drawn (0 = top-left, clockwise) that the quad's corner i lies on."""
    hits = []
    for q in quads:
        if q["reversed_border"]:
            continue
        d = np.abs(q["p"][:, None, :].astype(np.float64) - tag["corners"][None, :, :]).max(axis=2)   # (quad corner, drawn corner)
        near = d.argmin(axis=1)
        if d.min(axis=1).max() < 2.5 and sorted(near.tolist()) == [0, 1, 2, 3]:
            hits.append((tuple(int(v) for v in near), q["p"].astype(np.float64)))
    assert len(hits) == 1, ("quads on the tag's border square", len(hits), tag["frame"], tag["x"], tag["y"])
    return hits[0]


def read_orientation(tag, near, offset=READ_OFFSET):
    """How many quarter turns of the word (decode_lookup_ref.rotate, which turns the cell grid as np.rot90 does) the detector's first
    read of the tag has behind it: the tag is drawn k turns on, and a reader whose corner 0 lies on the drawn corner c reads c more."""
    return (near[offset % 4] + tag["k"]) % 4


def _on_square(p, corners):
    d = np.abs(np.asarray(p, dtype=np.float64)[:, None, :] - corners[None, :, :]).max(axis=2)
    return bool(d.min(axis=1).max() < 2.5 and sorted(d.argmin(axis=1).tolist()) == [0, 1, 2, 3])


def observed(records, quads, name):
    """Per tag of the selection what a detector said: {"near": tag_quad's, "records": the records centred on the tag with every corner
    within 2.5 px of a corner of its border square, "inner": how many more are centred on it (in d3 and dense16 a single data cell
    at a tag's centre can be a quad of its own that decodes: such a record lies inside the square and is no answer for the tag),
    "found", "id", "hamming" of the first of the tag's records (zeros without one), "p3": the quad corner its corner 3 lies on}.  records: per frame the records
    before reconcile (RECORD_DTYPE / capi.DET_DTYPE); quads: per frame the oracle's quads."""
    out = []
    for t in tags(name):
        near, qp = tag_quad(t, quads[t["frame"]])
        rec = records[t["frame"]]
        centred = [i for i in range(len(rec)) if np.abs(rec["c"][i] - t["centre"]).max() < CENTRED]
        at = [i for i in centred if _on_square(rec["p"][i], t["corners"])]
        o = {"near": near, "quad": qp, "records": at, "inner": len(centred) - len(at), "found": 0, "id": 0, "hamming": 0, "p3": 0}
        if at:
            o.update(found=1, id=int(rec["id"][at[0]]), hamming=int(rec["hamming"][at[0]]),
                     p3=int(np.abs(qp - rec["p"][at[0]][3][None, :]).max(axis=1).argmin()))
        out.append(o)
    return out


def row_of(o, offset=READ_OFFSET):
    """(found, id, hamming, rotation) of an observed() entry.  A record's homography is the decoded quad's times a turn by rotation * 90
    degrees, and its corner 3 is the image of (-1, -1), the decoded quad's corner 0 unturned: the rotation is the decoded quad's corner
    that the record's corner 3 lies on."""
    return (o["found"], o["id"], o["hamming"], (o["p3"] - offset) % 4 if o["found"] else 0)


def oracle_observed(name, max_hamming):
    """observed() of the oracle, without the quads' coordinates, kept per (family, max_hamming)."""
    def make():
        res = oracle_on(name, max_hamming)
        return tuple(observed([d["dets_raw"] for _, d in res], [d["quads"] for _, d in res], name))
    return _cached(("observed", name, max_hamming), make)


def expected_rows(name, max_hamming, orientations):
    """The scan's (found, id, hamming, rotation) for every tag whose first read is orientations[j] quarter turns on from the word."""
    dist, idx = nearest(name)
    return [ref.scan_from_nearest(np.roll(dist[t["word"]], -o), np.roll(idx[t["word"]], -o), max_hamming)
            for t, o in zip(tags(name), orientations)]


# ---- the scan as the kernel runs it, and three wrong forms of it (csrc/tools_hooks.h, AMDAT_MUTATE 56 - 58) -------------------------------
def kernel_scan(f, word, max_hamming, lane_keeps_later=False, turn_drops_lane63=False):
    """k_decode_wave's lookup of the word as first read: 64 lanes, lane l scans codes l, l + 64, ... and keeps its first (wrong build
    56, lane_keeps_later: its last) code at its smallest distance; the lanes' results are reduced to the smallest (distance, index);
    accepted within max_hamming, else the word is turned -- every bit from its source bit, by a ballot over lanes < nbits (wrong build
    57, turn_drops_lane63: without lane 63, whose bit, data bit 63, stays 0) -- up to three times.  (found, id, hamming, rotation)."""
    codes = np.array(f["codes"], dtype=np.uint64)
    lanes = np.arange(len(codes)) % 64
    n = f["nbits"]
    for r in range(4):
        hd = ref._popcount_u64(codes ^ np.uint64(word))
        best = int(hd.min())
        tied = np.flatnonzero(hd == best)
        if lane_keeps_later:
            last = {}
            for i in tied:
                last[int(lanes[i])] = int(i)
            bid = min(last.values())
        else:
            bid = int(tied[0])
        if best <= max_hamming:
            return (1, bid, best, r)
        word = ref.rotate(word, f["rot_src"])
        if turn_drops_lane63 and n == 64:
            word &= ~1
    return ref.NOT_FOUND


def border_samples(f):
    """The 8 * width_at_border border samples of the gray models in the kernel's order: (tagx, tagy, is_white) per index, float
    arithmetic as the decode stage's (a float multiply, add and divide, then 2 * (v - 0.5) in double)."""
    wb = np.float32(f["width_at_border"])
    h = np.float32(0.5)
    pats = [(-h, h, 0, 1, 1), (h, h, 0, 1, 0), (wb + h, h, 0, 1, 1), (wb - h, h, 0, 1, 0),
            (h, -h, 1, 0, 1), (h, h, 1, 0, 0), (h, wb + h, 1, 0, 1), (h, wb - h, 1, 0, 0)]
    out = []
    for p0, p1, p2, p3, white in pats:
        for i in range(int(wb)):
            x01 = np.float64((np.float32(p0) + np.float32(i) * np.float32(p2)) / wb)
            y01 = np.float64((np.float32(p1) + np.float32(i) * np.float32(p3)) / wb)
            out.append((2 * (x01 - 0.5), 2 * (y01 - 0.5), white))
    return out


def gray_models(f, img, quad, first=None):
    """The white and the black gray model of a tag, three coefficients each (v = C0 x + C1 y + C2 by least squares over the model's
    valid border samples), from the quad's corners; first: only samples with an index below it enter (wrong build 58: 64).  Also the
    number of valid samples at index 64 and above."""
    src = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], dtype=np.float64)
    A, b = [], []
    for (x, y), (u, v) in zip(src, quad):
        A += [[x, y, 1, 0, 0, 0, -x * u, -y * u], [0, 0, 0, x, y, 1, -x * v, -y * v]]
        b += [u, v]
    Hm = np.append(np.linalg.solve(np.array(A), np.array(b)), 1.0).reshape(3, 3)
    rows, late = {0: [], 1: []}, 0
    for sidx, (x, y, white) in enumerate(border_samples(f)):
        p = Hm @ np.array([x, y, 1.0])
        ix, iy = int(p[0] / p[2]), int(p[1] / p[2])
        if ix < 0 or iy < 0 or ix >= img.shape[1] or iy >= img.shape[0]:
            continue
        late += sidx >= 64
        if first is None or sidx < first:
            rows[white].append((x, y, 1.0, float(img[iy, ix])))
    out = []
    for white in (1, 0):
        m = np.array(rows[white])
        out.append(np.linalg.lstsq(m[:, :3], m[:, 3], rcond=None)[0])
    return out[0], out[1], late


# ---- four families in one handle -------------------------------------------------------------------------------------------------------------
FOUR = ("h5", "dense16", "std52", "d8")     # AT_MAX_FAMILIES; h5 and dense16 share one layout
FOUR_MAX_HAMMING = 2
FOUR_FRAMES = 2                             # the first frames of each of the four
FOUR_MAX_DETECTIONS = 1024                  # dense16 decodes most quads of every frame, std52's 350 a frame included


def four_frames():
    return tuple(img for n in FOUR for img in frames(n)[:FOUR_FRAMES])


def four_oracle():
    return oracle_frames("four", four_frames(), tuple(oracle_family(n) for n in FOUR), FOUR_MAX_HAMMING)
