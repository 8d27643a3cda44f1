"""Per-frame image sizes (amdAprilTagsSetPerFrameSizes): frames of different sizes -- a mixed camera rig, or windows inside larger
images -- in ONE submission.  The definition under test: every stage buffer and every record of every frame equals what the CPU oracle
gives for that frame submitted alone (tests/parity_util.py, unchanged), whatever the handle's own size, the frame's batch slot and
what the slot held before."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from isaac_ros_apriltag_amd import capi, synth  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
import parity_util as pu  # noqa: E402

PATHS = ("latency", "throughput")
FAM = ("tag36h11",)
INVALID_ARGUMENT, SIZE_MISMATCH = 1, 4

# (w, h, cols, rows, lo, hi) on a 1100 x 200 handle: two threshold blocks across x (1024 pixels each), seven down y, a ragged handle
# remainder.  Oracle detections per frame: 12, 12, 12, 6, 1, 1, 0 at decimate 1 and 2; 12, 12, 12, 5, 1, 0, 0 at decimate 3.
HANDLE_W, HANDLE_H = 1100, 200
MIXED = ((1100, 70, 12, 1, 40, 52),    # full handle width
         (1037, 67, 12, 1, 40, 50),    # ragged, beyond the 1024-pixel block edge
         (1024, 64, 12, 1, 38, 48),    # ends exactly on the block edge
         (300, 200, 3, 2, 50, 70),     # full handle height
         (96, 64, 1, 1, 36, 44),       # small frame
         (40, 33, 1, 1, 20, 24),       # tiny frame
         (16, 16, 1, 1, 8, 9))         # one cluster at decimate 1, no quad


def _k4(K):
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def _scene(w, h, cols, rows, lo, hi):
    img, K, _ = synth._grid_scene(w, h, [("tag36h11", (7 * (w + h) + i) % 587) for i in range(cols * rows)],
                                  cols, rows, w + h, lo, hi, 30, 25, 2.0)
    return np.ascontiguousarray(img), K


_scenes = {}


def _mixed():
    """The frames of the mixed batch, rendered once per session: [(img, K)] in table order."""
    if "mixed" not in _scenes:
        _scenes["mixed"] = [_scene(*f) for f in MIXED]
    return _scenes["mixed"]


def _admissible(w, h, decimate, tile):
    return 1 + (w - 1) // decimate >= tile and 1 + (h - 1) // decimate >= tile


def _block_noise(w, h, seed, cell=4):
    """Two-level block noise: cells of `cell` pixels, 60 or 190."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 2, size=((h + cell - 1) // cell, (w + cell - 1) // cell), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(c, np.ones((cell, cell), dtype=np.uint8))[:h, :w] * 130 + 60).astype(np.uint8)


def _submit_and_compare(det, frames, tensors, order, decimate, tile, **more):
    """One submission of frames[i] for i in `order` (slot k holds frame order[k]); every stage and every record of every slot
    against the oracle on that frame alone.  Returns (mismatches, oracle detections in all)."""
    g = det.detect_batch_ex([tensors[i] for i in order], max_dets=64, intrinsics=[_k4(frames[i][1]) for i in order])
    errs, total = [], 0
    for slot, i in enumerate(order):
        img, K = frames[i]
        e, odets = pu.compare_stages(det, slot, img, FAM, K, decimate, tile_size=tile, **more)
        e += pu.compare_detections(g[slot], odets, exact=True)
        errs += ["slot %d, frame %dx%d: %s" % (slot, img.shape[1], img.shape[0], x) for x in e]
        total += len(odets)
    return errs, total


def _handle(decimate=1, tile=4, max_batch=8, w=HANDLE_W, h=HANDLE_H, **kw):
    return AprilTagDetector(w, h, decimate=decimate, tile_size=tile, max_batch=max_batch, per_frame_sizes=True, **kw)


# ---- 1. every stage and every record of every frame -------------------------------------------------------------------------------
@pytest.mark.parametrize("decimate", (1, 2, 3))
@pytest.mark.parametrize("tile", (4, 8))
@pytest.mark.parametrize("path", PATHS)
def test_mixed_batch_every_stage(built, decimate, tile, path):
    frames = _mixed()
    idx = [i for i, f in enumerate(MIXED) if _admissible(f[0], f[1], decimate, tile)]   # (16 x 16 at decimate 3, tile 8: the refusal test)
    assert len(idx) == (6 if (decimate, tile) == (3, 8) else 7)
    tensors = [torch.from_numpy(f[0]).cuda() for f in frames]
    det = _handle(decimate, tile)
    det.set_submission_path(path)
    errs, total = _submit_and_compare(det, frames, tensors, idx, decimate, tile)
    assert total >= 40, total   # (equality is not equality of empty lists)
    assert not errs, errs[:6]
    # the same frames in reverse slot order: every slot now holds a frame of another size than before (stale extents, stale planes)
    errs, total = _submit_and_compare(det, frames, tensors, idx[::-1], decimate, tile)
    assert total >= 40, total
    assert not errs, errs[:6]
    det.close()


# ---- 2. graph replay -----------------------------------------------------------------------------------------------------------------
def test_graph_replay_across_size_pairs(built):
    """The captured launch graph of a two-frame submission is replayed for other size pairs: the extents travel through the descriptor
    block, not through the graph's kernel arguments."""
    frames = _mixed()
    tensors = [torch.from_numpy(f[0]).cuda() for f in frames]
    det = _handle(max_batch=2)
    total = 0
    for pair in ((0, 4), (3, 5), (4, 0)):
        errs, n = _submit_and_compare(det, frames, tensors, list(pair), 1, 4)
        assert not errs, (pair, errs[:6])
        total += n
    assert total >= 12 + 1 + 6 + 1 + 1 + 12
    capturing, live, retired = det.graph_replay()
    assert capturing and live == 1 and retired == 0, (capturing, live, retired)   # one graph, captured once, still live
    assert det.last_submission_path() == "latency"
    det.close()


# ---- 3. the cluster-size cap follows the frame -----------------------------------------------------------------------------------------
def _comb():
    img = np.full((64, 96), 200, dtype=np.uint8)
    img[6:58, 6:90] = 30
    for x in range(10, 86, 6):
        img[6:50, x:x + 3] = 200
    return img


def test_cluster_cap_is_the_frames(built):
    """A 96 x 64 comb whose one large cluster has 2832 points: above the frame's cap 3 (2 w + 2 h) = 960, below the 1100 x 200 handle's
    7020.  The oracle keeps no cluster for the frame alone (and one when the same pixels sit in an 1100 x 70 canvas): so must the handle."""
    img = _comb()
    K = synth.default_K(96, 64)
    _, alone = po.detect(img, families=FAM, params=pu.oracle_params(K), want_dump=True)
    canvas = np.full((70, 1100), 200, dtype=np.uint8)
    canvas[:64, :96] = img
    _, wide = po.detect(canvas, families=FAM, params=pu.oracle_params(synth.default_K(1100, 70)), want_dump=True)
    assert len(alone["clusters"]) == 0 and len(wide["clusters"]) == 1 and wide["clusters"][0][2] == 2832
    det = _handle(max_batch=1)
    for path in PATHS:
        det.set_submission_path(path)
        errs, _ = _submit_and_compare(det, [(img, K)], [torch.from_numpy(img).cuda()], [0], 1, 4)
        assert not errs, (path, errs[:6])
        assert int(det.debug(0, capi.DBG_COUNTS)[1]) == 0
    det.close()


# ---- 4. quad_sigma's identity and edge-copy rules follow the frame ----------------------------------------------------------------------
@pytest.mark.parametrize("decimate", (1, 2))
@pytest.mark.parametrize("sigma", (4.0, -4.0))
def test_quad_sigma_per_frame(built, decimate, sigma):
    """ksz = 17: in 17 x 40, 40 x 17 and 16 x 16 (working sizes at decimate 1; half of them at decimate 2) one axis or both fall under
    the identity rule n <= ksz, which the 96 x 64 handle's own size never does."""
    frames = [(_block_noise(17, 40, 1), synth.default_K(17, 40)), (_block_noise(40, 17, 2), synth.default_K(40, 17)),
              (_block_noise(16, 16, 3), synth.default_K(16, 16)), _scene(96, 64, 1, 1, 36, 44)]
    tensors = [torch.from_numpy(f[0]).cuda() for f in frames]
    det = _handle(decimate, 4, max_batch=4, w=96, h=64, quad_sigma=sigma)
    for path in PATHS:
        det.set_submission_path(path)
        for order in ([0, 1, 2, 3], [3, 2, 1, 0]):
            errs, _ = _submit_and_compare(det, frames, tensors, order, decimate, 4, quad_sigma=sigma)
            assert not errs, (path, order, errs[:6])
    det.close()


# ---- 5. colour ---------------------------------------------------------------------------------------------------------------------------
def _bt601(rgb):
    r, g, b = (rgb[..., i].astype(np.uint32) for i in range(3))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


@pytest.mark.parametrize("decimate", (1, 2))   # the fused loader of the one-pass threshold kernel; the conversion launch
@pytest.mark.parametrize("encoding", ("bgr8", "rgba8"))
def test_colour_mixed_batch(built, decimate, encoding):
    """The existing contract of colour submissions, per frame: the records of the mixed batch as bgr8 / rgba8 equal, bit for bit, those of
    the mono8 submission of the converted frames (which is held against the oracle stage by stage)."""
    frames = _mixed()
    rgb = [np.stack([f[0], f[0], f[0] // 2 + 40], axis=-1) for f in frames]
    mono = [(np.ascontiguousarray(_bt601(c)), f[1]) for c, f in zip(rgb, frames)]
    if encoding == "bgr8":
        col = [np.ascontiguousarray(c[..., ::-1]) for c in rgb]
    else:
        col = [np.ascontiguousarray(np.concatenate([c, np.full(c.shape[:2] + (1,), 255, np.uint8)], axis=-1)) for c in rgb]
    det = _handle(decimate)
    intr = [_k4(f[1]) for f in frames]
    tm = [torch.from_numpy(m[0]).cuda() for m in mono]
    errs, total = _submit_and_compare(det, mono, tm, list(range(len(mono))), decimate, 4)
    assert total >= 40 and not errs, (total, errs[:6])
    gm = det.detect_batch_ex(tm, max_dets=64, intrinsics=intr)
    gc = det.detect_batch_ex([torch.from_numpy(c).cuda() for c in col], max_dets=64, intrinsics=intr, encoding=encoding)
    for f, (a, b) in enumerate(zip(gc, gm)):
        assert not pu.compare_detections(a, b, exact=True), (MIXED[f][:2], pu.compare_detections(a, b, exact=True)[:3])
        w, h = det.debug(f, capi.DBG_COUNTS)[6:8]
        assert (int(w), int(h)) == (1 + (MIXED[f][0] - 1) // decimate, 1 + (MIXED[f][1] - 1) // decimate)
    det.close()


# ---- 6. a window inside a larger image ---------------------------------------------------------------------------------------------------
def test_window(built):
    """INTEGRATION.md, "mixed rigs and windows": dev_ptr at the window's first pixel (an unaligned address), the full image's pitch, the
    window's size, the principal point shifted by the window's origin.  Equal to the oracle on the cropped array."""
    W, H, x0, y0, w, h = 1100, 300, 517, 33, 300, 200
    full = _block_noise(W, H, 7, cell=9)
    full[y0:y0 + h, x0:x0 + w] = _mixed()[3][0]
    K = synth.default_K(W, H)
    Kw = K.copy()
    Kw[0, 2] -= x0
    Kw[1, 2] -= y0
    t = torch.from_numpy(full).cuda()
    crop = np.ascontiguousarray(full[y0:y0 + h, x0:x0 + w])
    det = _handle(max_batch=1)
    for path in PATHS:
        det.set_submission_path(path)
        g = det.detect_batch_ex([(t.data_ptr() + y0 * W + x0, W, w, h)], max_dets=64, intrinsics=[_k4(Kw)])[0]
        errs, odets = pu.compare_stages(det, 0, crop, FAM, Kw)
        errs += pu.compare_detections(g, odets, exact=True)
        assert len(odets) == 6 and not errs, (path, len(odets), errs[:6])
    # the host adds the window's origin to the pixel coordinates: the tags then lie where the full frame has them
    centres = np.array([d["center"] for d in g]) + (x0, y0)
    assert (centres[:, 0] > x0).all() and (centres[:, 0] < x0 + w).all() and (centres[:, 1] > y0).all() and (centres[:, 1] < y0 + h).all()
    det.close()


# ---- 7. refusals and the default -----------------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(capi.AprilTagsError) as e:
        fn()
    return e.value.code


@pytest.mark.parametrize("decimate,tile", ((1, 4), (3, 8)))
def test_refusals_and_default(built, decimate, tile):
    frames = _mixed()
    tensors = [torch.from_numpy(f[0]).cuda() for f in frames]
    big = torch.zeros((HANDLE_H + 1, HANDLE_W + 1), dtype=torch.uint8, device="cuda")
    det = AprilTagDetector(HANDLE_W, HANDLE_H, decimate=decimate, tile_size=tile, max_batch=2)

    def exact(order):
        errs, _ = _submit_and_compare(det, frames, tensors, order, decimate, tile)
        assert not errs, errs[:6]

    def small(i):   # frame i as a four-element tuple: its own size whatever the mode
        return (tensors[i].data_ptr(), MIXED[i][0], MIXED[i][0], MIXED[i][1])

    full = _scene(HANDLE_W, HANDLE_H, 6, 1, 60, 90)
    tfull = torch.from_numpy(full[0]).cuda()

    def exact_full():
        g = det.detect_batch_ex(tfull, max_dets=64, intrinsics=[_k4(full[1])])[0]
        errs, odets = pu.compare_stages(det, 0, full[0], FAM, full[1], decimate, tile_size=tile)
        errs += pu.compare_detections(g, odets, exact=True)
        assert len(odets) >= 5 and not errs, (len(odets), errs[:6])

    # mode off (the default): only the handle's own size
    assert _code(lambda: det.detect_batch_ex([small(4)])) == SIZE_MISMATCH
    exact_full()
    # ... and the setter is refused while a submission is in flight
    prep = det.prepare(tfull, max_dets=64)
    det.submit_prepared(prep)
    assert _code(lambda: det.set_per_frame_sizes(True)) == INVALID_ARGUMENT
    det.wait_prepared(prep)
    assert not det.per_frame_sizes
    exact_full()

    det.set_per_frame_sizes(True)
    # wider / taller than the handle
    assert _code(lambda: det.detect_batch_ex([(big.data_ptr(), HANDLE_W + 1, HANDLE_W + 1, 70)])) == SIZE_MISMATCH
    exact([4, 0])
    assert _code(lambda: det.detect_batch_ex([small(4), (big.data_ptr(), HANDLE_W + 1, 96, HANDLE_H + 1)])) == SIZE_MISMATCH
    exact([0, 4])
    # below the minimum: a working image without one full tile (16 x 16 at decimate 3, tile 8, is 6 x 6)
    tiny = (tile - 1) * decimate
    assert _code(lambda: det.detect_batch_ex([(big.data_ptr(), HANDLE_W + 1, tiny, 64)])) == SIZE_MISMATCH
    assert _code(lambda: det.detect_batch_ex([(big.data_ptr(), HANDLE_W + 1, 64, tiny)])) == SIZE_MISMATCH
    if (decimate, tile) == (3, 8):
        assert _code(lambda: det.detect_batch_ex([small(6)])) == SIZE_MISMATCH
    assert _code(lambda: det.detect_batch_ex([(big.data_ptr(), 0, 0, 64)])) == SIZE_MISMATCH
    exact([3, 5] if _admissible(40, 33, decimate, tile) else [3, 4])
    # a pitch smaller than the frame's own row
    assert _code(lambda: det.detect_batch_ex([(tensors[4].data_ptr(), 95, 96, 64)])) == INVALID_ARGUMENT
    exact([4, 3])
    # the setter with a submission in flight, mode on
    prep = det.prepare([tensors[4], tensors[3]], max_dets=64)
    det.submit_prepared(prep)
    assert _code(lambda: det.set_per_frame_sizes(False)) == INVALID_ARGUMENT
    det.wait_prepared(prep)
    assert det.per_frame_sizes
    exact([3, 4])
    # and off again: as at creation
    det.set_per_frame_sizes(False)
    assert _code(lambda: det.detect_batch_ex([small(4)])) == SIZE_MISMATCH
    exact_full()
    det.close()


# ---- 8. random sizes -----------------------------------------------------------------------------------------------------------------------
_RANDOM_N, _RANDOM_W, _RANDOM_H = 32, 272, 208


def _random_frames():
    if "random" not in _scenes:
        rng = np.random.default_rng(20240611)
        out = []
        for k in range(_RANDOM_N):
            w, h = int(rng.integers(8, _RANDOM_W + 1)), int(rng.integers(8, _RANDOM_H + 1))
            m = min(w, h)
            if m >= 48:   # a 20-pixel tag with its margin, rotation and tilt fits
                lo = max(20.0, 0.30 * m)
                out.append(_scene(w, h, 1, 1, lo, max(lo + 1.0, 0.42 * m)))
            else:
                out.append((_block_noise(w, h, 100 + k), synth.default_K(w, h)))
        _scenes["random"] = out
    return _scenes["random"]


@pytest.mark.parametrize("decimate", (1, 2))
@pytest.mark.parametrize("path", PATHS)
def test_random_sizes(built, decimate, path):
    frames = _random_frames()
    tensors = [torch.from_numpy(f[0]).cuda() for f in frames]
    det = _handle(decimate, 4, max_batch=_RANDOM_N, w=_RANDOM_W, h=_RANDOM_H)
    det.set_submission_path(path)
    det.detect_batch_ex(tensors, max_dets=64, intrinsics=[_k4(f[1]) for f in frames])
    errs, with_quads = [], 0
    for i, (img, K) in enumerate(frames):
        e, _ = pu.compare_stages(det, i, img, FAM, K, decimate)
        errs += ["frame %d, %dx%d: %s" % (i, img.shape[1], img.shape[0], x) for x in e]
        with_quads += 1 if len(det.debug(i, capi.DBG_QUADS)) else 0   # (equal to the oracle's where errs is empty)
    assert not errs, errs[:6]
    assert with_quads * 4 >= _RANDOM_N, with_quads
    det.close()


# ---- 9. the multi-camera node ----------------------------------------------------------------------------------------------------------------
def test_multi_camera_node_mixed_sizes(built):
    """Two streams of different sizes through one AprilTagMultiCameraNode with max_width / max_height set: one batched submission, and
    per stream the message an AprilTagNode of its own publishes for the same frame (a detector of that frame's size) -- the records of
    the per-frame-sizes detector on the two frames.  With the options left at 0 the second size is dropped, as before."""
    from isaac_ros_apriltag_amd import build as b
    from isaac_ros_apriltag_amd import node
    b.build_node()
    frames = [_mixed()[1], _mixed()[3]]   # 1037 x 67 and 300 x 200
    Ks = [[float(v) for v in K.reshape(-1)] for _, K in frames]

    def push(n, s, stamp):
        img = frames[s][0]
        return n.on_frame(s, img.ctypes.data, False, "mono8", img.shape[1], img.shape[0], img.shape[1], Ks[s], "cam%d" % s, stamp)

    multi = node.AprilTagMultiCameraNode(2, max_width=HANDLE_W, max_height=HANDLE_H)
    plain = node.AprilTagMultiCameraNode(2)   # max_width = max_height = 0: the first frame's size
    singles = [node.AprilTagNode() for _ in range(2)]
    det = _handle(max_batch=2)
    try:
        want = []
        for s in range(2):
            img = frames[s][0]
            dets, fid = singles[s].on_frame(img.ctypes.data, False, "mono8", img.shape[1], img.shape[0], img.shape[1], Ks[s], "cam%d" % s, (7, s))
            want.append(dets)
        assert [len(w) for w in want] == [12, 6]
        raw, cnt = det.detect_batch_raw([torch.from_numpy(f[0]).cuda() for f in frames], max_tags=64, intrinsics=[_k4(f[1]) for f in frames])
        assert cnt == [12, 6]
        for rnd in range(2):
            assert push(multi, 0, (7 + rnd, 0)) and multi.publishes(0) == rnd
            assert push(multi, 1, (7 + rnd, 1))   # completes the round: ONE submission of both sizes
            for s in range(2):
                assert multi.publishes(s) == rnd + 1
                dets, fid, stamp = multi.last(s)
                assert fid == "cam%d" % s and stamp == (7 + rnd, s)
                assert dets == want[s], (rnd, s)
                for i, d in enumerate(dets):
                    r = raw[s * 64 + i]
                    assert d["id"] == int(r.id) and d["corners"] == [[float(r.corners[k].x), float(r.corners[k].y)] for k in range(4)]
        # a frame larger than max_width x max_height is dropped
        bigger = np.zeros((HANDLE_H + 8, 64), dtype=np.uint8)
        assert not multi.on_frame(0, bigger.ctypes.data, False, "mono8", 64, HANDLE_H + 8, 64, Ks[0], "cam0", (9, 0))
        # the options left at 0: the handle takes the first frame's size and the other size is dropped, as before
        assert push(plain, 0, (7, 0)) and not push(plain, 1, (7, 1))
        assert plain.flush() == 1 and plain.publishes(0) == 1 and plain.publishes(1) == 0
        assert plain.last(0)[0] == want[0]
    finally:
        det.close()
        multi.close()
        plain.close()
        [n.close() for n in singles]


# ---- 10. one wrong build -----------------------------------------------------------------------------------------------------------------------
def test_cluster_cap_fails_on_the_wrong_build(built):
    """libapriltag_amd_mut6.so (csrc/tools_hooks.h, AMDAT_MUTATE=6: k_cluster_select takes the cluster-size cap from the handle instead
    of the frame) keeps the comb's cluster: test_cluster_cap_is_the_frames, in a process of its own, must FAIL on it and pass on the product
    library."""
    import subprocess
    from isaac_ros_apriltag_amd import build as bld
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(bld.lib_mutant(6)):
        bld.build_mutants()

    def run(lib):
        env = dict(os.environ)
        env.pop("AMDAT_LIB", None)
        if lib:
            env["AMDAT_LIB"] = lib
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-p", "no:cacheprovider",
                              "-k", "test_cluster_cap_is_the_frames"], capture_output=True, text=True, timeout=600, cwd=root, env=env)
        return out.returncode, [l for l in out.stdout.splitlines() if " passed" in l or " failed" in l or l.startswith("FAILED")], out
    rc_bad, tail_bad, out_bad = run("mut6")
    assert rc_bad == 1 and any(" failed" in l for l in tail_bad), (tail_bad, out_bad.stdout[-1500:], out_bad.stderr[-1500:])
    assert "clusters: gpu 1 vs oracle 0" in out_bad.stdout, out_bad.stdout[-1500:]   # the stage that differs, and how
    rc_ok, tail_ok, out_ok = run(None)
    assert rc_ok == 0 and any(" passed" in l for l in tail_ok) and not any(" failed" in l for l in tail_ok), (tail_ok, out_ok.stdout[-1500:])
