"""quad_sigma on the device (amdAprilTagsSetQuadSigma): the filtered working image equals the restatement (tests/quad_sigma_ref.py)
bit for bit, and every stage behind it equals the unchanged oracle run on the filtered frame -- at decimate 1 end to end, at
decimate > 1 through the quads (the oracle on J, the frame whose decimation is the filtered working image).  Every record, at every
decimate, equals the oracle that states quad_sigma itself (ato_params_t.quad_sigma: at decimate > 1 refinement and decode read the
untouched frame, which J is not).  Each case runs on both launch sets."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from isaac_ros_apriltag_amd import capi, synth  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402
import parity_util as pu  # noqa: E402
import quad_sigma_ref as qs  # noqa: E402

PATHS = ("latency", "throughput")
SIGMAS = (0.5, 0.8, 1.0, 2.0, 4.0, -0.8, -2.0)


def _k4(K):
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def _bt601(rgb):
    r, g, b = (rgb[..., i].astype(np.uint32) for i in range(3))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def _gray(det, f=0):
    w, h = det.debug(f, capi.DBG_COUNTS)[6:8]
    return det.debug(f, capi.DBG_GRAY).reshape(int(h), int(w))


@pytest.mark.parametrize("decimate,tile", [(1, 4), (2, 4), (3, 4), (1, 8), (2, 8), (3, 8)])
@pytest.mark.parametrize("path", PATHS)
def test_filtered_plane(built, decimate, tile, path):
    img, K, _ = synth.scene_c1()
    h, w = img.shape
    det = AprilTagDetector(w, h, decimate=decimate, tile_size=tile, intrinsics=_k4(K), max_batch=1)
    det.set_submission_path(path)
    t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    for s in SIGMAS:
        det.set_quad_sigma(s)
        det.detect_batch_ex(t, max_dets=64)
        want = qs.filter_image(qs.decimate(img, decimate), s)
        got = _gray(det)
        assert np.array_equal(got, want), (s, int((got != want).sum()))
        errs, _ = pu.compare_stages(det, 0, want, ("tag36h11",), K, 1, tile_size=tile) if decimate == 1 else ([], None)
        assert not [e for e in errs if e.startswith(("gray", "thresh"))], (s, errs[:3])
    det.close()


@pytest.mark.parametrize("shape,pitch,offset", [((477, 635), 640, 0), ((203, 301), 301, 0), ((33, 70), 83, 0), ((16, 20), 20, 0),
                                                ((203, 301), 320, 1)])
@pytest.mark.parametrize("path", PATHS)
def test_filtered_plane_ragged(built, shape, pitch, offset, path):
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w + offset)
    buf = rng.integers(0, 256, size=(h * pitch + offset + 16,), dtype=np.uint8)
    img = np.ascontiguousarray(buf[offset:offset + h * pitch].reshape(h, pitch)[:, :w])
    K = synth.default_K(w, h)
    tb = torch.from_numpy(buf).cuda()
    for decimate in (1, 2, 3):
        det = AprilTagDetector(w, h, decimate=decimate, intrinsics=_k4(K), max_batch=1)
        det.set_submission_path(path)
        for s in (0.8, 2.0, 4.0, -0.8):
            det.set_quad_sigma(s)
            det.detect_batch_ex([(tb.data_ptr() + offset, pitch)], max_dets=64)
            want = qs.filter_image(qs.decimate(img, decimate), s)
            got = _gray(det)
            assert np.array_equal(got, want), (decimate, s, int((got != want).sum()))
            if decimate == 1:
                errs, odets = pu.compare_stages(det, 0, want, ("tag36h11",), K, 1)
                assert not errs, (s, errs[:3])
        det.close()


@pytest.mark.parametrize("name,scene,families", [
    ("c1", lambda: synth.scene_c1(), ("tag36h11",)),
    ("pol", lambda: synth.scene_pol_golden(), ("tag36h11",)),
    ("c2", lambda: synth.scene_c2(), ("tag36h11",)),
    ("c5", lambda: synth.scene_c5(), ("tag36h11", "tag25h9")),
])
@pytest.mark.parametrize("path", PATHS)
def test_decimate1_end_to_end(built, name, scene, families, path):
    r = scene()
    img, K = r[0], r[1]
    h, w = img.shape
    det = AprilTagDetector(w, h, families=families, intrinsics=_k4(K), max_batch=1)
    det.set_submission_path(path)
    t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    for s in (0.8, 2.0, -0.8):
        det.set_quad_sigma(s)
        g = det.detect_batch_ex(t, max_dets=256)[0]
        errs, odets = pu.compare_stages(det, 0, qs.filter_image(img, s), families, K, 1)
        errs += pu.compare_detections(g, odets, exact=True)
        assert not errs, (s, errs[:5])
    det.close()


@pytest.mark.parametrize("name,scene,decimate", [
    ("c2_dec2", lambda: synth.scene_c2(), 2),
    ("c1_dec3", lambda: synth.scene_c1(), 3),
    ("c3_dec2", lambda: synth.scene_c3(), 2),
])
@pytest.mark.parametrize("path", PATHS)
def test_decimated_through_the_quads(built, name, scene, decimate, path):
    r = scene()
    img, K, truth = r[0], r[1], r[2]
    assert truth
    h, w = img.shape
    det = AprilTagDetector(w, h, decimate=decimate, intrinsics=_k4(K), max_batch=1)
    det.set_submission_path(path)
    t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    ids = {int(t["id"]) for t in truth}   # every tag of the scene
    for s in (0.8, -0.8, 2.0):
        det.set_quad_sigma(s)
        g = det.detect_batch_ex(t, max_dets=256)[0]
        J = qs.embed_decimated(img, qs.filter_image(qs.decimate(img, decimate), s), decimate)
        errs, odets = pu.compare_stages(det, 0, J, ("tag36h11",), K, decimate, records=False)   # (decode reads img, not J: records below)
        assert not errs, (s, errs[:5])
        got = {int(d["id"]) for d in g}
        assert ids <= got and {int(d["id"]) for d in odets} <= got, (s, sorted(ids), sorted(got))
        # ... and every stage and every record against the oracle with quad_sigma on the frame as submitted
        errs, odets = pu.compare_stages(det, 0, img, ("tag36h11",), K, decimate, quad_sigma=s)
        errs += pu.compare_detections(g, odets, exact=True)
        assert not errs, (s, errs[:5])
    det.close()


@pytest.mark.parametrize("decimate,tile", [(1, 4), (2, 4), (1, 8)])
@pytest.mark.parametrize("path", PATHS)
def test_colour_equals_mono8(built, decimate, tile, path):
    """Colour submissions give the records and DBG_GRAY of the mono8 submission of their converted frames; that one is checked stage by
    stage against the oracle on the filtered frame (decimate 1) or on J (decimate 2, through the quads)."""
    img, K, _ = synth.scene_c2(seed=1402)
    h, w = img.shape
    rng = np.random.default_rng(decimate * 10 + tile)
    base = img.astype(np.int32)
    rgb = np.stack([np.clip(base + rng.integers(-40, 41, size=(h, w)), 0, 255) for _ in range(3)], axis=2).astype(np.uint8)
    gray = _bt601(rgb)
    det = AprilTagDetector(w, h, decimate=decimate, tile_size=tile, intrinsics=_k4(K), max_batch=1, quad_sigma=0.8)
    det.set_submission_path(path)
    gm = det.detect_batch_ex(torch.from_numpy(gray).cuda(), max_dets=64)[0]
    pm = _gray(det)
    filt = qs.filter_image(qs.decimate(gray, decimate), 0.8)
    assert np.array_equal(pm, filt)
    if decimate == 1:
        errs, odets = pu.compare_stages(det, 0, filt, ("tag36h11",), K, 1, tile_size=tile)
        errs += pu.compare_detections(gm, odets, exact=True)
    else:
        errs, _ = pu.compare_stages(det, 0, qs.embed_decimated(gray, filt, decimate), ("tag36h11",), K, decimate, tile_size=tile, records=False)
    assert not errs, errs[:4]
    # every decimate: stages and records of the mono8 submission against the oracle with quad_sigma on the converted frame
    errs, odets = pu.compare_stages(det, 0, gray, ("tag36h11",), K, decimate, tile_size=tile, quad_sigma=0.8)
    errs += pu.compare_detections(gm, odets, exact=True)
    assert not errs and len(gm) == 10, (len(gm), errs[:4])
    for enc in ("rgb8", "bgr8", "rgba8", "bgra8"):
        nch = capi.ENC_CHANNELS[enc]
        px = np.zeros((h, w, nch), dtype=np.uint8)
        px[..., :3] = rgb if enc.startswith("rgb") else rgb[..., ::-1]
        if nch == 4:
            px[..., 3] = 255
        src = torch.from_numpy(np.ascontiguousarray(px.reshape(h, w * nch))).cuda()
        gc = det.detect_batch_ex([(src.data_ptr(), w * nch)], max_dets=64, encoding=enc)[0]
        assert np.array_equal(_gray(det), pm), enc
        assert not pu.compare_detections(gc, gm, exact=True), enc
    det.close()


# the sigmas at which the oracle finds every tag of the scene at that decimate (tests/test_quad_sigma_oracle_cpu.py asserts the same
# on the host): an exact comparison of records that are all there
_FULL_COUNT = [
    ("c2", 2, (0.8, 1.5, 2.0, 2.7, 3.2, 3.7, 4.0, -0.8, -1.5, -4.0)),
    ("c1", 3, (0.8, 1.5, 2.0, 2.7, 3.2, 3.7, -0.8, -1.5, -4.0)),
    ("c2", 4, (0.8, 1.5, -0.8, -1.5, -4.0)),
]


@pytest.mark.parametrize("name,decimate,sigmas", _FULL_COUNT, ids=["%s_dec%d" % (n, d) for n, d, _ in _FULL_COUNT])
@pytest.mark.parametrize("path", PATHS)
def test_decimated_records(built, name, decimate, sigmas, path):
    """Decimate 2, 3, 4 with the filter on, every tap width class: every tag of the scene is found, and every stage and every record
    (corners, homography, pose, margin) equals the oracle with quad_sigma bit for bit.  A library that refined on the filtered
    plane, skipped refinement or decoded from the wrong frame differs in the records alone."""
    img, K, truth = synth.scene_c2() if name == "c2" else synth.scene_c1()
    ids = sorted(int(t["id"]) for t in truth)
    h, w = img.shape
    det = AprilTagDetector(w, h, decimate=decimate, intrinsics=_k4(K), max_batch=1)
    det.set_submission_path(path)
    t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    for s in sigmas:
        det.set_quad_sigma(s)
        g = det.detect_batch_ex(t, max_dets=256)[0]
        errs, odets = pu.compare_stages(det, 0, img, ("tag36h11",), K, decimate, quad_sigma=s)
        errs += pu.compare_detections(g, odets, exact=True)
        assert not errs, (s, errs[:5])
        assert sorted(int(d["id"]) for d in g) == ids and len(odets) == len(ids), (s, [d["id"] for d in g])
    det.close()


def _edge_shapes(h):
    """Working-image sizes (W, H) for the half width h (ksz = 2 h + 1), aimed at k_quad_sigma (csrc/kernels_filter.h):
      * W - h - 2, the last filtered column, on 16 m - 1, 16 m, 16 m + 1 for 16 m = 128 (the edge of the 128-pixel tile) and 16 m = 48
        (inside a tile): the row pass's `interior` test of a 16-pixel unit and the per-pixel copy rule `xp <= P.W - T.h - 2` behind it
        -- a unit that is filtered whole, one whose last pixel is copied, one with a single filtered pixel;
      * H - h - 2, the last filtered row, on 31, 32, 33 and 63, 64, 65 (the edges of the 32-row tiles): the column pass's
        `y <= P.H - T.h - 2` in the last row of a tile and the first of the next, whose window reaches into the halo rows;
      * W or H equal to ksz (`rows_filter` / `cols_filter` false: the identity along that axis) and ksz + 1 (one filtered sample).
    Sizes below the 4-pixel threshold tile cannot be a handle and are left out (ksz 3)."""
    ksz = 2 * h + 1
    ws = [h + 2 + v for v in (127, 128, 129, 47, 48, 49)] + [ksz, ksz + 1, 70, 150]
    hs = [h + 2 + v for v in (31, 32, 33, 63, 64, 65)] + [40, 37, ksz, ksz + 1]
    return [(w, hh) for w, hh in zip(ws, hs) if min(w, hh) >= 4]


@pytest.mark.parametrize("decimate", [1, 2, 3, 4], ids=lambda d: "dec%d" % d)
@pytest.mark.parametrize("h", sorted(qs.SIGMA_OF_H), ids=lambda h: "h%d" % h)
def test_every_tap_width_on_edge_shapes(built, h, decimate):
    """DBG_GRAY == filter_image for one sigma per half width h = 1 .. 8 (h = 3, 5, 6, 7 run the instances KH = 4 and 8 with
    zero-padded taps, where the copy rule must use h, not KH), blur and sharpen, both launch sets, decimate 1 - 4 (loader kinds 0,
    5, 6, 7), on the shapes of _edge_shapes(h); noise frames, ragged full-resolution sizes, and every other frame at an odd base
    address with a pitch that is no multiple of 16 (the byte loader)."""
    sigma = qs.SIGMA_OF_H[h]
    assert len(qs.taps(sigma)) == 2 * h + 1
    shapes = _edge_shapes(h)
    assert len(shapes) >= 8
    rng = np.random.default_rng(1000 * h + decimate)
    for i, (W, H) in enumerate(shapes):
        w0 = (W - 1) * decimate + 1 + int(rng.integers(0, decimate))
        h0 = (H - 1) * decimate + 1 + int(rng.integers(0, decimate))
        offset, pitch = ((0, (w0 + 15) & ~15), (1, w0 + 3))[i & 1]
        buf = rng.integers(0, 256, size=(offset + h0 * pitch + 16,), dtype=np.uint8)
        img = np.ascontiguousarray(buf[offset:offset + h0 * pitch].reshape(h0, pitch)[:, :w0])
        tb = torch.from_numpy(buf).cuda()
        K = synth.default_K(w0, h0)
        det = AprilTagDetector(w0, h0, decimate=decimate, intrinsics=_k4(K), max_batch=1)
        work = qs.decimate(img, decimate)
        assert work.shape == (H, W)
        for path in PATHS:
            det.set_submission_path(path)
            for s in (sigma, -sigma):
                det.set_quad_sigma(s)
                det.detect_batch_ex([(tb.data_ptr() + offset, pitch)], max_dets=64)
                want = qs.filter_image(work, s)
                got = _gray(det)
                assert got.shape == want.shape and np.array_equal(got, want), (W, H, path, s, int((got != want).sum()),
                                                                                np.argwhere(got != want)[:4].tolist())
        det.close()


def _colour_buffer(rng, gray_like, enc, pad, offset):
    """An interleaved colour frame with random chroma around `gray_like` inside a flat buffer at `offset`, garbage behind every row;
    returns (flat host buffer, pitch, the numpy-converted gray frame)."""
    h, w = gray_like.shape
    nch = capi.ENC_CHANNELS[enc]
    base = gray_like.astype(np.int32)
    rgb = np.stack([np.clip(base + rng.integers(-45, 46, size=(h, w)), 0, 255) for _ in range(3)], axis=2).astype(np.uint8)
    pitch = w * nch + pad
    flat = rng.integers(0, 256, size=(offset + h * pitch + 16,), dtype=np.uint8)
    px = flat[offset:offset + h * pitch].reshape(h, pitch)[:, :w * nch].reshape(h, w, nch)
    px[..., :3] = rgb if enc.startswith("rgb") else rgb[..., ::-1]
    return flat, pitch, _bt601(rgb)


@pytest.mark.parametrize("enc", ["rgb8", "bgr8", "rgba8", "bgra8"])
@pytest.mark.parametrize("decimate", [1, 2])
@pytest.mark.parametrize("path", PATHS)
def test_colour_through_the_filter_off_the_fast_path(built, enc, decimate, path):
    """Colour frames with random chroma at ragged sizes, an odd base address and a pitch that breaks 16-byte alignment: at decimate 1
    the filter reads the colour frame through the byte loader (qs_load16 kinds 1 - 4 with `aligned` false), at decimate 2 it samples
    the conversion plane.  Every stage and every record against the oracle (with quad_sigma) on the numpy-converted frame, for a
    sigma of h == KH, one of h < KH and a sharpen; the tag is found every time."""
    full, K0, _ = synth.scene_c1()
    for ci, (y0, x0, hh, ww) in enumerate(((0, 0, 477, 635), (90, 121, 301, 403))):
        img = np.ascontiguousarray(full[y0:y0 + hh, x0:x0 + ww])
        K = K0.copy()
        K[0, 2] -= x0
        K[1, 2] -= y0
        rng = np.random.default_rng(17 * ci + decimate)
        nch = capi.ENC_CHANNELS[enc]
        pad = (3, 7)[ci] + 2 * ((ww * nch + (3, 7)[ci]) % 16 == 0)      # (a pitch that is no multiple of 16)
        flat, pitch, gray = _colour_buffer(rng, img, enc, pad=pad, offset=(1, 5)[ci])
        assert (pitch % 16) and ((1, 5)[ci] % 2)
        tb = torch.from_numpy(flat).cuda()
        det = AprilTagDetector(ww, hh, decimate=decimate, intrinsics=_k4(K), max_batch=1)
        det.set_submission_path(path)
        for s in (0.8, 1.7, -2.7):
            det.set_quad_sigma(s)
            g = det.detect_batch_ex([(tb.data_ptr() + (1, 5)[ci], pitch)], max_dets=64, encoding=enc)[0]
            assert np.array_equal(_gray(det), qs.filter_image(qs.decimate(gray, decimate), s)), (ci, s)
            errs, odets = pu.compare_stages(det, 0, gray, ("tag36h11",), K, decimate, quad_sigma=s)
            errs += pu.compare_detections(g, odets, exact=True)
            assert not errs, (ci, s, errs[:4])
            assert [int(d["id"]) for d in g] == [0], (ci, s, [d["id"] for d in g])
        det.close()


@pytest.mark.parametrize("enc", ["mono8", "bgr8"])
@pytest.mark.parametrize("decimate", [1, 2])
@pytest.mark.parametrize("path", PATHS)
def test_batch_of_mixed_alignment(built, enc, decimate, path):
    """One submission of three frames with the filter on: the first 16-byte aligned with an aligned pitch, the second at an odd
    address with a pitch of its own, the third aligned again -- `aligned` is a per-frame property of the descriptor, so a loader that
    took it from frame 0 (or from the last frame) reads the others wrongly.  Every stage and every record of every frame."""
    full, K, _ = synth.scene_c1()
    h, w = full.shape
    nch = capi.ENC_CHANNELS[enc]
    rng = np.random.default_rng(40 + decimate)
    layouts = ((0, 0), (3, 5), (0, 16))     # (offset, pitch pad); w * nch is a multiple of 16
    assert (w * nch) % 16 == 0
    tbs, ptrs, grays = [], [], []
    for i, (offset, pad) in enumerate(layouts):
        base = np.ascontiguousarray(np.roll(full, 37 * i, axis=1))   # every frame with content of its own
        if enc == "mono8":
            pitch = w + pad
            flat = rng.integers(0, 256, size=(offset + h * pitch + 16,), dtype=np.uint8)
            flat[offset:offset + h * pitch].reshape(h, pitch)[:, :w] = base
            gray = base
        else:
            flat, pitch, gray = _colour_buffer(rng, base, enc, pad, offset)
        tb = torch.from_numpy(flat).cuda()
        if offset == 0:
            assert tb.data_ptr() % 16 == 0
        tbs.append(tb); ptrs.append((tb.data_ptr() + offset, pitch)); grays.append(gray)
    det = AprilTagDetector(w, h, decimate=decimate, intrinsics=_k4(K), max_batch=3)
    det.set_submission_path(path)
    for s in (0.8, -1.7):
        det.set_quad_sigma(s)
        res = det.detect_batch_ex(ptrs, max_dets=64, encoding=enc)
        for i in range(3):
            errs, odets = pu.compare_stages(det, i, grays[i], ("tag36h11",), K, decimate, quad_sigma=s)
            errs += pu.compare_detections(res[i], odets, exact=True)
            assert not errs, (i, s, errs[:4])
            assert [int(d["id"]) for d in res[i]] == [0], (i, s)
    det.close()


def test_throughput_set_fourteen_frames(built):
    frames = [synth.scene_c2(seed=1234 + 7 * i)[0] for i in range(14)]
    K = synth.scene_c2()[1]
    det = AprilTagDetector(1920, 1080, intrinsics=_k4(K), max_batch=14, quad_sigma=0.8)
    res = det.detect_batch_ex(torch.from_numpy(np.stack(frames)).cuda(), max_dets=64)
    assert det.last_submission_path() == "throughput"
    for i, img in enumerate(frames):
        errs, odets = pu.compare_stages(det, i, qs.filter_image(img, 0.8), ("tag36h11",), K, 1)
        errs += pu.compare_detections(res[i], odets, exact=True)
        assert not errs, (i, errs[:4])
    det.close()


def test_setter_between_submissions(built):
    frames = [synth.scene_c2(seed=1234)[0], synth.scene_c1()[0]]
    frames[1] = np.ascontiguousarray(np.pad(frames[1], ((0, 1080 - 480), (0, 1920 - 640)), constant_values=128))
    K = synth.scene_c2()[1]
    det = AprilTagDetector(1920, 1080, intrinsics=_k4(K), max_batch=1)
    ts = [torch.from_numpy(f).cuda() for f in frames]
    sched = [0.0, 0.8, 0.8, -1.0, -1.0, 0.8, 0.8, 0.0, 0.0, 0.8, -1.0, 0.0]
    for i, s in enumerate(sched):
        det.set_quad_sigma(s)
        img, t = frames[i % 2], ts[i % 2]
        if i % 3 == 2:   # Submit / Wait
            prep = det.prepare(t, max_dets=64)
            det.submit_prepared(prep)
            with pytest.raises(capi.AprilTagsError) as e:
                det.set_quad_sigma(2.0)
            assert e.value.code == 1
            det.wait_prepared(prep)
            g = det.unpack(prep)[0]
        else:
            g = det.detect_batch_ex(t, max_dets=64)[0]
        errs, odets = pu.compare_stages(det, 0, qs.filter_image(img, s), ("tag36h11",), K, 1)
        errs += pu.compare_detections(g, odets, exact=True)
        assert not errs, (i, s, errs[:4])
    assert det._L.amdAprilTagsDebugGraphReplay(det._h, None, None) == 1
    det.close()


@pytest.mark.parametrize("path", PATHS)
def test_identity_values_change_nothing(built, path):
    import ctypes as C
    img, K, _ = synth.scene_c2(seed=1301)
    t = torch.from_numpy(img).cuda()

    def run(sigma):
        det = AprilTagDetector(1920, 1080, intrinsics=_k4(K), max_batch=1)
        det.set_submission_path(path)
        if sigma is not None:
            det.set_quad_sigma(sigma)
        g = det.detect_batch_ex(t, max_dets=64)[0]
        nb = C.c_size_t()
        det._L.amdAprilTagsGetDeviceBytes(det._h, C.byref(nb))
        live, retired = C.c_uint32(), C.c_uint32()
        det._L.amdAprilTagsDebugGraphReplay(det._h, C.byref(live), C.byref(retired))
        out = (g, _gray(det), nb.value, retired.value)
        det.close()
        return out

    g0, gray0, nb0, r0 = run(None)
    for s in (0.0, 0.3, -0.49):
        g, gray, nb, r = run(s)
        assert not pu.compare_detections(g, g0, exact=True), s
        assert np.array_equal(gray, gray0) and nb == nb0 and r == r0, s


@pytest.mark.parametrize("decimate", [1, 2])
def test_setter_refusals_on_a_live_handle(built, decimate):
    """NaN / inf: AMDAT_INVALID_ARGUMENT, |sigma| > 4: AMDAT_UNSUPPORTED -- and the setting in force before (0.8) still filters."""
    img, K, _ = synth.scene_c1()
    h, w = img.shape
    det = AprilTagDetector(w, h, decimate=decimate, intrinsics=_k4(K), max_batch=1, quad_sigma=0.8)
    L = det._L
    for bad, code in ((float("nan"), 1), (float("inf"), 1), (-float("inf"), 1), (4.5, 2), (-4.01, 2), (1e30, 2)):
        assert L.amdAprilTagsSetQuadSigma(det._h, bad) == code, bad
    t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    det.detect_batch_ex(t, max_dets=64)
    assert np.array_equal(_gray(det), qs.filter_image(qs.decimate(img, decimate), 0.8))
    assert L.amdAprilTagsSetQuadSigma(det._h, 4.0) == 0     # the largest accepted value
    assert L.amdAprilTagsSetQuadSigma(det._h, float(np.float32(4.0) * np.float32(1 + 2 ** -23))) == 2
    det.detect_batch_ex(t, max_dets=64)
    assert np.array_equal(_gray(det), qs.filter_image(qs.decimate(img, decimate), 4.0))
    det.close()


def _node_K9(K):
    return [K[0, 0], 0.0, K[0, 2], 0.0, K[1, 1], K[1, 2], 0.0, 0.0, 1.0]


def _same_dets(node_dets, handle_dets):
    """The node publishes float32 corners in its own order (corner_convention of the cuAprilTags records)."""
    if [d["id"] for d in node_dets] != [d["id"] for d in handle_dets]:
        return False
    return all(np.abs(np.array(n["corners"]) - g["p"][::-1]).max() < 1e-3 for n, g in zip(node_dets, handle_dets))


@pytest.mark.parametrize("encoding", ["mono8", "bgr8"])
def test_node_shell_and_multi_camera_node(built, encoding):
    """NodeOptions::quad_sigma 0.8 on both nodes: the same detections as a C ABI handle with the setter, for mono8 and bgr8."""
    from isaac_ros_apriltag_amd import build as b
    from isaac_ros_apriltag_amd import node as nd
    b.build_node()
    frames = [synth.scene_c2(seed=1234 + 9 * i)[0] for i in range(2)]
    K = synth.scene_c2()[1]
    K9 = _node_K9(K)
    rng = np.random.default_rng(5)
    bufs, grays = [], []
    for img in frames:
        if encoding == "mono8":
            bufs.append(np.ascontiguousarray(img)); grays.append(img)
        else:
            rgb = np.stack([np.clip(img.astype(np.int32) + rng.integers(-30, 31, size=img.shape), 0, 255) for _ in range(3)],
                           axis=2).astype(np.uint8)
            bufs.append(np.ascontiguousarray(rgb[..., ::-1]))
            grays.append(_bt601(rgb))
    step = 1920 * capi.ENC_CHANNELS[encoding]
    det = AprilTagDetector(1920, 1080, intrinsics=_k4(K), max_batch=1, quad_sigma=0.8)
    plain = AprilTagDetector(1920, 1080, intrinsics=_k4(K), max_batch=1)
    want, unfiltered = [], []
    for g in grays:
        tg = torch.from_numpy(np.ascontiguousarray(g)).cuda()
        want.append(det.detect_batch_ex(tg, max_dets=64)[0])
        errs, odets = pu.compare_stages(det, 0, qs.filter_image(g, 0.8), ("tag36h11",), K, 1)
        assert not errs + pu.compare_detections(want[-1], odets, exact=True)
        unfiltered.append(plain.detect_batch_ex(tg, max_dets=64)[0])
    det.close(); plain.close()
    assert not all(_same_dets([{"id": d["id"], "corners": d["p"][::-1].tolist()} for d in u], w) for u, w in zip(unfiltered, want))
    single = nd.AprilTagNode(quad_sigma=0.8)
    multi = nd.AprilTagMultiCameraNode(2, quad_sigma=0.8)
    try:
        for i, buf in enumerate(bufs):
            dets, _ = single.on_frame(buf.ctypes.data, False, encoding, 1920, 1080, step, K9, "cam%d" % i, (3, i))
            assert _same_dets(dets, want[i]), (i, [d["id"] for d in dets])
        for i, buf in enumerate(bufs):
            assert multi.on_frame(i, buf.ctypes.data, False, encoding, 1920, 1080, step, K9, "cam%d" % i, (4, i))
        for i in range(2):
            assert multi.publishes(i) == 1
            dets, _, _ = multi.last(i)
            assert _same_dets(dets, want[i]), (i, [d["id"] for d in dets])
    finally:
        single.close(); multi.close()
    bad = nd.AprilTagNode(quad_sigma=4.5)
    try:
        with pytest.raises(RuntimeError):
            bad.on_frame(bufs[0].ctypes.data, False, encoding, 1920, 1080, step, K9)
    finally:
        bad.close()
