"""quad_sigma on the device (amdAprilTagsSetQuadSigma): the filtered working image equals the restatement (tests/quad_sigma_ref.py)
bit for bit, and every stage behind it equals the unchanged oracle run on the filtered frame -- at decimate 1 end to end, at
decimate > 1 through the quads (the oracle on J, the frame whose decimation is the filtered working image).  Each case runs on both
launch sets."""
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
        errs, odets = pu.compare_stages(det, 0, J, ("tag36h11",), K, decimate)
        assert not errs, (s, errs[:5])
        got = {int(d["id"]) for d in g}
        assert ids <= got and {int(d["id"]) for d in odets} <= got, (s, sorted(ids), sorted(got))
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
        errs, _ = pu.compare_stages(det, 0, qs.embed_decimated(gray, filt, decimate), ("tag36h11",), K, decimate, tile_size=tile)
    assert not errs, errs[:4]
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
