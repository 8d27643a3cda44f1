"""Resize inside the submission (amdAprilTagsSetResize, k_resize_frames), fused with the rectification.  The definition under test
(DESIGN.md section 7c): the resized plane S of every frame equals the oracle's resize_mono8(G) byte for byte -- G the frame's gray plane
at its source size, convert(frame) or rectify(convert(frame)) -- and the frame's stage buffers and records are those of the same handle
given S as a mono8 frame, whatever the encoding, base address, pitch, source size, batch slot and launch set.  The oracle-side
preconditions (ten detections per target and setting, records that differ with and without rectification, 58 records in the batch, the
identity property) are asserted in tests/test_resize_cpu.py."""
import ctypes as C
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
import rectify_cases as rc  # noqa: E402
import resize_cases as zc  # noqa: E402

PATHS = ("latency", "throughput")
ENCODINGS = ("mono8", "rgb8", "bgr8", "rgba8", "bgra8")
INVALID_ARGUMENT, SIZE_MISMATCH = 1, 4
_cache = {}


def _code(fn):
    with pytest.raises(capi.AprilTagsError) as e:
        fn()
    return e.value.code


def _device_frame(arr, pad=0, offset=0):
    """arr ([H, W] or [H, W, C] uint8) in device memory with `pad` bytes behind every row and the first pixel `offset` bytes into the
    allocation: (tensor to keep alive, (dev_ptr, pitch, width, height))."""
    h, w = arr.shape[:2]
    row = w * (arr.shape[2] if arr.ndim == 3 else 1)
    pitch = row + pad
    buf = np.full(offset + pitch * h, 0xA5, dtype=np.uint8)   # (padding that is not 0: a tap read from it would show)
    buf[offset:].reshape(h, pitch)[:, :row] = arr.reshape(h, row)
    t = torch.from_numpy(buf).cuda()
    return t, (t.data_ptr() + offset, pitch, w, h)


# ---- 1. plane bytes ---------------------------------------------------------------------------------------------------------------------
# (source content, target, the handle): see the table in the docstring of test_plane_bytes
PLANE_CASES = (("noise301", (211, 157), "sized"), ("noise301", (301, 203), "sized"), ("noise301", (452, 305), "sized"),
               ("noise301", (75, 51), "sized"), ("noise1303", (640, 480), "fixed"), ("1x1", (8, 4), "sized"), ("2x3", (8, 4), "sized"))
_SHAPES = {"noise301": (203, 301), "noise1303": (907, 1303), "1x1": (1, 1), "2x3": (3, 2)}


def _plane_rgb(name):
    """[H, W, 3] RGB noise of the plane-byte cases."""
    if name not in _cache:
        h, w = _SHAPES[name]
        _cache[name] = np.random.default_rng(w * 1000 + h).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    return _cache[name]


def _gray_planes(name):
    """label -> (model or None, G) of a plane-byte case: rectification off, model_a, model_z and the identity model, scaled to the source
    size (the oracle's rectify_mono8 of the BT.601 gray)."""
    if ("G", name) not in _cache:
        rgb = _plane_rgb(name)
        h, w = rgb.shape[:2]
        gray = rc.bt601(rgb)
        out = {"off": (None, gray)}
        for label, model in (("Da", rc.model_a(w, h)), ("Dz", rc.model_z(w, h)), ("identity", rc.model_identity(w, h))):
            out[label] = (model, po.rectify_mono8(gray, *model))
        assert np.array_equal(out["identity"][1], gray)
        _cache[("G", name)] = out
    return _cache[("G", name)]


@pytest.fixture(scope="module")
def plane_handles(built):
    dets = {"sized": AprilTagDetector(640, 480, max_batch=1, per_frame_sizes=True), "fixed": AprilTagDetector(640, 480, max_batch=1)}
    yield dets
    [d.close() for d in dets.values()]


@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("name,target,handle", PLANE_CASES, ids=["%s-%dx%d" % (c[0], c[1][0], c[1][1]) for c in PLANE_CASES])
def test_plane_bytes(plane_handles, name, target, handle, encoding):
    """AMDAT_DBG_RESIZED == the oracle's resize_mono8(G), with rectification off and with Da, Dz and the identity model:
      301 x 203 -> 211 x 157 (a dword tail of 3), -> 301 x 203 (the identity: S == G), -> 452 x 305 (upscale), -> 75 x 51;
      1303 x 907 -> 640 x 480, a source larger than the handle, on a handle without per-frame sizes;
      1 x 1 and 2 x 3 -> 8 x 4: every clamp of the statement.
    The 301-wide frame sits at pitch 301 * channels + 16, 3 bytes into its allocation, padding 0xA5."""
    det = plane_handles[handle]
    dw, dh = target
    keep, frame = _device_frame(rc.encode(_plane_rgb(name), encoding), *((16, 3) if name == "noise301" else (0, 0)))
    if name == "noise301":
        assert frame[1] == 301 * capi.ENC_CHANNELS[encoding] + 16 and (frame[0] - keep.data_ptr()) == 3
    det.set_resize([target])
    bad = []
    for label, (model, G) in _gray_planes(name).items():
        det.set_rectification([model] if model else None)
        det.detect_batch_ex([frame], max_dets=64, intrinsics=[(100.0, 100.0, dw / 2.0, dh / 2.0)], encoding=encoding)
        plane = det.debug(0, capi.DBG_RESIZED).reshape(dh, dw)
        want = po.resize_mono8(G, dw, dh)
        ndiff = int((plane != want).sum())
        print("%s -> %dx%d %s %s: %d of %d bytes differ" % (name, dw, dh, encoding, label, ndiff, dw * dh))
        if ndiff:
            bad.append((label, ndiff))
        if (dh, dw) == G.shape:
            assert np.array_equal(want, G)   # the identity: S == G
        if model:
            assert _code(lambda: det.debug(0, capi.DBG_RECTIFIED)) == INVALID_ARGUMENT   # (that plane is never formed)
    del keep
    assert not bad, bad


# ---- 2. records ---------------------------------------------------------------------------------------------------------------------------
def _scene_tensor():
    if "scene_t" not in _cache:
        _cache["scene_t"] = torch.from_numpy(rc.scene()[0]).cuda()
    return _cache["scene_t"]


@pytest.mark.parametrize("setting", rc.SETTINGS, ids=lambda s: "d%d-t%d-qs%g" % s)
def test_records_rectified(built, setting):
    """scene_c2 (1920 x 1080) with Da, Knew_a on a 1280 x 720 handle: exactly the oracle's ten records on resize(rectify(frame))."""
    decimate, tile, sigma = setting
    K, D, Kn = rc.model_a()
    det = AprilTagDetector(1280, 720, decimate=decimate, tile_size=tile, quad_sigma=sigma, rectification=[(K, D, Kn)], resize=[(1280, 720)])
    g = det.detect_batch_ex(_scene_tensor(), max_dets=64, intrinsics=[rc.k4(zc.scaled_k(Kn, 1920, 1080, 1280, 720))])[0]
    want = zc.oracle_detections(1280, 720, setting, "a")
    errs = pu.compare_detections(g, want, exact=True)
    plane_ok = np.array_equal(det.debug(0, capi.DBG_RESIZED).reshape(720, 1280), zc.resized(1280, 720, "a"))
    det.close()
    assert len(want) == 10 and len(g) == 10 and not errs, (len(g), errs[:4])
    assert plane_ok


@pytest.mark.parametrize("decimate", (1, 2))
def test_records_odd_target(built, decimate):
    """Without rectification, a 1437 x 811 handle (a ratio that is no fraction of small integers; odd sizes): the oracle's ten records."""
    det = AprilTagDetector(1437, 811, decimate=decimate, resize=[(1437, 811)])
    g = det.detect_batch_ex(_scene_tensor(), max_dets=64, intrinsics=[rc.k4(zc.scaled_k(rc.scene()[1], 1920, 1080, 1437, 811))])[0]
    want = zc.oracle_detections(1437, 811, (decimate, 4, 0.0))
    errs = pu.compare_detections(g, want, exact=True)
    plane_ok = np.array_equal(det.debug(0, capi.DBG_RESIZED).reshape(811, 1437), zc.resized(1437, 811))
    det.close()
    assert len(want) == 10 and len(g) == 10 and not errs, (len(g), errs[:4])
    assert plane_ok


# ---- 3. stage dumps -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
def test_stage_dumps(built, path):
    """Threshold through quads of the resized rectified frame on each launch set: the oracle's on S."""
    K, D, Kn = rc.model_a()
    Ks = zc.scaled_k(Kn, 1920, 1080, 1280, 720)
    det = AprilTagDetector(1280, 720, rectification=[(K, D, Kn)], resize=[(1280, 720)])
    det.set_submission_path(path)
    g = det.detect_batch_ex(_scene_tensor(), max_dets=64, intrinsics=[rc.k4(Ks)])[0]
    assert det.last_submission_path() == path
    errs, odets = pu.compare_stages(det, 0, zc.resized(1280, 720, "a"), rc.FAM, Ks)
    errs += pu.compare_detections(g, odets, exact=True)
    det.close()
    assert len(odets) == 10 and not errs, errs[:6]


# ---- 4. batch plumbing --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("norect", "rect"))
@pytest.mark.parametrize("how", ("graph", "plain"))
def test_batch_plumbing(built, how, mode):
    """SubmitBatchColor / WaitBatchEx on a 1280 x 720 handle with per-frame sizes, decimate 2: eight bgr8 frames of three source sizes
    (full frames, crops in buffers of their own, a window at the full image's pitch), sizes = [(1280, 720), (1000, 600)], slot i with
    size i % 2 and camera kind i % 3 scaled to its source size.  Replayed from a captured graph and as plain enqueues, every slot's
    plane and records equal the oracle's -- the identity slots 3 and 4 and the anisotropic 1920 x 1080 -> 1000 x 600 among them."""
    frames, want = zc.batch_frames(), zc.batch_case(mode == "rect")
    assert sum(len(w[3]) for w in want) == 58   # (equality is not equality of empty lists)
    full = torch.from_numpy(frames[0]).cuda()
    crops = {1: torch.from_numpy(np.ascontiguousarray(frames[1])).cuda(), 4: torch.from_numpy(np.ascontiguousarray(frames[4])).cuda()}
    imgs = []
    for i in range(8):
        if i in crops:
            imgs.append((crops[i].data_ptr(), 1280 * 3, 1280, 720))
        elif i == 3:
            imgs.append((full.data_ptr() + (13 * 1920 + 389) * 3, 1920 * 3, 1000, 600))
        else:
            imgs.append((full.data_ptr(), 1920 * 3, 1920, 1080))
    det = AprilTagDetector(1280, 720, decimate=zc.BATCH_DECIMATE, max_batch=8, per_frame_sizes=True, resize=list(zc.BATCH_SIZES),
                           rectification=[w[0] for w in want] if mode == "rect" else None)
    det.set_submission_path("latency" if how == "graph" else "throughput")
    prep = det.prepare(imgs, max_dets=64, intrinsics=[w[1] for w in want], encoding="bgr8")
    for _ in range(2 if how == "graph" else 1):   # (graph: captured by the first submission, replayed by the second)
        det.submit_prepared(prep)
        det.wait_prepared(prep)
    capturing, live, retired = det.graph_replay()
    assert (live == 1 and capturing) if how == "graph" else live == 0, (capturing, live, retired)
    got = det.unpack(prep)
    errs = []
    for i in range(8):
        _, _, S, odets = want[i]
        plane = det.debug(i, capi.DBG_RESIZED)
        if plane.size != S.size:
            errs.append("slot %d: a plane of %d bytes, the oracle's has %d: they differ" % (i, plane.size, S.size))
        elif not np.array_equal(plane.reshape(S.shape), S):
            errs.append("slot %d: %d bytes of the resized plane differ" % (i, int((plane.reshape(S.shape) != S).sum())))
        errs += ["slot %d: %s" % (i, e) for e in pu.compare_detections(got[i], odets, exact=True)]
    det.close()
    print("\n".join(errs[:8]))
    assert not errs, errs[:6]


# ---- 5. the same as the three-step form ---------------------------------------------------------------------------------------------------
def test_equals_the_three_step_form(built):
    """amdAprilTagsRectifyMono8, then amdAprilTagsResizeMono8, into host-owned buffers, then DetectBatchEx on a plain 1280 x 720 handle:
    the same records and the same plane."""
    L = capi.lib()
    K, D, Kn = rc.model_a()
    Ks = rc.k4(zc.scaled_k(Kn, 1920, 1080, 1280, 720))
    src = _scene_tensor()
    mid = torch.empty_like(src)
    dst = torch.empty((720, 1280), dtype=torch.uint8, device="cuda")
    k, d5, kn = (C.c_double * 9)(*K.reshape(-1)), (C.c_double * 5)(*D), (C.c_double * 9)(*Kn.reshape(-1))
    assert L.amdAprilTagsRectifyMono8(src.data_ptr(), 1920, mid.data_ptr(), 1920, 1920, 1080, k, d5, kn, None) == 0
    assert L.amdAprilTagsResizeMono8(mid.data_ptr(), 1920, 1920, 1080, dst.data_ptr(), 1280, 1280, 720, None) == 0
    plain = AprilTagDetector(1280, 720)
    three_step = plain.detect_batch_ex(dst, max_dets=64, intrinsics=[Ks])[0]
    plain.close()
    det = AprilTagDetector(1280, 720, rectification=[(K, D, Kn)], resize=[(1280, 720)])
    one_step = det.detect_batch_ex(src, max_dets=64, intrinsics=[Ks])[0]
    plane = det.debug(0, capi.DBG_RESIZED).reshape(720, 1280)
    det.close()
    assert len(three_step) == 10 and not pu.compare_detections(one_step, three_step, exact=True)
    assert np.array_equal(plane, dst.cpu().numpy())


# ---- 6. the setter's contract ---------------------------------------------------------------------------------------------------------------
def test_setter_contract(built):
    img = np.ascontiguousarray(synth.scene_c1()[0])   # 640 x 480
    t = torch.from_numpy(img).cuda()
    S320, S160 = po.resize_mono8(img, 320, 240), po.resize_mono8(img, 160, 120)
    small = torch.from_numpy(S320).cuda()
    K320 = rc.k4(synth.default_K(320, 240))
    det = AprilTagDetector(320, 240, max_batch=2, per_frame_sizes=True)
    L, h = capi.lib(), det._h
    src = [(t.data_ptr(), 640, 640, 480)]

    def plane(shape=(240, 320)):
        det.detect_batch_ex(src, max_dets=64, intrinsics=[K320])
        return det.debug(0, capi.DBG_RESIZED).reshape(shape)

    # off is the default: a frame larger than the handle is refused, and there is no resized plane
    assert _code(lambda: det.detect_batch_ex(src, max_dets=64)) == SIZE_MISMATCH
    off = det.detect_batch_ex(small, max_dets=64, intrinsics=[K320])[0]
    assert _code(lambda: det.debug(0, capi.DBG_RESIZED)) == INVALID_ARGUMENT
    det.set_resize([(320, 240)])
    assert np.array_equal(plane(), S320)
    on = det.detect_batch_ex(src, max_dets=64, intrinsics=[K320])[0]
    assert not pu.compare_detections(on, off, exact=True)
    # refused calls leave the previous sizes in force
    for bad in ([(0, 240)], [(320, 0)], [(321, 240)], [(320, 241)], [(320, 240), (0, 1)], [(320, 240)] * 3):   # (the last: 3 > max_batch 2)
        assert _code(lambda: det.set_resize(bad)) == INVALID_ARGUMENT
        assert np.array_equal(plane(), S320)
    assert L.amdAprilTagsSetResize(h, 1, None) == INVALID_ARGUMENT and L.amdAprilTagsSetResize(None, 0, None) == INVALID_ARGUMENT
    prep = det.prepare(src, max_dets=64, intrinsics=[K320])
    det.submit_prepared(prep)
    assert _code(lambda: det.set_resize([(160, 120)])) == INVALID_ARGUMENT   # between Submit and Wait
    assert _code(lambda: det.set_resize(None)) == INVALID_ARGUMENT
    det.wait_prepared(prep)
    assert np.array_equal(det.debug(0, capi.DBG_RESIZED).reshape(240, 320), S320)
    # changing only the sizes retires no graph (and the replayed graph uses the new ones); an on/off change does
    assert np.array_equal(plane(), S320)
    capturing, live, retired0 = det.graph_replay()
    assert capturing and live >= 1
    det.set_resize([(160, 120)])
    assert np.array_equal(plane((120, 160)), S160)
    det.set_resize([(160, 120), (320, 240)])   # two sizes: slot 0 still takes the first
    assert np.array_equal(plane((120, 160)), S160)
    assert det.graph_replay() == (True, live, retired0)
    # a target that breaks the per-frame rules, or a source beyond 16384: AMDAT_SIZE_MISMATCH at submit, the setting stays
    det.set_resize([(320, 3)])   # (the working image has no full threshold tile)
    assert _code(lambda: det.detect_batch_ex(src, max_dets=64)) == SIZE_MISMATCH
    det.set_resize([(320, 240)])
    assert _code(lambda: det.detect_batch_ex([(t.data_ptr(), 16385, 16385, 1)], max_dets=64)) == SIZE_MISMATCH
    assert _code(lambda: det.detect_batch_ex([(t.data_ptr(), 640, 640, 16385)], max_dets=64)) == SIZE_MISMATCH
    assert np.array_equal(plane(), S320)
    assert det.graph_replay() == (True, live, retired0)
    fixed = AprilTagDetector(320, 240)   # per-frame sizes off: the target is the handle's size or nothing
    fixed.set_resize([(160, 120)])
    assert _code(lambda: fixed.detect_batch_ex(src, max_dets=64)) == SIZE_MISMATCH
    fixed.set_resize([(320, 240)])
    fixed.detect_batch_ex(src, max_dets=64)
    assert np.array_equal(fixed.debug(0, capi.DBG_RESIZED).reshape(240, 320), S320)
    fixed.close()
    # with rectification on as well the rectified plane is never formed
    M = rc.model_a(640, 480)
    det.set_rectification([M])
    assert np.array_equal(plane(), po.resize_mono8(po.rectify_mono8(img, *M), 320, 240))
    assert _code(lambda: det.debug(0, capi.DBG_RECTIFIED)) == INVALID_ARGUMENT
    det.set_rectification(None)
    # ThresholdOnly never resizes
    assert np.array_equal(plane(), S320)
    det.threshold_only(small)
    assert _code(lambda: det.debug(0, capi.DBG_RESIZED)) == INVALID_ARGUMENT
    assert np.array_equal(det.debug(0, capi.DBG_GRAY).reshape(240, 320), S320)
    assert _code(lambda: det.threshold_only(src)) == SIZE_MISMATCH
    # off: the graphs captured with the resize launch are retired, and the handle is one that never had the setting
    capturing, live, retired0 = det.graph_replay()
    det.set_resize(None)
    capturing, live_off, retired1 = det.graph_replay()
    assert capturing and live_off == 0 and retired1 == retired0 + live
    again = det.detect_batch_ex(small, max_dets=64, intrinsics=[K320])[0]
    assert _code(lambda: det.debug(0, capi.DBG_RESIZED)) == INVALID_ARGUMENT
    errs = pu.compare_stages(det, 0, S320, rc.FAM, synth.default_K(320, 240))[0]
    assert not pu.compare_detections(again, off, exact=True) and not errs, errs[:4]
    det.set_resize([(320, 240)])   # and on again retires the graph captured while it was off
    assert det.graph_replay()[2] == retired1 + 1
    assert np.array_equal(plane(), S320)
    det.close()


# ---- 7. the node shell ----------------------------------------------------------------------------------------------------------------------
def _p12(Kn):
    return [Kn[0, 0], Kn[0, 1], Kn[0, 2], 0.0, Kn[1, 0], Kn[1, 1], Kn[1, 2], 0.0, 0.0, 0.0, 1.0, 0.0]


@pytest.mark.parametrize("rectify", (False, True), ids=("plain", "rectify"))
@pytest.mark.parametrize("backends", ("CUDA", "HIP"))   # cuAprilTags mode, and the VPI mode that passes the scaled skew
def test_node_shell(built, backends, rectify):
    """AprilTagNode and a two-stream AprilTagMultiCameraNode with resize = (1280, 720), fed the 1080p host frame, publish what nodes
    without it publish for the oracle's S and a CameraInfo whose k is the scaled camera (K, or Knew with rectify)."""
    from isaac_ros_apriltag_amd import build as b
    from isaac_ros_apriltag_amd import node
    b.build_node()
    img = rc.scene()[0]
    cams = []
    for which, M in (("a", rc.model_a()), ("z", rc.model_z())):
        Kp = (M[2] if rectify else M[0]).copy()
        Kp[0, 1] = 0.75   # a skew (rectify: in P only): the pose must take it, scaled, in VPI mode
        cam = {"D": M[1], "S": zc.resized(1280, 720, which if rectify else None),
               "Ks": [float(v) for v in zc.scaled_k(Kp, 1920, 1080, 1280, 720).reshape(-1)]}
        if rectify:
            cam["K"], cam["P"] = [float(v) for v in M[0].reshape(-1)], _p12(Kp)
        else:
            cam["K"] = [float(v) for v in Kp.reshape(-1)]
        cams.append(cam)
    if not rectify:
        cams[1]["K"][2] += 3.0   # (two streams with one image: cameras that differ)
        Kp = np.array(cams[1]["K"]).reshape(3, 3)
        cams[1]["Ks"] = [float(v) for v in zc.scaled_k(Kp, 1920, 1080, 1280, 720).reshape(-1)]

    def feed(n, cam, fused, stream=None, stamp=(3, 0)):
        if fused:
            args = (img.ctypes.data, False, "mono8", 1920, 1080, 1920, cam["K"], "cam", stamp)
            more = {"D": cam["D"], "distortion_model": "plumb_bob", "P12": cam["P"]} if rectify else {}
        else:
            args, more = (cam["S"].ctypes.data, False, "mono8", 1280, 720, 1280, cam["Ks"], "cam", stamp), {}
        return n.on_frame(*args, **more) if stream is None else n.on_frame(stream, *args, **more)

    nodes = []
    try:
        for cam in cams:
            a, p = node.AprilTagNode(backends=backends, rectify=rectify, resize=(1280, 720)), node.AprilTagNode(backends=backends)
            nodes += [a, p]
            got, want = feed(a, cam, True), feed(p, cam, False)
            assert len(want[0]) == 10 and got == want
        multi = node.AprilTagMultiCameraNode(2, backends=backends, rectify=rectify, resize=(1280, 720))
        plain = node.AprilTagMultiCameraNode(2, backends=backends)
        nodes += [multi, plain]
        for rnd in range(2):   # the second round with the streams' cameras swapped
            order = cams if rnd == 0 else cams[::-1]
            for s in range(2):
                assert feed(multi, order[s], True, s, (4 + rnd, s)) and feed(plain, order[s], False, s, (4 + rnd, s))
            for s in range(2):
                assert multi.publishes(s) == rnd + 1 == plain.publishes(s)
                assert len(plain.last(s)[0]) == 10 and multi.last(s) == plain.last(s)
        assert multi.last(0) != multi.last(1)
    finally:
        [n.close() for n in nodes]


# ---- 8. the suite bites ---------------------------------------------------------------------------------------------------------------------
_SELECT = "(test_plane_bytes and noise301 and (mono8 or bgr8)) or test_batch_plumbing"
_NOISE = ["test_plane_bytes[noise301-%s-%s]" % (t, e) for t in ("211x157", "452x305", "75x51") for e in ("mono8", "bgr8")]
_BATCH = ["test_batch_plumbing[%s-%s]" % (h, m) for h in ("graph", "plain") for m in ("norect", "rect")]
_WRONG_BUILDS = {
    # the position without the half-pixel term: every resized byte but the identity's (301 x 203 -> 301 x 203 stays the identity)
    11: {"must_fail": tuple(_NOISE), "must_pass": ()},
    # every slot with sizes[0]: one size per submission is unaffected, the odd slots of the batch are not
    12: {"must_fail": tuple(_BATCH), "must_pass": tuple(_NOISE)},
}


@pytest.mark.parametrize("mutant", sorted(_WRONG_BUILDS))
def test_the_resize_tests_fail_on_the_wrong_builds(built, mutant):
    """libapriltag_amd_mut11.so and _mut12.so (csrc/tools_hooks.h, AMDAT_MUTATE): a selection of this file, in a process of its own,
    must FAIL on the wrong build where its error lives, and all of it passes on the product library."""
    import subprocess
    from isaac_ros_apriltag_amd import build as bld
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.exists(bld.lib_mutant(mutant)):
        bld.build_mutants()
    spec = _WRONG_BUILDS[mutant]

    def run(lib):
        env = dict(os.environ)
        env.pop("AMDAT_LIB", None)
        if lib:
            env["AMDAT_LIB"] = lib
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-rA", "-p", "no:cacheprovider",
                              "-k", _SELECT], capture_output=True, text=True, timeout=600, cwd=root, env=env)
        ids = lambda word: sorted(l.split("::", 1)[1].split(" ")[0] for l in out.stdout.splitlines() if l.startswith(word + " ") and "::" in l)
        return out, ids("PASSED"), ids("FAILED")
    out, passed, failed = run("mut%d" % mutant)
    assert out.returncode == 1, (out.stdout[-1500:], out.stderr[-1500:])
    for want in spec["must_fail"]:
        assert want in failed, (want, failed, passed)
    for want in spec["must_pass"]:
        assert want in passed, (want, failed, passed)
    assert "differ" in out.stdout   # what differs: bytes of the resized plane
    if "ok" not in _cache:   # (the product run is the same for both wrong builds)
        _cache["ok"] = run(None)
    out_ok, passed_ok, failed_ok = _cache["ok"]
    assert out_ok.returncode == 0 and not failed_ok and sorted(passed_ok) == sorted(passed + failed), (out_ok.stdout[-1500:], failed_ok)
