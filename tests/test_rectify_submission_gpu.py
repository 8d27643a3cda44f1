"""Rectification inside the submission (amdAprilTagsSetRectification, k_rectify_frames).  The definition under test: the rectified plane
of every frame equals the oracle's rectify(convert(frame)) byte for byte, and the frame's stage buffers and records are those of the
same handle given that plane as a mono8 frame -- whatever the encoding, base address, pitch, batch slot, launch set and frame size.
The oracle-side preconditions (ten detections per setting, records that differ from the unrectified frame's, the zero-filled region)
are asserted in tests/test_rectify_cpu.py."""
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

PATHS = ("latency", "throughput")
ENCODINGS = ("mono8", "rgb8", "bgr8", "rgba8", "bgra8")
INVALID_ARGUMENT = 1
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
def _plane_rgb(name):
    """[H, W, 3] RGB content of the plane-byte cases."""
    if name not in _cache:
        if name == "noise301":   # 301 x 203: the vector store's tail (301 = 75 dwords + 1), the last-column clamp, a second block across x
            _cache[name] = np.random.default_rng(301).integers(0, 256, size=(203, 301, 3), dtype=np.uint8)
        elif name == "c1":
            g = synth.scene_c1()[0]
            _cache[name] = np.ascontiguousarray(np.stack([g, g // 2 + 40, 255 - g // 3], axis=-1))
        else:   # 8 x 4: two dwords a row, one threshold tile down
            _cache[name] = np.random.default_rng(84).integers(0, 256, size=(4, 8, 3), dtype=np.uint8)
    return _cache[name]


@pytest.fixture(scope="module")
def plane_handle(built):
    det = AprilTagDetector(640, 480, max_batch=1, per_frame_sizes=True)
    yield det
    det.close()


@pytest.mark.parametrize("encoding", ENCODINGS)
@pytest.mark.parametrize("name", ("noise301", "c1", "8x4"))
def test_plane_bytes(plane_handle, name, encoding):
    """AMDAT_DBG_RECTIFIED == the oracle's rectify_mono8(gray(frame)) for Da, Dz (scaled to the size) and the identity, for which the
    plane is the gray frame itself.  The 301-wide frame sits at pitch 301 * channels + 16 (317 for mono8), 3 bytes into its allocation."""
    det = plane_handle
    rgb = _plane_rgb(name)
    h, w = rgb.shape[:2]
    gray = rc.bt601(rgb)
    keep, frame = _device_frame(rc.encode(rgb, encoding), *((16, 3) if name == "noise301" else (0, 0)))
    if name == "noise301" and encoding == "mono8":
        assert frame[1] == 317 and frame[0] % 4 == 3
    for label, (K, D, Kn) in (("Da", rc.model_a(w, h)), ("Dz", rc.model_z(w, h)), ("identity", rc.model_identity(w, h))):
        det.set_rectification([(K, D, Kn)])
        det.detect_batch_ex([frame], max_dets=64, intrinsics=[rc.k4(Kn)], encoding=encoding)
        plane = det.debug(0, capi.DBG_RECTIFIED).reshape(h, w)
        want = po.rectify_mono8(gray, K, D, Kn)
        print("%s %s %s: %d of %d bytes differ" % (name, encoding, label, int((plane != want).sum()), w * h))
        assert np.array_equal(plane, want), (label, int((plane != want).sum()))
        if label == "identity":
            assert np.array_equal(plane, gray)
        elif name != "8x4":
            assert not np.array_equal(plane, gray)
        if label == "Dz" and name != "8x4":
            assert (want[0, :] == 0).all() and (want[:, -1] == 0).all() and (want[h // 2] != 0).any()   # the zero-filled border exists
    del keep


# ---- 2. records ---------------------------------------------------------------------------------------------------------------------------
def _scene_tensor():
    if "scene_t" not in _cache:
        _cache["scene_t"] = torch.from_numpy(rc.scene()[0]).cuda()
    return _cache["scene_t"]


@pytest.mark.parametrize("setting", rc.SETTINGS, ids=lambda s: "d%d-t%d-qs%g" % s)
def test_records(built, setting):
    """scene_c2 with Da, Knew_a: exactly the oracle's ten records on the rectified frame."""
    decimate, tile, sigma = setting
    K, D, Kn = rc.model_a()
    det = AprilTagDetector(1920, 1080, decimate=decimate, tile_size=tile, quad_sigma=sigma, rectification=[(K, D, Kn)])
    g = det.detect_batch_ex(_scene_tensor(), max_dets=64, intrinsics=[rc.k4(Kn)])[0]
    want = rc.oracle_detections("a", setting)
    errs = pu.compare_detections(g, want, exact=True)
    plane_ok = np.array_equal(det.debug(0, capi.DBG_RECTIFIED).reshape(1080, 1920), rc.rectified("a"))
    det.close()
    assert len(want) == 10 and len(g) == 10 and not errs, (len(g), errs[:4])
    assert plane_ok


@pytest.mark.parametrize("path", PATHS)
def test_stage_dumps(built, path):
    """Threshold through quads of the rectified frame on each launch set: the oracle's on the rectified frame."""
    K, D, Kn = rc.model_a()
    det = AprilTagDetector(1920, 1080, rectification=[(K, D, Kn)])
    det.set_submission_path(path)
    g = det.detect_batch_ex(_scene_tensor(), max_dets=64, intrinsics=[rc.k4(Kn)])[0]
    assert det.last_submission_path() == path
    errs, odets = pu.compare_stages(det, 0, rc.rectified("a"), rc.FAM, Kn)
    errs += pu.compare_detections(g, odets, exact=True)
    det.close()
    assert len(odets) == 10 and not errs, errs[:6]


# ---- 3. batch plumbing --------------------------------------------------------------------------------------------------------------------
def _batch_case():
    """Eight bgr8 frames for a 1920 x 1080 handle with per-frame sizes: five full frames, two 1280 x 720 crops in buffers of their own, one
    1000 x 600 window at (389, 13) addressed inside the full image with that image's pitch.  Three camera models; slot i takes model
    i % 3.  Returns (frames as host arrays [H, W, 3] BGR, models, per slot: (rectified plane, oracle records at decimate 2))."""
    if "batch" not in _cache:
        g = rc.scene()[0]
        bgr = np.ascontiguousarray(np.stack([g // 2 + 40, g, g], axis=-1))   # B, G, R
        crop_a, crop_b, window = bgr[:720, :1280], bgr[360:, 640:], bgr[13:613, 389:1389]
        frames = [bgr, crop_a, bgr, window, crop_b, bgr, bgr, bgr]
        K = rc.camera(1920, 1080)
        models = [rc.model_a(), rc.model_z(), (K, [0.03, 0.0, 0.001, 0.0, 0.0], rc.knew_a(1920, 1080))]
        want, memo = [], {}
        for i, f in enumerate(frames):
            key = (id(f), i % 3)
            if key not in memo:
                Km, Dm, Kn = models[i % 3]
                R = po.rectify_mono8(rc.bt601(f[..., ::-1]), Km, Dm, Kn)
                memo[key] = (R, po.detect(R, families=rc.FAM, params=pu.oracle_params(Kn, 2))[0])
            want.append(memo[key])
        _cache["batch"] = (frames, models, want)
    return _cache["batch"]


@pytest.mark.parametrize("how", ("graph", "plain"))
def test_batch_plumbing(built, how):
    """SubmitBatchColor / WaitBatchEx with ncams = 3 and per-frame sizes, replayed from a captured graph and as plain enqueues: every frame
    equals the oracle on its own rectify(convert(frame)) with model i % 3."""
    frames, models, want = _batch_case()
    assert sum(len(w[1]) for w in want) >= 30   # (equality is not equality of empty lists)
    full = torch.from_numpy(frames[0]).cuda()
    crops = {1: torch.from_numpy(np.ascontiguousarray(frames[1])).cuda(), 4: torch.from_numpy(np.ascontiguousarray(frames[4])).cuda()}
    imgs = []
    for i, f in enumerate(frames):
        if i in crops:
            imgs.append((crops[i].data_ptr(), 1280 * 3, 1280, 720))
        elif i == 3:
            imgs.append((full.data_ptr() + (13 * 1920 + 389) * 3, 1920 * 3, 1000, 600))
        else:
            imgs.append((full.data_ptr(), 1920 * 3, 1920, 1080))
    det = AprilTagDetector(1920, 1080, decimate=2, max_batch=8, per_frame_sizes=True, rectification=models)
    det.set_submission_path("latency" if how == "graph" else "throughput")
    prep = det.prepare(imgs, max_dets=64, intrinsics=[rc.k4(models[i % 3][2]) for i in range(8)], encoding="bgr8")
    for _ in range(2 if how == "graph" else 1):   # (graph: captured by the first submission, replayed by the second)
        det.submit_prepared(prep)
        det.wait_prepared(prep)
    capturing, live, retired = det.graph_replay()
    assert (live == 1 and capturing) if how == "graph" else live == 0, (capturing, live, retired)
    got = det.unpack(prep)
    errs = []
    for i in range(8):
        R, odets = want[i]
        plane = det.debug(i, capi.DBG_RECTIFIED).reshape(R.shape)
        if not np.array_equal(plane, R):
            errs.append("slot %d: %d bytes of the rectified plane differ" % (i, int((plane != R).sum())))
        errs += ["slot %d: %s" % (i, e) for e in pu.compare_detections(got[i], odets, exact=True)]
    det.close()
    assert not errs, errs[:6]


# ---- 4. the same as the two-step form -----------------------------------------------------------------------------------------------------
def test_equals_the_two_step_form(built):
    """amdAprilTagsRectifyMono8 into a host-owned buffer, then DetectBatchEx on a handle without rectification: the same records."""
    L = capi.lib()
    K, D, Kn = rc.model_a()
    src = _scene_tensor()
    dst = torch.empty_like(src)
    k, d5, kn = (C.c_double * 9)(*K.reshape(-1)), (C.c_double * 5)(*D), (C.c_double * 9)(*Kn.reshape(-1))
    assert L.amdAprilTagsRectifyMono8(src.data_ptr(), 1920, dst.data_ptr(), 1920, 1920, 1080, k, d5, kn, None) == 0
    plain = AprilTagDetector(1920, 1080)
    two_step = plain.detect_batch_ex(dst, max_dets=64, intrinsics=[rc.k4(Kn)])[0]
    plain.close()
    det = AprilTagDetector(1920, 1080, rectification=[(K, D, Kn)])
    one_step = det.detect_batch_ex(src, max_dets=64, intrinsics=[rc.k4(Kn)])[0]
    plane = det.debug(0, capi.DBG_RECTIFIED).reshape(1080, 1920)
    det.close()
    assert len(two_step) == 10 and not pu.compare_detections(one_step, two_step, exact=True)
    assert np.array_equal(plane, dst.cpu().numpy())


# ---- 5. the setter's contract ---------------------------------------------------------------------------------------------------------------
def test_setter_contract(built):
    img, _, _ = synth.scene_c1()
    img = np.ascontiguousarray(img)
    t = torch.from_numpy(img).cuda()
    Ma, Mz = rc.model_a(640, 480), rc.model_z(640, 480)
    Ra, Rz = po.rectify_mono8(img, *Ma), po.rectify_mono8(img, *Mz)
    assert not np.array_equal(Ra, Rz)
    det = AprilTagDetector(640, 480, max_batch=2)
    L, h = capi.lib(), det._h

    def plane():
        det.detect_batch_ex(t, max_dets=64, intrinsics=[rc.k4(Ma[2])])
        return det.debug(0, capi.DBG_RECTIFIED).reshape(480, 640)

    # off is the default: no rectified plane
    off = det.detect_batch_ex(t, max_dets=64)[0]
    assert len(off) == 1 and _code(lambda: det.debug(0, capi.DBG_RECTIFIED)) == INVALID_ARGUMENT
    det.set_rectification([Ma])
    assert np.array_equal(plane(), Ra)
    # refused calls leave the previous models in force
    nan_d = (Mz[0], [0.12, float("nan"), 0, 0, 0], Mz[2])
    zero_fx = (Mz[0], Mz[1], np.array([[0.0, 0, 320.0], [0, 800.0, 240.0], [0, 0, 1]]))
    zero_fy = (Mz[0], Mz[1], np.array([[800.0, 0, 320.0], [0, 0.0, 240.0], [0, 0, 1]]))
    inf_k = (np.array([[float("inf"), 0, 320.0], [0, 333.0, 240.0], [0, 0, 1]]), Mz[1], Mz[2])
    for bad in ([nan_d], [zero_fx], [zero_fy], [inf_k], [Ma, nan_d], [Mz, Mz, Mz]):   # (the last: ncams 3 > max_batch 2)
        assert _code(lambda: det.set_rectification(bad)) == INVALID_ARGUMENT
        assert np.array_equal(plane(), Ra)
    assert L.amdAprilTagsSetRectification(h, 1, None) == INVALID_ARGUMENT and L.amdAprilTagsSetRectification(None, 0, None) == INVALID_ARGUMENT
    prep = det.prepare(t, max_dets=64, intrinsics=[rc.k4(Ma[2])])
    det.submit_prepared(prep)
    assert _code(lambda: det.set_rectification([Mz])) == INVALID_ARGUMENT   # between Submit and Wait
    assert _code(lambda: det.set_rectification(None)) == INVALID_ARGUMENT
    det.wait_prepared(prep)
    assert np.array_equal(det.debug(0, capi.DBG_RECTIFIED).reshape(480, 640), Ra)
    assert np.array_equal(plane(), Ra)
    # changing only the models retires no graph (and the replayed graph uses the new ones); an on/off change does
    capturing, live, retired0 = det.graph_replay()
    assert capturing and live >= 1
    det.set_rectification([Mz])
    assert np.array_equal(plane(), Rz)
    det.set_rectification([Mz, Ma])   # two cameras: slot 0 still takes the first
    assert np.array_equal(plane(), Rz)
    assert det.graph_replay() == (True, live, retired0)
    det.set_rectification(None)
    capturing, live_off, retired1 = det.graph_replay()
    assert capturing and live_off == 0 and retired1 == retired0 + live
    # ncams = 0: a handle that never had the setting
    again = det.detect_batch_ex(t, max_dets=64)[0]
    assert _code(lambda: det.debug(0, capi.DBG_RECTIFIED)) == INVALID_ARGUMENT
    fresh = AprilTagDetector(640, 480, max_batch=2)
    never = fresh.detect_batch_ex(t, max_dets=64)[0]
    errs = pu.compare_stages(det, 0, img, rc.FAM, synth.default_K(640, 480))[0]
    fresh.close()
    assert len(never) == 1 and not pu.compare_detections(again, never, exact=True) and not pu.compare_detections(off, never, exact=True)
    assert not errs, errs[:4]
    det.set_rectification([Ma])   # and on again retires the graph captured while it was off
    assert det.graph_replay()[2] == retired1 + 1
    assert np.array_equal(plane(), Ra)
    # ThresholdOnly never rectifies
    det.threshold_only(t)
    assert _code(lambda: det.debug(0, capi.DBG_RECTIFIED)) == INVALID_ARGUMENT
    assert np.array_equal(det.debug(0, capi.DBG_GRAY).reshape(480, 640), img)
    det.close()


# ---- 6. the node shell ----------------------------------------------------------------------------------------------------------------------
def _p12(Kn):
    return [Kn[0, 0], Kn[0, 1], Kn[0, 2], 0.0, Kn[1, 0], Kn[1, 1], Kn[1, 2], 0.0, 0.0, 0.0, 1.0, 0.0]


@pytest.mark.parametrize("backends", ("CUDA", "HIP"))   # cuAprilTags mode, and the VPI mode that passes Knew[0][1] as the skew
def test_node_shell(built, backends):
    """AprilTagNode and a two-stream AprilTagMultiCameraNode with rectify = true, fed the distorted host frames, publish what nodes with
    rectify = false publish for the oracle-rectified frames and a CameraInfo whose k is Knew."""
    from isaac_ros_apriltag_amd import build as b
    from isaac_ros_apriltag_amd import node
    b.build_node()
    img = rc.scene()[0]
    cams = []
    for which, M in (("a", rc.model_a()), ("z", rc.model_z())):
        Kn = M[2].copy()
        Kn[0, 1] = 0.75   # a skew in P only: the pose must take it in VPI mode, and the rectification must not
        cams.append({"K": [float(v) for v in M[0].reshape(-1)], "D": M[1], "P": _p12(Kn), "Knew": [float(v) for v in Kn.reshape(-1)],
                     "R": rc.rectified(which)})

    def feed(n, cam, rect, stream=None, stamp=(3, 0)):
        frame = img if rect else cam["R"]
        args = (frame.ctypes.data, False, "mono8", 1920, 1080, 1920, cam["K"] if rect else cam["Knew"], "cam", stamp)
        more = {"D": cam["D"], "distortion_model": "plumb_bob", "P12": cam["P"]} if rect else {}
        return n.on_frame(*args, **more) if stream is None else n.on_frame(stream, *args, **more)

    nodes = []
    try:
        for cam in cams:
            a, p = node.AprilTagNode(backends=backends, rectify=True), node.AprilTagNode(backends=backends)
            nodes += [a, p]
            got, want = feed(a, cam, True), feed(p, cam, False)
            assert len(want[0]) == 10 and got == want
        multi, plain = node.AprilTagMultiCameraNode(2, backends=backends, rectify=True), node.AprilTagMultiCameraNode(2, backends=backends)
        nodes += [multi, plain]
        for rnd in range(2):   # the second round with the streams' cameras swapped: the models follow the streams, round by round
            order = cams if rnd == 0 else cams[::-1]
            for s in range(2):
                assert feed(multi, order[s], True, s, (4 + rnd, s)) and feed(plain, order[s], False, s, (4 + rnd, s))
            for s in range(2):
                assert multi.publishes(s) == rnd + 1 == plain.publishes(s)
                assert len(plain.last(s)[0]) == 10 and multi.last(s) == plain.last(s)
        assert multi.last(0) != multi.last(1)
        # a model the shell does not rectify throws with a clear text, before anything is staged
        with pytest.raises(RuntimeError, match="plumb_bob"):
            multi.on_frame(0, img.ctypes.data, False, "mono8", 1920, 1080, 1920, cams[0]["K"], "cam", (9, 0), D=[0.1] * 4, distortion_model="equidistant")
        fresh = node.AprilTagNode(backends=backends, rectify=True)
        nodes.append(fresh)
        with pytest.raises(RuntimeError, match="plumb_bob"):
            fresh.on_frame(img.ctypes.data, False, "mono8", 1920, 1080, 1920, cams[0]["K"], "cam", (9, 0), D=[0.1] * 4, distortion_model="equidistant")
    finally:
        [n.close() for n in nodes]


# ---- 7. the suite bites ---------------------------------------------------------------------------------------------------------------------
_SELECT = "(test_plane_bytes and noise301 and (mono8 or bgr8)) or test_batch_plumbing"
_WRONG_BUILDS = {
    # the fixed-point source position truncated: every rectified byte whose position has a fraction of a half or more
    9: {"must_fail": ("test_plane_bytes[noise301-mono8]", "test_plane_bytes[noise301-bgr8]"), "must_pass": ()},
    # every frame with cams[0]: one camera per submission is unaffected, slots 1, 2, 4, 5, 7 of the batch are not
    10: {"must_fail": ("test_batch_plumbing[graph]", "test_batch_plumbing[plain]"),
         "must_pass": ("test_plane_bytes[noise301-mono8]", "test_plane_bytes[noise301-bgr8]")},
}


@pytest.mark.parametrize("mutant", sorted(_WRONG_BUILDS))
def test_the_rectify_tests_fail_on_the_wrong_builds(built, mutant):
    """libapriltag_amd_mut9.so and _mut10.so (csrc/tools_hooks.h, AMDAT_MUTATE): a selection of this file, in a process of its own,
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
    assert "differ" in out.stdout   # what differs: bytes of the rectified plane
    if "ok" not in _cache:   # (the product run is the same for both wrong builds)
        _cache["ok"] = run(None)
    out_ok, passed_ok, failed_ok = _cache["ok"]
    assert out_ok.returncode == 0 and not failed_ok and sorted(passed_ok) == sorted(passed + failed), (out_ok.stdout[-1500:], failed_ok)
