"""Rectification of rational_polynomial, equidistant and rotated (stereo-R) cameras inside the submission
(amdAprilTagsSetRectificationEx, k_rectify_frames_general / k_resize_frames_general, amdAprilTagsRectifyMono8Ex).  The definition under
test: the rectified plane of every frame equals tests/camera_models_ref.py's rectify(convert(frame)) under the slot's own camera, byte
for byte, and the records are the oracle's on that plane.  Where the new path overlaps the old one (plumb_bob, R = I) it equals the
oracle's ato_rectify_mono8 and the old call.  The reference's own preconditions are asserted in tests/test_camera_models_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from isaac_ros_apriltag_amd import capi  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
import camera_models_ref as cm  # noqa: E402
import parity_util as pu  # noqa: E402
import rectify_cases as rc  # noqa: E402

INVALID_ARGUMENT = 1
W, H = 301, 203
_cache = {}


def _code(fn):
    with pytest.raises(capi.AprilTagsError) as e:
        fn()
    return e.value.code


def _device_frame(arr, pad=0, offset=0):
    """arr ([H, W] or [H, W, C] uint8) in device memory with `pad` bytes (0xA5) behind every row and the first pixel `offset` bytes into
    the allocation: (tensor to keep alive, (dev_ptr, pitch, width, height))."""
    h, w = arr.shape[:2]
    row = w * (arr.shape[2] if arr.ndim == 3 else 1)
    pitch = row + pad
    buf = np.full(offset + pitch * h, 0xA5, dtype=np.uint8)
    buf[offset:].reshape(h, pitch)[:, :row] = arr.reshape(h, row)
    t = torch.from_numpy(buf).cuda()
    return t, (t.data_ptr() + offset, pitch, w, h)


def _want(name, cam):
    """The reference's plane of the noise image `name` under camera `cam` (scaled to the image), computed once."""
    key = ("want", name, cam)
    if key not in _cache:
        gray = rc.bt601(cm.noise(name))
        _cache[key] = cm.rectify(gray, *cm.cameras(gray.shape[1], gray.shape[0])[cam])
    return _cache[key]


@pytest.fixture(scope="module")
def plane_handle(built):
    det = AprilTagDetector(640, 480, max_batch=1, per_frame_sizes=True)
    yield det
    det.close()


# ---- 1. plane bytes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", cm.CAMERA_NAMES)
@pytest.mark.parametrize("encoding", ("mono8", "bgr8"))
@pytest.mark.parametrize("name", ("noise301", "8x4"))
def test_plane_bytes(plane_handle, name, encoding, cam):
    """AMDAT_DBG_RECTIFIED == the reference.  301 x 203: the store's tail, the clamp, a second block across x, at pitch + 16 and
    base + 3; 8 x 4: two dwords a row."""
    det = plane_handle
    rgb = cm.noise(name)
    h, w = rgb.shape[:2]
    K, D, Kn, kind, R = cm.cameras(w, h)[cam]
    keep, frame = _device_frame(rc.encode(rgb, encoding), *((16, 3) if name == "noise301" else (0, 0)))
    det.set_rectification([(K, D, Kn, kind, R)])
    det.detect_batch_ex([frame], max_dets=64, intrinsics=[rc.k4(Kn)], encoding=encoding)
    plane = det.debug(0, capi.DBG_RECTIFIED).reshape(h, w)
    want = _want(name, cam)
    print("%s %s %s: %d of %d bytes differ" % (name, encoding, cam, int((plane != want).sum()), w * h))
    assert np.array_equal(plane, want), int((plane != want).sum())
    if cam == "plumb_bob":   # the Ex call with plumb_bob, R = I: the oracle's plane and the old call's
        assert np.array_equal(plane, po.rectify_mono8(rc.bt601(rgb), K, D, Kn))
        det.set_rectification([(K, D, Kn)])
        det.detect_batch_ex([frame], max_dets=64, intrinsics=[rc.k4(Kn)], encoding=encoding)
        assert np.array_equal(det.debug(0, capi.DBG_RECTIFIED).reshape(h, w), plane)
    del keep


# ---- 2. the stand-alone call -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", cm.CAMERA_NAMES)
def test_stand_alone_call(built, cam):
    L = capi.lib()
    gray = rc.bt601(cm.noise("noise301"))
    keep, (ptr, pitch, w, h) = _device_frame(gray, 16, 3)
    dst = torch.full((h, 320), 0x5A, dtype=torch.uint8, device="cuda")
    model = capi.camera_model_ex(*cm.cameras(w, h)[cam])
    assert L.amdAprilTagsRectifyMono8Ex(ptr, pitch, dst.data_ptr(), 320, w, h, C.byref(model), None) == 0
    out = dst.cpu().numpy()
    assert np.array_equal(out[:, :w], _want("noise301", cam)) and (out[:, w:] == 0x5A).all()
    model.kind = 3
    assert L.amdAprilTagsRectifyMono8Ex(ptr, pitch, dst.data_ptr(), 320, w, h, C.byref(model), None) == INVALID_ARGUMENT
    assert L.amdAprilTagsRectifyMono8Ex(ptr, pitch, dst.data_ptr(), 320, w, h, None, None) == INVALID_ARGUMENT
    del keep


# ---- 3. a mixed submission ---------------------------------------------------------------------------------------------------------------
_MIXED = ("plumb_bob", "rational+R", "equidistant", "plumb_bob+R", "rational", "equidistant+R")


@pytest.mark.parametrize("how", ("graph", "plain"))
def test_mixed_submission(built, how):
    """Six 301 x 203 slots, six cameras of all kinds in one submission: every slot's plane is its own camera's; then three cameras
    for six slots (slot i takes camera i % 3)."""
    cams = cm.cameras(W, H)
    gray = rc.bt601(cm.noise("noise301"))
    keep, frame = _device_frame(gray, 16, 3)
    det = AprilTagDetector(640, 480, max_batch=8, per_frame_sizes=True)
    det.set_submission_path("latency" if how == "graph" else "throughput")
    errs = []
    for names in (_MIXED, _MIXED[:3]):
        det.set_rectification([cams[n] for n in names])
        prep = det.prepare([frame] * 6, max_dets=64, intrinsics=[rc.k4(cams[names[i % len(names)]][2]) for i in range(6)])
        for _ in range(2 if how == "graph" else 1):   # (graph: captured by the first submission, replayed by the second)
            det.submit_prepared(prep)
            det.wait_prepared(prep)
        capturing, live, retired = det.graph_replay()
        assert (live == 1 and capturing and retired == 0) if how == "graph" else live == 0, (capturing, live, retired)
        for i in range(6):
            plane = det.debug(i, capi.DBG_RECTIFIED).reshape(H, W)
            want = _want("noise301", names[i % len(names)])
            if not np.array_equal(plane, want):
                errs.append("%d cameras, slot %d: %d bytes of the rectified plane differ" % (len(names), i, int((plane != want).sum())))
    det.close()
    del keep
    assert not errs, errs


# ---- 4. the fused resize -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cam", ("rational+R", "equidistant"))
@pytest.mark.parametrize("encoding", ("mono8", "bgr8"))
@pytest.mark.parametrize("target", ((160, 120), (301, 203)), ids=("160x120", "301x203"))
def test_fused_resize(plane_handle, target, encoding, cam):
    """AMDAT_DBG_RESIZED == the oracle's resize of the reference's rectified plane (S == G at the source size)."""
    det = plane_handle
    dw, dh = target
    K, D, Kn, kind, R = cm.cameras(W, H)[cam]
    keep, frame = _device_frame(rc.encode(cm.noise("noise301"), encoding), 16, 3)
    G = _want("noise301", cam)
    try:
        det.set_rectification([(K, D, Kn, kind, R)])
        det.set_resize([target])
        det.detect_batch_ex([frame], max_dets=64, intrinsics=[(100.0, 100.0, dw / 2.0, dh / 2.0)], encoding=encoding)
        plane = det.debug(0, capi.DBG_RESIZED).reshape(dh, dw)
    finally:
        det.set_resize(None)
    want = po.resize_mono8(G, dw, dh)
    print("%s -> %dx%d %s: %d of %d bytes differ" % (cam, dw, dh, encoding, int((plane != want).sum()), dw * dh))
    assert np.array_equal(plane, want)
    if (dh, dw) == G.shape:
        assert np.array_equal(want, G)
    del keep


# ---- 5. records ----------------------------------------------------------------------------------------------------------------------------
def _scene_tensor():
    if "scene_t" not in _cache:
        _cache["scene_t"] = torch.from_numpy(rc.scene()[0]).cuda()
    return _cache["scene_t"]


@pytest.mark.parametrize("cam", ("rational+R", "equidistant"))
@pytest.mark.parametrize("setting", rc.SETTINGS, ids=lambda s: "d%d-t%d-qs%g" % s)
def test_records(built, setting, cam):
    """scene_c2 under the camera: exactly the oracle's ten records on the reference-rectified frame."""
    decimate, tile, sigma = setting
    model = cm.cameras()[cam]
    det = AprilTagDetector(1920, 1080, decimate=decimate, tile_size=tile, quad_sigma=sigma, rectification=[model])
    g = det.detect_batch_ex(_scene_tensor(), max_dets=64, intrinsics=[rc.k4(model[2])])[0]
    plane_ok = np.array_equal(det.debug(0, capi.DBG_RECTIFIED).reshape(1080, 1920), cm.rectified_scene(cam))
    det.close()
    want = cm.oracle_detections(cam, setting)
    errs = pu.compare_detections(g, want, exact=True)
    assert len(want) == 10 and len(g) == 10 and not errs, (len(g), errs[:4])
    assert plane_ok


@pytest.mark.parametrize("path", ("latency", "throughput"))
def test_stage_dumps(built, path):
    """Threshold through quads of the rectified frame on each launch set: the oracle's on the reference-rectified frame."""
    model = cm.cameras()["rational+R"]
    det = AprilTagDetector(1920, 1080, rectification=[model])
    det.set_submission_path(path)
    g = det.detect_batch_ex(_scene_tensor(), max_dets=64, intrinsics=[rc.k4(model[2])])[0]
    assert det.last_submission_path() == path
    errs, odets = pu.compare_stages(det, 0, cm.rectified_scene("rational+R"), rc.FAM, model[2])
    errs += pu.compare_detections(g, odets, exact=True)
    det.close()
    assert len(odets) == 10 and not errs, errs[:6]


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_graphs(built):
    cams = cm.cameras(W, H)
    gray = rc.bt601(cm.noise("noise301"))
    keep, frame = _device_frame(gray, 16, 3)
    det = AprilTagDetector(640, 480, max_batch=2, per_frame_sizes=True)
    L, h = capi.lib(), det._h

    def plane():
        det.detect_batch_ex([frame], max_dets=64, intrinsics=[rc.k4(cams["rational"][2])])
        return det.debug(0, capi.DBG_RECTIFIED).reshape(H, W)

    det.set_rectification([cams["rational+R"]])
    assert np.array_equal(plane(), _want("noise301", "rational+R"))
    K, D, Kn, kind, R = cams["equidistant+R"]
    nan_r, inf_r = R.copy(), R.copy()
    nan_r[1, 2], inf_r[0, 0] = float("nan"), float("inf")
    bad_lists = ([(K, D, Kn, 3, R)], [(K, D, Kn, 0xFFFFFFFF, R)],                    # an unknown kind
                 [(K, D, Kn, kind, nan_r)], [(K, D, Kn, kind, inf_r)],               # a non-finite R
                 [(K, D, Kn, kind, np.zeros((3, 3)))],                               # an R that was never filled in
                 [cams["rational"], (K, D, Kn, kind, np.zeros((3, 3)))],             # (the second camera's)
                 [(K, [0.1, float("nan"), 0, 0], Kn, kind, R)],                      # a non-finite D
                 [(K, [0.1, 0, 0, 0, 0.5], Kn, 2, R)], [(K, [0.1, 0, 0, 0, 0, 0.5], Kn, 0, R)],   # a coefficient beyond the kind's own
                 [cams["rational"]] * 3)                                             # ncams 3 > max_batch 2
    for bad in bad_lists:
        assert _code(lambda: det.set_rectification(bad)) == INVALID_ARGUMENT
        assert np.array_equal(plane(), _want("noise301", "rational+R"))   # the previous setting is in force
    assert L.amdAprilTagsSetRectificationEx(h, 1, None) == INVALID_ARGUMENT and L.amdAprilTagsSetRectificationEx(None, 0, None) == INVALID_ARGUMENT
    prep = det.prepare([frame], max_dets=64, intrinsics=[rc.k4(Kn)])
    det.submit_prepared(prep)
    assert _code(lambda: det.set_rectification([cams["equidistant"]])) == INVALID_ARGUMENT   # between Submit and Wait
    det.wait_prepared(prep)
    assert np.array_equal(plane(), _want("noise301", "rational+R"))
    # changing only the models retires no graph, whatever their kinds -- and the next submission uses the new ones
    capturing, live, retired0 = det.graph_replay()
    assert capturing and live >= 1
    for cam in ("equidistant", "plumb_bob+R", "plumb_bob", "rational", "equidistant+R", "plumb_bob"):
        det.set_rectification([cams[cam]])
        assert np.array_equal(plane(), _want("noise301", cam)), cam
        assert np.array_equal(plane(), _want("noise301", cam)), cam   # (replayed)
        assert det.graph_replay()[2] == retired0
    det.set_rectification([cams["plumb_bob"][:3], cams["plumb_bob"][:3]])   # the old call after the new one
    assert np.array_equal(plane(), _want("noise301", "plumb_bob")) and det.graph_replay()[2] == retired0
    det.set_rectification(None)   # off retires them
    capturing, live_off, retired1 = det.graph_replay()
    assert live_off == 0 and retired1 > retired0
    assert _code(lambda: plane()) == INVALID_ARGUMENT   # (no rectified plane)
    det.close()
    del keep


# ---- 7. the node shell -----------------------------------------------------------------------------------------------------------------------
def _p12(Kn):
    return [Kn[0, 0], Kn[0, 1], Kn[0, 2], 0.0, Kn[1, 0], Kn[1, 1], Kn[1, 2], 0.0, 0.0, 0.0, 1.0, 0.0]


def test_node_shell(built):
    """AprilTagNode(rectify="full") fed the distorted host frame publishes what a plain node publishes for the reference-rectified frame
    and a CameraInfo whose k is Knew; a two-stream AprilTagMultiCameraNode with one fisheye and one plumb_bob camera does so per stream,
    also with the cameras swapped in the second round."""
    from isaac_ros_apriltag_amd import build as b
    from isaac_ros_apriltag_amd import node
    b.build_node()
    img = rc.scene()[0]
    models = cm.cameras()
    names = {"rational+R": "rational_polynomial", "equidistant": "equidistant", "plumb_bob": "plumb_bob"}
    cams = {}
    for cam in names:
        K, D, Kn, kind, R = models[cam]
        cams[cam] = {"K": [float(v) for v in K.reshape(-1)], "D": list(D), "model": kind, "R": R, "P": _p12(Kn),
                     "Knew": [float(v) for v in Kn.reshape(-1)], "plane": cm.rectified_scene(cam)}
    assert np.array_equal(cams["plumb_bob"]["plane"], rc.rectified("a"))

    def feed(n, cam, rect, stream=None, stamp=(3, 0)):
        frame = img if rect else cam["plane"]
        args = (frame.ctypes.data, False, "mono8", 1920, 1080, 1920, cam["K"] if rect else cam["Knew"], "cam", stamp)
        more = {"D": cam["D"], "distortion_model": cam["model"], "P12": cam["P"], "R": cam["R"]} if rect else {}
        return n.on_frame(*args, **more) if stream is None else n.on_frame(stream, *args, **more)

    nodes = []
    try:
        a, p = node.AprilTagNode(rectify="full"), node.AprilTagNode()
        nodes += [a, p]
        got, want = feed(a, cams["rational+R"], True), feed(p, cams["rational+R"], False)
        assert len(want[0]) == 10 and got == want
        multi, plain = node.AprilTagMultiCameraNode(2, rectify="full"), node.AprilTagMultiCameraNode(2)
        nodes += [multi, plain]
        for rnd in range(2):
            order = [cams["equidistant"], cams["plumb_bob"]][::1 if rnd == 0 else -1]
            for s in range(2):
                assert feed(multi, order[s], True, s, (4 + rnd, s)) and feed(plain, order[s], False, s, (4 + rnd, s))
            for s in range(2):
                assert multi.publishes(s) == rnd + 1 == plain.publishes(s)
                assert len(plain.last(s)[0]) == 10 and multi.last(s) == plain.last(s)
        assert multi.last(0) != multi.last(1)
        # an unknown model still throws before anything is staged, and the text names the three known ones
        with pytest.raises(RuntimeError, match="'plumb_bob', 'rational_polynomial' and 'equidistant'"):
            multi.on_frame(0, img.ctypes.data, False, "mono8", 1920, 1080, 1920, cams["plumb_bob"]["K"], "cam", (9, 0), D=[0.1] * 4,
                           distortion_model="thin_prism")
        assert multi.publishes(0) == 2
    finally:
        [n.close() for n in nodes]


# ---- 8. atan_s on the device ---------------------------------------------------------------------------------------------------------------
def test_atan_s_on_the_device(built):
    a = np.concatenate([np.linspace(0.0, 3.0, 3072), np.logspace(-12, 3, 1016), [0.0, 1.0, 0.41421356237309503, 1000.0],
                        np.nextafter(1.0, [0.0, 2.0]), np.nextafter(0.41421356237309503, [0.0, 1.0])])
    assert a.size == 4096
    got = capi.debug_math(6, a, np.ones_like(a))
    want = cm.atan_s(a)
    ndiff = int((got.view(np.uint64) != want.view(np.uint64)).sum())
    print("atan_s: %d of %d results differ in their bits" % (ndiff, a.size))
    assert ndiff == 0


# ---- the suite bites -------------------------------------------------------------------------------------------------------------------------
_SELECT = "test_plane_bytes and noise301"
_PLANE_IDS = {cam: ["test_plane_bytes[noise301-%s-%s]" % (enc, cam) for enc in ("mono8", "bgr8")] for cam in cm.CAMERA_NAMES}


def _ids(*cams):
    return tuple(i for c in cams for i in _PLANE_IDS[c])


_WRONG_BUILDS = {
    # the general projection with R = I: every camera with a rotation is rectified as if it had none
    13: {"must_fail": _ids("plumb_bob+R", "rational+R", "equidistant+R"), "must_pass": _ids("plumb_bob", "rational", "equidistant")},
    # the rational denominator taken as 1
    14: {"must_fail": _ids("rational", "rational+R"), "must_pass": _ids("plumb_bob", "plumb_bob+R", "equidistant", "equidistant+R")},
}


@pytest.mark.parametrize("mutant", sorted(_WRONG_BUILDS))
def test_the_camera_model_tests_fail_on_the_wrong_builds(built, mutant):
    """libapriltag_amd_mut13.so and _mut14.so (csrc/tools_hooks.h, AMDAT_MUTATE): the 301 x 203 plane cases, in a process of their own,
    must FAIL on the wrong build where its error lives and pass where it does not, and all of them pass on the product library."""
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
    assert sorted(failed) == sorted(spec["must_fail"]) and sorted(passed) == sorted(spec["must_pass"]), (failed, passed)
    assert "differ" in out.stdout   # what differs: bytes of the rectified plane
    if "ok" not in _cache:   # (the product run is the same for both wrong builds)
        _cache["ok"] = run(None)
    out_ok, passed_ok, failed_ok = _cache["ok"]
    assert out_ok.returncode == 0 and not failed_ok and sorted(passed_ok) == sorted(passed + failed), (out_ok.stdout[-1500:], failed_ok)
