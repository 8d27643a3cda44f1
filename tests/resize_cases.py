"""Shared by tests/test_resize_cpu.py and tests/test_resize_submission_gpu.py: the scene, the camera models (tests/rectify_cases.py),
the oracle's resized frames and its records on them, and the batch case -- each computed once per process and never changed afterwards."""
import numpy as np

from oracle import pyoracle as po
import parity_util as pu
import rectify_cases as rc

FAM = rc.FAM
SW, SH = 1920, 1080   # scene_c2
# targets of the unrectified scene: 2/3, 1/2, a ratio that is no fraction of small integers (odd sizes: a dword tail of 1, a partial
# threshold tile), and an anisotropic one
TARGETS = ((1280, 720), (960, 540), (1437, 811), (1000, 720))
BATCH_SIZES = ((1280, 720), (1000, 600))
BATCH_DECIMATE = 2

_cache = {}


def scaled_k(K, sw, sh, dw, dh):
    """The camera of an image resized from sw x sh to dw x dh (image_proc's convention): fx, skew, cx times dw / sw; fy, cy times
    dh / sh.  Multiplied, then divided, as the node shell does."""
    K = np.array(K, dtype=np.float64).reshape(3, 3).copy()
    K[0, :] = K[0, :] * float(dw) / float(sw)
    K[1, :] = K[1, :] * float(dh) / float(sh)
    return K


def gray_plane(which=None):
    """G of scene_c2: the frame itself, or the oracle's rectified frame under model_a ("a") / model_z ("z")."""
    return rc.scene()[0] if which is None else rc.rectified(which)


def pose_camera(which=None):
    return rc.scene()[1] if which is None else (rc.knew_a(SW, SH) if which == "a" else rc.knew_z(SW, SH))


def resized(dw, dh, which=None):
    """The oracle's S = resize_mono8(G) of scene_c2."""
    key = ("S", dw, dh, which)
    if key not in _cache:
        _cache[key] = po.resize_mono8(gray_plane(which), dw, dh)
    return _cache[key]


def oracle_detections(dw, dh, setting=rc.SETTINGS[0], which=None):
    """The oracle's records on S at (decimate, tile_size, quad_sigma), posed with the scaled camera of that image."""
    key = ("dets", dw, dh, setting, which)
    if key not in _cache:
        decimate, tile, sigma = setting
        more = {"quad_sigma": sigma} if sigma else {}
        K = scaled_k(pose_camera(which), SW, SH, dw, dh)
        _cache[key] = po.detect(resized(dw, dh, which), families=FAM, params=pu.oracle_params(K, decimate, tile_size=tile, **more))[0]
    return _cache[key]


def batch_frames():
    """The eight bgr8 frames of the rectify test's batch ([H, W, 3] BGR host arrays, views of one 1080p image): five full frames, two
    1280 x 720 crops, and the 1000 x 600 window at (389, 13)."""
    if "frames" not in _cache:
        g = rc.scene()[0]
        bgr = np.ascontiguousarray(np.stack([g // 2 + 40, g, g], axis=-1))   # B, G, R
        crop_a, crop_b, window = bgr[:720, :1280], bgr[360:, 640:], bgr[13:613, 389:1389]
        _cache["frames"] = [bgr, crop_a, bgr, window, crop_b, bgr, bgr, bgr]
    return _cache["frames"]


def batch_model(i, w, h):
    """The camera model of slot i: kind i % 3 of the rectify test's three, scaled to the slot's source size w x h."""
    kind = i % 3
    if kind == 0:
        return rc.model_a(w, h)
    if kind == 1:
        return rc.model_z(w, h)
    return rc.camera(w, h), [0.03, 0.0, 0.001, 0.0, 0.0], rc.knew_a(w, h)


def batch_case(rectify):
    """Per slot i of the batch: (model or None, pose intrinsics (fx, fy, cx, cy), S, oracle records at decimate 2).  Slot i is resized to
    BATCH_SIZES[i % 2]; with `rectify` it is first rectified with batch_model(i, its width, its height)."""
    key = ("batch", bool(rectify))
    if key not in _cache:
        out, memo = [], {}
        for i, f in enumerate(batch_frames()):
            sh, sw = f.shape[:2]
            dw, dh = BATCH_SIZES[i % 2]
            mkey = (id(f), i % 2, i % 3 if rectify else -1)
            if mkey not in memo:
                G = rc.bt601(f[..., ::-1])
                model = batch_model(i, sw, sh) if rectify else None
                if rectify:
                    G = po.rectify_mono8(G, *model)
                S = po.resize_mono8(G, dw, dh)
                K = scaled_k(model[2] if rectify else rc.camera(sw, sh), sw, sh, dw, dh)
                memo[mkey] = (model, rc.k4(K), S, po.detect(S, families=FAM, params=pu.oracle_params(K, BATCH_DECIMATE))[0])
            out.append(memo[mkey])
        _cache[key] = out
    return _cache[key]
