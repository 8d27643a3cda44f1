"""Shared by tests/test_rectify_cpu.py and tests/test_rectify_submission_gpu.py: the camera models of the rectification tests, the
1080p scene they distort, and the oracle's results on it -- each computed once per process and never changed afterwards."""
import numpy as np

from isaac_ros_apriltag_amd import synth
from oracle import pyoracle as po
import parity_util as pu

FAM = ("tag36h11",)
DA = [-0.08, 0.01, 0.0005, -0.0007, 0.0]
DZ = [0.12, -0.03, 0.0, 0.0, 0.0]   # pincushion: the rectified frame reaches beyond the source, which leaves a zero-filled border
# (decimate, tile_size, quad_sigma): every setting has 10 oracle detections on scene_c2 rectified with DA, Knew_a
SETTINGS = ((1, 4, 0.0), (2, 4, 0.0), (3, 4, 0.0), (1, 8, 0.0), (1, 4, 0.8), (2, 4, -0.8))


def camera(w, h):
    """scene_c2's camera (synth.default_K(1920, 1080)) scaled to a w x h image."""
    sx, sy = w / 1920.0, h / 1080.0
    return np.array([[1000.0 * sx, 0, 960.0 * sx], [0, 1000.0 * sy, 540.0 * sy], [0, 0, 1]])


def knew_a(w, h):
    """K with both focal lengths x 0.97 and the principal point moved by (+6.5, -4.25) (of the 1080p image; scaled with the size)."""
    K = camera(w, h)
    K[0, 0] *= 0.97
    K[1, 1] *= 0.97
    K[0, 2] += 6.5 * w / 1920.0
    K[1, 2] -= 4.25 * h / 1080.0
    return K


def knew_z(w, h):
    K = camera(w, h)
    K[0, 0] *= 0.8
    K[1, 1] *= 0.8
    return K


def model_a(w=1920, h=1080):
    return camera(w, h), DA, knew_a(w, h)


def model_z(w=1920, h=1080):
    return camera(w, h), DZ, knew_z(w, h)


def model_identity(w, h):
    return camera(w, h), [0.0] * 5, camera(w, h)


def k4(K):
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def bt601(rgb):
    """The fixed-point BT.601 statement of amdAprilTagsConvertToMono8 on an [H, W, 3] RGB array."""
    r, g, b = (rgb[..., i].astype(np.uint32) for i in range(3))
    return ((4899 * r + 9617 * g + 1868 * b + 8192) >> 14).astype(np.uint8)


def encode(rgb, encoding):
    """[H, W, 3] RGB -> the interleaved frame of `encoding` (mono8: its BT.601 gray)."""
    if encoding == "mono8":
        return np.ascontiguousarray(bt601(rgb))
    c = rgb if encoding in ("rgb8", "rgba8") else rgb[..., ::-1]
    if encoding in ("rgba8", "bgra8"):
        c = np.concatenate([c, np.full(c.shape[:2] + (1,), 255, np.uint8)], axis=-1)
    return np.ascontiguousarray(c)


_cache = {}


def scene():
    """(img, K) of synth.scene_c2(): 1920 x 1080, ten tag36h11 tags."""
    if "scene" not in _cache:
        img, K, _ = synth.scene_c2()
        _cache["scene"] = (np.ascontiguousarray(img), K)
    return _cache["scene"]


def rectified(which="a"):
    """The oracle's rectified scene_c2 under model_a / model_z."""
    if ("rect", which) not in _cache:
        K, D, Kn = model_a() if which == "a" else model_z()
        _cache[("rect", which)] = po.rectify_mono8(scene()[0], K, D, Kn)
    return _cache[("rect", which)]


def oracle_detections(which="a", setting=SETTINGS[0], rectify=True):
    """The oracle's records on the (rectified) scene at (decimate, tile_size, quad_sigma), posed with the camera of that image."""
    key = ("dets", which, setting, rectify)
    if key not in _cache:
        decimate, tile, sigma = setting
        img = rectified(which) if rectify else scene()[0]
        Kpose = (knew_a(1920, 1080) if which == "a" else knew_z(1920, 1080)) if rectify else scene()[1]
        more = {"quad_sigma": sigma} if sigma else {}
        _cache[key] = po.detect(img, families=FAM, params=pu.oracle_params(Kpose, decimate, tile_size=tile, **more))[0]
    return _cache[key]
