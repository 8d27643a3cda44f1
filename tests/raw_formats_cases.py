"""Inputs of the raw-format tests, built once per process: noise frames, and the detection cases -- tag36h11 id 7 under
H = [[s, .15 s, cx], [-.1 s, s, cy], [0, 0, 1]], rendered with background 170, sigma 1.0, seed 3, tinted (R, G, B) = (1, 0.85, 0.6) gray
and mosaiced -- at the three sizes the GPU tests use.  tests/test_raw_formats_cpu.py asserts on the CPU oracle that every case holds
the record, so every list the GPU tests compare holds one."""
import functools

import numpy as np

from isaac_ros_apriltag_amd import synth

import raw_formats_ref as rf

SIZES = ((64, 48, 14.0, 32.0, 24.0), (97, 75, 20.0, 48.2, 37.7), (161, 119, 24.0, 81.3, 58.6))   # (w, h, s, cx, cy)
TINT = (100, 85, 60)    # per cent
TAG_ID = 7
FAMILIES = ("tag36h11",)


def K_of(w, h):
    return np.array([[100.0, 0.0, w / 2.0], [0.0, 100.0, h / 2.0], [0.0, 0.0, 1.0]])


def k4(w, h):
    K = K_of(w, h)
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def tint(gray, per_cent=TINT):
    """[h, w] -> [h, w, 3]: channel c is gray * per_cent[c] / 100, rounded (integers throughout)."""
    g = np.asarray(gray).astype(np.int64)
    return np.stack([(g * p + 50) // 100 for p in per_cent], axis=-1).astype(np.asarray(gray).dtype)


@functools.lru_cache(maxsize=None)
def tag_gray(size):
    w, h, s, cx, cy = SIZES[size]
    H = np.array([[s, 0.15 * s, cx], [-0.1 * s, s, cy], [0.0, 0.0, 1.0]])
    return synth.render(w, h, [{"family": "tag36h11", "id": TAG_ID, "H": H}], background=170, sigma=1.0, seed=3)


def low_bits(h, w, bits):
    """what a sensor leaves below the significant byte: a fixed pattern of `bits` bits"""
    y, x = np.mgrid[0:h, 0:w]
    return ((x * 7 + y * 3) & ((1 << bits) - 1)).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def tag_frame(size, encoding, shift=4):
    """The detection case of `size` as a frame of `encoding`: uint8, or uint16 with 16 - 8 - shift .. significant bits above `shift`
    (12-bit data at shift 4).  Read-only."""
    gray = tag_gray(size)
    pat = rf.pattern_of(encoding)
    v = gray if pat is None else rf.mosaic(tint(gray), pat)
    if rf.is16(encoding):
        v = (v.astype(np.uint16) << shift) | low_bits(v.shape[0], v.shape[1], shift)
    v = np.ascontiguousarray(v)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def noise_frame(size, encoding, seed=0):
    """Noise over the whole range of the sample type (16-bit: saturating samples at every shift below 8).  Read-only."""
    w, h = SIZES[size][:2]
    rng = np.random.default_rng(1000 * w + h + seed)
    v = rng.integers(0, 1 << 16, size=(h, w), dtype=np.uint16) if rf.is16(encoding) else rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def tag_ref(size, encoding, shift=4):
    """ref(tag_frame): the mono8 plane the records are compared on.  Read-only."""
    g = rf.convert(tag_frame(size, encoding, shift), encoding, shift)
    g.setflags(write=False)
    return g
