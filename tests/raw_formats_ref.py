"""The reference of the raw formats (csrc/raw_formats.h), stated twice: vectorised numpy (`convert`) and per pixel
in plain Python (`convert_pixelwise`).  tests/test_raw_formats_cpu.py shows that the two agree; the GPU tests compare the library
against `convert`, and the CPU oracle is fed its output as mono8 (the oracle does not know the formats).

A frame is a [h, w] array: uint8 for the 8-bit encodings, uint16 (any byte order of the array; the VALUES are the samples) for the
16-bit ones.  `samples_from_bytes` reads a row of bytes as the little-endian samples the library reads."""
import numpy as np

# the red site's phase (px, py) of the four patterns: one pattern shifted
PHASE = {"rggb": (0, 0), "grbg": (1, 0), "gbrg": (0, 1), "bggr": (1, 1)}
PATTERNS = ("rggb", "bggr", "gbrg", "grbg")   # in the order of the encoding values
ENCODINGS = tuple("bayer_%s8" % p for p in PATTERNS) + ("mono16",) + tuple("bayer_%s16" % p for p in PATTERNS)


def pattern_of(encoding):
    """"rggb" .. of a Bayer encoding, None of mono16."""
    return encoding[6:10] if encoding.startswith("bayer_") else None


def is16(encoding):
    return encoding.endswith("16")


def samples_from_bytes(rows):
    """[h, 2w] bytes -> [h, w] uint16 samples: s = byte 2x | byte 2x + 1 << 8."""
    rows = np.asarray(rows, dtype=np.uint8)
    return rows[:, 0::2].astype(np.uint16) | (rows[:, 1::2].astype(np.uint16) << 8)


def sample(raw, encoding, shift=8):
    """v(x, y), 0 .. 255, as int32: the byte, or min(255, s >> shift)."""
    raw = np.asarray(raw)
    if not is16(encoding):
        assert raw.dtype == np.uint8
        return raw.astype(np.int32)
    assert raw.dtype.kind == "u" and raw.dtype.itemsize == 2 and 0 <= shift <= 8
    return np.minimum(255, raw.astype(np.int32) >> shift)


def gray_bt601(r, g, b):
    return (4899 * r + 9617 * g + 1868 * b + 8192) >> 14


def demosaic_gray(v, pattern):
    """[h, w] samples -> [h, w] uint8 gray: bilinear with reflected neighbours, then gray_bt601."""
    v = np.asarray(v, dtype=np.int32)
    h, w = v.shape
    assert h >= 2 and w >= 2
    P = np.pad(v, 1, mode="reflect")   # index -1 -> 1, n -> n - 2: r(i, n)
    N, S, W, E = P[:-2, 1:-1], P[2:, 1:-1], P[1:-1, :-2], P[1:-1, 2:]
    NW, NE, SW, SE = P[:-2, :-2], P[:-2, 2:], P[2:, :-2], P[2:, 2:]
    cross, diag = (N + S + E + W + 2) >> 2, (NE + NW + SE + SW + 2) >> 2
    hor, ver = (E + W + 1) >> 1, (N + S + 1) >> 1
    px, py = PHASE[pattern]
    xr = ((np.arange(w) ^ px) & 1 == 0)[None, :]
    yr = ((np.arange(h) ^ py) & 1 == 0)[:, None]
    red, blue, g_red_row, g_blue_row = xr & yr, ~xr & ~yr, ~xr & yr, xr & ~yr
    R = np.select([red, blue, g_red_row, g_blue_row], [v, diag, hor, ver])
    G = np.select([red | blue], [cross], v)
    B = np.select([red, blue, g_red_row, g_blue_row], [diag, v, ver, hor])
    return gray_bt601(R, G, B).astype(np.uint8)


def convert(raw, encoding, shift=8):
    """The gray plane the library detects on."""
    v = sample(raw, encoding, shift)
    if encoding == "mono16":
        return v.astype(np.uint8)
    return demosaic_gray(v, pattern_of(encoding))


def _r(i, n):
    return -i if i < 0 else 2 * (n - 1) - i if i >= n else i


def convert_pixelwise(raw, encoding, shift=8):
    """The same, one pixel at a time from the issue's table."""
    raw = np.asarray(raw)
    h, w = raw.shape
    out = np.zeros((h, w), dtype=np.uint8)

    def v(x, y):
        s = int(raw[_r(y, h), _r(x, w)])
        return min(255, s >> shift) if is16(encoding) else s
    for y in range(h):
        for x in range(w):
            if encoding == "mono16":
                out[y, x] = v(x, y)
                continue
            px, py = PHASE[pattern_of(encoding)]
            n, s, e, wv = v(x, y - 1), v(x, y + 1), v(x + 1, y), v(x - 1, y)
            ne, nw, se, sw = v(x + 1, y - 1), v(x - 1, y - 1), v(x + 1, y + 1), v(x - 1, y + 1)
            red_col, red_row = (x - px) % 2 == 0, (y - py) % 2 == 0
            if red_col and red_row:
                R, G, B = v(x, y), (n + s + e + wv + 2) >> 2, (ne + nw + se + sw + 2) >> 2
            elif not red_col and not red_row:
                R, G, B = (ne + nw + se + sw + 2) >> 2, (n + s + e + wv + 2) >> 2, v(x, y)
            elif red_row:
                R, G, B = (e + wv + 1) >> 1, v(x, y), (n + s + 1) >> 1
            else:
                R, G, B = (n + s + 1) >> 1, v(x, y), (e + wv + 1) >> 1
            out[y, x] = (4899 * R + 9617 * G + 1868 * B + 8192) >> 14
    return out


def mosaic(rgb, pattern):
    """[h, w, 3] RGB -> the [h, w] frame a sensor with this pattern delivers (same dtype)."""
    rgb = np.asarray(rgb)
    h, w = rgb.shape[:2]
    px, py = PHASE[pattern]
    xr = ((np.arange(w) ^ px) & 1 == 0)[None, :]
    yr = ((np.arange(h) ^ py) & 1 == 0)[:, None]
    return np.where(xr & yr, rgb[..., 0], np.where(~xr & ~yr, rgb[..., 2], rgb[..., 1])).astype(rgb.dtype)
