"""quad_sigma restated in numpy: upstream's integer Gaussian taps, the two 1-D passes with their copy rule,
blur (sigma > 0) or sharpen (sigma < 0).  The taps use math.exp, the libm the library's host code calls."""
import math

import numpy as np


def taps(sigma):
    """Upstream's taps for quad_sigma: an empty list for the identity (ksz <= 1, |sigma| < 0.5)."""
    s = np.float32(abs(np.float32(sigma)))
    ksz = int(np.float32(4.0) * s)
    if ksz % 2 == 0:
        ksz += 1
    if ksz <= 1:
        return []
    h = ksz // 2
    sd = float(s)
    dk = [math.exp(-0.5 * ((i - h) / sd) * ((i - h) / sd)) for i in range(ksz)]
    acc = 0.0
    for v in dk:
        acc += v
    return [int((v / acc) * 255.0) for v in dk]


# one sigma for every half width h = ksz / 2 the library serves (|sigma| <= 4: h = 1 .. 8; h = 8 is sigma 4.0 alone), each used with
# both signs, and the ends of the accepted range
SIGMA_OF_H = {1: 0.8, 2: 1.2, 3: 1.7, 4: 2.2, 5: 2.7, 6: 3.2, 7: 3.7, 8: 4.0}
ALL_SIGMAS = tuple(s * sign for s in SIGMA_OF_H.values() for sign in (1, -1)) + (0.5, -0.5)


def pass_1d(x, k):
    """One pass along the last axis: y[i] = (sum_j k[j] x[i-h+j]) >> 8 for h <= i <= n-h-2, every other sample copied."""
    x = np.asarray(x, dtype=np.uint8)
    ksz = len(k)
    n = x.shape[-1]
    if ksz <= 1 or n <= ksz:
        return x.copy()
    h = ksz // 2
    y = x.copy()
    xi = x.astype(np.uint32)
    acc = np.zeros(x.shape[:-1] + (n - 2 * h - 1,), dtype=np.uint32)
    for j in range(ksz):
        acc += np.uint32(k[j]) * xi[..., j:j + n - 2 * h - 1]
    y[..., h:n - h - 1] = (acc >> 8).astype(np.uint8)
    return y


def filter_image(img, sigma):
    """F_sigma of a working image (uint8, H x W)."""
    g = np.asarray(img, dtype=np.uint8)
    k = taps(sigma)
    if not k:
        return g.copy()
    t = pass_1d(g, k)
    b = pass_1d(t.T, k).T
    if sigma > 0:
        return np.ascontiguousarray(b)
    return np.clip(2 * g.astype(np.int32) - b.astype(np.int32), 0, 255).astype(np.uint8)


def decimate(img, f):
    """The point-sampled working image of the threshold pass (th_load16): every f-th pixel of every f-th row, ceil(W0 / f) x ceil(H0 / f)."""
    return np.ascontiguousarray(np.asarray(img)[::f, ::f])


def embed_decimated(img, filtered, f):
    """J = img with J[f y, f x] = filtered[y, x]: the frame whose decimation is the filtered working image."""
    j = np.array(img, dtype=np.uint8, copy=True)
    j[::f, ::f] = filtered
    return j
