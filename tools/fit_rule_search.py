#!/usr/bin/env python3
"""Seeded searches on the oracle's per-cluster fit log (oracle/apriltag_oracle.c: ato_fit_rec_t) behind tests/fit_rule_frames.py; CPU only.

  blobs [seconds]   random dark blobs in an 11 x 11 window, 64 to a 160 x 160 frame, seeds 0, 1, 2, ...: of the clusters of 24 .. 60
                    points, how many leave by which reason, and the first examples of the narrow-window exits -- total error (5: every
                    side's mse at or under 10 but the mean above 10 sz / (sz + 4)), a kept quad the dot test decided, two maxima at the
                    cut's threshold value, a point lost to duplicate removal
  cut               thin rhombi (tests/fit_rule_frames.py: rhombus) per site of the cut to max_nmaxima corners: the frames whose
                    cluster is kept with its weakest corner at rank 10 or beyond among all maxima
"""
import itertools
import os
import sys
import time
from collections import Counter, defaultdict

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pyoracle as po  # noqa: E402
import fit_frames as ff  # noqa: E402
import fit_rule_frames as fr  # noqa: E402


def blob_frame(seed, cells=8, cell=20, n=11):
    rng = np.random.default_rng(seed)
    img = fr.ground(cells * cell, cells * cell)
    for cy, cx in itertools.product(range(cells), range(cells)):
        m = np.zeros((n, n), bool)
        for _ in range(int(rng.integers(1, 5))):   # a union of one to four rectangles, then 8 % of the window's pixels flipped
            x0, y0 = rng.integers(0, n - 3, 2)
            m[y0:y0 + rng.integers(2, n - y0 + 1), x0:x0 + rng.integers(2, n - x0 + 1)] = True
        m ^= rng.random((n, n)) < 0.08
        img[cy * cell + 4:cy * cell + 4 + n, cx * cell + 4:cx * cell + 4 + n][m] = fr.D
    return img


def blobs(budget):
    t0, seed, by, first = time.time(), 0, Counter(), defaultdict(list)
    while time.time() - t0 < budget:
        _, _, log = po.detect(blob_frame(seed), want_dump=True, want_fit_log=True)
        for r in log[(log["points_in"] >= 24) & (log["points_in"] <= 60)]:
            by[int(r["reason"])] += 1
            tags = [po.FIT_REASONS[r["reason"]]] if r["reason"] in (2, 3, 5, 7) else []
            tags += ["kept, dot-decided"] if r["reason"] == 10 and r["dot_changes"] == 1 else []
            tags += ["two maxima at the threshold"] if r["nties"] >= 2 else []
            tags += ["lost a duplicate"] if 0 <= r["points"] < r["points_in"] else []
            for t in tags:
                if len(first[t]) < 3:
                    first[t].append((seed, "%x" % r["key"], int(r["points_in"])))
        seed += 1
    print("%d frames, %d clusters of 24 .. 60 points: %s" % (seed, sum(by.values()), {po.FIT_REASONS[k]: v for k, v in sorted(by.items())}))
    for t in ("total error", "kept, dot-decided", "two maxima at the threshold", "lost a duplicate", "fewer than 24 after duplicate removal",
              "fewer than 4 maxima", "degenerate intersection"):
        print("  %-40s %s" % (t, first.get(t) or "none"))


def cut():
    # site -> (canvas, half lengths, acute angles, turns, (sigma, seed)s, maxima from .. to, points from .. to)
    sites = {"k_fit_small": ((80, 80), np.arange(12.0, 30.0), np.arange(10.5, 40, 1.5), 0.05 + 0.26 * np.arange(12), [(0.0, 0)], 11, 128, 24, 128),
             "up to 64": ((224, 120), (90.0,), np.arange(9.0, 14.01, 0.25), (0.05, 0.4, 0.8), [(0.0, 0)], 11, 64, 129, 10 ** 6),
             "up to 512": ((400, 400), (230.0, 250.0), np.arange(9.75, 12.01, 0.25), (0.6, 0.8, 1.0, 2.2), [(0.0, 0)], 65, 512, 769, 10 ** 6),
             "above 512": ((900, 900), (560.0, 600.0), np.arange(10.0, 12.01, 0.5), (np.pi / 4, np.pi / 4 + 0.02), [(1.0, 1), (1.0, 2), (2.0, 1), (2.0, 2)],
                           513, 10 ** 6, 769, 10 ** 6)}
    for site, ((w, h), hls, degs, turns, noises, lo, hi, plo, phi) in sites.items():
        n, ranks, ties = 0, Counter(), 0
        for hl, a, turn, (sigma, seed) in itertools.product(hls, degs, turns, noises):
            img = fr.ground(w, h)
            fr.fill(img, fr.turned(fr.rhombus(hl, a), turn, (w / 2, h / 2)))
            _, _, log = po.detect(ff.finish(img.astype(np.float64), sigma, seed), want_dump=True, want_fit_log=True)
            n += 1
            for r in log[(log["nmaxima"] >= lo) & (log["nmaxima"] <= hi) & (log["points_in"] >= plo) & (log["points_in"] <= phi)]:
                ties += r["nties"] >= 2
                if r["reason"] == 10:
                    ranks[int(r["weakest_rank"])] += 1
                    if r["weakest_rank"] >= 10:
                        print("  %s: half length %g, %g degrees, turn %.4f, sigma %g seed %d: %d points, %d maxima, weakest corner at rank %d"
                              % (site, hl, a, turn, sigma, seed, r["points_in"], r["nmaxima"], r["weakest_rank"]))
        print("%s: %d frames; kept quads by the rank of their weakest corner: %s; cuts with two maxima at the threshold: %d"
              % (site, n, dict(sorted(ranks.items())), ties))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "cut":
        cut()
    else:
        blobs(float(sys.argv[2]) if len(sys.argv) > 2 else 60.0)
