"""Shared by tests/test_pose_refine_cpu.py and tests/test_pose_refine_gpu.py: the seeded pose sets of the CPU tests, the oblique-tag
frame of the GPU test, and the oracle's records and the reference's refined records on the frames -- each computed once per process and
never changed afterwards."""
import math

import numpy as np

from isaac_ros_apriltag_amd import synth
from oracle import pyoracle as po
import bundle_cases as bc
import pose_refine_ref as pr

_cache = {}
ITERATIONS = 50   # upstream's estimate_tag_pose

# ---- the oblique-tag frame: 640 x 480, four tag36h11 tags of 0.1 m at 0.5 m, tilted 35 .. 60 degrees about four different axes ----------
WO, HO = 640, 480
SIZE_O = 0.1
INTR_O = (600.0, 600.0, 320.0, 240.0)
KO = np.array([[600.0, 0, 320.0], [0, 600.0, 240.0], [0, 0, 1]])
# (id, centre pixel, rotation angles about x, y, z in degrees): tilts of 35, 45, 52 and 60 degrees
OBLIQUE = ((3, (165.0, 122.0), (35.0, 0.0, 10.0)), (8, (475.0, 122.0), (0.0, -45.0, -20.0)),
           (21, (165.0, 358.0), (-52.0, 0.0, 95.0)), (34, (475.0, 358.0), (0.0, 60.0, 5.0)))
Z_O = 0.5


def oblique_pose(i):
    """(R, t) of tag i of the oblique frame."""
    _, (u, v), (rx, ry, rz) = OBLIQUE[i]
    R = synth.rot_xyz(math.radians(rx), math.radians(ry), math.radians(rz))
    t = Z_O * np.array([(u - INTR_O[2]) / INTR_O[0], (v - INTR_O[3]) / INTR_O[1], 1.0])
    return R, t


def oblique_frame():
    if "oblique" not in _cache:
        tags = []
        for i, (tid, _, _) in enumerate(OBLIQUE):
            R, t = oblique_pose(i)
            tags.append({"family": bc.FAM[0], "id": tid, "H": synth.homography_from_pose(R, t, KO, SIZE_O)})
        _cache["oblique"] = np.ascontiguousarray(synth.render(WO, HO, tags, background=150, sigma=1.0, seed=35))
    return _cache["oblique"]


def oblique_records():
    if "oblique_rec" not in _cache:
        _cache["oblique_rec"] = bc.oracle_records(oblique_frame(), INTR_O, tag_size=SIZE_O)
    return _cache["oblique_rec"]


def refined(key, records, intr, skew, tag_size, iterations=ITERATIONS, **kw):
    """The reference's refined records of a frame's oracle records, kept under `key`."""
    k = ("refined", key, iterations, tuple(sorted(kw)))
    if k not in _cache:
        _cache[k] = pr.refine_records(records, intr, skew, tag_size, iterations, **kw)
    return _cache[k]


def content_refined(name, iterations=ITERATIONS):
    """The refined records of a content frame of bundle_cases, under its slot's intrinsics and skew."""
    slot = bc.SLOTS[name][1]
    return refined(("content", name), bc.content_records(name), bc.INTR1[slot], bc.SKEW1[slot], bc.SIZE1, iterations)


# ---- seeded pose sets of the CPU tests -----------------------------------------------------------------------------------------------------
def rodrigues(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1.0 - math.cos(angle)) * (Kx @ Kx)


def random_pose(rng, tilt_lo, tilt_hi):
    """A 0.1 m tag at 0.6 .. 1.2 m, tilted by tilt_lo .. tilt_hi degrees about a random in-plane axis, turned about its normal."""
    tilt = math.radians(rng.uniform(tilt_lo, tilt_hi))
    az = rng.uniform(0.0, 2.0 * math.pi)
    roll = rng.uniform(0.0, 2.0 * math.pi)
    R = rodrigues((math.cos(az), math.sin(az), 0.0), tilt) @ rodrigues((0.0, 0.0, 1.0), roll)
    t = np.array([rng.uniform(-0.15, 0.15), rng.uniform(-0.1, 0.1), rng.uniform(0.6, 1.2)])
    return R, t


def project(R, t, intr, skew, size):
    """The exact corners p[k] of the tag (R, t) under the camera: K (R P_k + t) with P_k = size / 2 * (c_k, 0)."""
    fx, fy, cx, cy = intr
    out = []
    for c in pr.CORNERS:
        x = R @ np.array([size / 2.0 * c[0], size / 2.0 * c[1], 0.0]) + t
        out.append(((fx * x[0] + skew * x[1]) / x[2] + cx, fy * x[1] / x[2] + cy))
    return np.array(out)


def homography_of(p):
    """The homography c_k -> p[k] of four corners (the exact 8 x 8 solve)."""
    A, b = [], []
    for c, (u, v) in zip(pr.CORNERS, p):
        A.append([c[0], c[1], 1, 0, 0, 0, -c[0] * u, -c[1] * u])
        A.append([0, 0, 0, c[0], c[1], 1, -c[0] * v, -c[1] * v])
        b += [u, v]
    return np.append(np.linalg.solve(np.array(A), np.array(b)), 1.0)


def homography_pose(p, intr, skew, size):
    """The record's pose: the oracle's pose_from_homography on the corners' homography."""
    R, t = po.pose_from_homography(homography_of(p), intr[0], intr[1], intr[2], intr[3], size, skew=skew)
    return np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(t, dtype=np.float64)
