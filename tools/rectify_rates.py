"""Rectification measurements, each mode in a run of its own:

  step    n x 1080p frames (config 2, noise sigma 2, decimate 1), n = 8 and 256, mono8 and bgr8, three forms alternated step by step:
            plain     the unrectified submission (the same on a commit without amdAprilTagsSetRectification: the tool then runs
                      this form and the two-step form only)
            in-sub    amdAprilTagsSetRectification with n cameras, one DetectBatch[Color]Ex
            in-sub <camera>   the same through amdAprilTagsSetRectificationEx (k_rectify_frames_general), n cameras of one kind:
                      plumb_bob+R, rational, rational+R, equidistant, equidistant+R (--cameras; R a small stereo-like rotation)
            two-step  per frame amdAprilTagsRectifyMono8 on the caller's stream into a host-owned plane (bgr8: amdAprilTagsConvertToMono8
                      into a second host-owned plane first), then one mono8 DetectBatchEx on a handle without rectification
          Host clock around calls that end in a stream wait; the median of --steps steps each, with the minimum and the quartiles.
  kernel  one warmed in-sub submission of 256 frames per encoding, for `rocprofv3 --kernel-trace --stats` (k_rectify_frames).  Bytes per
          second on the algorithmic traffic: 2 N for mono8 (N = 1920 x 1080 x frames: every source byte once, every plane byte once),
          4 N for bgr8.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isaac_ros_apriltag_amd import capi, synth  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402

W, H = 1920, 1080
DA = [-0.08, 0.01, 0.0005, -0.0007, 0.0]


def model():
    K = synth.default_K(W, H)
    Kn = K.copy()
    Kn[0, 0] *= 0.97
    Kn[1, 1] *= 0.97
    Kn[0, 2] += 6.5
    Kn[1, 2] -= 4.25
    return K, DA, Kn


D_RATIONAL = [0.35, -0.12, 0.0005, -0.0007, 0.02, 0.42, -0.05, 0.01]
D_FISHEYE = [-0.03, 0.004, -0.0006, 0.0001]
CAMERAS = ("plumb_bob+R", "rational", "rational+R", "equidistant", "equidistant+R")


def rotation(rx=0.01, ry=-0.015, rz=0.004):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]]) @
            np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def model_ex(name):
    """(K, D, Knew, model_name, R) of one of CAMERAS: the cameras of tests/camera_models_ref.py."""
    K, D, Kn = model()
    kind = name.split("+")[0]
    if kind == "rational":
        D = D_RATIONAL
    elif kind == "equidistant":
        D = D_FISHEYE
        Kn = K.copy()
        Kn[0, 0] *= 0.7
        Kn[1, 1] *= 0.7
        Kn[0, 2] += 6.5
        Kn[1, 2] -= 4.25
    full = {"plumb_bob": "plumb_bob", "rational": "rational_polynomial", "equidistant": "equidistant"}[kind]
    return K, D, Kn, full, (rotation() if name.endswith("+R") else None)


def frames(n, encoding, distinct=8, seed=1234):
    imgs = [synth.scene_c2(seed=seed + i, sigma=2.0)[0] for i in range(distinct)]
    if encoding == "bgr8":
        imgs = [np.stack([g // 2 + 40, g, g], axis=-1) for g in imgs]
    t = torch.from_numpy(np.stack(imgs)).cuda()
    return t.repeat(((n + distinct - 1) // distinct,) + (1,) * (t.dim() - 1))[:n].contiguous()


def k4(K):
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def step_mode(args):
    L = capi.lib()
    K, D, Kn = model()
    k9, d5, kn9 = (C.c_double * 9)(*K.reshape(-1)), (C.c_double * 5)(*D), (C.c_double * 9)(*Kn.reshape(-1))
    have = hasattr(AprilTagDetector, "set_rectification")
    for n in args.frames:
        for enc in ("mono8", "bgr8"):
            batch = frames(n, enc)
            plane = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")                       # host-owned: the rectified frames
            gray = torch.empty((n, H, W), dtype=torch.uint8, device="cuda") if enc != "mono8" else None   # ... and the converted ones
            intr = [k4(Kn)] * n
            plain = AprilTagDetector(W, H, intrinsics=k4(Kn), max_batch=n)
            p_plain = plain.prepare(batch, max_dets=64, intrinsics=intr, encoding=enc)
            p_two = plain.prepare(plane, max_dets=64, intrinsics=intr)
            forms = {"plain": lambda: plain.run_prepared(p_plain)}

            def two_step():
                for i in range(n):
                    src = batch[i]
                    if gray is not None:
                        L.amdAprilTagsConvertToMono8(src.data_ptr(), W * 3, b"bgr8", W, H, gray[i].data_ptr(), W, None)
                        src = gray[i]
                    L.amdAprilTagsRectifyMono8(src.data_ptr(), W, plane[i].data_ptr(), W, W, H, k9, d5, kn9, None)
                plain.run_prepared(p_two)
            forms["two-step"] = two_step
            if have:
                rect = AprilTagDetector(W, H, intrinsics=k4(Kn), max_batch=n, rectification=[(K, D, Kn)] * n)
                p_rect = rect.prepare(batch, max_dets=64, intrinsics=intr, encoding=enc)
                forms["in-sub"] = lambda: rect.run_prepared(p_rect)
            general = []
            for cam in (args.cameras if have else ()):
                det = AprilTagDetector(W, H, intrinsics=k4(Kn), max_batch=n, rectification=[model_ex(cam)] * n)
                prep = det.prepare(batch, max_dets=64, intrinsics=[k4(model_ex(cam)[2])] * n, encoding=enc)
                forms["in-sub " + cam] = lambda det=det, prep=prep: det.run_prepared(prep)
                general.append(det)
            times = {f: [] for f in forms}
            for f in forms.values():   # warm every form: code objects, graphs, planes
                f()
                f()
            for _ in range(args.steps):
                for name, f in forms.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    f()
                    times[name].append((time.perf_counter() - t0) * 1e3)
            for name in forms:
                t = np.array(times[name])
                q1, med, q3 = np.percentile(t, (25, 50, 75))
                print("%3d x %s %-20s median %8.3f ms  (min %8.3f, quartiles %8.3f .. %8.3f, %d steps)" %
                      (n, enc, name, med, t.min(), q1, q3, len(t)), flush=True)
            if have:
                a, b = plain.unpack(p_two), rect.unpack(p_rect)
                same = all(len(x) == len(y) and all(np.array_equal(u["p"], v["p"]) for u, v in zip(x, y)) for x, y in zip(a, b))
                print("%3d x %s records of in-sub and two-step equal: %s (%.1f per frame)" % (n, enc, same, np.mean([len(x) for x in b])), flush=True)
                rect.close()
            [det.close() for det in general]
            plain.close()
            del batch, plane, gray


def kernel_mode(args):
    K, D, Kn = model()
    n = max(args.frames)
    for enc in ("mono8", "bgr8"):
        batch = frames(n, enc)
        det = AprilTagDetector(W, H, intrinsics=k4(Kn), max_batch=n, rectification=[(K, D, Kn)] * n)
        prep = det.prepare(batch, max_dets=64, intrinsics=[k4(Kn)] * n, encoding=enc)
        for _ in range(args.reps):
            det.run_prepared(prep)
        print("%s: %d submissions of %d frames; N = %d bytes per submission" % (enc, args.reps, n, W * H * n), flush=True)
        det.close()
        del batch


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("step", "kernel"))
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 256])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cameras", nargs="*", default=list(CAMERAS), choices=CAMERAS, help="step: the general cameras to time (none: --cameras)")
    a = ap.parse_args()
    (step_mode if a.mode == "step" else kernel_mode)(a)
