"""quad_sigma measurements, each mode in a run of its own:

  filter  256 x 1080p mono8, decimate 1 and 2, sigma 0.8 / 2 / 4: the threshold stage's HIP-event time with the filter on and off (the
          filter kernel alone: run this mode under `rocprofv3 --kernel-trace --stats`, k_quad_sigma<KH>).  TB/s on the algorithmic bytes:
          the source rows the decimation samples (H rows of W0 bytes) plus the plane written (N = W H): 2 N at decimate 1, 3 N at 2.
          The event difference is the filter's time only at decimate 1: at decimate 2 the unfiltered threshold also writes the plane.
  step    the bench's workload (256 x 1080p config 2, noise sigma 2, decimate 1), quad_sigma 0 / 0.8 / 2 alternated step by step, the
          median of --steps steps each, and the stage times of one profiled step per setting.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isaac_ros_apriltag_amd import synth  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402


def frames(n, distinct=16, seed=1234):
    imgs = [synth.scene_c2(seed=seed + i, sigma=2.0)[0] for i in range(distinct)]
    t = torch.from_numpy(np.stack(imgs)).cuda()
    return t.repeat((n + distinct - 1) // distinct, 1, 1)[:n].contiguous()


def filter_mode(args):
    batch = frames(args.frames)
    K = synth.default_K(1920, 1080)
    for dec in (1, 2):
        det = AprilTagDetector(1920, 1080, decimate=dec, intrinsics=(K[0, 0], K[1, 1], K[0, 2], K[1, 2]), max_batch=args.frames)
        prep = det.prepare(batch, max_dets=64)
        det.set_profiling(True)
        W, H = 1 + (1920 - 1) // dec, 1 + (1080 - 1) // dec
        base = None
        for s in (0.0, 0.8, 2.0, 4.0):
            det.set_quad_sigma(s)
            det.run_prepared(prep)
            ms = []
            for _ in range(args.reps):
                det.run_prepared(prep)
                ms.append(det.stage_ms()["threshold"])
            m = float(np.median(ms))
            if base is None:
                base = m
                print("decimate %d: threshold stage %.4f ms per %d frames without the filter" % (dec, m, args.frames), flush=True)
                continue
            f = m - base
            nbytes = float(H * 1920 + W * H) * args.frames
            print("decimate %d sigma %.1f: threshold stage %.4f ms, filter (difference) %.4f ms, %.2f TB/s on %.0f MB" %
                  (dec, s, m, f, nbytes / (f * 1e-3) / 1e12 if f > 0 else float("nan"), nbytes / 1e6), flush=True)
        det.close()


def step_mode(args):
    batch = frames(args.frames, distinct=args.frames, seed=1234)
    K = synth.default_K(1920, 1080)
    det = AprilTagDetector(1920, 1080, intrinsics=(K[0, 0], K[1, 1], K[0, 2], K[1, 2]), max_batch=args.frames)
    prep = det.prepare(batch, max_dets=64)
    sig = (0.0, 0.8, 2.0)
    times = {s: [] for s in sig}
    for s in sig:
        det.set_quad_sigma(s)
        det.run_prepared(prep)
        det.run_prepared(prep)
    for _ in range(args.steps):
        for s in sig:
            det.set_quad_sigma(s)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            det.run_prepared(prep)
            times[s].append((time.perf_counter() - t0) * 1e3)
    for s in sig:
        det.set_quad_sigma(s)
        det.set_profiling(True)
        det.run_prepared(prep)
        st = {k: round(v, 3) for k, v in det.stage_ms().items()}
        det.set_profiling(False)
        dets = np.mean([len(x) for x in det.unpack(prep)])
        print("quad_sigma %.1f: median %.3f ms per %d-frame step (min %.3f), %.1f detections per frame\n    stages %s" %
              (s, float(np.median(times[s])), args.frames, min(times[s]), dets, st), flush=True)
    det.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("filter", "step"))
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    (filter_mode if a.mode == "filter" else step_mode)(a)
