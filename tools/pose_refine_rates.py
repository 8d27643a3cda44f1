"""Pose-refinement measurements, the mode off against the mode on on ONE handle in one run:

  one-frame   the blocking one-frame call (graph replay) on a 1920 x 1080 frame with a 9 x 8 board of 72 tag36h11 tags at 96 px sides:
              72 records refined, nine waves
  throughput  a 256-frame submission of 1080p config-2 frames (ten tags each) (--frames)

  The handle runs blocks of --steps calls with the mode off, on (--iterations, 50), off, on (a change of the mode retires the captured
  graphs, so the modes are not alternated call by call); host clock around calls that end in a stream wait; per mode the median over
  its blocks with the minimum and the quartiles, and whether the tag records of the two modes are the same bytes.  The comparison is on
  against off within this run, never against another run's number.  --kernel adds the duration of k_pose_refine alone: the difference
  of the one-frame medians at --iterations and at 1 iteration is (iterations - 1) steps of the chain.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from isaac_ros_apriltag_amd import synth  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402
from bundle_rates import board72  # noqa: E402


def block(det, prep, steps):
    det.run_prepared(prep)   # warm: the mode's graph, its buffers
    det.run_prepared(prep)
    out = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        det.run_prepared(prep)
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def measure(det, prep, iterations, steps, label, kernel=False):
    times = {"off": [], "on": [], "one": []}
    outs = {}
    for mode in ("off", "on", "off", "on") + (("one",) if kernel else ()):
        det.set_pose_refinement({"off": 0, "on": iterations, "one": 1}[mode])
        times[mode] += block(det, prep, steps)
        outs[mode] = (bytes(prep["out"]), list(prep["cnt"]))
        if mode == "on":
            poses = det.refined_poses(prep["n"])
            flat = [p for f in poses for p in f]
            print("%s refinement on: %d records refined in %d frames, %d chose chain 1, %d without alternative, %d degenerate; median "
                  "err / err_homography %.3f" % (label, len(flat), len(poses), sum(p["chosen"] for p in flat), sum(p["status"] == 1 for p in flat),
                                                 sum(p["status"] == 2 for p in flat),
                                                 float(np.median([p["err"] / p["err_homography"] for p in flat])) if flat else 0.0), flush=True)
    for mode in ("off", "on") + (("one",) if kernel else ()):
        t = np.array(times[mode])
        q1, med, q3 = np.percentile(t, (25, 50, 75))
        print("%s refinement %-3s median %8.4f ms  (min %8.4f, quartiles %8.4f .. %8.4f, %d steps)" % (label, mode, med, t.min(), q1, q3, len(t)), flush=True)
    print("%s tag records of the two modes are the same bytes: %s; on - off = %.4f ms (medians)" %
          (label, outs["on"] == outs["off"], np.median(times["on"]) - np.median(times["off"])), flush=True)
    if kernel:
        d = np.median(times["on"]) - np.median(times["one"])
        print("%s %d iterations - 1 iteration = %.4f ms: %.2f us per iteration of the chain" % (label, iterations, d, 1e3 * d / max(iterations - 1, 1)), flush=True)


def main(args):
    img, _, intr = board72()
    det = AprilTagDetector(1920, 1080, intrinsics=intr, tag_size=0.096, max_batch=1)
    prep = det.prepare(torch.from_numpy(img).cuda(), max_dets=128)
    measure(det, prep, args.iterations, args.steps, "one-frame  1 x 1080p, 72-tag board", kernel=args.kernel)
    det.close()
    n = args.frames
    if n <= 0:
        return
    imgs = [synth.scene_c2(seed=1234 + i, sigma=2.0)[0] for i in range(8)]
    t = torch.from_numpy(np.stack(imgs)).cuda()
    batch = t.repeat((n + 7) // 8, 1, 1)[:n].contiguous()
    det = AprilTagDetector(1920, 1080, max_batch=n)
    prep = det.prepare(batch, max_dets=64)
    measure(det, prep, args.iterations, max(args.steps // 4, 5), "throughput %d x 1080p, config 2" % n)
    det.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--kernel", action="store_true")
    main(ap.parse_args())
