"""Bundle measurements, bundles off against bundles on on ONE handle in one run:

  one-frame   the blocking one-frame call (graph replay) on a 1920 x 1080 frame with a 9 x 8 board of 72 tag36h11 tags at 96 px sides,
              one bundle of the 72 members
  throughput  a 256-frame submission of 1080p config-2 frames (ten tags each), one bundle over their ten ids (--frames)

  The handle runs blocks of --steps calls with bundles off, on, off, on (a change of the mode retires the captured graphs, so the modes
  are not alternated call by call); host clock around calls that end in a stream wait; per mode the median over its blocks with the
  minimum and the quartiles, and whether the tag records of the two modes are the same bytes.  The comparison is on against off within
  this run, never against another run's number.
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isaac_ros_apriltag_amd import synth  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402


def board72():
    """(frame, bundle, intrinsics): 1920 x 1080, 72 tags at 96 px sides on a 128 px grid, slightly tilted."""
    size, pitch = 0.096, 0.128
    K = np.array([[1000.0, 0, 960.0], [0, 1000.0, 540.0], [0, 0, 1]])
    R = synth.rot_xyz(math.radians(3.0), math.radians(-4.0), math.radians(1.5))
    t = np.array([0.0, 0.0, 1.0])
    members = [(0, r * 9 + c, (c - 4.0) * pitch, (r - 3.5) * pitch, size) for r in range(8) for c in range(9)]
    tags = [{"family": "tag36h11", "id": m[1], "H": synth.homography_from_pose(R, t + R @ np.array([m[2], m[3], 0.0]), K, size)} for m in members]
    img = synth.render(1920, 1080, tags, background=150, sigma=2.0, seed=72)
    return np.ascontiguousarray(img), {"name": "board72", "members": members, "min_tags": 4}, (1000.0, 1000.0, 960.0, 540.0)


def measure(det, prep, bundle, steps, label):
    times = {"off": [], "on": []}
    outs = {}
    for mode in ("off", "on", "off", "on"):
        det.set_bundles([bundle] if mode == "on" else None)
        det.run_prepared(prep)   # warm: the mode's graph, its buffers
        det.run_prepared(prep)
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            det.run_prepared(prep)
            times[mode].append((time.perf_counter() - t0) * 1e3)
        outs[mode] = (bytes(prep["out"]), list(prep["cnt"]))
        if mode == "on":
            poses = det.bundle_poses(prep["n"])
            solved = sum(1 for f in poses if f[0]["status"] == 0)
            print("%s bundles on: %d of %d frames solved, frame 0 uses %d tags, rms %.3f px" %
                  (label, solved, len(poses), poses[0][0]["ntags"], math.sqrt(poses[0][0]["sq_err_sum"] / max(4 * poses[0][0]["ntags"], 1))), flush=True)
    for mode in ("off", "on"):
        t = np.array(times[mode])
        q1, med, q3 = np.percentile(t, (25, 50, 75))
        print("%s bundles %-3s median %8.4f ms  (min %8.4f, quartiles %8.4f .. %8.4f, %d steps)" % (label, mode, med, t.min(), q1, q3, len(t)), flush=True)
    print("%s tag records of the two modes are the same bytes: %s; on - off = %.4f ms (medians)" %
          (label, outs["on"] == outs["off"], np.median(times["on"]) - np.median(times["off"])), flush=True)


def main(args):
    img, bundle, intr = board72()
    det = AprilTagDetector(1920, 1080, intrinsics=intr, tag_size=0.096, max_batch=1)
    prep = det.prepare(torch.from_numpy(img).cuda(), max_dets=128)
    measure(det, prep, bundle, args.steps, "one-frame  1 x 1080p, 72-tag board")
    det.close()
    n = args.frames
    imgs = [synth.scene_c2(seed=1234 + i, sigma=2.0)[0] for i in range(8)]
    t = torch.from_numpy(np.stack(imgs)).cuda()
    batch = t.repeat((n + 7) // 8, 1, 1)[:n].contiguous()
    grid = {"name": "grid", "members": [(0, r * 5 + c, (c - 2.0) * 0.5, (r - 0.5) * 0.5, 0.22) for r in range(2) for c in range(5)], "min_tags": 3}
    det = AprilTagDetector(1920, 1080, max_batch=n)
    prep = det.prepare(batch, max_dets=64)
    measure(det, prep, grid, max(args.steps // 4, 5), "throughput %d x 1080p, config 2" % n)
    det.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    main(ap.parse_args())
