"""Rigid-bundle measurements, the mode off against the mode on on ONE handle in one run:

  one-frame   the blocking one-frame call (graph replay) on a 1920 x 1080 frame with a 9 x 8 board of 72 tag36h11 tags at 96 px sides,
              one rigid bundle of the 64 members with ids 0 .. 63 (every lane of the solving wave holds a tag), --iterations steps
  throughput  a 256-frame submission of 1080p config-2 frames (ten tags each), one rigid bundle over their ten ids (--frames)

  The handle runs blocks of --steps calls with the mode off, on, off, on (a change of the mode retires the captured graphs, so the modes
  are not alternated call by call); host clock around calls that end in a stream wait; per mode the median over its blocks with the
  minimum and the quartiles, and whether the tag records of the two modes are the same bytes.  The comparison is on against off within
  this run, never against another run's number.

  --only-off measures two off blocks alone and calls no entry point of the mode: copied into a checkout of the commit before the mode
  existed and run there in the same session, it gives the rows to hold this library's off rows against.
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
from isaac_ros_apriltag_amd import capi, synth  # noqa: E402
if os.environ.get("AMDAT_LIB"):   # measurement variant (isaac_ros_apriltag_amd.build.build_amd_variant)
    capi.LIB_PATH = os.path.join(ROOT, "isaac_ros_apriltag_amd", "libapriltag_amd_%s.so" % os.environ["AMDAT_LIB"])
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402

I3 = np.eye(3)


def board72(iterations):
    """(frame, rigid bundle, intrinsics): tools/bundle_rates.py's 72-tag frame; the bundle has the 64 members with ids below 64."""
    size, pitch = 0.096, 0.128
    K = np.array([[1000.0, 0, 960.0], [0, 1000.0, 540.0], [0, 0, 1]])
    R = synth.rot_xyz(math.radians(3.0), math.radians(-4.0), math.radians(1.5))
    t = np.array([0.0, 0.0, 1.0])
    cells = [(r * 9 + c, (c - 4.0) * pitch, (r - 3.5) * pitch) for r in range(8) for c in range(9)]
    tags = [{"family": "tag36h11", "id": i, "H": synth.homography_from_pose(R, t + R @ np.array([x, y, 0.0]), K, size)} for (i, x, y) in cells]
    img = synth.render(1920, 1080, tags, background=150, sigma=2.0, seed=72)
    members = [(0, i, I3, (x, y, 0.0), size) for (i, x, y) in cells if i < 64]
    return np.ascontiguousarray(img), {"name": "board64", "iterations": iterations, "members": members, "min_tags": 4}, (1000.0, 1000.0, 960.0, 540.0)


def measure(det, prep, bundle, steps, label, only_off):
    modes = ("off", "off") if only_off else ("off", "on", "off", "on")
    times = {m: [] for m in set(modes)}
    outs = {}
    for mode in modes:
        if not only_off:
            det.set_bundles_ex([bundle] if mode == "on" else None)
        det.run_prepared(prep)   # warm: the mode's graph, its buffers
        det.run_prepared(prep)
        for _ in range(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            det.run_prepared(prep)
            times[mode].append((time.perf_counter() - t0) * 1e3)
        outs[mode] = (bytes(prep["out"]), list(prep["cnt"]))
        if mode == "on":
            poses = det.bundle_poses_ex(prep["n"])
            solved = sum(1 for f in poses if f[0]["status"] == 0)
            print("%s rigid bundle on: %d of %d frames solved, frame 0 uses %d tags, chain %d, rms %.3f px" %
                  (label, solved, len(poses), poses[0][0]["ntags"], poses[0][0]["chosen"],
                   math.sqrt(poses[0][0]["sq_err_sum"] / max(4 * poses[0][0]["ntags"], 1))), flush=True)
    for mode in sorted(times, reverse=True):
        t = np.array(times[mode])
        q1, med, q3 = np.percentile(t, (25, 50, 75))
        print("%s rigid bundle %-3s median %8.4f ms  (min %8.4f, quartiles %8.4f .. %8.4f, %d steps)" % (label, mode, med, t.min(), q1, q3, len(t)), flush=True)
    if not only_off:
        print("%s tag records of the two modes are the same bytes: %s; on - off = %.4f ms (medians)" %
              (label, outs["on"] == outs["off"], np.median(times["on"]) - np.median(times["off"])), flush=True)


def main(args):
    print("library: %s" % os.path.basename(capi.LIB_PATH), flush=True)
    img, bundle, intr = board72(args.iterations)
    det = AprilTagDetector(1920, 1080, intrinsics=intr, tag_size=0.096, max_batch=1)
    prep = det.prepare(torch.from_numpy(img).cuda(), max_dets=128)
    measure(det, prep, bundle, args.steps, "one-frame  1 x 1080p, 72-tag board", args.only_off)
    det.close()
    n = args.frames
    imgs = [synth.scene_c2(seed=1234 + i, sigma=2.0)[0] for i in range(8)]
    t = torch.from_numpy(np.stack(imgs)).cuda()
    batch = t.repeat((n + 7) // 8, 1, 1)[:n].contiguous()
    grid = {"name": "grid", "iterations": args.iterations, "min_tags": 3,
            "members": [(0, r * 5 + c, I3, ((c - 2.0) * 0.5, (r - 0.5) * 0.5, 0.0), 0.22) for r in range(2) for c in range(5)]}
    det = AprilTagDetector(1920, 1080, max_batch=n)
    prep = det.prepare(batch, max_dets=64)
    measure(det, prep, grid, max(args.steps // 4, 5), "throughput %d x 1080p, config 2" % n, args.only_off)
    det.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--iterations", type=int, default=50)
    ap.add_argument("--only-off", action="store_true")
    main(ap.parse_args())
