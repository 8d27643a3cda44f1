"""Raw-frame mode measurements: n x 1080p mono8 frames (config 2, decimate 1; --sigma: the noise, 0 for noise-free
frames, on which rectification's blend removes no detector work), n = 64, for each of the three camera kinds with and without R, three
submissions:

    plain       the submission as it stands
    undistort   amdAprilTagsSetCornerUndistortion with n cameras of the row's kind (k_undistort_records behind k_reconcile)
    rectify     amdAprilTagsSetRectificationEx with the same n cameras (the front launch ahead of the detector)

and, with --refine, a fourth for the overhead figure beside pose refinement's:

    refine      amdAprilTagsSetPoseRefinement(50) on the plain submission

Default: all forms in one process, alternated step by step.  --only FORM: that form alone, one handle in the process (run the forms
as processes of their own to rule out that handles disturb each other).  Host clock around calls that end in a stream wait; the median
of --steps steps each, with the minimum and the quartiles, after --warmup calls per form.  Per form also: the detector's work (mean
boundary points, clusters and quads per frame: what the pixels cost behind the front stage), the records per frame, and the handle's
late waits.  The requirement is a comparison inside one row: undistort below rectify, same frames, same cameras.

--trace: no timing; a few submissions of the undistort and of the rectify form of the first camera, for
`rocprofv3 --kernel-trace --stats` (k_undistort_records against k_rectify_frames[_general])."""
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
import rectify_rates as rr  # noqa: E402

W, H = rr.W, rr.H
CAMERAS = ("plumb_bob", "plumb_bob+R", "rational", "rational+R", "equidistant", "equidistant+R")
FORMS = ("plain", "undistort", "rectify", "refine")


def frames(n, sigma, distinct=8, seed=1234):
    imgs = [synth.scene_c2(seed=seed + i, sigma=sigma)[0] for i in range(distinct)]
    t = torch.from_numpy(np.stack(imgs)).cuda()
    return t.repeat(((n + distinct - 1) // distinct, 1, 1))[:n].contiguous()


def handle(form, m, n):
    kw = {"undistort": {"corner_undistortion": [m] * n}, "rectify": {"rectification": [m] * n}, "refine": {"pose_refinement": 50}}.get(form, {})
    return AprilTagDetector(W, H, intrinsics=rr.k4(m[2]), max_batch=n, **kw)


def main(args):
    n = args.frames
    batch = frames(n, args.sigma)
    forms = [args.only] if args.only else [f for f in FORMS if f != "refine" or args.refine]
    for cam in args.cameras:
        m = rr.model_ex(cam)
        intr = [rr.k4(m[2])] * n
        dets = {f: handle(f, m, n) for f in forms}
        preps = {k: d.prepare(batch, max_dets=64, intrinsics=intr) for k, d in dets.items()}
        if args.trace:
            for k in ("undistort", "rectify"):
                for _ in range(args.warmup + 5):
                    dets[k].run_prepared(preps[k])
            print("trace: %d submissions each of undistort and rectify, %d frames, %s" % (args.warmup + 5, n, cam), flush=True)
            [d.close() for d in dets.values()]
            return
        times = {k: [] for k in dets}
        for k, d in dets.items():
            for _ in range(args.warmup):
                d.run_prepared(preps[k])
        for _ in range(args.steps):
            for k, d in dets.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d.run_prepared(preps[k])
                times[k].append((time.perf_counter() - t0) * 1e3)
        med = {}
        for k, d in dets.items():
            t = np.array(times[k])
            q1, med[k], q3 = np.percentile(t, (25, 50, 75))
            c = d.mean_counts(n)
            print("%3d x mono8 sigma %g %-14s %-10s median %8.3f ms  (min %8.3f, quartiles %8.3f .. %8.3f, %d steps; per frame %.0f points, "
                  "%.0f clusters, %.1f quads, %.1f records; %d late waits)" %
                  (n, args.sigma, cam, k, med[k], t.min(), q1, q3, len(t), c["npoints_raw"], c["nclusters"], c["nquads"],
                   float(np.mean(list(preps[k]["cnt"]))), d.late_waits()), flush=True)
        if not args.only:
            print("%3d x mono8 sigma %g %-14s undistort - plain %+.3f ms, rectify - plain %+.3f ms, undistort below rectify: %s" %
                  (n, args.sigma, cam, med["undistort"] - med["plain"], med["rectify"] - med["plain"], med["undistort"] < med["rectify"]) +
                  ("; refine - plain %+.3f ms" % (med["refine"] - med["plain"]) if args.refine else ""), flush=True)
        [d.close() for d in dets.values()]


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sigma", type=float, default=2.0)
    ap.add_argument("--refine", action="store_true")
    ap.add_argument("--only", choices=FORMS)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--cameras", nargs="*", default=list(CAMERAS), choices=CAMERAS)
    main(ap.parse_args())
