"""Tag-table measurement, all rows in one process and on one handle: a 64-frame 1080p config-2 submission
with no table, with a 587-entry table (every id of tag36h11, sizes of 5 .. 11 cm) and with the same table and listed_only, alternated
step by step after a warm-up.  Device events on the submission's stream around submit and wait; the median of --steps steps with the
minimum and the quartiles, as milliseconds per submission and frames per second.  Informational: there is no threshold."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from isaac_ros_apriltag_amd import synth  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402

W, H, NF = 1920, 1080, 64


def main(args):
    grays = [synth.scene_c2(seed=1234 + i, sigma=2.0)[0] for i in range(8)]
    frames = torch.from_numpy(np.stack(grays)).cuda().repeat((NF // 8, 1, 1)).contiguous()
    table = [("tag36h11", i, 0.05 + 0.01 * (i % 7)) for i in range(587)]
    det = AprilTagDetector(W, H, max_batch=NF)
    prep = det.prepare(frames, max_dets=64)
    stream = torch.cuda.Stream()
    forms = {"no table": lambda: det.set_tag_table(None), "587 entries": lambda: det.set_tag_table(table),
             "587 entries, listed_only": lambda: det.set_tag_table(table, True)}

    def step():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        det.submit_prepared(prep, stream=stream.cuda_stream)
        det.wait_prepared(prep)
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b)
    counts = {}
    for name, setup in forms.items():   # warm every form
        setup()
        step()
        step()
        counts[name] = float(np.mean(list(prep["cnt"])))
    times = {k: [] for k in forms}
    for _ in range(args.steps):
        for name, setup in forms.items():
            setup()
            torch.cuda.synchronize()
            times[name].append(step())
    for name in forms:
        t = np.asarray(times[name])
        q1, med, q3 = np.percentile(t, (25, 50, 75))
        print("submission %d x 1080p %-26s median %7.3f ms (min %7.3f, quartiles %7.3f .. %7.3f, %d steps)  %8.1f frames/s  %.1f records per frame" %
              (NF, name, med, t.min(), q1, q3, len(t), NF / med * 1e3, counts[name]), flush=True)
    assert det.late_waits() == 0
    det.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20, help="timed submissions per form")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device: there is no other way to take these numbers"
    main(args)
