"""What the pose covariance costs: one-frame submissions with pose_refinement = 50 of

  oblique   the 640 x 480 frame with four oblique tags (tests/pose_refine_cases.py), one wave of k_pose_refine
  board72   the 640 x 576 frame with 72 tags (tests/bundle_cases.py), nine waves

  on/off    two handles of this build, the covariance mode on (sigma 0.3 px) and off, alternated step by step after a warm-up; the
            host clock around each blocking DetectBatchEx call (it ends in a stream wait); the median of --steps steps each, with
            the quartiles
  builds    the mode off on this build and -- with --parent-tree DIR, a checkout of the parent commit with its libraries built --
            on the parent's, each in processes of their own, alternated for --rounds rounds: the medians per round, and the spread
            (max - min) of the parent's rounds, which is the margin for "no slower"

Usage: python tools/pose_cov_cost.py [--parent-tree DIR] [--steps 300] [--warmup 50] [--rounds 3]
One JSON line per measurement, and a last one with the summary."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("oblique", "board72")
ITERATIONS = 50
SIGMA = 0.3


def render(out_dir):
    """The two frames and their handles' parameters, from the test modules of this tree (host only)."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import bundle_cases as bc
    import pose_refine_cases as pc
    np.save(os.path.join(out_dir, "oblique.npy"), pc.oblique_frame())
    np.save(os.path.join(out_dir, "board72.npy"), bc.frame72())
    spec = {"oblique": {"w": pc.WO, "h": pc.HO, "tag_size": pc.SIZE_O, "intrinsics": list(pc.INTR_O), "tags": 4},
            "board72": {"w": bc.W2, "h": bc.H2, "tag_size": bc.SIZE2, "intrinsics": list(bc.INTR2), "tags": 72}}
    with open(os.path.join(out_dir, "spec.json"), "w") as f:
        json.dump(spec, f)


def child(tree, frames, steps, warmup, onoff):
    """One process on the GPU with the package of `tree`: the medians of every case, mode off (and on, alternated, with onoff)."""
    sys.path.insert(0, tree)
    import torch
    from isaac_ros_apriltag_amd.detector import AprilTagDetector
    spec = json.load(open(os.path.join(frames, "spec.json")))
    out = {"tree": tree, "onoff": onoff}
    for case in CASES:
        s = spec[case]
        frame = torch.from_numpy(np.load(os.path.join(frames, case + ".npy"))).cuda()
        dets, preps = [], []
        for on in ((False, True) if onoff else (False,)):
            kw = {"pose_covariance": SIGMA} if on else {}
            det = AprilTagDetector(s["w"], s["h"], tag_size=s["tag_size"], intrinsics=s["intrinsics"], pose_refinement=ITERATIONS, **kw)
            dets.append(det)
            preps.append(det.prepare(frame, max_dets=128))
        times = [[] for _ in dets]
        for step in range(warmup + steps):
            for k, (det, prep) in enumerate(zip(dets, preps)):
                t0 = time.perf_counter()
                det.run_prepared(prep)
                t1 = time.perf_counter()
                if step >= warmup:
                    times[k].append((t1 - t0) * 1e6)
        for k, (det, prep) in enumerate(zip(dets, preps)):
            assert int(prep["cnt"][0]) == s["tags"], (case, int(prep["cnt"][0]))
            q = np.percentile(times[k], [25, 50, 75])
            out["%s_%s_us" % (case, "on" if k else "off")] = [round(float(v), 2) for v in q]
            det.close()
    print(json.dumps(out))


def run_child(tree, frames, steps, warmup, onoff):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--frames", frames, "--steps", str(steps), "--warmup", str(warmup)]
    r = subprocess.run(cmd + (["--onoff"] if onoff else []), capture_output=True, text=True, timeout=240)
    if r.returncode != 0:   # (nothing more is started on the GPU after a failure)
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit("the measurement of %s ended with status %d" % (tree, r.returncode))
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    print(line, flush=True)
    return json.loads(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--onoff", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--frames")
    a = ap.parse_args()
    if a.child:
        child(a.tree, a.frames, a.steps, a.warmup, a.onoff)
        return
    with tempfile.TemporaryDirectory() as frames:
        render(frames)
        onoff = run_child(ROOT, frames, a.steps, a.warmup, True)
        summary = {}
        for case in CASES:
            summary["%s_on_minus_off_us" % case] = round(onoff[case + "_on_us"][1] - onoff[case + "_off_us"][1], 2)
        if a.parent_tree:
            med = {"parent": {c: [] for c in CASES}, "this": {c: [] for c in CASES}}
            for _ in range(a.rounds):
                for who, tree in (("parent", os.path.abspath(a.parent_tree)), ("this", ROOT)):
                    r = run_child(tree, frames, a.steps, a.warmup, False)
                    for c in CASES:
                        med[who][c].append(r[c + "_off_us"][1])
            for c in CASES:
                summary["%s_off_parent_us" % c] = med["parent"][c]
                summary["%s_off_this_us" % c] = med["this"][c]
                summary["%s_parent_spread_us" % c] = round(max(med["parent"][c]) - min(med["parent"][c]), 2)
                summary["%s_this_minus_parent_us" % c] = round(float(np.median(med["this"][c]) - np.median(med["parent"][c])), 2)
        print(json.dumps({"summary": summary}))


if __name__ == "__main__":
    main()
