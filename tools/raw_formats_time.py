"""Raw-format measurements (profiles/raw_formats_time.md), all rows in one process:

  conversion   the stand-alone conversion of 64 distinct 1920 x 1080 noise frames per call -- amdAprilTagsConvertRawToMono8 for
               bayer_rggb8, mono16 and bayer_rggb16, and beside them amdAprilTagsConvertToMono8 on rgb8 frames of the same size, the
               yardstick (k_to_mono8) -- device events around the 64 launches of a call, the versions alternated call by call after a
               warm-up; the median of --calls calls with the minimum and the quartiles, as microseconds per frame and as achieved
               bytes per second over the bytes the algorithm needs: source plus gray plane, 2 N for 8-bit sources, 3 N for 16-bit ones,
               4 N for rgb8 (N = 1920 * 1080).  Every stand-alone call ends in a stream wait, so a frame's time holds one launch and one
               wait beside the kernel: the same for every version.
  submission   64 frames of config 2 (eight distinct scenes, tinted and mosaiced as bayer_rggb8) through one DetectBatchColorEx, beside
               the same handle's mono8 submission of the converted planes, alternated step by step; host clock around the blocking
               calls; frames per second from the median step.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from isaac_ros_apriltag_amd import capi, synth  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402
import raw_formats_ref as rf  # noqa: E402

W, H, NF = 1920, 1080, 64


def stats(t):
    t = np.asarray(t, dtype=np.float64)
    q1, med, q3 = np.percentile(t, (25, 50, 75))
    return med, t.min(), q1, q3


def conversion(args):
    L = capi.lib()
    rng = np.random.default_rng(7)
    dst = torch.empty((NF, H, W), dtype=torch.uint8, device="cuda")
    src8 = torch.from_numpy(rng.integers(0, 256, size=(NF, H, W), dtype=np.uint8)).cuda()
    src16 = torch.from_numpy(rng.integers(0, 1 << 15, size=(NF, H, W), dtype=np.int16)).cuda()
    rgb = torch.from_numpy(rng.integers(0, 256, size=(NF, H, W, 3), dtype=np.uint8)).cuda()

    def raw(src, enc, bps):
        e = capi.ENCODINGS[enc]
        return lambda: [L.amdAprilTagsConvertRawToMono8(src[i].data_ptr(), W * bps, e, 8, W, H, dst[i].data_ptr(), W, None) for i in range(NF)]
    forms = {"bayer_rggb8": (raw(src8, "bayer_rggb8", 1), 2), "mono16": (raw(src16, "mono16", 2), 3), "bayer_rggb16": (raw(src16, "bayer_rggb16", 2), 3),
             "rgb8 (yardstick)": (lambda: [L.amdAprilTagsConvertToMono8(rgb[i].data_ptr(), W * 3, b"rgb8", W, H, dst[i].data_ptr(), W, None)
                                           for i in range(NF)], 4)}
    for f, _ in forms.values():   # warm every version: code objects
        assert not any(f()) and not any(f())
    times = {k: [] for k in forms}
    for _ in range(args.calls):
        for name, (f, _) in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            f()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / NF)   # microseconds per frame
    for name, (_, nbytes) in forms.items():
        med, lo, q1, q3 = stats(times[name])
        gbs = lambda us: nbytes * W * H / us * 1e-3
        print("conversion %-18s median %7.2f us/frame (min %7.2f, quartiles %7.2f .. %7.2f, %d calls of %d frames)  %7.1f GB/s over %d N bytes "
              "(best %7.1f)" % (name, med, lo, q1, q3, len(times[name]), NF, gbs(med), nbytes, gbs(lo)), flush=True)


def submission(args):
    grays = [synth.scene_c2(seed=1234 + i, sigma=2.0)[0] for i in range(8)]
    raws = [rf.mosaic(np.stack([g, (g.astype(np.uint16) * 85 // 100).astype(np.uint8), (g.astype(np.uint16) * 60 // 100).astype(np.uint8)], axis=-1),
                      "rggb") for g in grays]
    refs = [rf.convert(r, "bayer_rggb8") for r in raws]
    rep = lambda imgs: torch.from_numpy(np.stack(imgs)).cuda().repeat((NF // 8, 1, 1)).contiguous()
    t_raw, t_ref = rep(raws), rep(refs)
    det = AprilTagDetector(W, H, max_batch=NF)
    p_raw = det.prepare(t_raw, max_dets=64, encoding="bayer_rggb8")
    p_ref = det.prepare(t_ref, max_dets=64)
    forms = {"bayer_rggb8": lambda: det.run_prepared(p_raw), "mono8 of the converted planes": lambda: det.run_prepared(p_ref)}
    for f in forms.values():
        f()
        f()
    times = {k: [] for k in forms}
    for _ in range(args.steps):
        for name, f in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name in forms:
        med, lo, q1, q3 = stats(times[name])
        print("submission %d x 1080p %-30s median %7.3f ms (min %7.3f, quartiles %7.3f .. %7.3f, %d steps)  %8.1f frames/s" %
              (NF, name, med, lo, q1, q3, len(times[name]), NF / med * 1e3), flush=True)
    a, b = det.unpack(p_raw), det.unpack(p_ref)
    same = all(len(x) == len(y) and all(np.array_equal(u["p"], v["p"]) for u, v in zip(x, y)) for x, y in zip(a, b))
    print("submission records of the two forms equal: %s (%.1f per frame)" % (same, np.mean([len(x) for x in a])), flush=True)
    det.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=25, help="timed calls of 64 conversions per version (at least 20)")
    ap.add_argument("--steps", type=int, default=20, help="timed submissions per form")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device: there is no other way to take these numbers"
    conversion(args)
    submission(args)
