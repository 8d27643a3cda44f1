"""Resize measurements, all rows in one run:

  n frames (config 2, noise sigma 2, decimate 1; the 3840 x 2160 frames are the 1080p scenes with every pixel doubled), n = 8 and 64,
  3840 x 2160 -> 1920 x 1080 and 1920 x 1080 -> 1280 x 720, mono8 and bgr8, with and without rectification, two forms alternated
  step by step:
    in-sub  amdAprilTagsSetResize (and amdAprilTagsSetRectification with n cameras) on a handle of the target size, one
            DetectBatch[Color]Ex on the caller's frames
    in-sub <camera>   with rectification, the same through amdAprilTagsSetRectificationEx (k_resize_frames_general), n cameras of one
            kind: plumb_bob+R, rational, rational+R, equidistant, equidistant+R (--cameras; the cameras of tools/rectify_rates.py)
    chain   the host-side chain of the calls that exist without amdAprilTagsSetResize: per frame amdAprilTagsConvertToMono8 (bgr8 only),
            amdAprilTagsRectifyMono8 (with rectification only) and amdAprilTagsResizeMono8, each on the caller's stream into a host-owned
            plane, then one mono8 DetectBatchEx on a plain handle of the target size
  Host clock around calls that end in a stream wait; the median of --steps steps each, with the minimum and the quartiles, and whether
  the two forms gave the same records.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isaac_ros_apriltag_amd import capi, synth  # noqa: E402
from isaac_ros_apriltag_amd.detector import AprilTagDetector  # noqa: E402

DA = [-0.08, 0.01, 0.0005, -0.0007, 0.0]
PAIRS = (((3840, 2160), (1920, 1080)), ((1920, 1080), (1280, 720)))


def model(w, h):
    """scene_c2's camera scaled to w x h, mild barrel distortion, a slightly wider pinhole camera for the rectified image."""
    K = synth.default_K(1920, 1080)
    K[0, :] *= w / 1920.0
    K[1, :] *= h / 1080.0
    Kn = K.copy()
    Kn[0, 0] *= 0.97
    Kn[1, 1] *= 0.97
    Kn[0, 2] += 6.5 * w / 1920.0
    Kn[1, 2] -= 4.25 * h / 1080.0
    return K, DA, Kn


def model_ex(name, w, h):
    """rectify_rates.model_ex scaled to w x h."""
    import rectify_rates as rr
    K, D, Kn, kind, R = rr.model_ex(name)
    return scaled(K, 1920, 1080, w, h), D, scaled(Kn, 1920, 1080, w, h), kind, R


def scaled(K, sw, sh, dw, dh):
    K = K.copy()
    K[0, :] = K[0, :] * float(dw) / float(sw)
    K[1, :] = K[1, :] * float(dh) / float(sh)
    return K


def frames(n, encoding, sw, distinct=8, seed=1234):
    imgs = [synth.scene_c2(seed=seed + i, sigma=2.0)[0] for i in range(distinct)]
    if sw == 3840:
        imgs = [np.repeat(np.repeat(g, 2, axis=0), 2, axis=1) for g in imgs]
    if encoding == "bgr8":
        imgs = [np.stack([g // 2 + 40, g, g], axis=-1) for g in imgs]
    t = torch.from_numpy(np.stack(imgs)).cuda()
    return t.repeat(((n + distinct - 1) // distinct,) + (1,) * (t.dim() - 1))[:n].contiguous()


def k4(K):
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def main(args):
    L = capi.lib()
    for (sw, sh), (dw, dh) in PAIRS:
        K, D, Kn = model(sw, sh)
        k9, d5, kn9 = (C.c_double * 9)(*K.reshape(-1)), (C.c_double * 5)(*D), (C.c_double * 9)(*Kn.reshape(-1))
        for n in args.frames:
            for enc in ("mono8", "bgr8"):
                batch = frames(n, enc, sw)
                gray = torch.empty((n, sh, sw), dtype=torch.uint8, device="cuda") if enc != "mono8" else None   # host-owned planes
                rplane = torch.empty((n, sh, sw), dtype=torch.uint8, device="cuda")
                splane = torch.empty((n, dh, dw), dtype=torch.uint8, device="cuda")
                for rect in (False, True):
                    intr = [k4(scaled(Kn if rect else K, sw, sh, dw, dh))] * n
                    plain = AprilTagDetector(dw, dh, max_batch=n)
                    p_chain = plain.prepare(splane, max_dets=64, intrinsics=intr)
                    fused = AprilTagDetector(dw, dh, max_batch=n, resize=[(dw, dh)], rectification=[(K, D, Kn)] * n if rect else None)
                    p_fused = fused.prepare(batch, max_dets=64, intrinsics=intr, encoding=enc)

                    def chain():
                        for i in range(n):
                            src = batch[i]
                            if gray is not None:
                                L.amdAprilTagsConvertToMono8(src.data_ptr(), sw * 3, b"bgr8", sw, sh, gray[i].data_ptr(), sw, None)
                                src = gray[i]
                            if rect:
                                L.amdAprilTagsRectifyMono8(src.data_ptr(), sw, rplane[i].data_ptr(), sw, sw, sh, k9, d5, kn9, None)
                                src = rplane[i]
                            L.amdAprilTagsResizeMono8(src.data_ptr(), sw, sw, sh, splane[i].data_ptr(), dw, dw, dh, None)
                        plain.run_prepared(p_chain)
                    forms = {"in-sub": lambda: fused.run_prepared(p_fused), "chain": chain}
                    general = []
                    for cam in (args.cameras if rect else ()):
                        M = model_ex(cam, sw, sh)
                        det = AprilTagDetector(dw, dh, max_batch=n, resize=[(dw, dh)], rectification=[M] * n)
                        prep = det.prepare(batch, max_dets=64, intrinsics=[k4(scaled(M[2], sw, sh, dw, dh))] * n, encoding=enc)
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
                    tag = "%dx%d->%dx%d %2d x %s %s" % (sw, sh, dw, dh, n, enc, "rect+resize" if rect else "resize     ")
                    for name in forms:
                        t = np.array(times[name])
                        q1, med, q3 = np.percentile(t, (25, 50, 75))
                        print("%s %-20s median %8.3f ms  (min %8.3f, quartiles %8.3f .. %8.3f, %d steps)" %
                              (tag, name, med, t.min(), q1, q3, len(t)), flush=True)
                    a, b = plain.unpack(p_chain), fused.unpack(p_fused)
                    same = all(len(x) == len(y) and all(np.array_equal(u["p"], v["p"]) for u, v in zip(x, y)) for x, y in zip(a, b))
                    print("%s records of in-sub and chain equal: %s (%.1f per frame)" % (tag, same, np.mean([len(x) for x in b])), flush=True)
                    [det.close() for det in general]
                    fused.close()
                    plain.close()
                del batch, gray, rplane, splane


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--cameras", nargs="*", default=["plumb_bob+R", "rational", "rational+R", "equidistant", "equidistant+R"],
                    help="the general cameras to time in the rows with rectification (none: --cameras)")
    main(ap.parse_args())
