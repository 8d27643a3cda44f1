#!/usr/bin/env python3
"""bench.py -- AprilTag detections throughput at 1920x1080 (BASELINE.json configs[1] / configs[3]) on N GPUs.

A "step" is one pass of the whole hot path (threshold -> union-find CC -> clustering -> quad fit -> decode ->
pose) over one batch of B device-resident synthetic 1080p frames per GPU; detections are on the host when a
step ends.  Eight independent camera streams with distinct intrinsics (config 4) are packed 8/4/2/1 per GPU
for N = 1/2/4/8; per-GPU work is fixed (B frames per step), so the scaling is weak.  One process per GPU, no
data-path collective; rank 0 broadcasts the per-stream parameter block once (RCCL).

`python bench.py --gpus N` starts the N ranks itself (re-exec under torch.distributed.run) when it was not
launched by a distributed launcher; it never prints a line whose n_gpus differs from --gpus.

A plain run renders the frames, warms up, times --steps steps and prints ONE JSON line on rank 0 (metric, value, unit,
ms_per_step, ...).  `--dump-outputs DIR` writes the detections of the last timed step as DIR/<name>.npy.  `--full` adds
  roofline        -- the threshold pass (the kernel BASELINE.json's metric names), HIP-event timed
  cpu_baseline    -- the CPU restatement (oracle/) timed on the host's cores on a bounded sample
  stage_roofline  -- achieved HBM fraction of the other streaming stages (algorithmic bytes of DESIGN.md section 4)
  extra           -- batch-size sweep, bgr8 input, H2D-included rate, single-frame latency, sigma 0, decimate 2
  parity_gate     -- every frame of the batch (and the stages of 16) against the CPU restatement
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec
NUM_STREAMS = 8        # BASELINE.json configs[3]
W, H = 1920, 1080
METRIC = "AprilTag detections fps @1080p tag36h11, 1/2/4/8 GPU; HBM GB/s on threshold pass"


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256, help="frames per step per GPU (BASELINE.md protocol sweeps 1, 8, 64, 256)")
    ap.add_argument("--distinct", type=int, default=256, help="distinct rendered frames per GPU (spread over its streams)")
    ap.add_argument("--sigma", type=float, default=2.0)
    ap.add_argument("--decimate", type=int, default=1)
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend; gloo is for the shared-GPU smoke only")
    ap.add_argument("--shared-gpu", action="store_true",
                    help="smoke only: ranks may share a device (local_rank %% device_count) when the box has fewer GPUs than ranks")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure stage times, rooflines, the CPU baseline and the informational rows, "
                         "and run the parity gate against the CPU restatement")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the detections of the last timed step as DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: no CPU baseline and no parity gate")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: no threshold-only roofline")
    ap.add_argument("--small-row", type=int, default=0, help=argparse.SUPPRESS)   # (internal: one row of the batch sweep, own process)
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the informational measurements (sweep, H2D, latency, sigma 0, decimate 2)")
    return ap.parse_args(argv)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def maybe_spawn(args):
    """`python bench.py --gpus N` without a launcher: become the launcher."""
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        sys.stdout.flush()
        os.execvpe(cmd[0], cmd, env)


def render_frames(seed, n, sigma):
    """n frames of the config-2 generator, seeds seed .. seed+n-1 (threads: the renderer is C behind ctypes)."""
    from concurrent.futures import ThreadPoolExecutor
    from isaac_ros_apriltag_amd import synth
    with ThreadPoolExecutor(max_workers=min(32, os.cpu_count() or 1)) as ex:
        imgs = list(ex.map(lambda i: synth.scene_c2(seed=seed + i, sigma=sigma)[0], range(n)))
    return np.stack(imgs)


DUMP_LIMIT_BYTES = 60 << 20      # under the 64 MB the outputs may take, .npy headers included


def dump_outputs(outdir, prep, prefix=""):
    """The records the timed amdAprilTagsDetectBatchEx call handed back (prep['out'] / prep['cnt'], before anything else runs
    on the handle): per-frame counts, and every detection in frame order with the library's order inside a frame, all in
    float64 (the integer fields are exact in it).  A batch that could exceed 64 MB at max_dets records per frame is cut to
    evenly spaced frames; `frame` keeps each record's index in the batch."""
    n, max_dets = prep["n"], prep["max_dets"]
    rec = np.ctypeslib.as_array(prep["out"]).reshape(n, max_dets)
    cnt = np.ctypeslib.as_array(prep["cnt"]).astype(np.int64)
    frame_bytes = 8 * (1 + max_dets * (5 + 9 + 2 + 8 + 9 + 3))     # count + float64 values of max_dets records, as written below
    frames = np.linspace(0, n - 1, min(n, DUMP_LIMIT_BYTES // frame_bytes)).astype(np.int64)
    keep = np.arange(max_dets)[None, :] < cnt[frames, None]
    r = rec[frames][keep]
    arrays = {"count": cnt[frames], "frame": frames[np.nonzero(keep)[0]], "family": r["family"], "id": r["id"],
              "hamming": r["hamming"], "decision_margin": r["decision_margin"], "H": r["H"].reshape(-1, 3, 3),
              "center": r["c"], "corners": r["p"], "R": r["R"].reshape(-1, 3, 3), "t": r["t"]}
    os.makedirs(outdir, exist_ok=True)
    for k, v in arrays.items():
        np.save(os.path.join(outdir, prefix + k + ".npy"), np.ascontiguousarray(v, dtype=np.float64))


def build_native_oracle():
    """CPU leg per SURVEY 8(d): the restatement compiled -O3 -march=native ON THIS BOX (a library built in the
    build container could use instructions this host lacks).  Falls back to the portable -O2 build."""
    out = os.path.join(ROOT, "oracle", "libapriltag_oracle_native.so")
    src = os.path.join(ROOT, "oracle", "apriltag_oracle.c")
    cmd = ["gcc", "-O3", "-march=native", "-fPIC", "-std=gnu99", "-ffp-contract=off", "-fno-fast-math", "-shared", "-o", out, src, "-lm"]
    try:
        subprocess.check_call(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return out, "-O3 -march=native (built on this host)"
    except Exception:
        return None, "-O2 (portable build)"


def cpu_baseline(frames, intr, decimate, tag_size, budget_s=15.0):
    """CPU restatement on a bounded sample, frame-parallel over the host cores (ctypes drops the GIL).
    frames: [n,H,W] uint8; intr: per-frame (fx, fy, cx, cy)."""
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import parity_util as pu
    from oracle import pyoracle as po
    native, flags = build_native_oracle()
    if native:
        po.use_library(native)
    po.lib()

    def run(i):
        fx, fy, cx, cy = intr[i]
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
        return po.detect(frames[i], params=pu.oracle_params(K, decimate, tag_size))[0]

    t0 = time.perf_counter()
    run(0)
    t1 = time.perf_counter() - t0
    cores = os.cpu_count() or 1
    n = int(max(cores, min(len(frames) * 4, budget_s * cores / max(t1, 1e-3))))
    idx = [i % len(frames) for i in range(n)]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=cores) as ex:
        res = list(ex.map(run, idx))
    dt = time.perf_counter() - t0
    byframe = dict(zip(idx, res))
    rec = {"value": round(n / dt, 2), "unit": "frames/s", "cores": cores, "kind": "port",
           "sample": "%d x 1080p frames (%d distinct) of the same workload, oracle/apriltag_oracle.c %s, %d threads "
                     "frame-parallel; single thread %.2f frames/s; CPU restatement of AprilRobotics apriltag_detect "
                     "(AprilRobotics' binary is not part of the reference)" % (n, len(byframe), flags, cores, 1.0 / t1),
           "single_thread_fps": round(1.0 / t1, 3)}
    # Second row: a CPU path that is trying -- the same restatement with upstream's own cheaper forms
    # (sequential double moment sums instead of the checker's 128-bit exact ones, float border dot) through cheaper code (radix
    # sort of the slope keys, AprilRobotics' quick_decode table instead of a scan over 587 x 4 codes): ATO_VAR_SEQ_MOMENTS |
    # ATO_VAR_FLOAT_DOT | ATO_VAR_FAST_PATHS.  Detections are compared with the checker's on the same frames.
    fast_var = po.VAR_SEQ_MOMENTS | po.VAR_FLOAT_DOT | po.VAR_FAST_PATHS

    def run_fast(i):
        fx, fy, cx, cy = intr[i]
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
        prm = pu.oracle_params(K, decimate, tag_size)
        prm.variant = fast_var
        return po.detect(frames[i], params=prm)[0]
    run_fast(0)                                   # (builds the decode table once)
    t0 = time.perf_counter()
    run_fast(0)
    t1f = time.perf_counter() - t0
    nf = int(max(cores, min(len(frames) * 4, 0.6 * budget_s * cores / max(t1f, 1e-3))))
    idxf = [i % len(frames) for i in range(nf)]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=cores) as ex:
        resf = list(ex.map(run_fast, idxf))
    dtf = time.perf_counter() - t0
    same = all(len(a) == len(byframe[i]) and all(x["id"] == y["id"] and x["hamming"] == y["hamming"] and np.abs(x["p"] - y["p"]).max() < 1e-6
                                                  for x, y in zip(a, byframe[i])) for i, a in zip(idxf, resf))
    rec["upstream_forms"] = {"value": round(nf / dtf, 2), "unit": "frames/s", "cores": cores, "single_thread_fps": round(1.0 / t1f, 3),
                             "kind": "port", "sample": "%d frames; sequential double moment sums + float border dot (upstream's statements, "
                             "ATO_VAR_SEQ_MOMENTS | ATO_VAR_FLOAT_DOT), radix-sorted slope keys, quick_decode hash table (ATO_VAR_FAST_PATHS)" % nf,
                             "detections_equal_checker_ids_hamming_corners_1e-6": bool(same)}
    # optional third row: a real libapriltag.so, if this host has one (never required)
    try:
        from oracle import aprilrobotics_xcheck as ax
        real = ax.time_and_compare(frames[:min(len(frames), 8)], byframe, decimate)
        if real is not None:
            rec["aprilrobotics_libapriltag"] = real
    except Exception as e:  # the cross-check must never break the bench
        rec["aprilrobotics_libapriltag"] = {"error": str(e)[:200]}
    return rec, byframe


def threshold_roofline(frames_dev, decimate, reps=20):
    """Threshold pass alone over a batch whose in+out footprint exceeds the 256 MiB LLC."""
    from isaac_ros_apriltag_amd.detector import AprilTagDetector
    nrep = int(np.ceil(160 / frames_dev.shape[0]))
    big = frames_dev.repeat(nrep, 1, 1)[:160].contiguous()
    nb = big.shape[0]
    det = AprilTagDetector(W, H, decimate=decimate, max_batch=nb, max_points=4096, hash_slots=256,
                           max_clusters=256, max_quads=64, max_detections=16, device=frames_dev.device.index)
    det.set_profiling(True)
    for _ in range(3):
        det.threshold_only(big)
    ms = []
    for _ in range(reps):
        det.threshold_only(big)
        ms.append(det.stage_ms()["threshold"])
    det.close()
    w, h = 1 + (W - 1) // decimate, 1 + (H - 1) // decimate
    alg_bytes = 2.0 * w * h * nb
    avg_ms = float(np.mean(ms))
    achieved = alg_bytes / (avg_ms * 1e-3) / 1e9
    # HBM traffic per launch comes from separate rocprofv3 --pmc passes of the same launch shape
    # (tools/thr_only.py; FETCH_SIZE doubled per the gfx950 note of MI355X_MICROARCH.md), committed under
    # profiles/; bench.py cannot collect PMC counters itself.
    traffic, traffic_src = None, None
    for name in ("r06_threshold_pmc.json", "r05_threshold_pmc.json", "r04_threshold_pmc.json", "r03_threshold_pmc.json", "r02_threshold_pmc.json", "r01_threshold_pmc.json"):
        pmc = os.path.join(ROOT, "profiles", name)
        if decimate == 1 and os.path.exists(pmc):
            rec = json.load(open(pmc))
            if rec.get("frames_per_launch") == nb:
                traffic, traffic_src = rec["traffic_bytes"], "profiles/" + name
                break
    return {"bound": "hbm", "kernel": "k_threshold<%d>" % decimate, "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
            "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_src,
            "bytes_per_launch": alg_bytes, "avg_launch_ms": round(avg_ms, 4), "min_launch_ms": round(float(np.min(ms)), 4),
            "frames_per_launch": nb, "footprint_mib": round((big.numel() * 2) / 2 ** 20, 1)}


STAGE_KERNELS = {"threshold": ("k_threshold",), "cc_local": ("k_cc_local",), "points": ("k_points",), "scatter": ("k_scatter",),
                 "fit_quads": ("k_fit_prefilter", "k_fit_quads", "k_fit_small", "k_quad_finish")}


def stage_rooflines(stage_ms, nframes, counts, decimate):
    """Achieved HBM rate of the streaming stages IN THE PIPELINE (HIP-event stage times of this run) from their MINIMAL
    algorithmic bytes, with the measured HBM traffic of the same kernels beside it (rocprofv3 --pmc FETCH_SIZE x 2 +
    WRITE_SIZE on the 32-frame pipeline, committed under profiles/; bench.py cannot collect PMC counters itself).
    Per frame of N working pixels, P raw boundary points, Pk points in kept clusters:
      threshold  read N, write N                                                          2 N
      cc_local   read N (threshold image), write 4 N (labels)                             5 N
      points     read N + 4 N, write 4 B per raw point (one staging word)                 5 N + 4 P
      scatter    read 4 P, write 4 Pk                                                     4 P + 4 Pk
      fit_quads  read 4 B per point + the four gray bytes of its gradient                 8 Pk
    Representative / size gathers (points), the offset gather (scatter) and the quad fit's cumulative-moment scratch
    (48 B per point written and read back) are NOT algorithmic: they show up in traffic_ratio."""
    w, h = 1 + (W - 1) // decimate, 1 + (H - 1) // decimate
    N = float(w * h)
    P, Pk = counts["npoints_raw"], counts["npoints_kept"]
    alg = {"threshold": 2 * N, "cc_local": 5 * N, "points": 5 * N + 4 * P, "scatter": 4 * P + 4 * Pk, "fit_quads": 8 * Pk}
    pmc, pmc_src = None, None
    for name in ("r06_pipeline_pmc.json", "r05_pipeline_pmc.json", "r04_pipeline_pmc.json", "r03_pipeline_pmc.json"):
        path = os.path.join(ROOT, "profiles", name)
        if decimate == 1 and os.path.exists(path):
            pmc, pmc_src = json.load(open(path)), "profiles/" + name
            break
    out = {}
    for k, b in alg.items():
        ms = stage_ms.get(k)
        if not (ms and ms > 0):
            continue
        gbs = b * nframes / (ms * 1e-3) / 1e9
        rec = {"ms": round(ms, 3), "alg_bytes": int(b), "GB/s": round(gbs, 1), "frac_of_8TBs": round(gbs / HBM_PEAK_GBS, 4),
               "traffic_bytes": None, "traffic_ratio": None, "traffic_source": None}
        if pmc:
            per_frame = 1024.0 / (pmc["frames"] * pmc.get("submissions", 1))
            t = 0.0
            for kn in STAGE_KERNELS[k]:
                kr = pmc["kernels"].get(kn)
                if kr:
                    t += (2.0 * kr.get("FETCH_SIZE", {}).get("sum_KB", 0.0) + kr.get("WRITE_SIZE", {}).get("sum_KB", 0.0)) * per_frame
            if t > 0:
                rec.update(traffic_bytes=int(t), traffic_ratio=round(t / b, 2), traffic_source=pmc_src)
        out[k] = rec
    return out


def main():
    args = parse_args()
    if args.small_row:
        return small_row_main(args)
    maybe_spawn(args)
    import torch
    import torch.distributed as dist
    from isaac_ros_apriltag_amd import streams
    from isaac_ros_apriltag_amd.detector import AprilTagDetector
    from isaac_ros_apriltag_amd import capi

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        sys.stderr.write("bench.py: WORLD_SIZE=%d but --gpus %d; refusing to report a line for the wrong GPU count\n" % (world, args.gpus))
        sys.exit(2)
    assert torch.cuda.is_available(), "bench.py needs a HIP device (no CPU fallback)"
    ndev = torch.cuda.device_count()
    if local_rank >= ndev and not args.shared_gpu:
        sys.stderr.write("bench.py: rank %d has no GPU of its own (%d visible); --shared-gpu exists for smoke runs only\n" % (local_rank, ndev))
        sys.exit(2)
    dev_index = local_rank % ndev
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    observed_world = 1
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if args.backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=args.backend)
        observed_world = dist.get_world_size()
    coll_dev = dev if args.backend == "nccl" else torch.device("cpu")

    # ---- streams: 8 (or the next multiple of world) packed round-robin onto the ranks ------------------
    nstreams = world * int(np.ceil(NUM_STREAMS / world))
    block = streams.make_param_block(nstreams, W, H, args.decimate) if rank == 0 else None
    block = streams.broadcast_param_block(block, nstreams, device=coll_dev)   # the one collective: RCCL broadcast of intrinsics
    mine = streams.assign_streams(nstreams, world, rank)
    spr = len(mine)                                   # streams on this rank
    per_stream_distinct = max(1, args.distinct // spr)
    per_stream_batch = max(1, args.batch // spr)
    B = per_stream_batch * spr
    frames_np, intr = [], []
    for s in mine:
        sp = streams.stream_params(block, s)
        fr = render_frames(int(sp["seed"]), per_stream_distinct, args.sigma)
        reps = int(np.ceil(per_stream_batch / per_stream_distinct))
        sel = np.tile(np.arange(per_stream_distinct), reps)[:per_stream_batch]
        frames_np.append(fr[sel])
        intr += [(sp["fx"], sp["fy"], sp["cx"], sp["cy"])] * per_stream_batch
    frames_np = np.concatenate(frames_np)             # [B,H,W]: the step's batch, frames of stream 0 first
    tag_size = streams.stream_params(block, mine[0])["tag_size"]
    batch = torch.from_numpy(frames_np).to(dev)

    det = AprilTagDetector(W, H, families=("tag36h11",), decimate=args.decimate, intrinsics=intr[0], tag_size=tag_size,
                           max_batch=B, device=dev_index)
    prep = det.prepare(batch, max_dets=64, intrinsics=intr)   # marshalling once; a step is exactly one blocking C-ABI call
    for _ in range(args.warmup):
        det.run_prepared(prep)

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    barrier()
    step_ms = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        ts = time.perf_counter()
        det.run_prepared(prep)
        step_ms.append((time.perf_counter() - ts) * 1e3)
    torch.cuda.synchronize()
    dt_own = time.perf_counter() - t0          # this rank's own K steps (no barrier inside): what a straggler shows up in
    barrier()
    dt = time.perf_counter() - t0
    out = det.unpack(prep)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, prep, "rank%d_" % rank if rank else "")
    rank_fps = [B * args.steps / dt_own]
    if world > 1:
        tt = torch.tensor([dt], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
        mine_t = torch.tensor([B * args.steps / dt_own], dtype=torch.float64, device=coll_dev)
        all_t = [torch.zeros_like(mine_t) for _ in range(world)]
        dist.all_gather(all_t, mine_t)
        rank_fps = [float(t.item()) for t in all_t]
    flags = det.frame_flags(B)
    if args.full:
        det.set_profiling(True)
        det.run_prepared(prep)
        stage_ms = det.stage_ms()
        counts = det.mean_counts(B)
        det.set_profiling(False)
    mem = det.device_bytes()

    # Parity gate in the same run: EVERY rank compares ALL frames of its batch with the CPU restatement (ids exact; corners,
    # rotation and translation bit-identical).  Rank 0 goes first and alone -- its pass over the frames is also the timed
    # cpu_baseline leg, on all host cores -- while the other ranks wait at a barrier (about 20 s on the driver's box, far
    # below the process group's timeout of 10 minutes (RCCL) / 30 minutes (gloo)); then the other ranks check their own
    # frames side by side, each on its share of the cores.
    gate_ok = True
    stage_gate = None
    byframe = None
    cpu_rec = None
    gated = 0
    if args.full and not args.no_cpu_baseline:
        if rank == 0:
            cpu_rec, byframe = cpu_baseline(frames_np, intr, args.decimate, tag_size)
        if world > 1:
            dist.barrier()
        if rank != 0:
            from concurrent.futures import ThreadPoolExecutor
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import parity_util as pu
            from oracle import pyoracle as po
            po.lib()

            def run(i):
                fx, fy, cx, cy = intr[i]
                K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
                return po.detect(frames_np[i], params=pu.oracle_params(K, args.decimate, tag_size))[0]
            # distinct frames only (the batch cycles through them); threads: this rank's share of the host cores
            distinct_idx = sorted({int(i) for s_ in range(spr) for i in (s_ * per_stream_batch + np.arange(min(per_stream_batch, per_stream_distinct)))})
            nthr = max(1, (os.cpu_count() or 1) // max(1, world - 1))
            with ThreadPoolExecutor(max_workers=nthr) as ex:
                byframe = dict(zip(distinct_idx, ex.map(run, distinct_idx)))
        for i, odets in byframe.items():
            g = out[i]
            gate_ok &= len(g) == len(odets) and all(
                a["id"] == b["id"] and np.array_equal(a["p"], b["p"]) and np.array_equal(a["R"], b["R"]) and np.array_equal(a["t"], b["t"])
                for a, b in zip(g, odets))
        gated = len(byframe)
        # ... and the STAGES of a sample of them: the ten tag detections of a frame say nothing about
        # the thousands of clusters that end as rejected quads or no quad at all, so for 16 evenly spaced frames of the batch
        # the library's threshold image, labels, cluster list and QUAD list (count and CRC of the sorted list: key, four float
        # corners, border direction) of the timed submission shape are compared with the oracle's dump of the same frame.
        from concurrent.futures import ThreadPoolExecutor
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import parity_util as pu
        from oracle import pyoracle as po
        keys = sorted(byframe)
        sample = [keys[int(round(j))] for j in np.linspace(0, len(keys) - 1, min(16, len(keys)))]

        def odigest(i):
            fx, fy, cx, cy = intr[i]
            K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
            return pu.stage_digest_oracle(po.detect(frames_np[i], params=pu.oracle_params(K, args.decimate, tag_size), want_dump=True)[1])
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
            odig = list(ex.map(odigest, sample))
        stage_bad = [i for i, od in zip(sample, odig) if pu.stage_digest_gpu(det, i) != od]
        stage_gate = {"frames": len(sample), "mismatches": len(stage_bad), "submission_path": det.last_submission_path(),
                      "quads_per_frame_mean": round(float(np.mean([d["nquads"] for d in odig])), 1)}
        gate_ok &= not stage_bad
    gated_all = [gated]
    if world > 1:
        gt = torch.tensor([1.0 if gate_ok else 0.0], dtype=torch.float64, device=coll_dev)
        dist.all_reduce(gt, op=dist.ReduceOp.MIN)
        gate_all = bool(gt.item() > 0.5)
        gm = torch.tensor([float(gated)], dtype=torch.float64, device=coll_dev)
        ga = [torch.zeros_like(gm) for _ in range(world)]
        dist.all_gather(ga, gm)
        gated_all = [int(t.item()) for t in ga]
    else:
        gate_all = gate_ok

    extra = {}
    if rank == 0 and args.full and not args.no_extra:
        extra = extra_measurements(det, batch, frames_np, intr, args, torch, dev, tag_size, dev_index)
    det.close()

    if rank == 0:
        fps = world * B * args.steps / dt
        ndet = [len(o) for o in out]
        rec = {
            "metric": METRIC,
            "value": round(fps, 1), "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u8 (threshold/CC/clustering), f64 (quad fit/decode/pose)", "data": "synthetic",
            "config": {"workload": "BASELINE.json configs[1] frames (1920x1080 mono8, 10 tag36h11 per frame, ids 0-9, background 150 + "
                                   "noise sigma=%g) arriving as configs[3]'s %d camera streams with distinct intrinsics, packed %d per GPU; "
                                   "%d distinct frames per GPU, device-resident" % (args.sigma, nstreams, spr, per_stream_distinct * spr),
                       "frames_per_step_per_gpu": B, "decimate": args.decimate, "streams": nstreams, "streams_per_gpu": spr,
                       "world_size_seen_by_%s" % ("rccl" if args.backend == "nccl" else args.backend): observed_world,
                       "parallelism": "%d independent streams, %d per GPU, RCCL broadcast of intrinsics only" % (nstreams, spr),
                       # every rank's own rate over its K steps (frames/s): a straggler GPU is visible here, `value` uses the max-over-ranks time
                       "per_rank_fps": {"min": round(min(rank_fps), 1), "max": round(max(rank_fps), 1), "mean": round(float(np.mean(rank_fps)), 1),
                                        "ranks": [round(v, 1) for v in rank_fps]}},
            "detections_per_frame": float(np.mean(ndet)), "frame_flags_nonzero": int(sum(1 for f in flags if f)),
            "step_ms_median": round(float(np.median(step_ms)), 3), "step_ms_min": round(float(np.min(step_ms)), 3),
            "fps_median_step": round(B / (float(np.median(step_ms)) * 1e-3), 1), "fps_best_step": round(B / (float(np.min(step_ms)) * 1e-3), 1),
            **({"stage_ms_per_step": {k: round(v, 3) for k, v in stage_ms.items()},
                "stage_roofline": stage_rooflines(stage_ms, B, counts, args.decimate),
                "frame_content_mean": counts} if args.full else {}),
            "device_bytes_handle": mem,
        }
        if extra:
            rec["extra"] = extra
        if cpu_rec is not None:
            rec["cpu_baseline"] = cpu_rec
        if args.full and not args.no_roofline:
            rec["roofline"] = threshold_roofline(batch[:min(B, 160)], args.decimate)
            thr = rec["stage_roofline"].get("threshold")
            if thr:   # the same kernel inside the timed pipeline (B frames, HIP-event stage time of this run)
                rec["roofline"]["in_pipeline"] = {"frames_per_launch": B, "ms": thr["ms"], "achieved": thr["GB/s"], "frac": thr["frac_of_8TBs"]}
        if byframe is not None:
            # correctness gate in the same run: ids exact; corners, rotation and translation bit-identical to the CPU restatement
            rec["parity_gate"] = "pass" if gate_all else "FAIL"      # AND over all ranks
            rec["parity_gate_frames_rank0"] = len(byframe)
            rec["parity_gate_frames_per_rank"] = gated_all
            # rank 0's stage-level sample (every rank runs its own; a mismatch anywhere fails parity_gate)
            rec["parity_gate_stages"] = stage_gate
        print(json.dumps(rec))
        sys.stdout.flush()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def small_handle_row(b, args, dev_index):
    """One row of the batch sweep in a process of its own (see extra_measurements): `python bench.py --small-row b`."""
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--small-row", str(b), "--sigma", str(args.sigma), "--decimate", str(args.decimate)]
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["BENCH_SMALL_ROW_DEVICE"] = str(dev_index)
    try:
        out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=300, check=True).stdout.decode()
        return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    except Exception as e:   # (informational row: never fails the bench line)
        sys.stderr.write("bench.py: small-handle row %d not measured in its own process (%r)\n" % (b, e))
        return None


def small_row_main(args):
    import torch
    from isaac_ros_apriltag_amd import streams
    from isaac_ros_apriltag_amd.detector import AprilTagDetector
    b = args.small_row
    dev_index = int(os.environ.get("BENCH_SMALL_ROW_DEVICE", "0"))
    torch.cuda.set_device(dev_index)
    block = streams.make_param_block(NUM_STREAMS, W, H, args.decimate)
    sp = streams.stream_params(block, 0)
    frames = torch.from_numpy(render_frames(int(sp["seed"]), b, args.sigma)).to(torch.device("cuda", dev_index))
    K = (sp["fx"], sp["fy"], sp["cx"], sp["cy"])
    det = AprilTagDetector(W, H, families=("tag36h11",), decimate=args.decimate, intrinsics=K, tag_size=sp["tag_size"], max_batch=b,
                           device=dev_index)
    p = det.prepare(frames, max_dets=64, intrinsics=[K] * b)
    for _ in range(5):
        det.run_prepared(p)
    ts = []
    for _ in range(max(3, min(100, 1024 // b))):
        t = time.perf_counter()
        det.run_prepared(p)
        ts.append(time.perf_counter() - t)
    nd = [len(d) for d in det.unpack(p)]
    det.close()
    print(json.dumps({"fps_median": round(b / float(np.median(ts)), 1), "ms_median": round(float(np.median(ts)) * 1e3, 3),
                      "ms_min": round(float(np.min(ts)) * 1e3, 3), "own_process": True, "detections_per_frame": float(np.mean(nd))}))


def extra_measurements(det, batch, frames_np, intr, args, torch, dev, tag_size, dev_index):
    """Informational rows of BASELINE.md's protocol; none of them is `value`."""
    from isaac_ros_apriltag_amd.detector import AprilTagDetector
    ex = {}
    B = batch.shape[0]
    # batch-size sweep (frames of stream 0 first, so small batches are one stream).  64 and 256 frames run on the step's handle.  One
    # and eight frames -- one camera, eight cameras: the live shapes -- run on a handle of their own size IN A PROCESS OF THEIR OWN, as
    # a node holds it: a handle of up to eight frames replays captured launch graphs on plain streams, a throughput-sized one has
    # prioritised side streams (csrc/detector.hip), and on this runtime a small handle created after a prioritised one in the same
    # process finds its graph branches on that handle's hardware queues (0.49 against 0.38 ms per frame; INTEGRATION.md, "stream
    # priorities"; the row measured that way is kept beside it as same_process_ms_median).
    sweep = {}
    def timed(dsw, b, reps):
        p = dsw.prepare(batch[:b], max_dets=64, intrinsics=intr[:b])
        dsw.run_prepared(p)
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            dsw.run_prepared(p)
            ts.append(time.perf_counter() - t)
        return ts
    for b in (1, 8, 64, 256):
        if b > B:
            continue
        reps = max(3, min(40, 512 // b))
        row = None
        if b <= 8:
            dsw = AprilTagDetector(W, H, families=("tag36h11",), decimate=args.decimate, intrinsics=intr[0], tag_size=tag_size,
                                   max_batch=b, device=dev_index)
            same = float(np.median(timed(dsw, b, reps))) * 1e3
            dsw.close()
            row = small_handle_row(b, args, dev_index)
            if row is not None:
                row["same_process_ms_median"] = round(same, 3)
            else:
                row = {"fps_median": round(b / (same * 1e-3), 1), "ms_median": round(same, 3), "ms_min": None, "own_process": False}
        else:
            ts = timed(det, b, reps)
            row = {"fps_median": round(b / float(np.median(ts)), 1), "ms_median": round(float(np.median(ts)) * 1e3, 3),
                   "ms_min": round(float(np.min(ts)) * 1e3, 3)}
        sweep[str(b)] = row
    ex["batch_sweep"] = sweep
    # the reference's own input format (its cuAprilTags branch takes rgb8 / bgr8 uchar3 frames, src/apriltag_node.cpp:469-486): the
    # same B frames as bgr8 -- the gray value in all three channels, so that the BT.601 statement gives the mono8 frame back exactly
    # and the records must equal the mono8 run's -- through amdAprilTagsDetectBatchColorEx, whose threshold pass reads the interleaved
    # frame, writes the gray plane and thresholds in one launch: 3 N read + 2 N written per frame
    if args.decimate == 1:
        try:
            bgr = batch.unsqueeze(-1).expand(-1, -1, -1, 3).contiguous()
            pm = det.prepare(batch, max_dets=64, intrinsics=intr)
            det.run_prepared(pm)
            ref = det.unpack(pm)
            pc = det.prepare(bgr, max_dets=64, intrinsics=intr, encoding="bgr8")
            det.run_prepared(pc)
            got = det.unpack(pc)
            same = len(ref) == len(got) and all(len(a) == len(b) and all(x["id"] == y["id"] and np.array_equal(x["p"], y["p"]) and np.array_equal(x["R"], y["R"])
                                                                       for x, y in zip(a, b)) for a, b in zip(ref, got))
            tm, tc = [], []
            for _ in range(5):
                t = time.perf_counter(); det.run_prepared(pm); tm.append(time.perf_counter() - t)
                t = time.perf_counter(); det.run_prepared(pc); tc.append(time.perf_counter() - t)
            det.set_profiling(True)
            det.run_prepared(pc)
            thr_ms = det.stage_ms()["threshold"]
            det.set_profiling(False)
            N = float(W * H)
            gbs = 5.0 * N * B / (thr_ms * 1e-3) / 1e9
            row = {"fps_median": round(B / float(np.median(tc)), 1), "ms_median": round(float(np.median(tc)) * 1e3, 3),
                   "mono8_ms_median_same_loop": round(float(np.median(tm)) * 1e3, 3),
                   "vs_mono8": round(float(np.median(tm)) / float(np.median(tc)), 4), "records_equal_mono8_run": bool(same),
                   "threshold_pass_in_pipeline": {"kernel": "k_threshold<1, bgr8>", "ms": round(thr_ms, 4), "alg_bytes_per_frame": int(5 * N),
                                                  "GB/s": round(gbs, 1), "frac_of_8TBs": round(gbs / HBM_PEAK_GBS, 4)}}
            del bgr, pc
            # the colour threshold launch alone, 160 frames per launch like the mono8 roofline measurement (995 MB in, 663 MB out)
            nb = 160
            big = batch.repeat(int(np.ceil(nb / B)), 1, 1)[:nb].unsqueeze(-1).expand(-1, -1, -1, 3).contiguous()
            dt = AprilTagDetector(W, H, max_batch=nb, max_points=4096, hash_slots=256, max_clusters=256, max_quads=64, max_detections=16,
                                  device=dev_index)
            dt.set_profiling(True)
            for _ in range(3):
                dt.threshold_only(big, encoding="bgr8")
            ms = []
            for _ in range(12):
                dt.threshold_only(big, encoding="bgr8")
                ms.append(dt.stage_ms()["threshold"])
            dt.close()
            del big
            g2 = 5.0 * N * nb / (float(np.mean(ms)) * 1e-3) / 1e9
            row["threshold_pass_alone"] = {"frames_per_launch": nb, "avg_launch_ms": round(float(np.mean(ms)), 4), "min_launch_ms": round(float(np.min(ms)), 4),
                                           "bytes_per_launch": 5.0 * N * nb, "GB/s": round(g2, 1), "frac_of_8TBs": round(g2 / HBM_PEAK_GBS, 4)}
            ex["bgr8_input"] = row
        except Exception as e:   # (informational row: never in the way of the line)
            ex["bgr8_input"] = {"error": repr(e)[:300]}
    # H2D-included: the same B frames start in pinned host memory every step.  (a) serial: copy, then detect;
    # (b) double-buffered: the copy of step k+1 runs on a side stream while the blocking call of step k computes
    host = torch.from_numpy(frames_np).pin_memory()
    bufs = [torch.empty_like(batch), torch.empty_like(batch)]
    preps = [det.prepare(b, max_dets=64, intrinsics=intr) for b in bufs]
    ts = []
    for _ in range(4):
        t = time.perf_counter()
        bufs[0].copy_(host, non_blocking=True)
        torch.cuda.synchronize()
        det.run_prepared(preps[0])
        ts.append(time.perf_counter() - t)
    ex["fps_h2d_included"] = round(B / float(np.median(ts[1:])), 1)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        bufs[0].copy_(host, non_blocking=True)
    side.synchronize()
    nsteps = 6
    t = time.perf_counter()
    for k in range(nsteps):
        det.submit_prepared(preps[k & 1])                         # amdAprilTagsSubmitBatch: this step's frames, returns at once
        with torch.cuda.stream(side):
            bufs[(k + 1) & 1].copy_(host, non_blocking=True)     # next step's frames over PCIe meanwhile
        det.wait_prepared(preps[k & 1])                           # amdAprilTagsWaitBatchEx
        side.synchronize()
    ex["fps_h2d_included_double_buffered"] = round(nsteps * B / (time.perf_counter() - t), 1)
    t = time.perf_counter()
    bufs[0].copy_(host, non_blocking=True)
    torch.cuda.synchronize()
    ex["h2d_GBs"] = round(host.numel() / (time.perf_counter() - t) / 1e9, 2)
    # same scenes without background noise, and the noisy frames at AprilRobotics' default quad_decimate = 2
    if args.sigma > 0:
        cf = render_frames(1234, 8, 0.0)
        cb = torch.from_numpy(cf).to(dev).repeat(int(np.ceil(B / 8)), 1, 1)[:B].contiguous()
        cp = det.prepare(cb, max_dets=64, intrinsics=intr)
        det.run_prepared(cp)
        t = time.perf_counter()
        for _ in range(3):
            det.run_prepared(cp)
        ex["fps_same_scenes_sigma0"] = round(3 * B / (time.perf_counter() - t), 1)
    if args.decimate == 1:
        d2 = AprilTagDetector(W, H, families=("tag36h11",), decimate=2, intrinsics=intr[0], tag_size=tag_size, max_batch=B, device=dev_index)
        p2 = d2.prepare(batch, max_dets=64, intrinsics=intr)
        d2.run_prepared(p2)
        t = time.perf_counter()
        for _ in range(3):
            d2.run_prepared(p2)
        ex["fps_same_frames_decimate2"] = round(3 * B / (time.perf_counter() - t), 1)
        d2.close()
    return ex


if __name__ == "__main__":
    main()
