"""bench.py must never report a line for a GPU count it did not run on (round-1 verdict: `--gpus 8` silently ran one rank
and printed n_gpus: 1).  No GPU needed: the refusal happens before any device is touched."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_world_size_mismatch_is_refused():
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2
    assert "refusing" in r.stderr and r.stdout.strip() == ""


def test_self_spawn_command_line():
    """Without a launcher, --gpus N re-executes under torch.distributed.run with N ranks on 127.0.0.1."""
    sys.path.insert(0, ROOT)
    import bench
    captured = {}

    def fake_exec(path, argv, env):
        captured["argv"] = argv
        captured["env"] = env
        raise SystemExit(0)
    old, old_argv = os.execvpe, sys.argv
    env_backup = os.environ.pop("WORLD_SIZE", None)
    try:
        os.execvpe = fake_exec
        sys.argv = ["bench.py", "--gpus", "4", "--steps", "3"]
        try:
            bench.maybe_spawn(bench.parse_args(["--gpus", "4", "--steps", "3"]))
        except SystemExit:
            pass
    finally:
        os.execvpe, sys.argv = old, old_argv
        if env_backup is not None:
            os.environ["WORLD_SIZE"] = env_backup
    a = captured["argv"]
    assert "torch.distributed.run" in a and a[a.index("--nproc-per-node") + 1] == "4"
    assert a[a.index("--master-addr") + 1] == "127.0.0.1" and a[-4:] == ["--gpus", "4", "--steps", "3"]
    assert captured["env"].get("HSA_ENABLE_IPC_MODE_LEGACY") == "0"
    # one GPU: no spawn
    assert bench.maybe_spawn(bench.parse_args(["--gpus", "1"])) is None


def test_plain_run_is_the_default_and_dump_is_float64(tmp_path):
    """--full is off unless asked for; --dump-outputs writes the records of the prepared submission, frame by frame in the
    library's order, as float64 arrays, and cuts a batch that could exceed 64 MB to evenly spaced frames."""
    import ctypes
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from isaac_ros_apriltag_amd import capi
    a = bench.parse_args(["--steps", "7", "--dump-outputs", str(tmp_path)])
    assert not a.full and a.steps == 7 and a.dump_outputs == str(tmp_path)
    assert bench.parse_args(["--full"]).full
    n, md = 3, 4
    out = (capi.DetectionEx * (n * md))()
    cnt = (ctypes.c_uint32 * n)(2, 0, 1)
    for f, i, tid in ((0, 0, 5), (0, 1, 3), (2, 0, 9)):
        r = out[f * md + i]
        r.id, r.hamming, r.decision_margin = tid, 1, 0.5 * tid
        r.p[3][1], r.R[8], r.t[2] = 10.0 + tid, 1.0, 2.0 * tid
    out[1 * md].id = 77                                  # beyond frame 1's count: not a record
    bench.dump_outputs(str(tmp_path), {"n": n, "max_dets": md, "out": out, "cnt": cnt})
    ld = {k: np.load(str(tmp_path / (k + ".npy"))) for k in ("count", "frame", "id", "hamming", "decision_margin", "corners", "R", "t", "H", "center", "family")}
    assert all(v.dtype == np.float64 for v in ld.values())
    assert ld["count"].tolist() == [2, 0, 1] and ld["frame"].tolist() == [0, 0, 2] and ld["id"].tolist() == [5, 3, 9]
    assert ld["corners"].shape == (3, 4, 2) and ld["corners"][:, 3, 1].tolist() == [15.0, 13.0, 19.0]
    assert ld["R"].shape == (3, 3, 3) and ld["t"][:, 2].tolist() == [10.0, 6.0, 18.0]
    assert ld["decision_margin"].tolist() == [2.5, 1.5, 4.5] and ld["H"].shape == (3, 3, 3) and ld["center"].shape == (3, 2)
    # a batch whose records could exceed the limit: fixed, evenly spaced frames, under 64 MB in all
    n = 4000
    big = (capi.DetectionEx * (n * 64))()
    bench.dump_outputs(str(tmp_path / "big"), {"n": n, "max_dets": 64, "out": big, "cnt": (ctypes.c_uint32 * n)(*([64] * n))})
    total = sum(os.path.getsize(str(p)) for p in (tmp_path / "big").iterdir())
    kept = np.load(str(tmp_path / "big" / "count.npy")).size
    assert total <= 64 << 20 and 0 < kept < n
    assert np.array_equal(np.unique(np.load(str(tmp_path / "big" / "frame.npy"))), np.linspace(0, n - 1, kept).astype(np.int64))
