"""bench.py's multi-rank contract on the CPU (VERDICT r4 "Next round" #4).

`bench.py --gpus N` must never silently measure one GPU: without WORLD_SIZE it starts N rank
processes itself (before anything touches a GPU), under torch.distributed.run WORLD_SIZE must
equal --gpus.  Both launch forms are run here with the CPU plumbing session (`--device cpu`,
gloo), and the JSON's aggregate is checked against its own clock: value = N * steps over the
slowest rank's timed region."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
ARGS = ["--device", "cpu", "--steps", "6", "--warmup", "1", "--width", "256", "--height", "144",
        "--bitrate-kbps", "800"]


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _env():
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def _check(r, n):
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 prints exactly one JSON line
    out = json.loads(lines[0])
    assert out["n_gpus"] == n and out["config"]["global_batch"] == n and out["device"] == "cpu"
    steps = out["steps"]
    assert out["value"] == pytest.approx(n * steps / (out["ms_per_step"] * steps / 1000.0), rel=2e-3)
    assert out["encoded_fps_per_gpu"] == pytest.approx(out["value"] / n, rel=1e-3)
    return out


def test_bench_self_launches_ranks_without_world_size():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--full"] + ARGS, cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=300)
    out = _check(r, 2)
    # (the density probe runs with --full)
    # the node metric is every rank's own measured density, summed (VERDICT r5 weak #3b)
    by_rank = out["sessions_per_gpu_measured_by_rank"]
    assert len(by_rank) == 2 and all(isinstance(k, int) for k in by_rank)
    assert out["sessions_per_node_measured"] == sum(by_rank)
    assert out["sessions_per_gpu_measured_min"] == min(by_rank) and out["sessions_per_gpu_measured_max"] == max(by_rank)


def test_bench_rank_failure_stops_the_job():
    """A rank that dies before the rendezvous must not leave the others blocked in it: the
    self-launcher polls every child, stops the rest and returns the failing code."""
    import time

    env = dict(_env(), MXDESK_BENCH_FAIL_RANK="1")
    t0 = time.monotonic()
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2"] + ARGS, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=200)
    assert r.returncode == 3 and "stopping the others" in r.stderr
    assert time.monotonic() - t0 < 120


def test_bench_under_torchrun():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr=127.0.0.1", f"--master-port={_free_port()}", str(ROOT / "bench.py"), "--gpus", "2"] + ARGS
    r = subprocess.run(cmd, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=300)
    _check(r, 2)


def test_bench_rejects_gpus_world_size_mismatch():
    env = dict(_env(), WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "4"] + ARGS, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]


def test_bench_single_gpu_default():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py")] + ARGS, cwd=ROOT, env=_env(),
                       capture_output=True, text=True, timeout=300)
    out = _check(r, 1)
    assert out["mean_psnr_y_db"] > 30
    # a plain run times its steps only: no probe ran
    assert out["full"] is False and out["density_probe"] is None and out["sessions_per_node_measured"] is None


def test_bench_dump_outputs_is_reproducible(tmp_path):
    """--dump-outputs: float .npy files of what the last timed step produced, the same from run to
    run (the barcode's clock follows the frame number), and --steps sets the timed steps."""
    import numpy as np

    dumps = []
    for d in (tmp_path / "a", tmp_path / "b"):
        r = subprocess.run([sys.executable, str(ROOT / "bench.py")] + ARGS + ["--dump-outputs", str(d)], cwd=ROOT,
                           env=_env(), capture_output=True, text=True, timeout=300)
        out = _check(r, 1)
        dumps.append({p.stem: np.load(p) for p in sorted(d.glob("*.npy"))})
    a, b = dumps
    assert set(a) == set(b) == {"au", "au_bytes", "qp", "frame_id", "psnr", "recon_y", "recon_uv"}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    steps = out["steps"]
    assert steps == 6 and a["au_bytes"].shape == (steps,) and a["psnr"].shape == (steps, 3)
    assert a["au"].size == a["au_bytes"][-1] and a["recon_y"].shape[0] >= 144 and a["recon_y"].shape[1] >= 256
    for k in a:
        assert np.array_equal(a[k], b[k]), k
