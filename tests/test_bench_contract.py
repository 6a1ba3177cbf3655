"""The driver contract of bench.py, exercised end-to-end on CPU
(DTP_BENCH_CPU=1): the exact torchrun launch line the benchmark driver
uses, env rendezvous, parameter broadcast, timed loop, and the single
JSON result line with all required fields."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup",
            "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"]


def _run_bench(nproc, extra=()):
    from dist_tuto_pth_amd.dist import _free_port
    env = dict(os.environ)
    env["DTP_BENCH_CPU"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), "bench.py",
           "--gpus", str(nproc), "--steps", "3", "--warmup", "1",
           "--batch", "8", *extra]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout  # exactly ONE JSON line (rank 0)
    return json.loads(lines[0])


@pytest.mark.timeout(300)
def test_bench_torchrun_world2_json_contract():
    d = _run_bench(2)
    for k in REQUIRED:
        assert k in d, k
    assert d["n_gpus"] == 2
    assert d["steps"] == 3 and d["warmup"] == 1
    assert d["metric"] == "ConvNet samples/sec"
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["data"] == "synthetic"
    assert d["config"]["global_batch"] == 16        # 8 per rank, weak
    assert d["config"]["parallelism"] == "dp2"
    assert d["value"] > 0 and d["ms_per_step"] > 0


@pytest.mark.timeout(420)
def test_bench_torchrun_world8_json_contract():
    """First-shot hardening for the driver's 8-GPU node (VERDICT r1
    #7): the exact torchrun launch line at world 8, on CPU."""
    d = _run_bench(8)
    assert d["n_gpus"] == 8
    assert d["config"]["global_batch"] == 64
    assert d["config"]["parallelism"] == "dp8"
    assert d["value"] > 0


@pytest.mark.timeout(420)
def test_bench_torchrun_world8_ddp_mode():
    d = _run_bench(8, extra=("--mode", "ddp"))
    assert d["n_gpus"] == 8
    assert d["config"]["grad_sync"] == "ddp"


@pytest.mark.timeout(300)
def test_bench_allreduce_world4_args_cpu():
    """bench_allreduce's torchrun arg/env path must be launch-clean.
    DTP_BENCH_CPU=1 runs the same rendezvous + arg parsing and times
    the gloo all-reduce (the rccl/fullmesh/ring algos need GPUs)."""
    from dist_tuto_pth_amd.dist import _free_port
    env = dict(os.environ)
    env["DTP_BENCH_CPU"] = "1"
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           "--nproc-per-node=4", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()),
           "benchmarks/bench_allreduce.py", "--size-mb", "1",
           "--iters", "2", "--warmup", "1", "--pipeline-depth", "3",
           "--algos", "rccl"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True,
                         text=True, timeout=240)
    assert out.returncode == 0, (out.stdout[-1000:], out.stderr[-2000:])
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 4
    assert "rccl" in d["results"]


def test_bench_single_process_json():
    env = dict(os.environ)
    env["DTP_BENCH_CPU"] = "1"
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
         "--batch", "8"],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=180)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads([ln for ln in out.stdout.splitlines()
                    if ln.startswith("{")][-1])
    assert d["n_gpus"] == 1


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes, as float32 .npy files, the loss and the
    updated state of one step through the timed path taken from the
    seeded initial state, so the arrays depend on neither run nor step
    count (bit for bit on CPU, where summation order is fixed).  --full
    is accepted and leaves the result line's meaning alone."""
    import numpy as np
    env = dict(os.environ)
    env["DTP_BENCH_CPU"] = "1"
    results = []
    for name, steps, extra in (("a", 2, []), ("b", 3, ["--full"])):
        out = subprocess.run(
            [sys.executable, "bench.py", "--gpus", "1", "--steps",
             str(steps), "--warmup", "1", "--batch", "8", "--dump-outputs",
             str(tmp_path / name), *extra],
            cwd=ROOT, env=env, capture_output=True, text=True, timeout=180)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out.stdout
        results.append(json.loads(lines[0]))
    for d, steps in zip(results, (2, 3)):
        for k in REQUIRED:
            assert k in d, k
        assert d["steps"] == steps and d["ms_per_step"] > 0
        assert d["metric"] == "ConvNet samples/sec"
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted(p.name for p in (tmp_path / "b").iterdir())
    assert "loss.npy" in files
    for layer in ("conv1", "conv2", "fc1", "fc2"):
        for kind in ("param", "grad", "momentum"):
            assert f"{kind}.{layer}.weight.npy" in files
            assert f"{kind}.{layer}.bias.npy" in files
    total = 0
    for f in files:
        a = np.load(tmp_path / "a" / f)
        b = np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and np.isfinite(a).all(), f
        assert np.array_equal(a, b), f
        total += a.nbytes
    assert total <= 64 << 20
    # the dumped step really trained: its momentum buffer is the gradient
    mom = np.load(tmp_path / "a" / "momentum.fc2.weight.npy")
    assert np.abs(mom).max() > 0
