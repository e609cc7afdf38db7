"""bench.py's plain run, --dump-outputs and --full: the option parsing and
the output writer on the CPU, one plain run on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY_KEYS = ("roofline", "kernel_breakdown", "strong_scaling", "dropout_on", "adjacency_feed", "callers",
                  "bf16_mode", "fp16_mode", "real_density_c92", "strong_split_one_gpu", "end_to_end_run_epoch",
                  "cpu_baseline", "ms_per_step_event_instrumented")


def test_dump_outputs_writes_float32_and_a_fixed_sample(tmp_path):
    import bench
    small = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    rows = 4 * bench.DUMP_ARRAY_MAX_BYTES // (1024 * 4)          # four times the per-array limit
    big = torch.arange(rows * 1024, dtype=torch.float32).reshape(rows, 1024)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big})
    a, b = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert a.dtype == np.float32 and np.array_equal(a, small.numpy())
    assert b.dtype == np.float32 and b.nbytes == bench.DUMP_ARRAY_MAX_BYTES and b.shape == (rows // 4, 1024)
    # whole rows of the source, in their order, and the same rows in every run
    first = (b[:, 0] / 1024).astype(np.int64)
    assert np.all(np.diff(first) > 0) and np.array_equal(b, big.numpy()[first])
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))
    bench.dump_outputs(str(tmp_path / "a"), {"small": small}, rank=1)
    assert np.array_equal(np.load(tmp_path / "a" / "rank1_small.npy"), a)


def test_bench_refuses_zero_steps():
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "0", "--warmup", "1"], cwd=ROOT,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr, (r.returncode, r.stderr[-2000:])


@pytest.mark.gpu
def test_plain_bench_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run prints the headline line without any --full leg and
    --dump-outputs writes the last timed step's arrays: float32, the shapes of
    config 3 (h_T and dL/dh0 sampled to 128 graphs), finite, below 64 MB."""
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    res = json.loads(lines[0])
    assert all(k in res for k in HEADLINE_KEYS) and not [k for k in FULL_ONLY_KEYS if k in res], sorted(res)
    assert res["steps"] == 3 and res["warmup"] == 1 and res["full"] is False and res["n_gpus"] == 1
    assert res["unit"] == "graphs/s" and res["higher_is_better"] is True and res["dtype"] == "fp32"
    assert res["ms_per_step"] > 0 and abs(res["value"] - 256 / (res["ms_per_step"] * 1e-3)) <= 1e-6 * res["value"]
    h, C = 256, 8
    shapes = {"hT": (128, 128, h), "dh0": (128, 128, h),
              "edge_weights": (C, h, h), "edge_biases": (C, 1, h), "gates_kernel": (2 * h, 2 * h),
              "gates_bias": (2 * h,), "candidate_kernel": (2 * h, h), "candidate_bias": (h,)}
    want = {k: s for k, s in shapes.items() if k in ("hT", "dh0")}
    for k, s in shapes.items():
        if k not in want:
            want["grad_" + k] = want["weight_" + k] = s
    assert sorted(os.listdir(out)) == sorted(k + ".npy" for k in want)
    total = 0
    for k, s in want.items():
        x = np.load(out / (k + ".npy"))
        total += x.nbytes
        assert x.dtype == np.float32 and x.shape == s and np.isfinite(x).all() and np.abs(x).max() > 0, k
    assert total <= 64e6
