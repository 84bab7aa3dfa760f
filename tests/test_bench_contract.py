"""bench.py driver-contract tests: JSON schema, single- and multi-process."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

REQUIRED_KEYS = {
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
}


def _last_json_line(out: str) -> dict:
    lines = [ln for ln in out.strip().splitlines() if ln.startswith("{")]
    assert lines, f"no JSON line in output:\n{out[-2000:]}"
    return json.loads(lines[-1])


def test_bench_single_process_contract():
    proc = subprocess.run(
        [sys.executable, "bench.py", "--steps", "2", "--warmup", "1",
         "--scale", "tiny", "--windows", "1", "--batch-windows", "1"],
        cwd=ROOT, capture_output=True, text=True, timeout=900,
    )
    assert proc.returncode == 0, proc.stderr[-2000:]
    res = _last_json_line(proc.stdout)
    assert REQUIRED_KEYS <= set(res)
    assert res["n_gpus"] == 1
    assert res["value"] > 0
    assert res["scaling"] == "weak"
    assert res["higher_is_better"] is True
    assert res["config"]["parallelism"] == "dp1"
    assert res["data"] == "synthetic"


def _run_dump(out_dir, *extra):
    proc = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "1", "--warmup", "0",
         "--scale", "tiny", "--windows", "1", "--batch-windows", "1",
         "--dump-outputs", str(out_dir), *extra],
        cwd=ROOT, capture_output=True, text=True, timeout=900,
    )
    assert proc.returncode == 0, proc.stderr[-2000:]
    return _last_json_line(proc.stdout)


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last timed step's outputs as float .npy
    files, identical inputs give matching outputs from run to run, and
    --full keeps the plain result line's meaning."""
    import numpy as np

    res_a = _run_dump(tmp_path / "a")
    res_b = _run_dump(tmp_path / "b", "--full")
    for res in (res_a, res_b):
        assert REQUIRED_KEYS <= set(res)
        assert res["steps"] == 1 and res["ms_per_step"] > 0
        assert res["metric"] == "trace_events_per_sec_graphsage_lstm_train"
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == sorted(p.name for p in (tmp_path / "b").iterdir())
    assert {"node_logit.npy", "edge_logit.npy", "seq_logit.npy",
            "loss_total.npy", "params.npy"} <= set(names)
    total = 0
    for name in names:
        a = np.load(tmp_path / "a" / name)
        b = np.load(tmp_path / "b" / name)
        total += a.nbytes
        assert a.dtype in (np.float32, np.float64) and a.size > 0
        assert a.shape == b.shape and np.isfinite(a).all()
        if name.endswith("_logit.npy"):
            # steps=1, warmup=0: logits are a pure forward function of the
            # seeded weights and inputs.  Another seed moves them by O(1) of
            # their range; summation order in bf16 by a few 2^-8 of it.
            assert np.abs(a - b).max() <= 0.05 * np.abs(a).max(), name
    assert total <= 64 * 1000 * 1000


def test_dump_outputs_caps_with_fixed_sample(tmp_path, monkeypatch):
    import numpy as np
    import torch

    import bench

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 2 * (1000 + 64))
    big = torch.arange(5000, dtype=torch.float64)
    small = torch.ones(3, 4, dtype=torch.bfloat16)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    x, y = np.load(tmp_path / "x" / "big.npy"), np.load(tmp_path / "y" / "big.npy")
    assert x.dtype == np.float32 and x.shape == (1000,)
    assert np.array_equal(x, y) and np.all(np.diff(x) > 0)  # same seeded subset
    assert np.array_equal(np.load(tmp_path / "x" / "small.npy"), np.ones(12, np.float32))


@pytest.mark.timeout(900)
def test_bench_torchrun_world2_gloo():
    """The driver's multi-rank launch shape, on CPU with gloo (world=2)."""
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    proc = subprocess.run(
        [
            sys.executable, "-m", "torch.distributed.run",
            "--nnodes=1", "--nproc-per-node", "2",
            "--master-addr", "127.0.0.1", "--master-port", "29517",
            "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1",
            "--scale", "tiny", "--windows", "1", "--batch-windows", "1",
        ],
        cwd=ROOT, capture_output=True, text=True, timeout=800, env=env,
    )
    assert proc.returncode == 0, proc.stderr[-3000:]
    res = _last_json_line(proc.stdout)
    assert res["n_gpus"] == 2
    assert res["config"]["parallelism"] == "dp2"
    assert res["value"] > 0


def test_bench_torchrun_world4_gloo():
    """World-4 launch contract: the 8-GPU driver run
    differs from world-2 only in degree; exercise a deeper rank fan-out on
    gloo so bucket-order determinism holds beyond the pairwise case."""
    env = dict(os.environ)
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    proc = subprocess.run(
        [
            sys.executable, "-m", "torch.distributed.run",
            "--nnodes=1", "--nproc-per-node", "4",
            "--master-addr", "127.0.0.1", "--master-port", "29519",
            "bench.py", "--gpus", "4", "--steps", "2", "--warmup", "1",
            "--scale", "tiny", "--windows", "1", "--batch-windows", "1",
        ],
        cwd=ROOT, capture_output=True, text=True, timeout=1200, env=env,
    )
    assert proc.returncode == 0, proc.stderr[-3000:]
    res = _last_json_line(proc.stdout)
    assert res["n_gpus"] == 4
    assert res["config"]["parallelism"] == "dp4"
    assert res["value"] > 0
