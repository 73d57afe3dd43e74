"""bench.py's contract on a real GPU: one JSON line on stdout with the fields the driver reads, the roofline and CPU-baseline
objects, the torch.distributed code path over a 1-rank RCCL group (GCGCN_FORCE_DIST=1: communicator, coalesced all-reduce of the
four flat gradient tensors after every replayed step, barrier, MAX over ranks), the strong-scaling flag, and the WHOLE N > 1
control flow with two ranks (``--gpus 2 --dist-backend gloo``: both ranks share the test box's one card and the collectives travel
over gloo -- every rank must issue the same collective sequence from start to finish or the run hangs).  Run as child processes,
like the driver runs it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None, timeout=300):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, env=e, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, f"stdout must carry exactly one line, got {len(lines)}"
    return json.loads(lines[0])


def test_bench_line_contract(gpu_device):
    d = _run(["--config", "c1", "--steps", "6", "--warmup", "2", "--full"])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2 and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f32" and d["data"] == "synthetic" and d["higher_is_better"] is True and d["unit"] == "docs/s"
    assert "workload" in d["config"] and "model" not in d["config"] and d["config"]["mode"] == "graph"
    assert abs(d["value"] - 8 * 1e3 / d["ms_per_step"]) / d["value"] < 1e-3                 # docs/s = B / step time
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["bound"] in ("hbm", "mfma") and 0 < rf["frac"] < 1 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 2e-3
    assert "after" in rf["sampled_on"]                                                    # the timed region itself carries no events
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "documents" in cb["sample"]


def test_bench_plain_run_is_the_headline_and_dumps_the_last_step(gpu_device, tmp_path):
    """Without --full the line carries the headline figure and nothing measured outside the timed region; --dump-outputs
    writes the output and every gradient of the last timed step, float32, within 64 MB, the same elements on every run."""
    runs = []
    for r in range(2):
        d = _run(["--config", "c1", "--steps", "5", "--warmup", "1", "--dump-outputs", str(tmp_path / str(r))])
        assert d["steps"] == 5 and d["ms_per_step"] > 0 and abs(d["value"] - 8 * 1e3 / d["ms_per_step"]) / d["value"] < 1e-3
        for k in ("roofline", "roofline_hbm", "time_shares_ms_per_step", "extra", "cpu_baseline"):
            assert k not in d, k
        runs.append({f: np.load(tmp_path / str(r) / f) for f in sorted(os.listdir(tmp_path / str(r)))})
    a, b = runs
    assert {"out.npy", "x.grad.npy", "e1.grad.npy", "e2.grad.npy", "graphcnn.1.flat.grad.npy"} <= set(a) and set(a) == set(b)
    assert sum(os.path.getsize(tmp_path / "0" / f) for f in a) <= 64e6
    assert a["out.npy"].shape == (8, 16, 128) and a["x.grad.npy"].shape == (8, 16, 128)
    for f in a:
        assert a[f].dtype == np.float32 and a[f].shape == b[f].shape and np.isfinite(a[f]).all(), f
        assert np.abs(a[f] - b[f]).max() <= 1e-4 * max(1.0, np.abs(a[f]).max()), f


def test_bench_distributed_path_on_one_rank_and_strong_scaling_flag(gpu_device):
    d = _run(["--config", "c1", "--steps", "6", "--warmup", "2", "--no-cpu-baseline", "--global-batch", "16"], env={"GCGCN_FORCE_DIST": "1"})
    assert d["n_gpus"] == 1 and d["scaling"] == "strong" and d["config"]["global_batch"] == 16 and "B=16/GPU" in d["config"]["workload"]
    assert d["config"]["grad_allreduce"].startswith("one coalesced collective")
    assert d["value"] > 0 and "cpu_baseline" not in d


@pytest.mark.timeout(600)
def test_bench_two_ranks_complete_and_print_one_line(gpu_device):
    """Round-3 verdict: the sampling steps after the timed region all-reduced on rank 0 only, so any N > 1 run would have hung
    before its JSON line.  Two real ranks, self-launched through torch.distributed.run exactly like ``--gpus N`` without the
    driver's environment; the profiling / warm-replay steps (rank 0 only, or a per-rank count) now issue no collectives."""
    d = _run(["--gpus", "2", "--dist-backend", "gloo", "--config", "c1", "--steps", "4", "--warmup", "1", "--full", "--no-cpu-baseline"],
             timeout=540)
    assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 16 and d["config"]["parallelism"] == "dp2"
    assert d["steps"] == 4 and d["warmup"] == 1 and d["scaling"] == "weak" and d["value"] > 0
    assert abs(d["value"] - 16 * 1e3 / d["ms_per_step"]) / d["value"] < 1e-3               # whole-job docs/s = global batch / step time
    assert d["roofline"] is not None and "cpu_baseline" not in d
