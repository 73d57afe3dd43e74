#!/usr/bin/env python3
"""SURVEY 8 row f2 measurement: the fused pair-BCE loss (forward + backward) on MI355X against its HBM roofline, with
the trainer's own formulation (N^2 - N nn.BCELoss calls in a Python loop, config/Config.py:355-366) timed beside it on
the host CPU for one document.  Algorithmic bytes: forward reads logits + labels (8 B per element), backward reads both
and writes dlogits (12 B per element).

--stats: instead, the loss FORWARD with and without a TrainStats (the accuracy counters of Config.py:376-393, one more launch
that reads the logits once more: 4 B per element) and the counters' launch alone, in one process, the three variants
alternating round by round; the median over the rounds is reported, as text and as one JSON line (--out FILE writes it too)."""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import gcgcn_amd
from oracle import gcgcn_oracle as O

ap = argparse.ArgumentParser()
ap.add_argument("--stats", action="store_true", help="time the loss forward with and without TrainStats")
ap.add_argument("--out", default=None, help="with --stats: also write the JSON result line to this file")
a = ap.parse_args()

dev = torch.device("cuda:0")
B, N, R = 32, 64, 97
g = torch.Generator().manual_seed(0)
x = (torch.randn(B, N, N, R, generator=g) * 3).to(dev).requires_grad_()
y = (torch.rand(B, N, N, R, generator=g) < 0.03).float().to(dev)
w = torch.ones(B, device=dev)


def timed(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


if a.stats:
    xd, stats = x.detach(), gcgcn_amd.TrainStats(dev)
    variants = {"loss_fwd_us": lambda: gcgcn_amd.pair_bce_loss(xd, y),
                "loss_fwd_with_stats_us": lambda: gcgcn_amd.pair_bce_loss(xd, y, stats=stats),
                "stats_alone_us": lambda: stats.update(xd, y)}
    for fn in variants.values():
        for _ in range(20): fn()
    torch.cuda.synchronize()
    rounds = {k: [] for k in variants}
    for _ in range(9):                      # alternate the variants, so that a neighbour's load lands on all of them
        for k, fn in variants.items():
            rounds[k].append(timed(fn, 200))
    res = {k: round(statistics.median(v), 2) for k, v in rounds.items()}
    res.update({k.replace("_us", "_min_max_us"): [round(min(v), 2), round(max(v), 2)] for k, v in rounds.items()})
    elems = float(B) * N * N * R
    res.update(B=B, N=N, R=R, rounds=9, iters_per_round=200,
               loss_fwd_GBps=round(8.0 * elems / res["loss_fwd_us"] / 1e3), stats_alone_GBps=round(4.0 * elems / res["stats_alone_us"] / 1e3),
               stats_extra_us=round(res["loss_fwd_with_stats_us"] - res["loss_fwd_us"], 2))
    stats.reset()
    stats.update(xd, y)
    assert stats.get().total == B * N * (N - 1) and stats.get().documents == B, "the counters' launch did not count every pair"
    print(f"loss forward B={B} N={N} R={R}: {res['loss_fwd_us']:.1f} us without stats, {res['loss_fwd_with_stats_us']:.1f} us with "
          f"(+{res['stats_extra_us']:.1f} us); the counters' launch alone {res['stats_alone_us']:.1f} us "
          f"= {res['stats_alone_GBps']} GB/s of its 4 B per element (the loss forward: {res['loss_fwd_GBps']} GB/s of its 8 B)")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)


def step():
    x.grad = None
    gcgcn_amd.pair_bce_loss(x, y).backward(w)

for _ in range(20): step()
torch.cuda.synchronize()
us = timed(step, 200)
nbytes = 20.0 * B * N * N * R
print(f"HIP pair_bce fwd+bwd: B={B} N={N} R={R}: {us:.1f} us/step = {B / us * 1e6:.0f} docs/s, "
      f"{nbytes / us / 1e3:.0f} GB/s of algorithmic traffic = {nbytes / us / 1e3 / 8000:.3f} of the 8 TB/s HBM roofline")
xc, yc = x.detach()[0].cpu().requires_grad_(), y[0].cpu()
t0 = time.perf_counter()
O.pair_bce_loss_loop(xc, yc).backward()
dt = time.perf_counter() - t0
print(f"trainer's loop on the host CPU ({torch.get_num_threads()} threads), one document N={N}: {dt:.2f} s = {1 / dt:.2f} docs/s")
