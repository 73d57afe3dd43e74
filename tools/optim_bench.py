#!/usr/bin/env python3
"""Optimiser step alone, at a BERT-base-shaped parameter set (the tensor list of gcgcn_amd.BertModel(BertConfig())), as hipGraph
replays in one process: median of --reps replays with min-max, and GB/s against the bytes each row has to move.

  a  plain Adam, one group, the old entry points (gcgcn_adam_step_dev)                     FusedAdam(capturable=True)
  b  the same plain group through the new entry points (gcopt_adamw_step_dev)             ... clip_scope="global"
  c  weight decay, --groups groups (decay / no-decay by name), one clipping norm          ... bert_param_groups, clip_scope="global"
  d  torch.optim.AdamW (--decoupled) or Adam (capturable=True, foreach=True) behind clip_grad_norm_

Bytes per element: the update reads p, g, m, v and writes p, m, v (28; 36 with amsgrad, which reads and writes max_exp_avg_sq);
clipping reads g once more for the norm (4).  Row d is charged the same 28 plus clip_grad_norm_'s minimum of 12 (read g for the
norm, read and write g to scale it); what torch's kernels really move is more.

  python tools/optim_bench.py --decoupled [--weight-decay 0.01] [--amsgrad] [--groups 2] [--max-grad-norm 1.0] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gcgcn_amd  # noqa: E402
from gcgcn_amd.optim import FusedAdam  # noqa: E402


class _Named(torch.nn.Module):
    """The parameter set under BertModel's names, values on the device (the encoder itself is not run here)."""

    def __init__(self, shapes, dev):
        super().__init__()
        self._names = []
        for i, (name, shape) in enumerate(shapes):
            self.register_parameter(f"p{i}", torch.nn.Parameter(torch.randn(*shape, device=dev) * 0.02))
            self._names.append(name)

    def named_parameters(self, *a, **k):
        return [(n, p) for n, (_, p) in zip(self._names, super().named_parameters())]


def replay_ms(step, reps):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--weight-decay", type=float, default=0.01)
    ap.add_argument("--decoupled", action="store_true", help="rows c and d: AdamW's decoupled decay (without it: L2 decay, torch.optim.Adam)")
    ap.add_argument("--amsgrad", action="store_true", help="row c (and d) with amsgrad")
    ap.add_argument("--groups", type=int, default=2, choices=(1, 2), help="row c: 2 = decay / no-decay groups, 1 = everything decays")
    ap.add_argument("--max-grad-norm", type=float, default=1.0, help="0: no clipping in any row")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    shapes = [(n, tuple(p.shape)) for n, p in gcgcn_amd.BertModel(gcgcn_amd.BertConfig()).named_parameters()]
    torch.manual_seed(0)
    mgn = a.max_grad_norm if a.max_grad_norm > 0 else None
    rows = {}

    def bench(key, what, make_opt, bytes_per_elem, clip_after=False):
        model = _Named(shapes, dev)
        params = [p for _, p in model.named_parameters()]
        for p in params:
            p.grad = torch.randn_like(p) * 1e-2
        opt = make_opt(model, params)

        def step():
            if clip_after and mgn is not None:
                torch.nn.utils.clip_grad_norm_(params, mgn, foreach=True)
            opt.step()

        ms = replay_ms(step, a.reps)
        n = sum(p.numel() for p in params)
        med = statistics.median(ms)
        rows[key] = dict(what=what, tensors=len(params), elements=n, median_ms=round(med, 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4),
                         bytes_per_element=bytes_per_elem, gb_per_s=round(n * bytes_per_elem / med / 1e6, 1))
        print(f"{key}  {what}: median {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}), {rows[key]['gb_per_s']} GB/s at {bytes_per_elem} B/element",
              flush=True)
        del opt, model, params
        torch.cuda.empty_cache()

    clip = 4 if mgn is not None else 0
    ams = 8 if a.amsgrad else 0
    bench("a", "plain Adam, old entry points", lambda m, ps: FusedAdam(ps, lr=1e-4, capturable=True, max_grad_norm=mgn), 28 + clip)
    bench("b", "plain Adam, new entry points", lambda m, ps: FusedAdam(ps, lr=1e-4, capturable=True, max_grad_norm=mgn, clip_scope="global"),
          28 + clip)

    def groups_of(m, ps):
        return gcgcn_amd.bert_param_groups(m, a.weight_decay) if a.groups == 2 else [{"params": ps, "weight_decay": a.weight_decay}]

    bench("c", f"{'decoupled' if a.decoupled else 'L2'} decay{', amsgrad' if a.amsgrad else ''}, {a.groups} group(s), one clipping norm",
          lambda m, ps: FusedAdam(groups_of(m, ps), lr=1e-4, decoupled_weight_decay=a.decoupled, amsgrad=a.amsgrad, capturable=True, max_grad_norm=mgn,
                                  clip_scope="global"), 28 + clip + ams)
    mk = torch.optim.AdamW if a.decoupled else torch.optim.Adam
    bench("d", f"torch.optim.{mk.__name__}(capturable=True, foreach=True) behind clip_grad_norm_",
          lambda m, ps: mk(groups_of(m, ps), lr=1e-4, weight_decay=a.weight_decay, amsgrad=a.amsgrad, capturable=True, foreach=True),
          28 + (12 if mgn is not None else 0) + ams, clip_after=True)
    line = json.dumps({"tool": "optim_bench", "device": torch.cuda.get_device_name(0), "reps": a.reps, "max_grad_norm": mgn, "rows": rows})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
