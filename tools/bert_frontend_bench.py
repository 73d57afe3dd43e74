"""The BERT graph model's own glue either side of the tail, config.bert_frontend "cat" against "folded", in ONE process: forward +
backward of the front-end pair and of the [CLS] logit tail, same tensors, same session.

    python tools/bert_frontend_bench.py [--shapes 4,512,42 32,512,42] [--reps 30 --warmup 5] [--out profiles/bert_frontend_bench.json]

  front end, "cat"    : two F.embedding gathers, torch.cat, functional.token_context at K = 808 (what models.py runs with
                        frontend_impl = "hip"), gradients to the states, both tables, weight and bias
  front end, "folded" : functional.bert_token_context, the same five gradients
  tail, "cat"         : models.py's mask, multiply and add over [B,N,N,R] (n_valid given), autograd's backward
  tail, "folded"      : functional.pair_logit_bias
The tail runs at the model's padded entity count (--tail-n, 64) and R = 97 with a ragged n_valid.

Timing: HIP events around each step on the current stream, warm-up steps first, the two settings INTERLEAVED rep by rep (so that a
drift of the clocks hits both), median and min / max over the repetitions -- eager, and captured into a hipGraph (forward + backward)
whose replays are timed the same way.  The id range check of the HIP functions (a host read in eager mode) is left on, as the model
runs it.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DW, DC, DN, HD, P, NER, R = 768, 20, 20, 128, 512, 7, 97


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    return e0, e1


def make_steps(B, T, N, NT, dev):
    from gcgcn_amd import functional as Fn
    g = torch.Generator().manual_seed(17)
    r = lambda *s, k=1.0: (torch.randn(*s, generator=g) * k).to(dev)
    keep = torch.rand(B, T, generator=g) < 0.3
    pos = (torch.randint(0, P, (B, T), generator=g) * keep).to(dev)
    ner = (torch.randint(0, NER, (B, T), generator=g) * keep).to(dev)
    leaves = [t.requires_grad_() for t in (r(B, T, DW), r(P, DC), r(NER, DN), r(HD, DW + DC + DN, k=0.1), r(HD, k=0.1))]
    states, coref_w, ner_w, W, b = leaves
    node_pos = torch.zeros(B, N, T)
    for n in range(N):                                                             # one mention of 1-3 tokens per entity
        s = int(torch.randint(0, T - 3, (1,), generator=g))
        ln = 1 + n % 3
        node_pos[:, n, s:s + ln] = 1.0 / ln
    node_pos = node_pos.to(dev)
    dctx, dnode = r(B, T, HD), r(B, N, HD)
    logits, cls = r(B, NT, NT, R).requires_grad_(), r(B, R).requires_grad_()
    dout = r(B, NT, NT, R)
    nv = torch.randint(NT // 4, NT + 1, (B,), generator=g).to(dev)

    def front_cat():
        x = torch.cat([states, F.embedding(pos, coref_w, padding_idx=0), F.embedding(ner, ner_w, padding_idx=0)], dim=-1)
        return torch.autograd.grad(Fn.token_context(x, W, b, node_pos), leaves, [dctx, dnode])

    def front_folded():
        return torch.autograd.grad(Fn.bert_token_context(states, pos, ner, coref_w, ner_w, W, b, node_pos), leaves, [dctx, dnode])

    def tail_cat():
        add = cls[:, None, None, :]
        ok = torch.arange(NT, device=dev)[None, :] < nv[:, None]
        add = add * (ok[:, :, None] & ok[:, None, :]).unsqueeze(-1).to(add.dtype)
        return torch.autograd.grad(logits + add, [logits, cls], dout)

    def tail_folded():
        return torch.autograd.grad(Fn.pair_logit_bias(logits, cls, nv), [logits, cls], dout)

    return {"front end": {"cat": front_cat, "folded": front_folded}, "tail": {"cat": tail_cat, "folded": tail_folded}}


def time_pair(steps, reps, warmup):
    """{setting: stats} eager and replayed, the settings interleaved rep by rep."""
    out = {}
    for _ in range(warmup):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in steps}
    for _ in range(reps):
        for k, fn in steps.items():
            ev[k].append(event_ms(fn))
    torch.cuda.synchronize()
    out["eager"] = {k: stats([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}
    graphs, held = {}, []
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for fn in steps.values():
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for k, fn in steps.items():
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[k]):
            held.append(fn())
    for _ in range(warmup):
        for gr in graphs.values():
            gr.replay()
    torch.cuda.synchronize()
    ev = {k: [] for k in steps}
    for _ in range(reps):
        for k, gr in graphs.items():
            ev[k].append(event_ms(gr.replay))
    torch.cuda.synchronize()
    out["hipGraph"] = {k: stats([a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}
    for mode in out.values():
        mode["folded / cat"] = round(mode["folded"]["median_ms"] / mode["cat"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["4,512,42", "32,512,42"], help="B,T,N of the front-end pair")
    ap.add_argument("--tail-n", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bert_frontend_bench needs a GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "widths": [DW, DC, DN], "tail": {"N": a.tail_n, "R": R}, "shapes": {}}
    for shape in a.shapes:
        B, T, N = (int(v) for v in shape.split(","))
        steps = make_steps(B, T, N, a.tail_n, dev)
        res["shapes"][shape] = {name: time_pair(pair, a.reps, a.warmup) for name, pair in steps.items()}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
