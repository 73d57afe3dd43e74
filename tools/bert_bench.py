#!/usr/bin/env python3
"""Forward + backward time of the BERT encoder (gcgcn_amd.BertModel), impl="hip" against impl="torch" (fp32) on the same device in
the same process: one encoder layer and the 12-layer base encoder at (B, T) = (4, 512) and (8, 256), eval-mode arithmetic with
gradients (dropout off: both implementations then compute the same function), eager and as one replayed hipGraph; and the HIP
layer's time split: each non-GEMM kernel timed on its own through the C ABI, the rest is the GEMM layer.

    python tools/bert_bench.py [--layers 12] [--iters 20] [--json out.json]
    python tools/bert_bench.py --lengths {full,ragged} [--shape 4x512] [--layers 12] [--iters 20] [--json out.json]
    python tools/bert_bench.py --matmul fp32 bf16 [--lengths ragged] [--shape 4x512] [--layers 12] [--iters 10] [--json out.json]
    python tools/bert_bench.py --attention fp32 bf16 [--matmul fp32 bf16] [--shape 4x512] [--layers 12] [--iters 10] [--json out.json]
    python tools/bert_bench.py --embeddings torch fused [--lengths {full,ragged}] [--shape 4x512] [--layers 12] [--iters 10] [--json out.json]

With --lengths only the HIP encoder runs, as one replayed hipGraph, twice on the same token counts in the same process: the
prefix-mask path (attention_mask = arange(T) < t_valid, every row computed) and the length path (lengths = t_valid, live tokens
only).  ``full``: every document at T -- the feature's overhead.  ``ragged``: a fixed seeded draw, uniform integers in [T/8, T];
seed and mean are printed.  --shape restricts the run to one (B, T), so that a caller can give every run its own time limit.

With --matmul only the HIP encoder runs, as one replayed hipGraph, once per listed setting of BertModel(matmul=...), back to back in
the same process on the same inputs (median, min and max of --iters samples; with --lengths on those token counts through
lengths=), followed by one layer's twelve Linear products timed alone through the C ABI: the fp32 GEMM layer's launch against the
bf16 kernel's, with the achieved TF/s.  With --lengths the bf16 setting runs twice, back to back on the same data: option bf16_rows = 0
(its products ignore the row-block list: dense launches) and 1 (live row blocks), columns ``..._rows0`` / ``..._rows1``.

With --attention the same graph-replay runs go over every listed combination of BertModel(matmul=..., attention=...) (--matmul
defaults to fp32 alone), and the kernel-alone section times the attention core through gcgcn_bert_attn_fwd_mx / _bwd_mx at each
listed setting, back to back in the same process on the same data, with the achieved TF/s (4 and 10 B H T^2 64 flop).

With --embeddings only the HIP encoder runs, once per listed setting of BertModel(embeddings=...), in the same process on the same
inputs with the settings INTERLEAVED rep by rep (median, min and max of --iters samples each), eager and as one replayed hipGraph:
the embeddings stage alone (a model without encoder layers, forward + backward) and the --layers encoder; with --lengths on those
token counts through lengths=.  The stage's device kernel count per forward + backward is read from torch's profiler.

Prints one table and, with --json, writes the numbers.  DESIGN.md section 8.9 holds the tables of record."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gcgcn_amd  # noqa: E402
from gcgcn_amd import _lib, BertConfig, BertModel  # noqa: E402


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def timed_stats(fn, iters, warmup=3):
    """(median, min, max) ms of `iters` samples."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def timed_interleaved(fns, iters, warmup=3):
    """{name: (median, min, max) ms}: the functions take turns, rep by rep, so that drift of the machine hits every one alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def kernel_count(step):
    """Device kernels (memsets and copies included) of one call of `step`, from torch's profiler; None where it reports none.  The
    wrappers' id range check (a host read, skipped under capture) is switched off for the count: it is no part of the stage."""
    from torch.profiler import ProfilerActivity, profile
    from gcgcn_amd import functional
    was, functional.check_ids = functional.check_ids, False
    try:
        step()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
    finally:
        functional.check_ids = was
    n = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    return n or None


LENGTH_SEED = 2024
ROWS_OPTION = b"bf16_rows"      # 0: the bf16 products ignore the row-block list


def draw_lengths(kind, B, T):
    """Token counts of the --lengths runs: every document at T, or the fixed seeded draw from [T/8, T]."""
    if kind == "full":
        return torch.full((B,), T, dtype=torch.int32)
    g = torch.Generator().manual_seed(LENGTH_SEED + 1000 * B + T)
    return torch.randint(T // 8, T + 1, (B,), generator=g).to(torch.int32)


def model_step(layers, impl, B, T, dev, t_valid=None, by_lengths=False, matmul="fp32", attention="fp32", embeddings="torch"):
    """t_valid None: the masks this tool has always used.  Otherwise the prefix mask of these counts, or (by_lengths) lengths=t_valid."""
    cfg = BertConfig(num_hidden_layers=layers, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    torch.manual_seed(0)
    model = BertModel(cfg, impl=impl, matmul=matmul, attention=attention, embeddings=embeddings).to(dev).train()
    g = torch.Generator().manual_seed(1)
    ids = torch.randint(0, cfg.vocab_size, (B, T), generator=g).to(dev)
    counts = torch.tensor([T - 37 * (b % 3) for b in range(B)]) if t_valid is None else t_valid.cpu()
    mask = (torch.arange(T)[None, :] < counts[:, None]).float().to(dev)
    dy = torch.randn(B, T, cfg.hidden_size, generator=g).to(dev)
    tv = None if t_valid is None else t_valid.to(dev)

    def step():
        model.zero_grad(set_to_none=True)
        if by_lengths:
            out, pooled = model(ids, output_all_encoded_layers=False, lengths=tv)
        else:
            out, pooled = model(ids, attention_mask=mask, output_all_encoded_layers=False)
        ((out * dy).sum() + pooled.sum()).backward()
    return step


def graphed(step):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    return graph.replay


def kernel_split(B, T, dev, iters):
    """ms of each non-GEMM kernel of one HIP layer at base size, forward and backward, timed alone (random data)."""
    D, H, I = 768, 12, 3072
    R = B * T
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    qkv, dqkv = torch.randn(B, T, 3 * D, device=dev), torch.empty(B, T, 3 * D, device=dev)
    kb = torch.zeros(B, T, device=dev)
    ctx, dctx = torch.empty(B, T, D, device=dev), torch.randn(B, T, D, device=dev)
    lse, delta = torch.empty(B, H, T, device=dev), torch.empty(B, H, T, device=dev)
    x, res, y, dx, dres = (torch.randn(R, D, device=dev) for _ in range(5))
    w, b, dw, db = (torch.randn(D, device=dev) for _ in range(4))
    mean, rstd = torch.empty(R, device=dev), torch.empty(R, device=dev)
    ws = torch.empty(_lib.lib().gcgcn_res_ln_ws_bytes(D) // 4, device=dev)
    z, gz, bi = torch.randn(R, I, device=dev), torch.empty(R, I, device=dev), torch.randn(I, device=dev)
    out = {}
    out["attn_fwd"] = timed(lambda: _lib.call("gcgcn_bert_attn_fwd", B, T, H, 64, p(qkv), p(kb), p(ctx), p(lse), None, 0, 0.0, st), iters)
    out["attn_bwd"] = timed(lambda: _lib.call("gcgcn_bert_attn_bwd", B, T, H, 64, p(qkv), p(kb), p(ctx), p(lse), p(dctx), p(dqkv), p(delta), None, 0,
                                              0.0, st), iters)
    out["res_ln_fwd x2"] = 2 * timed(lambda: _lib.call("gcgcn_res_ln_fwd", R, D, p(x), p(b), p(res), p(w), p(b), p(y), p(mean), p(rstd), None, 0, 0.0,
                                                       st), iters)
    out["res_ln_bwd x2"] = 2 * timed(lambda: _lib.call("gcgcn_res_ln_bwd", R, D, p(y), p(x), p(b), p(res), p(w), p(mean), p(rstd), p(dx), p(dres),
                                                       p(dw), p(db), p(ws), ws.numel() * 4, None, 0, 0.0, st), iters)
    out["gelu_fwd"] = timed(lambda: _lib.call("gcgcn_bias_gelu_fwd", R, I, p(z), p(bi), p(gz), st), iters)
    out["gelu_bwd"] = timed(lambda: _lib.call("gcgcn_bias_gelu_bwd", R, I, p(gz), p(z), p(bi), p(gz), st), iters)
    return out


def core_split(B, T, dev, iters, settings):
    """The attention core alone at base size through the _mx entry points, random data, dropout off: one row per setting."""
    D, H = 768, 12
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    qkv, dqkv = torch.randn(B, T, 3 * D, device=dev), torch.empty(B, T, 3 * D, device=dev)
    kb = torch.zeros(B, T, device=dev)
    ctx, dctx = torch.empty(B, T, D, device=dev), torch.randn(B, T, D, device=dev)
    lse, delta = torch.empty(B, H, T, device=dev), torch.empty(B, H, T, device=dev)
    out = []
    for name in settings:
        attn = ("fp32", "bf16").index(name)
        f = timed_stats(lambda: _lib.call("gcgcn_bert_attn_fwd_mx", B, T, H, 64, p(qkv), p(kb), None, p(ctx), p(lse), None, 0, 0.0, st, attn), iters)
        b = timed_stats(lambda: _lib.call("gcgcn_bert_attn_bwd_mx", B, T, H, 64, p(qkv), p(kb), None, p(ctx), p(lse), p(dctx), p(dqkv), p(delta),
                                          None, 0, 0.0, st, attn), iters)
        flop = 1e-9 * B * H * T * T * 64
        out.append({"attention": name, "fwd_ms": f[0], "fwd_min_ms": f[1], "fwd_max_ms": f[2], "bwd_ms": b[0], "bwd_min_ms": b[1],
                    "bwd_max_ms": b[2], "fwd_tflops": 4 * flop / f[0], "bwd_tflops": 10 * flop / b[0]})
    return out


def product_split(B, T, dev, iters):
    """One base-size layer's twelve Linear products alone, random data: (name, M, N, K, fp32 ms, bf16 ms).  The fp32 launch is the GEMM
    layer's stand-alone one with its own split choice (in the layer the backward's pairs share a group launch)."""
    D, I, R = 768, 3072, B * T
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    ws = torch.empty(16 << 20, device=dev)
    out = []
    for lin, (N, K) in (("qkv", (3 * D, D)), ("attn.out", (D, D)), ("intermediate", (I, D)), ("output", (D, I))):
        x, w, dy = torch.randn(R, K, device=dev), torch.randn(N, K, device=dev), torch.randn(R, N, device=dev)
        y, dx, dw = torch.empty(R, N, device=dev), torch.empty(R, K, device=dev), torch.empty(N, K, device=dev)
        # (form, a_kc, b_kc, A, lda, B, ldb, C, ldc, M, N, K)
        probs = (("fwd  nt", 1, 1, x, K, w, K, y, N, R, N, K), ("dx   nn", 1, 0, dy, N, w, K, dx, K, R, K, N), ("dw   tn", 0, 0, dy, N, x, K, dw, K, N, K, R))
        for name, akc, bkc, A, lda, Bm, ldb, C, ldc, m, n, k in probs:
            f32 = timed(lambda: _lib.call("gcgcn_gemm", m, n, k, p(A), lda, akc, p(Bm), ldb, bkc, p(C), ldc, 1, 0, 0, 0, 1.0, None, 0, 0, 0, 0, p(ws),
                                          ws.numel(), st), iters)
            b16 = timed(lambda: _lib.call("gcgcn_gemm_bf16", akc, bkc, p(A), lda, p(Bm), ldb, p(C), ldc, m, n, k, None, None, 0, p(ws), ws.numel() * 4,
                                          st), iters)
            out.append({"product": f"{lin} {name}", "M": m, "N": n, "K": k, "fp32_ms": f32, "bf16_ms": b16,
                        "fp32_tflops": 2e-9 * m * n * k / f32, "bf16_tflops": 2e-9 * m * n * k / b16})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json")
    ap.add_argument("--lengths", choices=("full", "ragged"), help="the HIP encoder's prefix-mask path against its length path on these token counts")
    ap.add_argument("--shape", help="BxT: this shape only (default: 4x512 and 8x256)")
    ap.add_argument("--matmul", nargs="+", choices=("fp32", "bf16"), help="the HIP encoder with these matmul settings, back to back")
    ap.add_argument("--attention", nargs="+", choices=("fp32", "bf16"), help="the HIP encoder with these attention settings (times --matmul)")
    ap.add_argument("--embeddings", nargs="+", choices=("torch", "fused"), help="the HIP encoder with these embeddings settings, interleaved")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.backends.cuda.matmul.allow_tf32 = False
    rows = []
    shapes = ((4, 512), (8, 256)) if not a.shape else (tuple(int(v) for v in a.shape.lower().split("x")),)
    if a.embeddings:
        for B, T in shapes:
            tv = draw_lengths(a.lengths, B, T) if a.lengths else None
            if tv is not None:
                print(f"B={B} T={T} lengths={a.lengths} seed={LENGTH_SEED} t_valid={tv.tolist()} mean={tv.float().mean().item():.1f}", flush=True)
            for layers in sorted({0, a.layers}):
                r = {"B": B, "T": T, "layers": layers, "lengths": a.lengths, "t_valid": None if tv is None else tv.tolist()}
                steps = {e: model_step(layers, "hip", B, T, dev, tv, tv is not None, embeddings=e) for e in a.embeddings}
                if layers == 0:
                    for e, step in steps.items():
                        r[f"{e}_kernels"] = kernel_count(step)
                for mode, fns in (("eager", steps), ("graph", {e: graphed(s) for e, s in steps.items()})):
                    for e, (med, lo, hi) in timed_interleaved(fns, a.iters).items():
                        r[f"{e}_{mode}_ms"], r[f"{e}_{mode}_min_ms"], r[f"{e}_{mode}_max_ms"] = med, lo, hi
                    del fns
                del steps
                torch.cuda.empty_cache()
                rows.append(r)
                what = "embeddings stage alone" if layers == 0 else f"layers={layers:2d}"
                print(f"B={B} T={T} {what} lengths={a.lengths}: " + "  ".join(f"{k}={v:.4f}" for k, v in r.items() if k.endswith("_ms"))
                      + "".join(f"  {k}={v}" for k, v in r.items() if k.endswith("_kernels")), flush=True)
        shapes = ()
    elif a.matmul or a.attention:
        combos = [(mm, at) for mm in (a.matmul or ["fp32"]) for at in (a.attention or ["fp32"])]
        for B, T in shapes:
            tv = draw_lengths(a.lengths, B, T) if a.lengths else None
            if tv is not None:
                print(f"B={B} T={T} lengths={a.lengths} seed={LENGTH_SEED} t_valid={tv.tolist()} mean={tv.float().mean().item():.1f}", flush=True)
            for layers in sorted({1, a.layers}):
                r = {"B": B, "T": T, "layers": layers, "lengths": a.lengths, "t_valid": None if tv is None else tv.tolist()}
                for mm, at in combos:
                    step = model_step(layers, "hip", B, T, dev, tv, tv is not None, matmul=mm, attention=at)
                    key = mm if not a.attention else f"mm_{mm}_attn_{at}"
                    # bf16 products with lengths: the dense launches (bf16_rows = 0) and the row-block ones (1) back to back on this data;
                    # the option is read at launch, so each side captures its own graph
                    for on in ((0, 1) if (mm == "bf16" and tv is not None) else (None,)):
                        k = key if on is None else f"{key}_rows{on}"
                        if on is not None:
                            _lib.call("gcgcn_set_option", ROWS_OPTION, on)
                        r[f"{k}_graph_ms"], r[f"{k}_min_ms"], r[f"{k}_max_ms"] = timed_stats(graphed(step), a.iters)
                    _lib.call("gcgcn_set_option", ROWS_OPTION, 1)
                    del step
                    torch.cuda.empty_cache()
                rows.append(r)
                print(f"B={B} T={T} layers={layers:2d} lengths={a.lengths}: " + "  ".join(f"{k}={v:.3f}" for k, v in r.items() if k.endswith("_ms")),
                      flush=True)
            if a.attention and not a.lengths:
                cs = core_split(B, T, dev, a.iters, a.attention)
                rows.append({"B": B, "T": T, "core": cs})
                for q in cs:
                    print(f"B={B} T={T} attention core alone, attention={q['attention']}: fwd {q['fwd_ms']:.4f} ms ({q['fwd_min_ms']:.4f}-"
                          f"{q['fwd_max_ms']:.4f}) {q['fwd_tflops']:5.1f} TF/s   bwd {q['bwd_ms']:.4f} ms ({q['bwd_min_ms']:.4f}-{q['bwd_max_ms']:.4f}) "
                          f"{q['bwd_tflops']:5.1f} TF/s", flush=True)
            if a.matmul and not a.lengths:
                split = product_split(B, T, dev, a.iters)
                rows.append({"B": B, "T": T, "products": split})
                for q in split:
                    print(f"B={B} T={T} {q['product']:22s} ({q['M']:5d},{q['N']:5d},{q['K']:5d})  fp32 {q['fp32_ms']:.4f} ms {q['fp32_tflops']:6.1f} TF/s   "
                          f"bf16 {q['bf16_ms']:.4f} ms {q['bf16_tflops']:6.1f} TF/s", flush=True)
        shapes = ()
    elif a.lengths:
        for B, T in shapes:
            tv = draw_lengths(a.lengths, B, T)
            print(f"B={B} T={T} lengths={a.lengths} seed={LENGTH_SEED} t_valid={tv.tolist()} mean={tv.float().mean().item():.1f} "
                  f"({tv.float().mean().item() / T:.3f} of T)", flush=True)
            for layers in sorted({1, a.layers}):
                r = {"B": B, "T": T, "layers": layers, "lengths": a.lengths, "seed": LENGTH_SEED, "t_valid": tv.tolist()}
                for name, by_lengths in (("mask", False), ("len", True)):
                    step = model_step(layers, "hip", B, T, dev, tv, by_lengths)
                    r[f"hip_{name}_graph_ms"] = timed(graphed(step), a.iters)
                    del step
                    torch.cuda.empty_cache()
                rows.append(r)
                print(f"B={B} T={T} layers={layers:2d} lengths={a.lengths}: " + "  ".join(f"{k}={v:.3f}" for k, v in r.items() if k.endswith("_ms"))
                      + f"  len/mask={r['hip_len_graph_ms'] / r['hip_mask_graph_ms']:.3f}", flush=True)
        shapes = ()
    for B, T in shapes:
        for layers in (1, a.layers):
            r = {"B": B, "T": T, "layers": layers}
            for impl in ("torch", "hip"):
                step = model_step(layers, impl, B, T, dev)
                r[f"{impl}_eager_ms"] = timed(step, a.iters)
                r[f"{impl}_graph_ms"] = timed(graphed(step), a.iters)
                del step
                torch.cuda.empty_cache()
            rows.append(r)
            print(f"B={B} T={T} layers={layers:2d}: " + "  ".join(f"{k}={v:.3f}" for k, v in r.items() if k.endswith("_ms")), flush=True)
        split = kernel_split(B, T, dev, a.iters)
        rows.append({"B": B, "T": T, "split_ms": split})
        print(f"B={B} T={T} one HIP layer, non-GEMM kernels alone: " + "  ".join(f"{k}={v:.3f}" for k, v in split.items()), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
