"""EncoderLSTM forward + backward, impl="torch" (torch.nn.LSTM, MIOpen on ROCm) against impl="hip" (csrc/lstm.hip), in ONE process:
same parameters, same input, same session.

    python tools/encoder_bench.py [--B 32 --T 512 --I 140 --reps 30 --warmup 5] [--out profiles/encoder_bench.json]
    python tools/encoder_bench.py --lengths [--lib-old build/ab_old.so] --out profiles/encoder_bench_lengths.json
    python tools/encoder_bench.py --recurrent fp32 bf16 [--lengths]          (writes profiles/encoder_bench_bf16.json; ab_recurrent)

--lengths: per-document lengths (a fixed-seed draw, uniform in [T/4, T], the first document at T as in a collated batch; kept on the
device, written into the JSON) go to both implementations, and impl="hip" without them is timed in the same interleaved loop as
"hip, lengths=None".  --lib-old: the library of another revision (tools/ab_build.sh) is loaded next to this tree's and the two are
timed through the C ABI (gcgcn_lstm_fwd + gcgcn_lstm_bwd, no lengths, the same buffers), interleaved rep by rep: "abi" in the JSON.

Timing: HIP events around each step on the current stream, warm-up steps first, the two sides INTERLEAVED rep by rep (so that a
drift of the clocks hits both), median and min / max over the repetitions.  The hip side is additionally captured into a hipGraph
(forward + backward) and its replays timed the same way.  The hip side's launches are timed on their own through the library's per-launch
timer: "lstm_fwd" / "lstm_bwd" (the two recurrence kernels; the timer stamps the kernel's own begin and end), "lstm_hprev",
"lstm_gemm" (the launches the GEMM layer makes one problem at a time: the input projection and the gradient problems a group
launch cannot carry), "gemm_group" and "gemm_splitk_reduce" (the group launch of the remaining gradient problems and the reduce:
only the encoder runs in this process, so these two tags are its own).
Model beside it: a 16-row tile's step is 1024 v_mfma_f32_16x16x4_f32 on one compute unit, 32 cycles each per SIMD -> 3.4 us at
2.4 GHz, 1.75 ms for T = 512; the backward recurrence has the same count.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4), "reps": len(ms)}


def ab_abi(a, _lib, enc, x, dy, event_ms):
    """gcgcn_lstm_fwd + gcgcn_lstm_bwd of this tree's library and of a.lib_old on the same buffers, interleaved rep by rep."""
    from gcgcn_amd import functional as F_
    H, nd, B, T, I = 128, 2, a.B, a.T, a.I
    r = enc.rnns[0]
    w_ih, w_hh = torch.cat([r.weight_ih_l0, r.weight_ih_l0_reverse]).detach(), torch.cat([r.weight_hh_l0, r.weight_hh_l0_reverse]).detach()
    bias = torch.cat([r.bias_ih_l0 + r.bias_hh_l0, r.bias_ih_l0_reverse + r.bias_hh_l0_reverse]).detach()
    h0, c0 = (p.detach().expand(nd, B, H).contiguous() for p in (enc.init_hidden[0], enc.init_c[0]))
    xd = x.detach()
    e = lambda *s: torch.empty(*s, device=x.device)
    out, csave, gates, dgates = e(B, T, nd * H), e(B, T, nd * H), e(B * T, nd * 4 * H), e(B * T, nd * 4 * H)
    dx, dw_ih, dw_hh, db, dh0, dc0 = e(B, T, I), e(nd * 4 * H, I), e(nd * 4 * H, H), e(nd * 4 * H), e(nd, B, H), e(nd, B, H)
    ws = e(_lib.lib().gcgcn_lstm_ws_bytes(B, T, I, H, nd) // 4 + 4)
    p, st = F_._p, F_._stream
    libs = {"this tree": _lib.lib(), "old": ctypes.CDLL(os.path.abspath(a.lib_old))}
    for name in ("gcgcn_lstm_fwd", "gcgcn_lstm_bwd"):
        fn = getattr(libs["old"], name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]

    def step(h):
        rc = h.gcgcn_lstm_fwd(B, T, I, H, nd, p(xd), p(w_ih), p(w_hh), p(bias), p(h0), p(c0), p(out), p(gates), p(csave), st())
        rc |= h.gcgcn_lstm_bwd(B, T, I, H, nd, p(xd), p(w_ih), p(w_hh), p(h0), p(c0), p(out), p(gates), p(csave), p(dy), p(dgates), p(dx),
                               p(dw_ih), p(dw_hh), p(db), p(dh0), p(dc0), p(ws), ws.numel() * 4, st())
        assert rc == 0, h.gcgcn_last_error()

    got = {}
    for k, h in libs.items():
        for _ in range(a.warmup):
            step(h)
        torch.cuda.synchronize()
        got[k] = (out.clone(), dx.clone(), dw_hh.clone())
    same = all(torch.equal(u, v) for u, v in zip(got["this tree"], got["old"]))
    ev = {k: [] for k in libs}
    for _ in range(a.reps):
        for k, h in libs.items():
            ev[k].append(event_ms(lambda: step(h)))
    torch.cuda.synchronize()
    res = {k: stats([e0.elapsed_time(e1) for e0, e1 in v]) for k, v in ev.items()}
    res["out, dx, dw_hh bitwise equal"] = same
    return res


def ab_recurrent(a, _lib, H, dev):
    """EncoderLSTM(impl="hip", recurrent=s) for every s of --recurrent in ONE process, same parameters and input, interleaved rep by
    rep: HIP events per step, eager and hipGraph replay, and -- one step per (rep, setting, kernel) inside a window of the library's
    per-launch timer -- the two recurrence kernels on their own.  The acceptance of the bf16 setting: each kernel's bf16 MEDIAN below
    the fp32 kernel's MINIMUM over the same reps."""
    from gcgcn_amd.models import EncoderLSTM
    torch.manual_seed(7)
    enc = {}
    for s in a.recurrent:
        enc[s] = EncoderLSTM(a.I, H, 1, True, True, 0.0, False, impl="hip", recurrent=s).to(dev).train()
        if len(enc) == 1:
            for p in enc[s].parameters():                      # the reference's reset_parameters: N(0, 0.1^2)
                p.data.normal_(0, 0.1)
        else:
            enc[s].load_state_dict(enc[a.recurrent[0]].state_dict(), strict=True)
    x = torch.randn(a.B, a.T, a.I, device=dev, requires_grad=True)
    dy = torch.randn(a.B, a.T, 2 * H, device=dev)
    lens = None
    if a.lengths:
        lens = torch.randint(max(1, a.T // 4), a.T + 1, (a.B,), generator=torch.Generator().manual_seed(11))
        lens[0] = a.T
        lens = lens.to(device=dev, dtype=torch.int32)

    def step(s):
        for p in enc[s].parameters():
            p.grad = None
        x.grad = None
        enc[s](x, lens).backward(dy)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    graphs, dx = {}, {}
    for s in a.recurrent:
        for _ in range(a.warmup):
            step(s)
        torch.cuda.synchronize()
        dx[s] = x.grad.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step(s)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs[s] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[s]):
            step(s)
        torch.cuda.synchronize()
        for _ in range(a.warmup):
            graphs[s].replay()
    ev = {(s, how): [] for s in a.recurrent for how in ("eager", "hipGraph replay")}
    for _ in range(a.reps):
        for s in a.recurrent:
            ev[s, "eager"].append(event_ms(lambda: step(s)))
            ev[s, "hipGraph replay"].append(event_ms(graphs[s].replay))
    torch.cuda.synchronize()
    impl = {s: {how: stats([e0.elapsed_time(e1) for e0, e1 in ev[s, how]]) for how in ("eager", "hipGraph replay")} for s in a.recurrent}

    tags = ("lstm_fwd", "lstm_bwd")                          # a prefix filter: the bf16 kernels' tags are lstm_fwd_bf16 / lstm_bwd_bf16
    per = {(s, tag): [] for s in a.recurrent for tag in tags}
    for _ in range(a.reps):
        for s in a.recurrent:
            for tag in tags:
                _lib.call("gcgcn_prof_start", tag.encode(), 64)
                step(s)
                torch.cuda.synchronize()
                ms, n, w = ctypes.c_double(0), ctypes.c_int(0), ctypes.c_double(0)
                _lib.call("gcgcn_prof_stop", ctypes.byref(ms), ctypes.byref(n), ctypes.byref(w))
                assert n.value == 1, (s, tag, n.value)
                per[s, tag].append(ms.value)
    T_run = a.T if lens is None else int(lens.max())
    kernels = {s: {tag: dict(stats(per[s, tag]), us_per_time_step=round(1e3 * statistics.median(per[s, tag]) / T_run, 3)) for tag in tags}
               for s in a.recurrent}
    line = {"metric": "EncoderLSTM(impl=hip) forward + backward, one bidirectional layer, per recurrent setting", "unit": "ms",
            "config": {"B": a.B, "T": a.T, "input": a.I, "H": H, "device": torch.cuda.get_device_name(0)},
            "timing": "one process, settings interleaved rep by rep; HIP events per step; kernels: library timer, kernel begin to end",
            "impl": impl, "recurrence_kernels": kernels,
            "model": {"fp32 us_per_time_step": 3.4, "bf16 us_per_time_step": 0.2,
                      "note": "MFMA issue only: 1024 v_mfma_f32_16x16x4_f32 (32 cycles) / 128 v_mfma_f32_16x16x32_bf16 (16 cycles) per "
                              "step and compute unit over 4 SIMDs at 2.4 GHz"}}
    if "fp32" in a.recurrent and "bf16" in a.recurrent:
        line["bf16 against fp32"] = {
            tag: {"median_ratio": round(kernels["bf16"][tag]["median_ms"] / kernels["fp32"][tag]["median_ms"], 4),
                  "bf16 median below fp32 min": kernels["bf16"][tag]["median_ms"] < kernels["fp32"][tag]["min_ms"]} for tag in tags}
        line["bf16 against fp32"]["max_abs_dx_difference"] = (dx["bf16"] - dx["fp32"]).abs().max().item()
    if a.lengths:
        line["lengths"] = lens.tolist()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--recurrent", nargs="+", choices=("fp32", "bf16"), default=None,
                    help="time EncoderLSTM(impl='hip') under these recurrent settings instead (default --out: profiles/encoder_bench_bf16.json)")
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--T", type=int, default=512)
    ap.add_argument("--I", type=int, default=140)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lengths", action="store_true", help="hand per-document lengths (fixed seed) to the encoders")
    ap.add_argument("--lib-old", default=None, help="another revision's library: gcgcn_lstm_fwd + _bwd of both, interleaved")
    ap.add_argument("--out", default=None, help="the JSON is also written there (default: profiles/encoder_bench.json)")
    a = ap.parse_args()
    from gcgcn_amd import _lib
    from gcgcn_amd.models import EncoderLSTM
    dev = torch.device("cuda:0")
    H = 128
    if a.recurrent:
        line = ab_recurrent(a, _lib, H, dev)
        print(json.dumps(line))
        out = a.out or os.path.join(ROOT, "profiles", "encoder_bench_bf16.json")
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")
        return
    a.out = a.out or os.path.join(ROOT, "profiles", "encoder_bench.json")
    torch.manual_seed(7)
    enc = {"torch": EncoderLSTM(a.I, H, 1, True, True, 0.0, False).to(dev).train()}
    for p in enc["torch"].parameters():                        # the reference's reset_parameters: N(0, 0.1^2)
        p.data.normal_(0, 0.1)
    enc["hip"] = EncoderLSTM(a.I, H, 1, True, True, 0.0, False, impl="hip").to(dev).train()
    enc["hip"].load_state_dict(enc["torch"].state_dict(), strict=True)
    x = torch.randn(a.B, a.T, a.I, device=dev, requires_grad=True)
    dy = torch.randn(a.B, a.T, 2 * H, device=dev)
    lens = None
    if a.lengths:
        lens = torch.randint(max(1, a.T // 4), a.T + 1, (a.B,), generator=torch.Generator().manual_seed(11))
        lens[0] = a.T
        lens = lens.to(device=dev, dtype=torch.int32)

    def step(name, lengths="as asked"):
        m = enc[name]
        for p in m.parameters():
            p.grad = None
        x.grad = None
        m(x, lens if lengths == "as asked" else lengths).backward(dy)

    def event_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        return e0, e1

    for _ in range(a.warmup):
        step("torch"), step("hip")
    torch.cuda.synchronize()
    # what the two compute, once (not a test: tests/test_lstm_gpu.py is)
    step("torch")
    gx_t = x.grad.clone()
    step("hip")
    diff = (x.grad - gx_t).abs().max().item()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step("hip")
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step("hip")
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        graph.replay()

    ev = {"torch": [], "hip": [], "hip, hipGraph replay": []}
    if a.lengths:
        ev["hip, lengths=None"] = []
        for _ in range(a.warmup):
            step("hip", None)
    for _ in range(a.reps):
        ev["torch"].append(event_ms(lambda: step("torch")))
        ev["hip"].append(event_ms(lambda: step("hip")))
        ev["hip, hipGraph replay"].append(event_ms(graph.replay))
        if a.lengths:
            ev["hip, lengths=None"].append(event_ms(lambda: step("hip", None)))
    torch.cuda.synchronize()
    res = {k: stats([e0.elapsed_time(e1) for e0, e1 in v]) for k, v in ev.items()}
    abi = ab_abi(a, _lib, enc["hip"], x, dy, event_ms) if a.lib_old else None

    kernels = {}
    for tag in ("lstm_fwd", "lstm_bwd", "lstm_hprev", "lstm_gemm", "gemm_group", "gemm_splitk_reduce"):
        _lib.call("gcgcn_prof_start", tag.encode(), 4096)
        for _ in range(5):
            step("hip")
        torch.cuda.synchronize()
        ms, n, w = ctypes.c_double(0), ctypes.c_int(0), ctypes.c_double(0)
        _lib.call("gcgcn_prof_stop", ctypes.byref(ms), ctypes.byref(n), ctypes.byref(w))
        kernels[tag] = {"ms_per_step": round(ms.value / 5, 4), "launches_per_step": n.value / 5}
    for tag in ("lstm_fwd", "lstm_bwd"):
        kernels[tag]["us_per_time_step"] = round(1e3 * kernels[tag]["ms_per_step"] / a.T, 3)
    line = {"metric": "EncoderLSTM forward + backward, one bidirectional layer", "unit": "ms", "dtype": "f32",
            "config": {"B": a.B, "T": a.T, "input": a.I, "H": H, "device": torch.cuda.get_device_name(0)},
            "timing": "HIP events per step, sides interleaved, median (min, max)", "impl": res,
            "hip_kernels (library timer, kernel begin to end)": kernels,
            "model": {"us_per_time_step": 3.4, "ms_per_recurrence_launch": round(3.4e-3 * a.T, 3),
                      "note": "1024 v_mfma_f32_16x16x4_f32 per step on one compute unit, 32 cycles per SIMD, 2.4 GHz"},
            "max_abs_dx_difference_hip_vs_torch": diff}
    if a.lengths:
        line["lengths"] = lens.tolist()
    if abi:
        line["abi (gcgcn_lstm_fwd + gcgcn_lstm_bwd, lengths=None, this tree against --lib-old, interleaved)"] = abi
    print(json.dumps(line))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(line, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
