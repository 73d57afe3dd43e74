"""What tests/test_lstm_bf16_cpu.py and tests/test_lstm_bf16_gpu.py share: the cases, the float64 references and the bounds of
lstm_layer(..., recurrent="bf16") ("bf16 recurrence").

Reference: functional.lstm_layer_bf16_definition on the CPU in float64 (never the HIP path's output), on lstm_cases.case's inputs,
the cotangent applied as given, gradients by autograd.  Computed once per case and shared (lru_cache); nobody writes to it.

Bounds.  The form is lstm_cases': |got - ref| <= ATOL * max(1, max|ref|) + RTOL * |ref|, every element, every tensor.

1. LOOSE, end to end.  A float32 and a float64 run of the definition can put an h or a dgates element on different sides of a bf16
   boundary, after which the two runs differ by a bf16 ulp of that element, not by a float32 one.  The rule: start from lstm_cases'
   (1e-5, 1e-4), run the definition on the CPU in float32 against its float64 run over the GPU suite's cases (SWEEP and
   lstm_len_cases.CASES), double both constants until the worst fraction is at or below 0.1.  Worst fractions at (1e-5, 1e-4),
   float32 definition against float64 definition, CPU, every tensor:
       SWEEP   (17,1,140) 0.04   (17,2,140) 4.8   (17,3,140) 4.7   (16,3,140) 9.0   (33,3,140) 6.3   (17,3,256) 3.7
               (17,37,140) 51.6   (2,512,140) 55.2   (17,3,140) nd=1 9.2
       CASES   (1,1,1) 0.004   (3,5,7) 1.6   (17,3,140) 0.11 and 4.3   (16,4,140) 1.2   (33,37,140) 29.2   (33,6,140) 1.2
               (2,512,140; 512, 200) 69.8 (dh0)   (17,5,140) nd=1 0.53
   overall 69.8; 69.8 / 2^10 = 0.068 <= 0.1 < 69.8 / 2^9 = 0.136: TEN doublings, LOOSE = 1024, the constants in force are
   (1.024e-2, 1.024e-1).  test_lstm_bf16_cpu.py asserts the 0.1 at these constants and prints the fractions.  At that size the
   bound is wider than the distance between the bf16 and the fp32 layer on random data (150 - 280 of the fp32 bound on the same
   cases): it catches errors of the size of the tensor and nothing finer.  Precision rests on 2 and 3, which do not use it.
2. Step replay (replay below), flip-free: every step is recomputed in float64 from the buffers the run under test itself wrote
   (out, csave, the activated gates, dgates), so every rounding takes that run's own fp32 bits as input.  The same rule sets its
   bound: the float32 CPU run of the same recurrence (replay feeding itself) against its float64 replay is, at lstm_cases'
   (1e-5, 1e-4), at 0.070 (17,3,140), 0.123 and 0.117 (33,37,140, without / with lengths) and 0.082 / 0.067 (2,512,140) of the
   bound, the activated gates every time (out <= 0.053, csave <= 0.032, dgates <= 0.006, dh0 <= 0.012, dc0 <= 0.006).  0.123 > 0.1:
   ONE doubling, REPLAY = 2, the constants in force are (2e-5, 2e-4); test_lstm_bf16_cpu.py asserts the 0.1 there.
3. Representable operands: T = 1 with h0 and W_hh already bf16 values has no rounding in the product; out and dc0 meet lstm_cases'
   bound against float64 nn.LSTM."""
import functools

import torch

from lstm_cases import ATOL, H, RTOL, case, frac_of_bound, param_names, worst  # noqa: F401  (re-exported for the two test files)
from lstm_len_cases import CASES as LEN_CASES

LOOSE = 1024.0           # ten doublings of lstm_cases' (ATOL, RTOL): the scale argument of frac_of_bound / worst
REPLAY = 2.0             # one doubling: the step replay's bound

# (B, T, I, nd): the end-to-end sweep without lengths
SWEEP = [(1, 1, 1, 2)] + [(b, 3, 140, 2) for b in (1, 15, 16, 17, 33)] + [(17, t, 140, 2) for t in (1, 2, 37)] + [(17, 3, 256, 2), (2, 512, 140, 2),
                                                                                                               (17, 3, 140, 1)]
SWEEP_IDS = [f"{B}x{T}x{I}-nd{nd}" for B, T, I, nd in SWEEP]
# (B, T, I, lens or None): the step replay's shapes, both directions, with and without lengths
REPLAY_SHAPES = [(17, 3, 140, None), (17, 3, 140, tuple([3, 2, 1, 3] * 4) + (1,)), (33, 37, 140, None),
                 (33, 37, 140, tuple((7 * i) % 37 + 1 for i in range(33))), (2, 512, 140, None), (2, 512, 140, (512, 200))]
REPLAY_IDS = [f"{B}x{T}x{I}-{'full' if lens is None else 'min%d' % min(lens)}" for B, T, I, lens in REPLAY_SHAPES]


def bf16_round(t):
    """r(.): one rounding to bf16, nearest even, back in t's dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def run_definition(c, nd, dtype, lens=None, device="cpu", rounding=True, dy=None):
    """functional.lstm_layer_bf16_definition forward + backward on the case's tensors in `dtype`: {"out", "dx", "dh0", "dc0", "d<param>"...}."""
    from gcgcn_amd.functional import lstm_layer_bf16_definition
    t = {k: v.detach().to(device=device, dtype=dtype).clone().requires_grad_() for k, v in c.items() if k != "dy"}
    ln = None if lens is None else torch.tensor(lens, dtype=torch.int64, device=device)
    out = lstm_layer_bf16_definition(t["x"], *(t[n] for n in param_names(nd)[:4]), t["h0"], t["c0"], *(t[n] for n in param_names(nd)[4:]), lengths=ln,
                                     rounding=rounding)
    out.backward((c["dy"] if dy is None else dy).to(device=device, dtype=dtype))
    res = {"out": out.detach(), "dx": t["x"].grad, "dh0": t["h0"].grad, "dc0": t["c0"].grad}
    res.update({"d" + n: t[n].grad for n in param_names(nd)})
    return res


@functools.lru_cache(maxsize=None)
def reference(B, T, I, nd=2, lens=None, seed=0):
    """The definition in float64 on the CPU."""
    return run_definition(case(B, T, I, nd, seed), nd, torch.float64, lens)


def run_hip(c, nd, dev, lens=None, recurrent="bf16", dy=None):
    """gcgcn_amd.lstm_layer forward + backward on the device; recurrent=None calls without the keyword."""
    import gcgcn_amd
    t = {k: v.detach().to(dev).requires_grad_() for k, v in c.items() if k != "dy"}
    kw = {} if recurrent is None else {"recurrent": recurrent}
    out = gcgcn_amd.lstm_layer(t["x"], *(t[n] for n in param_names(nd)[:4]), t["h0"], t["c0"], *(t[n] for n in param_names(nd)[4:]),
                               lengths=None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev), **kw)
    out.backward((c["dy"] if dy is None else dy).to(dev))
    res = {"out": out.detach(), "dx": t["x"].grad, "dh0": t["h0"].grad, "dc0": t["c0"].grad}
    res.update({"d" + n: t[n].grad for n in param_names(nd)})
    return res


# ---- the step replay ---------------------------------------------------------------------------------------------------------------
def stacked(c, nd):
    """The case's parameters as the C ABI takes them: w_ih [nd * 4H][I], w_hh [nd * 4H][H], bias = b_ih + b_hh, h0 / c0 [nd][B][H]."""
    pn = param_names(nd)
    B = c["x"].shape[0]
    return dict(w_ih=torch.cat([c[n] for n in pn[0::4]], 0), w_hh=torch.cat([c[n] for n in pn[1::4]], 0),
                bias=torch.cat([c[pn[4 * d + 2]] + c[pn[4 * d + 3]] for d in range(nd)], 0),
                h0=c["h0"].detach().expand(nd, B, H).contiguous(), c0=c["c0"].detach().expand(nd, B, H).contiguous())


def replay(c, nd, lens, bufs, dtype=torch.float64):
    """Every step of the bf16 recurrence recomputed on the CPU in `dtype` from the buffers of the run under test.

    bufs: float32 CPU tensors out / csave [B][T][nd H], gates (activated) / dgates [B][T][nd 4H] of that run.  Forward, every t:
    gates_t = xproj_t + r(out[t-1]) r(W_hh)^T with xproj the product of x and W_ih in `dtype` (the run's own gates buffer was
    overwritten by the activated gates), the cell update from csave[t-1]; backward: dh_t = dout_t + r(dgates[t+1]) r(W_hh), dc carried
    here.  r(.) is applied to the float32 values, so no rounding can fall differently than in the run.  "t-1" / "t+1" are the
    direction's previous / next step; the row's first step takes h0 / c0; with lens, row b is active at t < lens[b] and the
    expectation at an inactive step is 0 in out and dgates (csave and gates are not asked for there).
    bufs=None: the recurrence feeds ITSELF in `dtype` -- an emulation of the kernels, used as the float32 CPU run.
    -> ({name: expected}, {name: bool mask of the elements that are asked for, or None = all})."""
    st = stacked(c, nd)
    x, dy = c["x"].to(dtype), c["dy"].to(dtype)
    B, T, _ = x.shape
    ln = torch.full((B,), T, dtype=torch.int64) if lens is None else torch.tensor(lens, dtype=torch.int64)
    self_fed = bufs is None
    exp = dict(out=torch.zeros(B, T, nd * H, dtype=dtype), csave=torch.zeros(B, T, nd * H, dtype=dtype), gates=torch.zeros(B, T, nd * 4 * H, dtype=dtype),
               dgates=torch.zeros(B, T, nd * 4 * H, dtype=dtype), dh0=torch.zeros(nd, B, H, dtype=dtype), dc0=torch.zeros(nd, B, H, dtype=dtype))
    src = exp if self_fed else {k: v.float() for k, v in bufs.items()}
    r = lambda t: bf16_round(t.float()).to(dtype)
    for d in range(nd):
        hs, gs = slice(d * H, (d + 1) * H), slice(d * 4 * H, (d + 1) * 4 * H)
        w_hh_r = r(st["w_hh"][gs])
        xproj = x @ st["w_ih"][gs].to(dtype).t() + st["bias"][gs].to(dtype)
        h0, c0 = st["h0"][d].to(dtype), st["c0"][d].to(dtype)
        order = list(range(T - 1, -1, -1)) if d else list(range(T))
        prev = lambda t: t + 1 if d else t - 1                                     # the direction's previous step
        first = lambda t: (ln - 1 <= t)[:, None] if d else torch.full((B, 1), t == 0)   # the ROW's first step (an inactive one counts as first)
        for t in order:
            act = (t < ln)[:, None]
            if not bool(act.any()):
                continue
            tp = min(max(prev(t), 0), T - 1)
            hp = torch.where(first(t), h0, src["out"][:, tp, hs].to(dtype))
            cp = torch.where(first(t), c0, src["csave"][:, tp, hs].to(dtype))
            gi, gf, gg, go = (xproj[:, t] + r(hp) @ w_hh_r.t()).chunk(4, 1)
            gi, gf, gg, go = torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gg), torch.sigmoid(go)
            cn = gf * cp + gi * gg
            z = torch.zeros_like(cn)
            exp["out"][:, t, hs] = torch.where(act, go * torch.tanh(cn), z)
            exp["csave"][:, t, hs] = torch.where(act, cn, z)
            exp["gates"][:, t, gs] = torch.where(act, torch.cat([gi, gf, gg, go], 1), torch.zeros(B, 4 * H, dtype=dtype))
        dc = torch.zeros(B, H, dtype=dtype)
        for t in reversed(order):
            act = (t < ln)[:, None]
            if not bool(act.any()):
                continue
            tn = t - 1 if d else t + 1                                             # the direction's NEXT step, whose dgates come back
            rec = r(src["dgates"][:, tn, gs]) @ w_hh_r if 0 <= tn < T else torch.zeros(B, H, dtype=dtype)
            gi, gf, gg, go = src["gates"][:, t, gs].to(dtype).chunk(4, 1)
            tp = min(max(prev(t), 0), T - 1)
            cp = torch.where(first(t), c0, src["csave"][:, tp, hs].to(dtype))
            tc = torch.tanh(src["csave"][:, t, hs].to(dtype))
            dh = dy[:, t, hs] + rec
            dcv = dc + dh * go * (1 - tc * tc)
            da = torch.cat([dcv * gg * gi * (1 - gi), dcv * cp * gf * (1 - gf), dcv * gi * (1 - gg * gg), dh * tc * go * (1 - go)], 1)
            exp["dgates"][:, t, gs] = torch.where(act, da, torch.zeros_like(da))
            dc = torch.where(act, dcv * gf, dc)
        # dh0 is the dh handed back by the row's first step: its dgates times W_hh
        t_first = (ln - 1).clamp(min=0) if d else torch.zeros(B, dtype=torch.int64)
        exp["dh0"][d] = r(src["dgates"][torch.arange(B), t_first][:, gs]) @ w_hh_r
        exp["dc0"][d] = dc
    live = (torch.arange(T)[None, :] < ln[:, None])[:, :, None]
    masks = dict(out=None, dgates=None, dh0=None, dc0=None, csave=live.expand(B, T, nd * H), gates=live.expand(B, T, nd * 4 * H))
    return exp, masks


def replay_fractions(got, exp, masks, label):
    """Largest error of every replayed tensor as a fraction of the replay's bound (REPLAY), over the elements that are asked for."""
    fr = {}
    for k, m in masks.items():
        g, e = got[k].double().reshape(exp[k].shape), exp[k].double()
        if m is not None:
            g, e = torch.where(m, g, torch.zeros_like(g)), torch.where(m, e, torch.zeros_like(e))
        fr[k] = frac_of_bound(g, e, REPLAY)
    k = max(fr, key=fr.get)
    print(f"{label}: worst {fr[k]:.3f} of the bound ({k}); " + " ".join(f"{n}={v:.3f}" for n, v in fr.items()))
    return fr


# ---- special inputs ------------------------------------------------------------------------------------------------------------------
def representable_case(B, nd):
    """T = 1 with h0 and W_hh already bf16 values: the recurrent product has no rounding."""
    c = dict(case(B, 1, 140, nd, seed=3))
    c["h0"] = bf16_round(c["h0"])
    for n in param_names(nd)[1::4]:
        c[n] = bf16_round(c[n])
    return c


def discriminating_case(nd=2):
    """T = 1, B = 2.  h0[u] = 1 + 3/1024 for even u and 1 for odd u: every element rounds to 1 in bf16 (3/1024 is below half an ulp, 1/256).
    Every row of W_hh holds +64 at the even units and -64 at the odd ones: r(h0) r(W_hh)^T = 64 * (64 - 64) = 0, while the unrounded
    product is 64 * 64 * 3/1024 = 12 in every gate: a route that does not round the operand computes another layer altogether."""
    c = dict(case(2, 1, 140, nd, seed=4))
    sign = torch.tensor([1.0, -1.0]).repeat(H // 2)
    c["h0"] = (1 + (3 / 1024) * (sign > 0).float()).expand(nd, 1, H).contiguous()
    for n in param_names(nd)[1::4]:
        c[n] = (64.0 * sign).expand(4 * H, H).contiguous()
    return c
