"""What tests/test_bert_attn_bf16_cpu.py and tests/test_bert_attn_bf16_gpu.py share: the reference of ``attention="bf16"`` and its
bounds.  Configs, seeded parameters, inputs, masks and the bound's FORM are tests/bert_cases.py's, tests/bert_length_cases.py's and
tests/bert_bf16_cases.py's.

Reference: ``gcgcn_amd.bert.Bf16AttentionFn`` in float64 on the CPU (``attn_def`` below: the definition on packed qkv), and for layers
and models ``torch_layer`` / ``BertModel(impl="torch", attention="bf16")`` in float64, with ``matmul`` as the test sets it.  Computed
once per case (lru_cache); nobody writes to it.

Bound: |got - ref| <= ATOL * max(1, max|ref|) + RTOL * |ref|, every element; never derived from the HIP path's output.

Layer and model tests (BOUNDS[matmul]).  The rule is bert_bf16_cases': the float32 CPU run of ``impl="torch", attention="bf16"``
against its float64 run at MODEL_SWEEP x CONFIGS (eval mode, outputs and every gradient) has to sit at or below 0.1 of the bound,
else both constants are doubled until it does.  Measured fractions with bert_bf16_cases' (4e-2, 4e-2)
(test_bert_attn_bf16_cpu.test_float32_within_a_tenth_of_the_bound prints them at the constants in force):
  matmul="fp32"   D=128 H=2 (3,33): 0.235   (2,130): 0.098      D=192 H=3 (3,33): 0.224   (2,130): 0.275
  matmul="bf16"   D=128 H=2 (3,33): 0.417   (2,130): 1.300      D=192 H=3 (3,33): 0.486   (2,130): 0.902
Neither passes, so the constants are raised by the rule, per matmul setting: (1.6e-1, 1.6e-1) for matmul="fp32" (worst 0.069) and
(6.4e-1, 6.4e-1) for matmul="bf16" (worst 0.081).  One tensor sets both: the gradient of attention.self.key.bias.  It is exactly zero
in exact arithmetic (a softmax does not see a shift common to its keys: every row of dS sums to zero), and with bf16 operands it is
the sum of the ROUNDING ERRORS of r(dS) -- 0.036 at its largest element at (2,130), against 16 for the key weight's gradient -- so
any perturbation of dS (another summation order; with matmul="bf16" a flipped operand rounding upstream) redraws it entirely: the
float32 run misses it by 0.053, more than its size.  Every other tensor sits at or below 0.24 of (4e-2, 4e-2) with matmul="bf16" and
0.02 with matmul="fp32".  A wrong lane map or a dropped k-step is an error of the size of the tensor on EVERY tensor; the core tests
below hold the kernels to a bound 250 times tighter.

Core alone (CORE_ATOL, CORE_RTOL): q, k, v and dctx are the same fp32 values in the run and in the reference and round the same way;
only P and dS, computed in another precision and order, can sit on the other side of a bf16 rounding boundary, a step of 2^-8 of
that one element.  Set by the same rule on the core alone: the float32 CPU run of ``Bf16AttentionFn`` against its float64 run over
ATTN_T x KINDS, starting from bert_cases' (2e-5, 2e-4) and doubling both until the run sits at or below 0.1.  Found: 8.18 of the
bound at (2e-5, 2e-4) -- ctx at (3, 64) "holes", one flipped P element; dqkv is worst at (1, 512) with 6.85 -- hence seven doublings,
(2.56e-3, 2.56e-2), where the run sits at 0.064.  (Without the penalty shift in ``Bf16AttentionFn`` the float32 run of the "dead"
documents, every key at -10000, loses the scores' low bits and sits at 63 of (2e-5, 2e-4); the kernels shift by c_b likewise.)"""
import functools

import torch

from gcgcn_amd import bert as bert_mod
from gcgcn_amd.bert import BertModel

import bert_bf16_cases as LB
from bert_cases import attn_case, config, model_case, state
from bert_length_cases import attn_len_case, layer_len_case, per_document

BOUNDS = {"fp32": (4 * LB.ATOL, 4 * LB.RTOL), "bf16": (16 * LB.ATOL, 16 * LB.RTOL)}      # layers and models: matmul -> (ATOL, RTOL)
CORE_RTOL, CORE_ATOL = 2.56e-2, 2.56e-3       # the core alone

ATTN_T = [(3, 1), (3, 15), (3, 16), (3, 17), (3, 33), (3, 63), (3, 64), (3, 65), (3, 130), (1, 512)]
KINDS = ["none", "prefix", "holes", "dead"]
LEN_CASES = [(3, 48, (48, 0, 17), False), (4, 64, (64, 33, 16, 0), True)]      # (B, T, lengths, key-bias holes)


# ---- the core alone ----------------------------------------------------------------------------------------------------------------
def attn_def(case, H, dtype, keep=None, scale=1.0, fn=None):
    """{"ctx", "lse", "dqkv"} of the bf16 definition on packed qkv; keep [B,H,T,T] bool replays a dropout mask (scale = 1 / (1 - p)).
    fn(q, k, v, penalty, m) -> (ctx, lse): Bf16AttentionFn.apply by default."""
    fn = bert_mod.Bf16AttentionFn.apply if fn is None else fn
    qkv = case["qkv"].to(dtype).clone().detach().requires_grad_()
    B, T, D3 = qkv.shape
    D = D3 // 3
    split = lambda t: t.reshape(B, T, H, 64).permute(0, 2, 1, 3)
    q, k, v = (split(qkv[..., i * D:(i + 1) * D]) for i in range(3))
    pen = None if case["key_bias"] is None else case["key_bias"].to(dtype)[:, None, None, :]
    m = torch.ones(B, H, T, T, dtype=dtype) if keep is None else keep.to(dtype) * scale
    ctx, lse = fn(q, k, v, pen, m)
    ctx = ctx.permute(0, 2, 1, 3).reshape(B, T, D)
    (ctx * case["dctx"].to(dtype)).sum().backward()
    return {"ctx": ctx.detach(), "lse": lse.detach(), "dqkv": qkv.grad}


@functools.lru_cache(maxsize=None)
def attn_reference(B, T, H, kind):
    return attn_def(attn_case(B, T, H, kind), H, torch.float64)


@functools.lru_cache(maxsize=None)
def attn_len_reference(B, T, H, lengths, holes=False):
    """bert_length_cases.attn_len_reference with the bf16 definition: every document alone, truncated; zeros on padding rows."""
    c = attn_len_case(B, T, H, holes)
    D = H * 64
    ref = {"ctx": torch.zeros(B, T, D, dtype=torch.float64), "lse": torch.zeros(B, H, T, dtype=torch.float64),
           "dqkv": torch.zeros(B, T, 3 * D, dtype=torch.float64)}
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        sub = {k: (None if v is None else v[b:b + 1, :n]) for k, v in c.items()}
        r = attn_def(sub, H, torch.float64)
        ref["ctx"][b, :n], ref["lse"][b, :, :n], ref["dqkv"][b, :n] = r["ctx"][0], r["lse"][0], r["dqkv"][0]
    return ref


@functools.lru_cache(maxsize=None)
def discriminating_case(B=2, T=33, H=2):
    """Inputs on which fp32 operands and bf16 operands give answers that differ at order one.  Query coordinates are
    s_i (32 + 3 b / 32) with b in {0, 1} and s_i a power of two in {1, 1/2, 1/4}: bf16 has a spacing of s_i / 4 there and every
    coordinate rounds to s_i 32.  Keys are +-32 vectors with 32 coordinates of each sign, exact in bf16.  The rounded scores are
    s_i 128 (sum of the key's signs) = 0 on every key -- P is uniform -- while the fp32 scores are (3 s_i / 8) sum_d sign_d b_d, of
    standard deviation 1.5 s_i across the keys.  Values are N(0, 1 / 8^2), which keeps dq, dk and dv at one scale (the bound's
    absolute term follows the largest of the three); the cotangent is N(0, 1)."""
    g = torch.Generator().manual_seed(4242)
    D = 64 * H
    s = torch.tensor([1.0, 0.5, 0.25])[torch.arange(T) % 3][None, :, None]
    q = s * (32.0 + 0.09375 * torch.randint(0, 2, (B, T, D), generator=g).float())
    signs = torch.cat([torch.ones(32), -torch.ones(32)])
    k = 32.0 * torch.stack([signs[torch.randperm(64, generator=g)] for _ in range(B * T * H)]).view(B, T, D)
    v = torch.randn(B, T, D, generator=g) / 8.0
    return {"qkv": torch.cat([q, k, v], -1), "key_bias": None, "dctx": torch.randn(B, T, D, generator=g)}


def core_bound(ref):
    ref = ref.detach().double().cpu()
    return CORE_ATOL * max(1.0, ref.abs().max().item()) + CORE_RTOL * ref.abs()


def core_frac(got, ref, atol=None, rtol=None):
    """Largest |got - ref| as a fraction of the core bound (<= 1 passes); NaN / inf anywhere gives inf."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not torch.isfinite(got).all():
        return float("inf")
    atol, rtol = CORE_ATOL if atol is None else atol, CORE_RTOL if rtol is None else rtol
    bound = atol * max(1.0, ref.abs().max().item()) + rtol * ref.abs()
    return ((got - ref).abs() / bound).max().item()


def core_worst(got, ref, label, **kw):
    fr = {k: core_frac(got[k], ref[k], **kw) for k in ref}
    print(f"{label}: " + " ".join(f"{n}={v:.3f}" for n, v in sorted(fr.items(), key=lambda kv: -kv[1])) + " of the core bound")
    return fr


def share_outside(got, ref):
    """The share of elements outside the core bound."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).abs() > core_bound(ref)).double().mean().item()


# ---- layers and models -------------------------------------------------------------------------------------------------------------
def frac_of_bound(got, ref, matmul, atol=None, rtol=None):
    """Largest |got - ref| as a fraction of the bound of the run's matmul setting (<= 1 passes); NaN / inf anywhere gives inf."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not torch.isfinite(got).all():
        return float("inf")
    a, r = BOUNDS[matmul]
    a, r = a if atol is None else atol, r if rtol is None else rtol
    bound = a * max(1.0, ref.abs().max().item()) + r * ref.abs()
    return ((got - ref).abs() / bound).max().item()


def worst(got, ref, label, matmul, **kw):
    """Prints the case's largest error as a fraction of the bound, per tensor, and returns {name: fraction}."""
    fr = {k: frac_of_bound(got[k], ref[k], matmul, **kw) for k in ref}
    k = max(fr, key=fr.get)
    print(f"{label}: worst {fr[k]:.3f} of the bound ({k}); " + " ".join(f"{n}={v:.3f}" for n, v in sorted(fr.items(), key=lambda kv: -kv[1])[:6]))
    return fr


def fresh_model(D, H, impl="torch", dtype=torch.float64, device="cpu", p=0.0, matmul="fp32", attention="bf16"):
    m = BertModel(config(D, H, 2, p), impl=impl, matmul=matmul, attention=attention)
    m.load_state_dict(state(D, H))
    return m.to(device=device, dtype=dtype)


run_model = LB.run_model


@functools.lru_cache(maxsize=None)
def model_reference(D, H, B, T, matmul, kind="prefix"):
    return run_model(fresh_model(D, H, matmul=matmul), model_case(D, H, B, T, kind))


@functools.lru_cache(maxsize=None)
def model_len_reference(D, H, B, T, lengths, matmul):
    return per_document(fresh_model(D, H, matmul=matmul), model_case(D, H, B, T), lengths)


def _layer_kw(matmul):
    kw = {"attention": bert_mod.bf16_attention}
    if matmul == "bf16":
        kw["linear"] = bert_mod.bf16_linear
    return kw


def layer_torch(x, kb, params, H, dy, matmul, dtype=torch.float64, drop=lambda s, t: t):
    """One layer of the definition: {"y", "dx", "d00" .. "d15"}."""
    x = x.to(dtype).clone().requires_grad_()
    ps = [t.to(dtype).clone().requires_grad_() for t in params]
    y = bert_mod.torch_layer(x, None if kb is None else kb.to(dtype), ps, H, drop, **_layer_kw(matmul))
    (y * dy.to(dtype)).sum().backward()
    res = {"y": y.detach(), "dx": x.grad}
    res.update({f"d{i:02d}": t.grad for i, t in enumerate(ps)})
    return res


@functools.lru_cache(maxsize=None)
def layer_len_reference(D, H, B, T, lengths, matmul):
    """Every document alone, truncated, no mask, with the bf16 attention (and the Linears of matmul)."""
    c = layer_len_case(D, H, B, T, lengths)
    ps = [t.double().clone().requires_grad_() for t in c["params"]]
    y, dx = torch.zeros(B, T, D, dtype=torch.float64), torch.zeros(B, T, D, dtype=torch.float64)
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        x = c["x"][b:b + 1, :n].double().clone().requires_grad_()
        yb = bert_mod.torch_layer(x, None, ps, H, lambda s, t: t, **_layer_kw(matmul))
        (yb * c["dy"][b:b + 1, :n].double()).sum().backward()
        y[b, :n], dx[b, :n] = yb[0].detach(), x.grad[0]
    res = {"y": y, "dx": dx}
    res.update({f"d{i:02d}": (t.grad if t.grad is not None else torch.zeros_like(t)) for i, t in enumerate(ps)})
    return res
