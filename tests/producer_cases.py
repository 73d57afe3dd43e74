"""Cases, float64 reference and bound of the edge-feature producer's edge suites (test_producer_edges_cpu.py checks the cases
themselves without a GPU, test_producer_edges_gpu.py runs csrc/producer.hip on them).  Importable without a GPU.

Inputs.  make_case() is seeded and deterministic; the float32 masters live on the CPU, kernel and reference read the same
values.  Beside what test_producer_gpu.synth_doc draws it
  * cycles the range lengths through 1, 2, 3, 4, 5, 7, 8 (and draws some up to T), so the 4-row unroll of prod_word_fwd_kernel
    and its remainder both run;
  * places dead slots anywhere in [0, T), live slots at token 0 -- of which the first pair's reaches T (and so crosses token 512
    where T does), the second pair's ends just past token 512, and beside each of them lies a dead slot that crosses token 512;
  * with ``holes`` punches holes into every range and gives live slots a second stretch anywhere in [1, T);
  * hands the first ND live, unmasked tokens of the batch the ids 0 .. ND-1 on the head side and a permutation of them on the
    tail side: every row of the score table's gradient is exercised;
  * writes junk where a correct producer never looks: position ids of masked tokens, of dead slots and of padding pairs are out
    of range (>= ND as uint8; negative, >= ND, INT_MAX / INT_MIN and beyond 32 bits as int32 / int64) -- the reference gets a copy
    with 0 there, functional.check_position_ids stays off; node rows of padding entities hold +-1e3 (finite: d W = dnterm^T node
    multiplies them by an exact zero); sen / pos of padding pairs hold random bits and junk ids.

Reference.  oracle.gcgcn_oracle.edge_features_folded in float64, per document on the real slices [:n] (n = n_valid[b]); gradients by
autograd on that graph with an independent random cotangent; parameter and table gradients accumulate over the documents in
float64.  Padding rows are zero.  reference() also returns the float64 sentence scores of every (slot, side), from the oracle's own
``trace`` argument.

relu flips.  The sentence attention weights are relu(score); a live score within rounding of zero can have one sign in float32 and
the other in float64.  E is continuous there, the gradients are not: the cotangent of every real pair that has a live score with
|score| < 1e-4 (about a hundred float32 roundings of a score of order one) is zero, E is still compared.  At most 2 % of a case's
live pairs may go that way (test_producer_edges_cpu.py; a case that breaks it gets another seed, never a larger cap).

1e-10 divisor.  A pair whose S slots are all live is divided by 1e-10 (the reference's quirk, glove:205, 212): values near 1e10.
Such pairs keep E in the comparison (per pair row, with the row's own max|ref|) and get a zero cotangent -- except in the cases
where they are ALL the live pairs there are (S = 1, and mask="all_live"): there their cotangent is scaled by 1e-10 instead, as in
test_edges_more_pairs_than_waves, which checks the gradients of that path too.  A row divided by 1e-10 is proportional to its
sentence scores, so a float32 rounding of a score of a few 1e-3 is already 1e-5 of the whole row: those all-1e-10 cases draw every
sentence score in [0.5, 2.5] (attention_all bias 1.5, |weight| summing to at most 1), the other cases scores of either sign; the
large mixed cases (``keep_padded``) keep the last slot of every pair padded, and a small case that still draws such a row gets
another seed (SEEDS).

Bound (the project's own, tests/test_edge_gpu.py): |got - ref| <= 1e-5 * max(1, max|ref|) + 1e-4 * |ref|, per tensor, on every
element; for E per pair row."""
import functools
from types import SimpleNamespace

import torch

from gcgcn_amd import params as P_
from oracle import gcgcn_oracle as O

RTOL, ATOL = 1e-4, 1e-5
FLIP_MARGIN, FLIP_CAP = 1e-4, 0.02
LENS = (1, 2, 3, 4, 5, 7, 8)
DTYPES = {"int64": torch.int64, "int32": torch.int32, "uint8": torch.uint8}
DEFAULTS = dict(B=2, N=4, S=2, T=20, Hd=8, P=5, ND=5, dtype="uint8", nv=None, live=0.6, holes=False, mask="random", keep_padded=False, seed=0)
PARAM_KEYS = tuple(P_.producer_shapes(8, 5))
GRAD_KEYS = ("d ctx", "d node", "d dis_table") + tuple("d " + k for k in PARAM_KEYS)

# the smallest shapes at which each branch of csrc/producer.hip is still taken
SEEDS = {("Hd", 1): 1, ("T", 1): 3, ("T", 4): 1, ("T", 16): 3, ("T", 64): 2, ("S", 7): 1, ("N", 64): 1, ("N", 91): 5, ("ND", 1): 1,
         ("ND", 65): 2, ("P", 20): 3, ("ragged", 5): 1}    # cases whose seed 0 draws badly conditioned inputs (test_producer_edges_cpu.py)


def _sweep(name, values, **fixed):
    return [dict({name: v}, **fixed, **({"seed": SEEDS[(name, v)]} if (name, v) in SEEDS else {})) for v in values]


SWEEPS = {
    "Hd": _sweep("Hd", (1, 3, 63, 64, 65, 128, 129, 256, 257, 512)),
    "Hd x ND": [dict(Hd=256, ND=21), dict(Hd=257, ND=21)],
    "T": _sweep("T", (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 511, 512, 513, 2048), N=3),
    "S": _sweep("S", (1, 7, 8, 9, 16, 17, 31), N=3, T=12),
    "N": _sweep("N", (1, 2, 15, 16, 17, 45, 46, 64), S=1, T=8) + [dict(N=91, S=1, T=8, live=1.0, seed=SEEDS["N", 91]),
                                                                  dict(N=46, S=2, T=8, keep_padded=True, seed=1)],
    "ND": _sweep("ND", (1, 2, 21, 63, 64, 65, 100), dtype="int32"),
    "P": _sweep("P", (1, 3, 20, 33)),
    "dtype": [dict(dtype=d, Hd=65, T=65) for d in ("int64", "int32", "uint8")],
    "masks": [dict(holes=True), dict(mask="token0"), dict(mask="all_live"), dict(mask="none_live"), dict(mask="one_live")],
    "ragged": [dict(B=4, N=n, nv=(n, 0, 1, n - 1), keep_padded=n > 5, seed=SEEDS.get(("ragged", n), 0)) for n in (5, 17, 46)],
    "B": [dict(B=b) for b in (1, 3, 5)],
    "full": [dict(mask="all_live", N=5, S=3, Hd=24)],
}
FOUR_WAYS = {"Hd": SWEEPS["Hd"], "ragged": SWEEPS["ragged"], "N": [k for k in SWEEPS["N"] if k["N"] in (46, 91)], "ND": SWEEPS["ND"]}
ALL_CASES = [(fam, kw) for fam, kws in SWEEPS.items() for kw in kws]


def kw_id(kw):
    return " ".join(f"{k}={v}" for k, v in kw.items()).replace(" ", "-") or "default"


def make_case(**kw):
    c = SimpleNamespace(**dict(DEFAULTS, **kw))
    c.id = kw_id(kw)
    B, N, S, T, Hd, P, ND = c.B, c.N, c.S, c.T, c.Hd, c.P, c.ND
    c.ns = [N] * B if c.nv is None else list(c.nv)
    assert len(c.ns) == B and all(0 <= n <= N for n in c.ns)
    g = torch.Generator().manual_seed(1000003 * B + 10007 * N + 101 * S + 13 * T + 7 * Hd + 3 * P + 5 * ND + c.seed + sum(c.ns)
                                      + 97 * sorted(DTYPES).index(c.dtype))
    rand = lambda *s: torch.rand(*s, generator=g)
    rint = lambda lo, hi, s: torch.randint(lo, hi, s, generator=g)
    c.ragged = c.nv is not None
    c.n_valid = torch.tensor(c.ns, dtype=torch.int32) if c.ragged else None
    c.real = torch.arange(N)[None, :] < torch.tensor(c.ns)[:, None]
    c.pair = c.real[:, :, None] & c.real[:, None, :]
    c.ctx = torch.tanh(torch.randn(B, T, Hd, generator=g))
    c.node = rand(B, N, Hd) * 2 - 1
    c.table = torch.randn(ND, P, generator=g) * 0.5
    u = lambda shp, k: (rand(*shp) * 2 - 1) / k ** 0.5                              # nn.Linear's initial ranges
    c.sd = {}
    for k, shp in P_.producer_shapes(Hd, P).items():
        fan_in = P_.producer_shapes(Hd, P)[k[:k.rindex(".")] + ".weight"][1]
        c.sd[k] = u(shp, fan_in)
    c.scale_full = S == 1 or c.mask == "all_live"
    VEC = "sentence_attention.attention_all."
    if c.scale_full:                                # every live pair is divided by 1e-10: all sentence scores in [0.5, 2.5] (module docstring)
        c.sd[VEC + "weight"] /= max(1.0, float(c.sd[VEC + "weight"].abs().sum()))
        c.sd[VEC + "bias"][:] = 1.5
    else:                                           # scores of either sign, spread of order one
        c.sd[VEC + "weight"] *= 3.0
        c.sd[VEC + "bias"] *= 0.1
    # ---- sentence masks -----------------------------------------------------------------------------------
    slots = (B, N, N, S)
    live = rand(*slots) < c.live
    if c.mask == "all_live":
        live[:] = True
    elif c.mask == "none_live":
        live[:] = False
    elif c.mask == "one_live":
        live[:] = False
        live[B - 1, N - 1, 0, S - 1] = True
    if c.keep_padded:
        live[..., S - 1] = False
    ln = torch.tensor(LENS)[torch.arange(B * N * N * S) % len(LENS)].view(slots)
    ln = torch.where(rand(*slots) < 0.15, rint(1, T + 1, slots), ln).clamp(max=T)
    if c.mask == "token0":
        ln = torch.where(live, torch.ones_like(ln), ln)
    t0 = torch.where(live, torch.zeros_like(ln), rint(1, max(T, 2), slots))         # dead slots: anywhere past token 0
    t0 = torch.where(~live & (rand(*slots) < 0.3), T - ln, t0)                       # ... some of them end at T
    t0 = torch.where(~live, t0.clamp(min=1), t0)
    t1 = (t0 + ln).clamp(max=T)
    t1 = torch.where(~live & (rand(*slots) < 0.2), t0, t1)                           # ... and some are empty
    if c.mask == "random" and c.live < 1.0:
        for p, end in ((0, T), (1, min(T, 516))):                                    # the long live slots and their dead neighbours
            if p < N * N and (p == 0 or T > 512):
                i, j = divmod(p, N)
                live[0, i, j, 0], t0[0, i, j, 0], t1[0, i, j, 0] = True, 0, end
                if S > 1:
                    live[0, i, j, S - 1], t0[0, i, j, S - 1], t1[0, i, j, S - 1] = False, max(1, min(510, T - 1)), min(T, 516)
    ar = torch.arange(T).view(1, 1, 1, 1, T)
    sen = (ar >= t0.unsqueeze(-1)) & (ar < t1.unsqueeze(-1))
    if c.holes:
        a = rint(1, max(T, 2), slots).unsqueeze(-1)
        sen = (sen | (live.unsqueeze(-1) & (ar >= a) & (ar < a + 3))) & (rand(B, N, N, S, T) < 0.7)
        sen[..., 0] = live
    padp = ~c.pair
    sen[padp] = (rand(B, N, N, S, T) < 0.5)[padp]                                    # padding pairs: random bits, token 0 included
    c.sen = sen
    c.live_slots = sen[..., 0] & c.pair.unsqueeze(-1)
    c.rows, c.pairs = int(c.live_slots.sum()), int(c.live_slots.any(-1).sum())
    c.full = c.pair & c.live_slots.all(-1)                                           # divisor 1e-10
    # ---- distance ids ---------------------------------------------------------------------------------------
    used = sen & c.live_slots.unsqueeze(-1)                                          # live, unmasked tokens of real pairs
    at = used.reshape(-1).nonzero().squeeze(1)
    c.live_tokens = int(at.numel())
    c.covers = c.live_tokens >= ND
    ids = []
    for _ in range(2):
        k = torch.zeros(B * N * N * S * T, dtype=torch.int64)
        k[at] = rint(0, ND, (at.numel(),))
        first = at[torch.randperm(at.numel(), generator=g)[:ND]]
        k[first] = torch.randperm(ND, generator=g)[:first.numel()]
        ids.append(k.view(B, N, N, S, T))
    c.ph_ref, c.pt_ref = ids                                                          # what the reference reads: 0 wherever unused
    junk = {"uint8": list(range(ND, 256)) or [0], "int32": [-1, -7, ND, ND + 1000, 2 ** 31 - 1, -2 ** 31],
            "int64": [-1, -7, ND, ND + 1000, 2 ** 31 - 1, -2 ** 31, 2 ** 40 + 3, -2 ** 40]}[c.dtype]
    junk = torch.tensor(junk, dtype=torch.int64)
    c.ph, c.pt = (torch.where(used, k, junk[rint(0, len(junk), k.shape)]).to(DTYPES[c.dtype]) for k in ids)
    c.used = used
    # ---- padding entities: large finite junk ----------------------------------------------------------------
    pad = ~c.real
    c.node[pad] = (1e3 * (rint(0, 2, c.node.shape) * 2 - 1).float() * (0.5 + rand(*c.node.shape)))[pad]
    # sums over the pairs stay of order one; past 1 024 pairs smaller still: d word_attention.attention_all.bias is analytically zero
    # (the softmax does not see that bias), so the rounding of its cancelling terms meets the bound's absolute floor
    p = max(c.pairs, 1)
    c.cot0 = torch.randn(B, N, N, Hd, generator=g) * min(1.0, 8 / p ** 0.5, 256 / p)
    return c


# ------------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------------
def cotangent(c, scores):
    """The case's float32 cotangent: zero on pairs with a live score inside the flip margin, zero (or scaled by 1e-10) on the
    pairs divided by 1e-10.  -> (cot, fraction of the live pairs taken out for a possible flip)."""
    near = ((scores.abs() < FLIP_MARGIN) & c.live_slots.unsqueeze(-1)).any(-1).any(-1)
    cot = c.cot0.clone()
    cot[near] = 0.0
    cot[c.full] *= 1e-10 if c.scale_full else 0.0
    return cot, float(near.sum()) / max(1, c.pairs)


def reference(c, dtype=torch.float64, cot=None):
    """-> {"E" [B,N,N,Hd], "d ctx", "d node", "d dis_table", "d <parameter>" x 16, "scores" [B,N,N,S,2], "cot", "flips"}; padding
    rows zero.  cot: the cotangent to use (the float32 oracle takes the float64 run's); None derives it from this run's scores."""
    B, N, S, Hd = c.B, c.N, c.S, c.Hd
    cast = lambda t: t.detach().to(dtype)
    sd = {f"{k.split('.', 1)[0]}.0.{k.split('.', 1)[1]}": cast(v).requires_grad_() for k, v in c.sd.items()}
    ctx, node, table = (cast(t).requires_grad_() for t in (c.ctx, c.node, c.table))
    outs, scores = [], torch.full((B, N, N, S, 2), float("inf"), dtype=dtype)
    for b, n in enumerate(c.ns):
        tr = {}
        outs.append(None if n == 0 else O.edge_features_folded(ctx[b], c.sen[b, :n, :n], c.ph_ref[b, :n, :n], c.pt_ref[b, :n, :n],
                                                               node[b, :n], table, sd, 0, trace=tr))
        if n:
            scores[b, :n, :n, :, 0], scores[b, :n, :n, :, 1] = tr["score_h"], tr["score_t"]
    flips = None
    if cot is None:
        cot, flips = cotangent(c, scores)
    E = torch.zeros(B, N, N, Hd, dtype=dtype)
    loss = 0.0
    for b, (n, o) in enumerate(zip(c.ns, outs)):
        if n:
            E[b, :n, :n] = o.detach()
            loss = loss + (o * cot[b, :n, :n].to(dtype)).sum()
    loss.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    ref = {"E": E, "d ctx": zero(ctx), "d node": zero(node), "d dis_table": zero(table)}
    ref.update({"d " + k: zero(sd[f"{k.split('.', 1)[0]}.0.{k.split('.', 1)[1]}"]) for k in c.sd})
    ref.update(scores=scores, cot=cot, flips=flips)
    return ref


@functools.lru_cache(maxsize=None)
def _cached(key):
    c = make_case(**dict(key))
    return c, reference(c)


def case_and_ref(kw):
    """One case and its float64 reference, computed once and shared (never modified) by every test that runs it."""
    return _cached(tuple(sorted(kw.items())))


# ------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------
def ratios(got, ref):
    """Per tensor: the largest |got - ref| / bound over all elements (E: per pair row with the row's own max|ref|)."""
    res = {}
    for k in ("E",) + GRAD_KEYS:
        r = ref[k].detach().double()
        a = got[k].detach().cpu().double()
        assert a.shape == r.shape, f"{k}: shape {tuple(a.shape)} != {tuple(r.shape)}"
        assert torch.isfinite(r).all(), f"{k}: the reference itself is not finite"
        top = r.abs().amax(dim=-1, keepdim=True) if k == "E" else r.abs().max()
        bound = ATOL * top.clamp(min=1.0) + RTOL * r.abs()
        q = torch.nan_to_num((a - r).abs() / bound, nan=float("inf"), posinf=float("inf"))
        res[k] = q.max().item() if q.numel() else 0.0
    return res


def short(res):
    """One line: E, the three input gradients, the worst parameter gradient and its name."""
    k, v = max(((k, v) for k, v in res.items() if k[2:] in PARAM_KEYS), key=lambda t: t[1])
    return " ".join(f"{n}={res[n]:.4f}" for n in ("E", "d ctx", "d node", "d dis_table")) + f" params={v:.4f} ({k[2:]})"
