"""The edge-tensor passes against a plain float64 reference, at their edges.

Kernels under test: edge_fwd / edge_bwd / edge_bcast (csrc/edge.hip, csrc/edge_body.hpp), the GATAttention passenger
(csrc/gat_body.hpp), the N > 64 route through softmax_bwd + colsum + node_score_bwd (csrc/rowops.hip) and the compact-row
consumers (csrc/compact.hip).  The shapes walk every branch those kernels take on a shape: VEC = 4 / VEC = 1, the second
column chunk (D > 256 resp. D > 64), the 16-row unroll boundary of the row loop, N = 64 / 65, the gat_dlogit_slices steps
at D = 64 and 256, the compact rows' D <= 512 bound and their columns lane + 64 k >= D.

Reference: oracle.gcgcn_oracle.gat_attention per document on the float64 slices x[b, :n], E[b, :n, :n] (n = n_valid[b]),
E[b, :n, :n].mean(1) for the edge mean, both padded with zeros; gradients by torch autograd on that float64 graph, with
independent random cotangents on A, Ebar and the input alias.  Dense E holds NaN on padding rows and columns; padding pairs
of the compact cases point at a NaN row of Ec -- a kernel that reads or averages padding returns NaN.

Bound (the project's own, as in test_compact_rows_equal_the_dense_edge_tensor): |got - ref| <= 1e-5 * max(1, max|ref|) +
1e-4 * |ref|, per tensor, every element.  Each case prints its largest error as a fraction of that bound.
"""
import math
from types import SimpleNamespace

import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib, functional as F_, params as P_
from oracle import gcgcn_oracle as O

RTOL, ATOL = 1e-4, 1e-5
DH = 8
P_DROP = 0.3

N_SWEEP = (1, 2, 3, 4, 5, 13, 16, 17, 29, 63, 64, 65, 100)
D_SWEEP = (1, 3, 4, 63, 64, 66, 252, 256, 260, 516)
DENSE_SHAPES = [(n, d) for d in (68, 70) for n in N_SWEEP] + [(n, d) for n in (5, 65) for d in D_SWEEP]
VARIANT_SHAPES = [(17, 68), (65, 70)]
VARIANTS = ("no_ebar", "no_alias", "no_dE")
MEAN_SHAPES = [(n, d) for d in (6, 68) for n in N_SWEEP] + [(17, 1), (17, 260)]
COMPACT_SHAPES = [(n, 130) for n in (1, 3, 4, 5, 17, 64, 65, 100)] + [(n, d) for n in (5, 65) for d in (1, 63, 64, 65, 512)]
COMPACT_TRAIN_SHAPES = [(17, 130), (65, 130)]
PATTERNS = ("random", "dead", "live", "rows")
GAT_KEYS = P_.GAT_KEYS


# ------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------
def make_case(N, D, ragged, pattern=None, masked=False, seed=0):
    """Asymmetric random inputs of one case (float32 masters on the CPU; the float64 reference reads the same values).
    pattern: None = dense E, else the compact rows' prow pattern."""
    g = torch.Generator().manual_seed(1000003 * N + 101 * D + 7 * int(ragged) + 13 * PATTERNS.index(pattern or "random") + seed)
    B = 4 if ragged else 2
    ns = [N, 0, 1, max(N - 1, 1)] if ragged else [N] * B
    c = SimpleNamespace(B=B, N=N, D=D, Dh=DH, ns=ns, ragged=ragged, pattern=pattern)
    c.nv = torch.tensor(ns, dtype=torch.int32) if ragged else None
    real = torch.zeros(B, N, dtype=torch.bool)
    for b, n in enumerate(ns):
        real[b, :n] = True
    c.real = real
    c.pair = real[:, :, None] & real[:, None, :]
    c.x = (torch.rand(B, N, D, generator=g) * 2 - 1) * real[..., None]                     # zero on padding rows (the ABI requires it)
    s = 1.0 / math.sqrt(D)                                                                 # logits of about unit scale
    c.sd = {}
    for k in ("linear_node_h", "linear_node_t", "linear_edge_r"):
        c.sd[k + ".weight"] = torch.randn(DH, D, generator=g) * s
        c.sd[k + ".bias"] = torch.randn(DH, generator=g) * 0.1
    c.sd["wt.weight"] = torch.randn(1, 3 * DH, generator=g) / math.sqrt(DH)
    c.sd["wt.bias"] = torch.randn(1, generator=g) * 0.1
    if pattern is None:
        c.e = torch.randn(B, N, N, D, generator=g)
        c.e[~c.pair] = float("nan")
    else:
        if pattern == "random":
            live = torch.rand(B, N, N, generator=g) < 0.3
        elif pattern == "dead":
            live = torch.zeros(B, N, N, dtype=torch.bool)
        elif pattern == "live":
            live = torch.ones(B, N, N, dtype=torch.bool)
        else:                                                                              # alternating all-live / all-dead rows
            live = torch.zeros(B, N, N, dtype=torch.bool)
            live[:, ::2, :] = True
        live &= c.pair
        Q = int(live.sum())
        c.Q = Q
        c.prow = torch.full((B, N, N), -1, dtype=torch.int32)
        c.prow[live] = torch.randperm(Q, generator=g).to(torch.int32)
        c.prow[~c.pair] = Q + 1                                                            # padding pairs: the NaN row (in range)
        c.Ec = torch.randn(Q + 2, D, generator=g)                                          # row Q: spare capacity, never referenced
        c.Ec[Q + 1] = float("nan")
        c.bias = torch.randn(D, generator=g)
    c.mask = None
    if masked:
        c.mask = torch.rand(B, N, N, generator=g) < 0.4
        for b, n in enumerate(ns):
            if n >= 3:
                c.mask[b, 1, :] = True                                                     # a fully masked real row
                c.mask[b, 2, :] = False                                                    # a row with nothing masked
    c.cA = torch.randn(B, N, N, generator=g)
    c.cE = torch.randn(B, N, D, generator=g)
    c.cX = torch.randn(B, N, D, generator=g)
    c.cE2 = torch.randn(B, N, D, generator=g)                                              # the mean-only consumer's cotangent
    return c


def cpu_keep(c):
    """A keep-mask for the CPU-only conditioning test (the GPU tests replay the kernels' own)."""
    g = torch.Generator().manual_seed(c.N * 31 + c.D)
    return torch.rand(c.B, c.N, c.N, generator=g) >= P_DROP


# ------------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------------
def _leaf(t, dtype, grad=True):
    return t.detach().to(dtype).clone().requires_grad_(grad)


def _edge_leafs(c, dtype, e_grad=True):
    """-> (E [B,N,N,D] as the reference sees it, dict of the leaves it was built from)."""
    if c.pattern is None:
        e = _leaf(c.e, dtype, e_grad)
        return e, {"dE": e}
    Ec, bias = _leaf(c.Ec, dtype), _leaf(c.bias, dtype)
    e = torch.where((c.prow >= 0).unsqueeze(-1), Ec[c.prow.clamp_min(0).long()], bias.expand(c.B, c.N, c.N, -1))
    return e, {"dEc": Ec, "dbias": bias}


def _grads(leafs):
    return {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in leafs.items() if v.requires_grad}


def ref_gat(c, dtype=torch.float64, keep=None, variant="full"):
    """GATAttention + edge mean of case c in `dtype`, forward and backward."""
    B, N, D = c.B, c.N, c.D
    x = _leaf(c.x, dtype)
    sd = {k: _leaf(v, dtype) for k, v in c.sd.items()}
    e, leafs = _edge_leafs(c, dtype, variant != "no_dE")
    A, Ebar = [], []
    for b, n in enumerate(c.ns):
        if n == 0:                                                                          # contributes nothing
            A.append(torch.zeros(N, N, dtype=dtype)), Ebar.append(torch.zeros(N, D, dtype=dtype))
            continue
        es = e[b, :n, :n]
        a = O.gat_attention(x[b, :n], es, sd, mask=None if c.mask is None else c.mask[b, :n, :n],
                            keep=None if keep is None else keep[b, :n, :n], p=P_DROP, apply_mask=c.mask is not None)
        A.append(torch.nn.functional.pad(a, (0, N - n, 0, N - n)))
        Ebar.append(torch.nn.functional.pad(es.mean(1), (0, 0, 0, N - n)))
    A, Ebar = torch.stack(A), torch.stack(Ebar)
    loss = (A * c.cA.to(dtype)).sum()
    if variant != "no_ebar":
        loss = loss + (Ebar * c.cE.to(dtype)).sum()
    if variant != "no_alias":
        loss = loss + (x * c.cX.to(dtype)).sum()                                            # the alias output is x itself
    loss.backward()
    out = {"A": A.detach(), "Ebar": Ebar.detach(), "dX": x.grad}
    out.update(_grads(leafs))
    out.update({"grad " + k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in sd.items()})
    return out


def ref_mean(c, dtype=torch.float64):
    """The edge mean alone (what a MAGGC hop runs) of case c, forward and backward."""
    e, leafs = _edge_leafs(c, dtype)
    Ebar = []
    for b, n in enumerate(c.ns):
        Ebar.append(torch.nn.functional.pad(e[b, :n, :n].mean(1), (0, 0, 0, c.N - n)) if n else torch.zeros(c.N, c.D, dtype=dtype))
    Ebar = torch.stack(Ebar)
    (Ebar * c.cE2.to(dtype)).sum().backward()
    out = {"Ebar": Ebar.detach()}
    out.update(_grads(leafs))
    return out


# ------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------
def check(family, case, got, ref):
    """Every element of every tensor of `ref` against `got` under the bound; prints the case's largest error / bound."""
    assert set(ref) <= set(got), f"{case}: missing {sorted(set(ref) - set(got))}"
    worst, worst_k, bad = 0.0, "-", []
    for k, r in ref.items():
        r = r.detach().double().cpu()
        a = got[k].detach().double().cpu()
        assert a.shape == r.shape, f"{case} {k}: shape {tuple(a.shape)} != {tuple(r.shape)}"
        if r.numel() == 0:
            continue
        assert torch.isfinite(r).all(), f"{case} {k}: the reference itself is not finite"
        bound = ATOL * max(1.0, r.abs().max().item()) + RTOL * r.abs()
        ratio = torch.nan_to_num((a - r).abs() / bound, nan=float("inf"), posinf=float("inf")).max().item()
        if ratio > worst:
            worst, worst_k = ratio, k
        if not ratio <= 1.0:
            bad.append(f"{k}: {ratio:.3g} x bound")
    print(f"[edge-err] {family} {case}: {worst:.4f} of the bound ({worst_k})")
    assert not bad, f"{family} {case}: " + "; ".join(bad)
    return worst


def case_id(c, extra=""):
    return f"N={c.N} D={c.D} {'ragged' if c.ragged else 'dense'}{' ' + c.pattern if c.pattern else ''}{' ' + extra if extra else ''}"


# ------------------------------------------------------------------------------------------------------
# GPU runs
# ------------------------------------------------------------------------------------------------------
def off1(t, dev, fill=None):
    """A contiguous view that starts one float into a larger buffer (4 bytes past a 16-byte boundary)."""
    buf = torch.empty(t.numel() + 1, device=dev)
    v = buf[1:].view(t.shape)
    if fill is None:
        v.copy_(t)
    else:
        v.fill_(fill)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _module(c, dev, train):
    m = gcgcn_amd.GATAttention(c.D, c.Dh, dropout=P_DROP, apply_mask=c.mask is not None).to(dev)
    m.load_state_dict(c.sd, strict=True)
    return m.train(train)


def run_gat(c, dev, train=False, variant="full", misaligned=False):
    """GATAttention (+ the parked edge mean) through the module, forward and backward.  -> (results, keep-mask or None)."""
    put = (lambda t: off1(t, dev)) if misaligned else (lambda t: t.to(dev).clone())
    m = _module(c, dev, train)
    xg = put(c.x).requires_grad_()
    nvg = None if c.nv is None else c.nv.to(dev)
    if c.pattern is None:
        eg = put(c.e).requires_grad_(variant != "no_dE")
        edge, leafs = eg, {"dE": eg}
    else:
        Ecg, bg = put(c.Ec).requires_grad_(), put(c.bias).requires_grad_()
        edge, leafs = F_.CompactEdges(Ecg, c.prow.to(dev), bg, nvg), {"dEc": Ecg, "dbias": bg}
    mask = None if c.mask is None else c.mask.to(dev)
    snaps, orig = [], F_.rng_snapshot

    def spy(d, lazy=False):
        s = orig(d, lazy)
        snaps.append(s)
        return s
    F_.rng_snapshot = spy
    try:
        gcgcn_amd.manual_seed(4321)
        if variant == "no_alias":
            a, xa = m(xg, edge, mask, n_valid=nvg), None
        else:
            a, xa = m(xg, edge, mask, n_valid=nvg, return_input_alias=True)
    finally:
        F_.rng_snapshot = orig
    ebar = F_.take_edge_mean(edge, nvg)
    assert ebar is not None
    outs, cots = [a], [put(c.cA)]
    if variant != "no_ebar":
        outs.append(ebar), cots.append(put(c.cE))
    if xa is not None:
        outs.append(xa), cots.append(put(c.cX))
    torch.autograd.backward(outs, cots)
    keep = None
    if train:
        assert len(snaps) == 1
        keep = F_.dropout_keep_mask(snaps[0], _lib.SALT_GAT, P_DROP, c.B * c.N * c.N).view(c.B, c.N, c.N).cpu()
    got = {"A": a.detach(), "Ebar": ebar.detach(), "dX": xg.grad}
    got.update({k: v.grad for k, v in leafs.items() if v.requires_grad})
    got.update({"grad " + k: v for k, v in m.named_grads().items()})
    return {k: v.cpu() for k, v in got.items()}, keep


def check_padding(c, got):
    """The stated contracts: outputs and dE exactly zero on padding, dEc rows beyond the live pairs exactly zero."""
    if c.ragged:
        if "A" in got:
            assert (got["A"][~c.pair] == 0).all(), "A: padding must be exactly zero"
        assert (got["Ebar"][~c.real] == 0).all(), "Ebar: padding rows must be exactly zero"
        if "dE" in got:
            assert (got["dE"][~c.pair] == 0).all(), "dE: padding must be exactly zero"
    if "dEc" in got:
        assert (got["dEc"][c.Q:] == 0).all(), "dEc: rows beyond the live pairs must stay exactly zero"


def gat_case_runs(c, dev, family, train=False, variant="full", misaligned=False, extra=""):
    got, keep = run_gat(c, dev, train, variant, misaligned)
    ref = ref_gat(c, keep=keep, variant=variant)
    check(family, case_id(c, extra), got, ref)
    check_padding(c, got)
    return got


# ---- 1. dense GATAttention + edge mean, eval mode ----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("N,D", DENSE_SHAPES)
def test_gat_dense_eval(gpu_device, N, D, ragged):
    gat_case_runs(make_case(N, D, ragged), gpu_device, "gat_dense")


@pytest.mark.gpu
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("N,D", VARIANT_SHAPES)
def test_gat_dense_null_operands(gpu_device, N, D, variant, ragged):
    """dEbar NULL (Ebar unused), dX_in NULL (no alias), dE NULL (E needs no gradient)."""
    gat_case_runs(make_case(N, D, ragged), gpu_device, "gat_dense", variant=variant, extra=variant)


# ---- 2. opt-in mask ----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,D", [(5, 68), (65, 70)])
def test_gat_dense_masked(gpu_device, N, D):
    c = make_case(N, D, True, masked=True)
    got = gat_case_runs(c, gpu_device, "gat_dense", extra="masked")
    gone = (c.mask | ~c.real[:, None, :]).all(-1, keepdim=True)                           # every REAL column of the row masked
    part = c.mask & c.pair & ~gone
    assert part.any() and (got["A"][part] == 0).all()                                      # masked pairs carry no weight ...
    assert gone[0, 1] and not gone[0, 2]
    torch.testing.assert_close(got["A"][0, 1], torch.full((N,), 1.0 / N))                  # the fully masked row: uniform


# ---- 3. train mode -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("N,D", VARIANT_SHAPES)
def test_gat_dense_train(gpu_device, N, D, ragged):
    c = make_case(N, D, ragged)
    got = gat_case_runs(c, gpu_device, "gat_dense", train=True, extra="train")
    dropped = (got["A"][c.pair] == 0).float().mean().item()
    assert abs(dropped - P_DROP) < 0.1, f"drop rate {dropped}"


# ---- 4. misalignment ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
def test_gat_dense_misaligned_through_the_modules(gpu_device, ragged):
    """X, E and the cotangents start one float into their allocations: the scalar instantiations of the attention forward
    and of edge_bwd.  Against the reference, not the aligned run (the logit's summation order differs)."""
    gat_case_runs(make_case(17, 68, ragged), gpu_device, "gat_dense", misaligned=True, extra="misaligned")


def _raw_gat(c, dev, ebar_off, dE_off):
    B, N, D, Dh = c.B, c.N, c.D, c.Dh
    nan = float("nan")
    x, e, nv = c.x.to(dev), c.e.to(dev), c.nv.to(dev)
    flat = P_.pack_gat(c.sd, D, torch.empty(P_.gat_layout(D, Dh)[-1]), Dh).to(dev)
    uvc, s = torch.empty(2 * D + 1, device=dev), torch.empty(B, N, device=dev)
    P = torch.full((B, N, N), nan, device=dev)
    ebar = off1(c.cE, dev, fill=nan) if ebar_off else torch.full((B, N, D), nan, device=dev)
    _lib.call("gcgcn_gat_fwd", B, N, D, Dh, F_._p(x), F_._p(e), F_._p(nv), F_._p(flat), None, 0.0, F_._p(uvc), F_._p(s), F_._p(P),
              None, F_._p(ebar), None, None, 0, None, 0, F_._stream())
    cA, cE, cX = c.cA.to(dev), c.cE.to(dev), c.cX.to(dev)
    dX = torch.full((B, N, D), nan, device=dev)
    dE = off1(c.e, dev, fill=nan) if dE_off else torch.full((B, N, N, D), nan, device=dev)
    dflat = torch.full_like(flat, nan)
    dlogit, ds = torch.empty(B, N, N, device=dev), torch.empty(B, N, device=dev)
    dvpart, duvc = torch.empty(B * N, D, device=dev), torch.empty(2 * D + 1, device=dev)
    scratch = torch.empty(max(int(_lib.lib().gcgcn_gat_bwd_scratch(B, N, D)), 1), device=dev)
    _lib.call("gcgcn_gat_bwd", B, N, D, Dh, F_._p(x), F_._p(e), F_._p(nv), F_._p(flat), None, 0.0, F_._p(uvc), F_._p(P), F_._p(cA),
              F_._p(cE), F_._p(cX), F_._p(dX), F_._p(dE), F_._p(dflat), F_._p(dlogit), F_._p(ds), F_._p(dvpart), F_._p(duvc),
              F_._p(scratch), None, F_._stream())
    torch.cuda.synchronize()
    got = {"A": P, "Ebar": ebar, "dX": dX, "dE": dE}
    got.update({"grad " + k: v for k, v in P_.unpack_gat(dflat, D, Dh).items()})
    return {k: v.cpu() for k, v in got.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["Ebar", "dE"])
def test_gat_dense_one_misaligned_operand(gpu_device, which):
    """Raw ABI: only Ebar (gcgcn_gat_fwd), respectively only dE (gcgcn_gat_bwd), starts 4 bytes into its allocation."""
    c = make_case(17, 68, True)
    got = _raw_gat(c, gpu_device, which == "Ebar", which == "dE")
    check("gat_dense", case_id(c, f"raw, {which} misaligned"), got, ref_gat(c))
    check_padding(c, got)


# ---- 5. the edge mean alone --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("N,D", MEAN_SHAPES)
def test_edge_mean_alone(gpu_device, N, D, ragged):
    """gcgcn_edge_mean_fwd / _bwd into NaN-filled outputs."""
    c = make_case(N, D, ragged)
    dev = gpu_device
    e, cE = c.e.to(dev), c.cE2.to(dev)
    nv = None if c.nv is None else c.nv.to(dev)
    ebar = torch.full((c.B, N, D), float("nan"), device=dev)
    dE = torch.full((c.B, N, N, D), float("nan"), device=dev)
    _lib.call("gcgcn_edge_mean_fwd", c.B, N, D, F_._p(e), F_._p(nv), F_._p(ebar), F_._stream())
    _lib.call("gcgcn_edge_mean_bwd", c.B, N, D, F_._p(cE), F_._p(nv), F_._p(dE), F_._stream())
    got = {"Ebar": ebar.cpu(), "dE": dE.cpu()}
    check("edge_mean", case_id(c), got, ref_mean(c))
    if ragged:
        assert (got["Ebar"][~c.real] == 0).all() and (got["dE"][~c.pair] == 0).all(), "padding must be exactly zero"


# ---- 6. compact consumers ----------------------------------------------------------------------------
def run_mean_compact(c, dev):
    Ecg, bg = c.Ec.to(dev).requires_grad_(), c.bias.to(dev).requires_grad_()
    nvg = None if c.nv is None else c.nv.to(dev)
    ebar = F_.edge_mean(F_.CompactEdges(Ecg, c.prow.to(dev), bg, nvg), nvg)
    ebar.backward(c.cE2.to(dev))
    return {"Ebar": ebar.detach().cpu(), "dEc": Ecg.grad.cpu(), "dbias": bg.grad.cpu()}


def compact_case_runs(c, dev, train=False):
    extra = "train" if train else ""
    got = gat_case_runs(c, dev, "gat_compact", train=train, extra=extra)
    got2 = run_mean_compact(c, dev)
    check("mean_compact", case_id(c, extra), got2, ref_mean(c))
    check_padding(c, got2)
    return got, got2


@pytest.mark.gpu
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("N,D", COMPACT_SHAPES)
def test_compact_eval(gpu_device, N, D, pattern, ragged):
    compact_case_runs(make_case(N, D, ragged, pattern), gpu_device)


@pytest.mark.gpu
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("N,D", COMPACT_TRAIN_SHAPES)
def test_compact_train(gpu_device, N, D, ragged):
    compact_case_runs(make_case(N, D, ragged, "random"), gpu_device, train=True)


@pytest.mark.gpu
def test_compact_width_bound_is_loud(gpu_device):
    """D = 516 > 512: the forward calls and the mean-only backward refuse."""
    dev = gpu_device
    c = make_case(5, 516, False, "random")
    ce = F_.CompactEdges(c.Ec.to(dev), c.prow.to(dev), c.bias.to(dev), None)
    m = _module(c, dev, False)
    with pytest.raises(RuntimeError, match="compact rows support"):
        m(c.x.to(dev), ce)
    with pytest.raises(RuntimeError, match="compact rows support"):
        F_.edge_mean(ce)
    dEc, dbias = torch.zeros_like(ce.Ec), torch.empty(c.D, device=dev)
    rowbuf, cE = torch.empty(2 * c.B * c.N, device=dev), c.cE2.to(dev)
    with pytest.raises(RuntimeError, match="compact rows support"):
        _lib.call("gcgcn_edge_mean_bwd_compact", c.B, c.N, c.D, F_._p(ce.prow), None, F_._p(cE), F_._p(dEc), F_._p(dbias),
                  F_._p(rowbuf), F_._stream())
    torch.cuda.synchronize()


# ---- 7. repeatability --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N,D,pattern", [(65, 70, None), (65, 130, "random")])
def test_two_runs_are_bitwise_equal(gpu_device, N, D, pattern):
    """'Every sum in a fixed order': ragged, train mode, the same dropout snapshot -> identical bits."""
    c = make_case(N, D, True, pattern)
    runs = []
    for _ in range(2):
        got, keep = run_gat(c, gpu_device, train=True)
        got["keep"] = keep
        if pattern is not None:
            got.update({"mean " + k: v for k, v in run_mean_compact(c, gpu_device).items()})
        runs.append(got)
    assert set(runs[0]) == set(runs[1])
    for k in runs[0]:
        assert torch.isfinite(runs[0][k].float()).all(), k
        assert torch.equal(runs[0][k], runs[1][k]), f"{k}: two runs differ"


# ---- 8. conditioning (CPU) ---------------------------------------------------------------------------
def all_parameter_sets():
    """(kind, case kwargs, train, variant) of every case above."""
    sets = []
    for ragged in (False, True):
        sets += [("gat", dict(N=n, D=d, ragged=ragged), False, "full") for n, d in DENSE_SHAPES]
        sets += [("gat", dict(N=n, D=d, ragged=ragged), False, v) for n, d in VARIANT_SHAPES for v in VARIANTS]
        sets += [("gat", dict(N=n, D=d, ragged=ragged), True, "full") for n, d in VARIANT_SHAPES]           # + misaligned, repeat
        sets += [("mean", dict(N=n, D=d, ragged=ragged), False, "full") for n, d in MEAN_SHAPES]
        sets += [("compact", dict(N=n, D=d, ragged=ragged, pattern=p), False, "full") for n, d in COMPACT_SHAPES for p in PATTERNS]
        sets += [("compact", dict(N=n, D=d, ragged=ragged, pattern="random"), True, "full") for n, d in COMPACT_TRAIN_SHAPES]
    sets += [("gat", dict(N=n, D=d, ragged=True, masked=True), False, "full") for n, d in ((5, 68), (65, 70))]
    return sets


def test_float32_oracle_meets_the_bound_on_every_case():
    """The inputs are well conditioned: the oracle evaluated in float32 stays inside the bound against the float64 reference
    on every parameter set of this file, so the reference alone does not use the bound up."""
    worst = 0.0
    for kind, kw, train, variant in all_parameter_sets():
        c = make_case(**kw)
        keep = cpu_keep(c) if train else None
        extra = " ".join(s for s in ("train" if train else "", variant if variant != "full" else "", "masked" if c.mask is not None else "") if s)
        if kind != "mean":
            worst = max(worst, check("oracle_fp32_gat", case_id(c, extra), ref_gat(c, torch.float32, keep, variant),
                                     ref_gat(c, torch.float64, keep, variant)))
        if kind != "gat":
            worst = max(worst, check("oracle_fp32_mean", case_id(c, extra), ref_mean(c, torch.float32), ref_mean(c, torch.float64)))
    print(f"[edge-err] float32 oracle, worst case: {worst:.4f} of the bound")
