"""The classifier head (csrc/head.hip) against a plain float64 reference, at its kernels' edges.

Kernels under test: head_gemm_kernel<1..4>, head_bil2_kernel<1..3>, head_bil3_kernel<1..3> (plain and split four ways over K +
head_bil_combine_kernel), head_dw_kernel, the compacted pair rows of a ragged batch (head_index / head_prow / head_feat_fwd /
head_pad / head_node_bwd / head_table_rel_bwd and the GEMM layer's products on a device-side row count), the two table kernels.
The cases walk what head_plan branches on -- R at 32 / 64 / 65 / 96 / 97 / 128, dense / ragged, the three generation settings
and each of the four A/B options -- plus pair counts at the tile edges (63 / 64 / 65 and 127 / 128 / 129 rows), device-side
counts either side of the 32 768 launch-shape boundary, N = 1, empty documents, an all-empty batch, other Hd / nf / Pt / Pr /
dis_plus / ND, and padding that holds junk.  Every case asserts through gcgcn_debug_head_plan that it reaches the plan it was
written for.

Reference: oracle.gcgcn_oracle.classifier_head in float64, per document on the real slices feats[b, :n], type[b, :n],
rel[b, :n, :n] (n = n_valid[b]); gradients by torch autograd on that float64 graph with an independent random cotangent;
parameter and table gradients summed over documents in float64.  The float32 masters live on the CPU: kernel and reference
read the same values.  Cases above 4 096 pairs run the same oracle function in float64 on the device with plain torch ops
(test_device_reference_equals_cpu_reference ties the two to 1e-12).

Bound (the project's own, tests/test_edge_gpu.py): |got - ref| <= 1e-5 * max(1, max|ref|) + 1e-4 * |ref|, per tensor, on every
element.  The float32 oracle itself uses at most 0.051 of it on these inputs (test_float32_oracle_is_well_inside_the_bound keeps
that under 0.25).  Each GPU case prints its worst error as a fraction of the bound, per tensor.  Measured on an MI355X over all
152 GPU cases (no bound raised): logits 0.25, d feats 0.24, d dense_layer.weight 0.27 / bias 0.18, d bili_layer_01.weight 0.13 /
bias 0.01, d classification_layer_01.weight 0.04 / bias 0.01, d ner_emb 0.25, d dis_embed 0.20.
"""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib, functional as F_, params as P_
from oracle import gcgcn_oracle as O

RTOL, ATOL = 1e-4, 1e-5
HW = 128
OPTS_DEFAULT = {"head_v1": -1, "head_bil3": 1, "head_bil3_bwd": 1, "head_dw3": 1, "head_compact": 1}
GENERATIONS = {"by_size": {}, "gen1": {"head_v1": 1}, "gen2": {"head_v1": 0}}
SWITCHES = ("head_bil3", "head_bil3_bwd", "head_dw3", "head_compact")
GEMM, TILE64, TILE128 = 0, 1, 2
PARAM_KEYS = tuple(P_.HEAD_STATE_ORDER)


# ------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------
def make_case(B, N, R, nv=None, Hd=128, nf=3, Pt=20, Pr=20, dis_plus=10, ND=None, seed=0):
    """Random inputs of one case, float32 on the CPU.  nv: the documents' entity counts (None = a batch without n_valid).  The
    largest document holds every node type and every relative-position id when it has room for them."""
    ND = 2 * dis_plus + 1 if ND is None else ND
    g = torch.Generator().manual_seed(100003 * B + 1009 * N + 31 * R + 7 * Hd + 3 * nf + Pt + 5 * ND + seed + (0 if nv is None else 17 + sum(nv)))
    c = SimpleNamespace(B=B, N=N, R=R, Hd=Hd, nf=nf, Pt=Pt, Pr=Pr, dis_plus=dis_plus, ND=ND, ragged=nv is not None)
    c.ns = [N] * B if nv is None else list(nv)
    assert len(c.ns) == B and all(0 <= n <= N for n in c.ns)
    c.nv = None if nv is None else torch.tensor(c.ns, dtype=torch.int32)
    c.real = torch.arange(N)[None, :] < torch.tensor(c.ns)[:, None]
    c.pair = c.real[:, :, None] & c.real[:, None, :]
    c.count = int(c.pair.sum())
    c.feats = [torch.rand(B, N, Hd, generator=g) * 2 - 1 for _ in range(nf)]
    c.ntype = torch.randint(0, 7, (B, N), generator=g)
    c.rel = torch.randint(-dis_plus, dis_plus + 1, (B, N, N), generator=g)
    b, n = max(enumerate(c.ns), key=lambda t: t[1])
    c.covers = n >= 7 and n * n >= 2 * dis_plus + 1
    if c.covers:
        c.ntype[b, :7] = torch.randperm(7, generator=g)
        blk = c.rel[b, :n, :n].reshape(-1)
        blk[torch.randperm(n * n, generator=g)[:2 * dis_plus + 1]] = torch.arange(-dis_plus, dis_plus + 1)
        c.rel[b, :n, :n] = blk.view(n, n)
    c.cot = torch.randn(B, N, N, R, generator=g)
    Fin = Hd * nf + Pt + Pr
    u = lambda *s, k: (torch.rand(*s, generator=g) * 2 - 1) / k ** 0.5           # nn.Linear / nn.Bilinear initial ranges
    c.sd = {"dense_layer.weight": u(HW, Fin, k=Fin), "dense_layer.bias": u(HW, k=Fin),
            "bili_layer_01.weight": u(R, HW, HW, k=HW), "bili_layer_01.bias": u(R, k=HW),
            "classification_layer_01.weight": u(R, 2 * HW, k=2 * HW), "classification_layer_01.bias": u(R, k=2 * HW),
            "ner_emb.weight": torch.randn(7, Pt, generator=g) * 0.3, "dis_embed.weight": torch.randn(ND, Pr, generator=g) * 0.3}
    return c


def case_id(c):
    return (f"B={c.B} N={c.N} R={c.R} Hd={c.Hd} nf={c.nf} Pt={c.Pt} Pr={c.Pr} dp={c.dis_plus} ND={c.ND} "
            f"{'nv=' + (str(c.ns) if c.B <= 4 else str(c.count) + ' pairs') if c.ragged else 'dense'}")


# ------------------------------------------------------------------------------------------------------
# reference
# ------------------------------------------------------------------------------------------------------
def reference(c, dtype=torch.float64, device="cpu"):
    """-> {"logits" [B,N,N,R] (zero on padding pairs), "d f<k>" [B,N,Hd] (zero on padding rows), "d <parameter / table>"}."""
    cast = lambda t: t.detach().to(device=device, dtype=dtype)
    sd = {k: cast(v).requires_grad_() for k, v in c.sd.items()}
    feats = [cast(f).requires_grad_() for f in c.feats]
    ntype, rel, cot = c.ntype.to(device), c.rel.to(device), cast(c.cot)
    logits = torch.zeros(c.B, c.N, c.N, c.R, dtype=dtype, device=device)
    for b, n in enumerate(c.ns):
        if n == 0:
            continue
        out = O.classifier_head([f[b, :n] for f in feats], ntype[b, :n], rel[b, :n, :n], sd, c.dis_plus)
        (out * cot[b, :n, :n]).sum().backward()                                    # leaves accumulate over the documents
        logits[b, :n, :n] = out.detach()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    ref = {"logits": logits}
    ref.update({f"d f{k}": zero(f) for k, f in enumerate(feats)})
    ref.update({"d " + k: zero(v) for k, v in sd.items()})
    return ref


@functools.lru_cache(maxsize=None)
def _cached(key):
    c = make_case(*key[:3], nv=key[3], **dict(key[4]))
    return c, reference(c)


def case_and_ref(B, N, R, nv=None, **kw):
    """One case and its CPU float64 reference, computed once and shared (never modified) by every test that runs it."""
    return _cached((B, N, R, None if nv is None else tuple(nv), tuple(sorted(kw.items()))))


# ------------------------------------------------------------------------------------------------------
# the kernels
# ------------------------------------------------------------------------------------------------------
class options:
    """Set head options for a block; the defaults come back whatever happens inside."""

    def __init__(self, **opts):
        self.opts = dict(OPTS_DEFAULT, **opts)

    def __enter__(self):
        for k, v in self.opts.items():
            _lib.call("gcgcn_set_option", k.encode(), v)
        return self.opts

    def __exit__(self, *exc):
        for k, v in OPTS_DEFAULT.items():
            _lib.call("gcgcn_set_option", k.encode(), v)


def plan_of(c):
    out = (ctypes.c_int32 * 6)()
    _lib.call("gcgcn_debug_head_plan", c.B, c.N, c.R, int(c.ragged), ctypes.cast(out, ctypes.c_void_p))
    return dict(zip(("compact", "fwd", "bwd_e", "dw", "fwd_by_count", "bwd_by_count"), out))


def plan_rule(c, opts):
    """What include/gcgcn.h and head_plan's comments promise for this shape under these options."""
    pairs = c.B * c.N * c.N
    past96 = 64 < c.R <= 97
    gen1 = opts["head_v1"] != 0 if opts["head_v1"] >= 0 else (pairs + 127) // 128 < 256
    compact = bool(c.ragged and opts["head_compact"] and past96)
    fwd = TILE128 if opts["head_bil3"] and past96 else TILE64 if compact or not gen1 else GEMM
    bwd = (TILE128 if opts["head_bil3_bwd"] else TILE64) if compact or not gen1 else GEMM
    dw = int(compact or bool(opts["head_dw3"] and past96 and not gen1))
    return {"compact": int(compact), "fwd": fwd, "bwd_e": bwd, "dw": dw, "fwd_by_count": int(compact and fwd == TILE128),
            "bwd_by_count": int(compact and bwd == TILE128)}


def run_head(c, dev, feats=None, ntype=None, rel=None, cot=None):
    """Forward + backward on the GPU -> the same dict of tensors as reference()."""
    dims = (c.Hd, c.nf, c.Pt, c.Pr, c.R)
    flat = torch.zeros(P_.head_layout(*dims)[-1])
    P_.pack_head(c.sd, *dims, flat)
    flat = flat.to(dev).requires_grad_()
    fg = [f.to(dev).requires_grad_() for f in (c.feats if feats is None else feats)]
    ner, dis = c.sd["ner_emb.weight"].to(dev).requires_grad_(), c.sd["dis_embed.weight"].to(dev).requires_grad_()
    out = F_.classifier_head(fg, (c.ntype if ntype is None else ntype).to(dev), (c.rel if rel is None else rel).to(dev), ner, dis, flat,
                             c.R, None if c.nv is None else c.nv.to(dev), c.dis_plus)
    out.backward((c.cot if cot is None else cot).to(dev))
    got = {"logits": out.detach()}
    got.update({f"d f{k}": f.grad for k, f in enumerate(fg)})
    got.update({"d " + k: v for k, v in P_.unpack_head(flat.grad, *dims).items()})
    got["d ner_emb.weight"], got["d dis_embed.weight"] = ner.grad, dis.grad
    return got


# ------------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------------
def ratios(c, got, ref, compact):
    """Per tensor: the largest |got - ref| / bound over the elements the head defines (logits of padding pairs are defined --
    exactly zero -- on the compacted path only)."""
    assert set(ref) <= set(got), f"missing {sorted(set(ref) - set(got))}"
    res = {}
    for k, r in ref.items():
        r = r.detach().double()
        a = got[k].detach().to(r.device).double()
        assert a.shape == r.shape, f"{k}: shape {tuple(a.shape)} != {tuple(r.shape)}"
        if r.numel() == 0:
            continue
        assert torch.isfinite(r).all(), f"{k}: the reference itself is not finite"
        bound = ATOL * max(1.0, r.abs().max().item()) + RTOL * r.abs()
        q = torch.nan_to_num((a - r).abs() / bound, nan=float("inf"), posinf=float("inf"))
        if k == "logits" and c.ragged and not compact:
            q = q[c.pair.to(q.device)]
        res[k] = q.max().item() if q.numel() else 0.0
    return res


def check(family, c, got, ref, compact, extra=""):
    res = ratios(c, got, ref, compact)
    print(f"[head-err] {family} {case_id(c)} {extra}: " + " ".join(f"{k}={v:.4f}" for k, v in res.items()))
    bad = [f"{k}: {v:.3g} x bound" for k, v in res.items() if not v <= 1.0]
    assert not bad, f"{family} {case_id(c)} {extra}: " + "; ".join(bad)
    if c.ragged:
        pad = ~c.real.to(got["logits"].device)
        for k in range(c.nf):
            assert float(got[f"d f{k}"][pad].abs().sum()) == 0.0, f"d f{k} of padding entities must be exactly zero"
        if compact and c.count < c.B * c.N * c.N:
            assert float(got["logits"][~c.pair.to(pad.device)].abs().max()) == 0.0, "logits of padding pairs must be exactly zero"
    assert float(got["d ner_emb.weight"][0].abs().sum()) == 0.0, "row 0 of d ner_emb (padding_idx) must be exactly zero"
    return res


def run_and_check(family, dev, c, ref, opts, want=None, extra=""):
    """Under `opts`: the plan is the one the rule names (and holds what `want` pins), then forward + backward against ref."""
    with options(**opts) as full:
        plan = plan_of(c)
        assert plan == plan_rule(c, full), f"{case_id(c)} {extra}: plan {plan}, the rule says {plan_rule(c, full)}"
        for k, v in (want or {}).items():
            assert plan[k] == v, f"{case_id(c)} {extra}: this case was written for {k} = {v}, the plan has {plan[k]}"
        got = run_head(c, dev)
    return got, check(family, c, got, ref, bool(plan["compact"]), extra)


# ------------------------------------------------------------------------------------------------------
# CPU: the bound is not vacuous
# ------------------------------------------------------------------------------------------------------
SMALL_SHAPES = [(9, 97, 3, 128), (13, 5, 2, 128), (20, 128, 1, 64)]


@pytest.mark.parametrize("N,R,nf,Hd", SMALL_SHAPES, ids=[f"N={s[0]} R={s[1]} nf={s[2]} Hd={s[3]}" for s in SMALL_SHAPES])
def test_float32_oracle_is_well_inside_the_bound(N, R, nf, Hd):
    """The float32 oracle against the float64 oracle on the smallest cases: under a quarter of the bound on every tensor
    (measured: at most 0.051, also at N = 45), so the inputs are well conditioned and the bound leaves a kernel no slack a
    plain float32 evaluation does not need."""
    c = make_case(2, N, R, nv=[N, max(N // 2, 1)], Hd=Hd, nf=nf)
    res = ratios(c, reference(c, torch.float32), reference(c), compact=True)
    print(f"[head-err] float32 oracle {case_id(c)}: " + " ".join(f"{k}={v:.4f}" for k, v in res.items()))
    assert max(res.values()) < 0.25, res


def test_plan_rule_matches_the_library():
    """The rule the cases are written against equals head_plan on every (R, raggedness, option) combination they use
    (no GPU: the plan is a host function)."""
    for R in (1, 31, 32, 33, 64, 65, 95, 96, 97, 98, 127, 128):
        for nv in (None, [9, 0, 4]):
            for B, N in ((3, 9), (9, 64)):
                c = SimpleNamespace(B=B, N=N, R=R, ragged=nv is not None)
                for v1 in (-1, 0, 1):
                    for off in (None,) + SWITCHES:
                        with options(head_v1=v1, **({off: 0} if off else {})) as full:
                            assert plan_of(c) == plan_rule(c, full), (B, N, R, nv, full)


# ------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------
R_SWEEP = (1, 31, 32, 33, 64, 65, 95, 96, 97, 98, 127, 128)
RAGGED_SWEEP = [9, 0, 4]


@pytest.mark.gpu
@pytest.mark.parametrize("gen", list(GENERATIONS))
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("R", R_SWEEP)
def test_r_sweep(gpu_device, R, ragged, gen):
    """Every R at which a kernel branches, dense and with an empty document in the batch, under the three generation settings:
    R = 65 .. 96 takes the kernels that keep column / row 96 on the vector ALU although it does not exist there."""
    c, ref = case_and_ref(3, 9, R, RAGGED_SWEEP if ragged else None)
    assert c.covers
    run_and_check("R sweep", gpu_device, c, ref, GENERATIONS[gen], extra=gen)


@pytest.mark.gpu
@pytest.mark.parametrize("off", SWITCHES)
@pytest.mark.parametrize("ragged", [False, True], ids=["dense", "ragged"])
@pytest.mark.parametrize("R", (65, 96, 97))
def test_r_past_64_with_one_switch_off(gpu_device, R, ragged, off):
    """The relation counts served by the 128-pair tile / head_dw_kernel with each A/B option switched off in turn (second
    generation forced for the dense batch, so that each option decides something)."""
    c, ref = case_and_ref(3, 9, R, RAGGED_SWEEP if ragged else None)
    want = {"head_bil3": {"fwd": TILE64}, "head_bil3_bwd": {"bwd_e": TILE64}, "head_dw3": {"dw": int(ragged)},
            "head_compact": {"compact": 0}}[off]
    run_and_check("switch off", gpu_device, c, ref, {"head_v1": 0, off: 0}, want, extra=f"{off}=0")


TILE_DENSE = {63: (7, 3), 64: (1, 8), 65: (65, 1), 121: (1, 11), 128: (2, 8), 162: (2, 9)}     # pairs = B N^2: (B, N)
TILE_COMPACT = {63: [7, 3, 2, 1], 64: [8], 65: [8, 1], 127: [11, 2, 1, 1], 128: [8, 8], 129: [8, 8, 1]}
BIL2 = {"head_bil3": 0, "head_bil3_bwd": 0}


@pytest.mark.gpu
@pytest.mark.parametrize("tile,rows", [(128, 121), (128, 128), (128, 162), (64, 63), (64, 64), (64, 65)])
def test_tile_boundaries_dense(gpu_device, tile, rows):
    """Pair counts at the edges of the 128-pair tile (head_bil3) and of the 64-pair tile (head_bil2), every pair slot computed."""
    B, N = TILE_DENSE[rows]
    assert B * N * N == rows
    c, ref = case_and_ref(B, N, 97)
    t = TILE128 if tile == 128 else TILE64
    run_and_check("tile edge", gpu_device, c, ref, dict({"head_v1": 0}, **(BIL2 if tile == 64 else {})), {"fwd": t, "bwd_e": t, "dw": 1, "compact": 0})


@pytest.mark.gpu
@pytest.mark.parametrize("tile,rows", [(128, 127), (128, 128), (128, 129), (64, 63), (64, 64), (64, 65)])
def test_tile_boundaries_compacted(gpu_device, tile, rows):
    """The same edges on the compacted rows of a ragged batch padded to N = 12 (128-pair tiles: split four ways over K)."""
    nv = TILE_COMPACT[rows]
    assert sum(n * n for n in nv) == rows
    c, ref = case_and_ref(len(nv), 12, 97, nv)
    t = TILE128 if tile == 128 else TILE64
    run_and_check("tile edge", gpu_device, c, ref, dict({"head_v1": 0}, **(BIL2 if tile == 64 else {})),
                  {"fwd": t, "bwd_e": t, "dw": 1, "compact": 1, "fwd_by_count": int(tile == 128)})


LAUNCH_SHAPES = {32767: [64] * 7 + [63, 11, 2, 1], 32768: [64] * 8, 32769: [64] * 8 + [1]}


@pytest.mark.gpu
@pytest.mark.parametrize("count", list(LAUNCH_SHAPES))
def test_launch_shape_boundary(gpu_device, count):
    """Device-side counts either side of 32 768, where head_pass switches between the four-way K split + combine and the plain
    128-pair tiles (both are launched, one leaves): exactly one of them must have run.  Float64 reference on the device."""
    nv = LAUNCH_SHAPES[count]
    c = make_case(len(nv), 64, 97, nv=nv)
    assert c.count == count
    ref = reference(c, device=gpu_device)
    got, _ = run_and_check("launch shape", gpu_device, c, ref, {}, {"compact": 1, "fwd": TILE128, "bwd_e": TILE128, "dw": 1,
                                                                    "fwd_by_count": 1, "bwd_by_count": 1})
    if count < c.B * 64 * 64:
        assert float(got["logits"][~c.pair.to(gpu_device)].abs().max()) == 0.0
    again = run_head(c, gpu_device)
    assert all(torch.equal(got[k], again[k]) for k in got), "two runs differ"


@pytest.mark.gpu
def test_device_reference_equals_cpu_reference(gpu_device):
    """The float64 reference computed on the device (plain torch ops) against the one computed on the CPU: 1e-12 relative."""
    c, ref = case_and_ref(3, 9, 97, RAGGED_SWEEP)
    dref = reference(c, device=gpu_device)
    for k, r in ref.items():
        d = (dref[k].cpu() - r).abs().max().item()
        assert d <= 1e-12 * max(1.0, r.abs().max().item()), f"{k}: {d}"


SMALL = [(1, 1, None), (3, 1, None), (3, 1, [1, 0, 1]), (3, 9, [0, 1, 9]), (2, 5, [1, 1])]


@pytest.mark.gpu
@pytest.mark.parametrize("R", (97, 5))
@pytest.mark.parametrize("B,N,nv", SMALL, ids=[f"B={b} N={n} {'dense' if v is None else v}" for b, n, v in SMALL])
def test_small_and_empty_documents(gpu_device, B, N, nv, R):
    """N = 1, one-entity and empty documents beside a full one (R = 97: compacted rows; R = 5: every slot computed)."""
    c, ref = case_and_ref(B, N, R, nv)
    for gen in GENERATIONS:
        run_and_check("small", gpu_device, c, ref, GENERATIONS[gen], extra=gen)


@pytest.mark.gpu
@pytest.mark.parametrize("R", (97, 5))
def test_all_empty_batch(gpu_device, R):
    """Every document empty.  On the compacted path the device-side count is 0: every tile kernel leaves before it clamps with
    count - 1, head_dw_kernel and the GEMM layer's count-in-K products run zero k-steps and store zeros, the count-in-M products
    walk zero tiles, head_table_rel_bwd's item range is empty.  Exact zeros everywhere (the dense layer's weight gradient is an
    exact zero times the finite feature rows)."""
    c, ref = case_and_ref(3, 4, R, [0, 0, 0])
    assert c.count == 0
    got, _ = run_and_check("all empty", gpu_device, c, ref, {}, {"compact": int(R == 97)})
    for k, v in got.items():
        if k == "logits" and R != 97:
            continue                                                               # every slot computed: padding logits are unspecified
        assert float(v.abs().max()) == 0.0, f"{k} must be exactly zero"


DIMS = [dict(Hd=4), dict(Hd=64), dict(Hd=132), dict(nf=1), dict(nf=4), dict(Pt=4, Pr=36), dict(dis_plus=3, ND=7), dict(ND=32)]


@pytest.mark.gpu
@pytest.mark.parametrize("R,ragged", [(97, True), (97, False), (5, True)], ids=["R=97 ragged", "R=97 dense", "R=5 ragged"])
@pytest.mark.parametrize("dims", DIMS, ids=[" ".join(f"{k}={v}" for k, v in d.items()) for d in DIMS])
def test_other_dimensions(gpu_device, dims, R, ragged):
    """Feature widths off the tile (Hd = 4, 132), one and four feature groups, unequal table widths, a 7-row and a 32-row distance
    table; every node type and every relative-position id present."""
    c, ref = case_and_ref(3, 9, R, RAGGED_SWEEP if ragged else None, **dims)
    assert c.covers and set(c.ntype[c.real].tolist()) == set(range(7))
    assert set(c.rel[c.pair].tolist()) == set(range(-c.dis_plus, c.dis_plus + 1))
    run_and_check("dims", gpu_device, c, ref, {"head_v1": 0} if not ragged else {})


def junk_padding(c, seed):
    """The case's inputs with padding that a correct head never lets through: feature rows of padding entities hold +-1e3
    (finite: include/gcgcn.h), their ids and the ids of padding pairs other in-range values, dlogits of padding pairs NaN."""
    g = torch.Generator().manual_seed(seed)
    pad, padp = ~c.real, ~c.pair
    feats = []
    for f in c.feats:
        f = f.clone()
        f[pad] = (1e3 * (torch.randint(0, 2, f.shape, generator=g) * 2 - 1).float() * (0.5 + torch.rand(f.shape, generator=g)))[pad]
        feats.append(f)
    ntype, rel, cot = c.ntype.clone(), c.rel.clone(), c.cot.clone()
    ntype[pad] = torch.randint(0, 7, ntype.shape, generator=g)[pad]
    rel[padp] = torch.randint(-c.dis_plus, c.dis_plus + 1, rel.shape, generator=g)[padp]
    cot[padp] = float("nan")
    return dict(feats=feats, ntype=ntype, rel=rel, cot=cot)


@pytest.mark.gpu
@pytest.mark.parametrize("R,opts", [(97, {}), (5, {}), (97, {"head_compact": 0, "head_v1": 0})],
                         ids=["R=97 compacted", "R=5 every slot", "R=97 every slot gen2"])
def test_padding_contents_do_not_matter(gpu_device, R, opts):
    """Two runs with different junk in the padding: everything real is bitwise equal between them and within the bound of the
    reference (which never sees the padding), d feats of padding rows exactly zero, no NaN from the padded dlogits.  This pins
    the header's contract: ids and dlogits of padding may hold anything, padded feature rows anything finite."""
    c, ref = case_and_ref(3, 9, R, [9, 2, 5])
    with options(**opts) as full:
        plan = plan_of(c)
        assert plan == plan_rule(c, full) and plan["compact"] == int(R == 97 and not opts)
        runs = [run_head(c, gpu_device, **junk_padding(c, seed)) for seed in (1, 2)]
    pair = c.pair.to(gpu_device)
    for got in runs:
        if not plan["compact"]:
            got["logits"] = torch.where(pair[..., None], got["logits"], torch.zeros_like(got["logits"]))   # unspecified slots
        check("padding", c, got, ref, True)
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), f"{k} depends on what the padding holds"


@pytest.mark.gpu
def test_refusals(gpu_device):
    """A distance table of more than 32 rows is refused where the forward is called (it used to run forward and fail in the
    backward pass with "bad shape"), by the Python wrapper and by the library; R > 128 and widths that are no multiple of 4
    keep their refusals."""
    dev = gpu_device

    def call(R=97, Hd=128, Pt=20, Pr=20, ND=21, raw=False):
        c = make_case(1, 4, min(R, 128), Hd=Hd, Pt=Pt, Pr=Pr, ND=ND)
        flat = torch.zeros(P_.head_layout(Hd, 3, Pt, Pr, R)[-1], device=dev)
        args = [f.to(dev) for f in c.feats], c.ntype.to(dev), c.rel.to(dev), c.sd["ner_emb.weight"].to(dev), c.sd["dis_embed.weight"].to(dev)
        if raw:                                                                    # past the wrapper's own check: the library's
            return F_.HeadFn.apply(flat, args[3], args[4], args[1], args[2], None, R, 10, *args[0])
        return F_.classifier_head(*args, flat, R)

    with pytest.raises(ValueError, match="at most 32 rows"):
        call(ND=33)
    with pytest.raises(RuntimeError, match=r"head_fwd.*33 rows.*at most 32"):
        call(ND=33, raw=True)
    assert call(ND=32).shape == (1, 4, 4, 97)
    with pytest.raises(RuntimeError, match="head_sizes: bad arguments"):
        call(R=129)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        call(Hd=6)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        call(Pt=6)
