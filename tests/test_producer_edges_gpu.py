"""The edge-feature producer (csrc/producer.hip) against a plain float64 reference, at its kernels' edges.

Kernels under test: prod_index_a / prod_index_b, prod_table_fwd / prod_word_fwd / prod_tmax / prod_sent_fwd / prod_expand /
prod_poison, prod_gather, prod_sent_bwd and its deterministic route (prod_sent_bwd_det -> prod_nterm_owner + prod_dwb_fin),
prod_word_bwd_rows / prod_word_bwd_tok, prod_table_bwd / prod_table_fin, the two column-sum kernels, prod_wpair, prod_count, and
the GEMM layer's guarded paths under them.  The cases (producer_cases.SWEEPS) walk what those kernels branch on: the hidden width
either side of every column-chunk count HC = 1 / 2 / 4 / 8, widths that are no multiple of 4 (the attention vectors' gradients
through g.dwb and four copies, the lanes-over-columns body of prod_word_bwd_rows), the table backward above 64 KiB of dynamic LDS,
T around the 4-row unroll, the 16-token chunks, the wave and the second 512-token trip up to the 2 048 limit, S around the 8-byte
liveness groups up to 31, N up to the second trip of index pass A and past the persistent grids of the row kernels, distance
tables of 1 .. 100 rows (past the 64 lanes of the table backward's id walk), P off the GEMM tile, the three id dtypes, masks with
holes / of token 0 only / all live / none live / one live slot, ragged batches with an empty and a one-entity document, B = 1 / 3
/ 5 -- every one with junk in the places a correct producer never reads (producer_cases).

Every case runs dense with the default backward; the Hd, ragged, N = 46 / 91 and ND groups also with deterministic=True (which must
repeat bit for bit), compact=True (compared through .dense()) and both.  Every run checks prod.last_counts against the live slots
and pairs counted on the CPU.

Bound: |got - ref| <= 1e-5 * max(1, max|ref|) + 1e-4 * |ref| per tensor on every element, E per pair row (producer_cases.ratios);
no tensor has a raised bound.  Each run prints its worst error as a fraction of the bound.  Measured on an MI355X over all 138 runs
(the float32 oracle on the CPU: test_producer_edges_cpu.py): E 0.23 (Hd = 257), d ctx 0.044 (N = 45), d node 0.019, d dis_table
0.025 (Hd = 512), the sixteen parameter gradients at most 0.12 (d sentence_attention.attention_all.bias at N = 64; d
word_attention.attention_all.bias, analytically zero, 0.10 at Hd = 256); the default backward's atomics move these by a few
0.001 between runs.  Before prod_table_bwd_kernel walked more than 64 ids the ND = 65 case missed the bound
by 34 x (d ctx) to 179 x (d word_attention.attention_all.weight) and ND = 100 by up to 25 000 x; every other case passed as it
stands, the 90 KiB launch of the table backward (Hd = 256 / 257, ND = 21) included.
"""
import os

import numpy as np
import pytest
import torch

import gcgcn_amd
from gcgcn_amd import params as P_
import producer_cases as C

pytestmark = pytest.mark.gpu

MODES = {"dense": (False, False), "dense-det": (False, True), "compact": (True, False), "compact-det": (True, True)}
OUT_KEYS = ("E",) + C.GRAD_KEYS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prodedges_nd21_parent.npz")


def run_producer(c, cot, dev, compact=False, det=False):
    """Forward + backward on the GPU -> the same tensors as producer_cases.reference(), and the device-side counts."""
    prod = gcgcn_amd.EdgeFeatureProducer(c.Hd, c.P)
    prod.load_state_dict(c.sd, strict=True)
    prod = prod.to(dev)
    ctx, node, table = (t.to(dev).requires_grad_() for t in (c.ctx, c.node, c.table))
    nv = None if c.n_valid is None else c.n_valid.to(dev)
    e = prod(ctx, c.sen.to(dev), c.ph.to(dev), c.pt.to(dev), node, table, n_valid=nv, compact=compact, deterministic=det)
    if compact:
        e = e.dense()
    e.backward(cot.to(dev))
    got = {"E": e.detach(), "d ctx": ctx.grad, "d node": node.grad, "d dis_table": table.grad}
    got.update({"d " + k: v for k, v in P_.unpack_producer(prod.flat.grad, c.Hd, c.P).items()})
    return got, prod.last_counts.tolist()


def check(fam, c, ref, dev, mode="dense"):
    compact, det = MODES[mode]
    got, counts = run_producer(c, ref["cot"], dev, compact, det)
    assert counts[:3] == [c.rows, c.pairs, 0], f"{fam} {c.id} {mode}: device counts {counts}, the CPU counts {c.rows} slots in {c.pairs} pairs"
    res = C.ratios(got, ref)
    print(f"[prod-err] {fam} {c.id} {mode}: {C.short(res)}")
    bad = [f"{k}: {v:.3g} x bound" for k, v in res.items() if not v <= 1.0]
    assert not bad, f"{fam} {c.id} {mode}: " + "; ".join(bad)
    if c.ragged:
        assert float(got["d node"][~c.real.to(dev)].abs().sum()) == 0.0, "d node of padding entities must be exactly zero"
        assert float(got["E"][~c.pair.to(dev)].abs().sum()) == 0.0, "E of padding pairs must be exactly zero"
    if det:
        again, _ = run_producer(c, ref["cot"], dev, compact, det)
        for k in OUT_KEYS:
            assert torch.equal(got[k], again[k]), f"{fam} {c.id} {mode}: {k} does not repeat bit for bit"
    return got


def _params(sweeps, modes):
    return [pytest.param(fam, kw, m, id=f"{fam}:{C.kw_id(kw)}:{m}") for fam, kws in sweeps.items() for kw in kws for m in modes]


@pytest.mark.parametrize("fam,kw,mode", _params(C.SWEEPS, ["dense"]))
def test_sweeps_dense_default_backward(gpu_device, fam, kw, mode):
    c, ref = C.case_and_ref(kw)
    check(fam, c, ref, gpu_device, mode)


@pytest.mark.parametrize("fam,kw,mode", _params(C.FOUR_WAYS, ["dense-det", "compact", "compact-det"]))
def test_sweeps_deterministic_and_compact(gpu_device, fam, kw, mode):
    c, ref = C.case_and_ref(kw)
    check(fam, c, ref, gpu_device, mode)


def test_nd21_is_bitwise_what_the_parent_computed(gpu_device):
    """The table backward walks the distance ids in chunks of 64 lanes since ND > 64 became correct; for ND <= 64 that is the walk it
    always did.  The fixture holds the deterministic backward's results of the ND = 21 case as the library computed them before
    the change: every tensor must still equal them to the last bit."""
    kw = next(k for k in C.SWEEPS["ND"] if k["ND"] == 21)
    c, ref = C.case_and_ref(kw)
    got, _ = run_producer(c, ref["cot"], gpu_device, det=True)
    z = np.load(GOLDEN)
    assert np.array_equal(z["cot"], ref["cot"].numpy()), "the case generator no longer draws the inputs the fixture was recorded on"
    for k in OUT_KEYS:
        assert np.array_equal(z[k], got[k].cpu().numpy()), f"{k} differs from the parent's"


def test_refusals(gpu_device):
    """S = 32, T = 2 049, Hd = 513 and the backward at Hd = 512, ND = 21 (180 KiB of LDS for prod_table_bwd) are refused on the
    host, as a Python exception, before anything of the refused call is launched."""
    dev = gpu_device

    def call(backward=False, **kw):
        c = C.make_case(B=1, N=2, **kw)
        prod = gcgcn_amd.EdgeFeatureProducer(c.Hd, c.P).to(dev)
        ctx, node, table = (t.to(dev).requires_grad_() for t in (c.ctx, c.node, c.table))
        e = prod(ctx, c.sen.to(dev), c.ph.to(dev), c.pt.to(dev), node, table)
        if backward:
            try:
                e.sum().backward()
            except RuntimeError:
                torch.cuda.synchronize()
                assert ctx.grad is None and node.grad is None and table.grad is None and prod.flat.grad is None
                raise
        return e

    with pytest.raises(RuntimeError, match=r"producer"):
        call(S=32, T=4)
    with pytest.raises(RuntimeError, match=r"T=2049 tokens exceed the LDS budget"):
        call(S=1, T=2049)
    with pytest.raises(RuntimeError, match=r"hidden width 513"):
        call(Hd=513, T=4)
    assert call(Hd=512, ND=21, T=4).shape == (1, 2, 2, 512)              # the forward is accepted ...
    with pytest.raises(RuntimeError, match=r"LDS budget of the table backward"):
        call(backward=True, Hd=512, ND=21, T=4)                          # ... its backward is not
    assert torch.isfinite(call(backward=True, Hd=512, ND=5, T=4)).all()  # 45 KiB: accepted
    torch.cuda.synchronize()
