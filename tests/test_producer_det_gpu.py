"""The bit-reproducible producer backward on the GPU (csrc/producer.hip: prod_sent_bwd_det -> prod_nterm_owner + prod_dwb_fin,
behind gcgcn_producer_bwd_det / EdgeFeatureProducer.deterministic): repeats to the last bit, the CPU oracle at the tolerances of
test_producer_matches_oracle, the default (atomics) path at its own repeat-run tolerance, the edges of the three kernels, a
captured hipGraph, and the C entry's refusals.  Every GPU test starts on NaN-poisoned free memory (conftest): a partial row or a
dnterm row that a kernel forgot to write shows up as NaN."""
import ctypes
import functools

import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib, functional as F_, params as P_
from test_producer_gpu import _oracle, synth_doc

pytestmark = pytest.mark.gpu

SHAPES = [                                             # the four shapes of test_producer_matches_oracle
    (2, 6, 3, 40, 64, 20, torch.int64, True),
    (1, 12, 5, 120, 128, 20, torch.uint8, True),
    (2, 5, 2, 33, 24, 7, torch.int32, False),
    (1, 42, 5, 512, 128, 20, torch.int64, True),
]
SHAPE_IDS = [f"B{s[0]}-N{s[1]}-S{s[2]}-T{s[3]}-Hd{s[4]}" for s in SHAPES]
VEC, VEC_B = "sentence_attention.attention_all.weight", "sentence_attention.attention_all.bias"
PGRID, PW = 2048, 4                                    # csrc/producer.hip: workgroups of the row kernels, waves in each


def _require_symbol():
    """Fails loudly on a library without the deterministic entry (instead of passing by luck of the atomics)."""
    out = ctypes.c_int64(-1)
    _lib.call("gcgcn_producer_det_elems", 2, 6, 64, 10, ctypes.cast(ctypes.pointer(out), ctypes.c_void_p))
    assert out.value > 0
    assert gcgcn_amd.EdgeFeatureProducer.deterministic is False


def _producer(Hd, P, dev, seed=0):
    torch.manual_seed(seed)
    return gcgcn_amd.EdgeFeatureProducer(Hd, P).to(dev)


def _run(prod, inputs, cot, det, dev, nv=None, compact=False, caps=None):
    """One forward + backward; every result detached on the device."""
    ctx, node, table, sen, ph, pt = inputs
    prod.deterministic = det
    prod.zero_grad()
    cg, ng, tg = (t.to(dev).requires_grad_() for t in (ctx, node, table))
    kw = {} if caps is None else dict(max_live_slots=caps[0], max_live_pairs=caps[1])
    e = prod(cg, sen.to(dev), ph.to(dev), pt.to(dev), ng, tg, n_valid=None if nv is None else nv.to(dev), compact=compact, **kw)
    if compact:
        e = e.dense()
    (e * cot.to(dev)).sum().backward()
    return dict(E=e.detach(), dctx=cg.grad, dnode=ng.grad, dtable=tg.grad, dflat=prod.flat.grad.clone(), counts=prod.last_counts.tolist())


GRADS = ("dctx", "dnode", "dtable", "dflat")


def _assert_bitwise(a, b, what):
    for k in ("E",) + GRADS:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs (max |diff| {(a[k] - b[k]).abs().max().item():.3e})"


def _assert_repeat_tolerance(got, want, what):
    """The existing repeat-run tolerance of test_producer_matches_oracle."""
    for k in GRADS:
        torch.testing.assert_close(got[k], want[k], rtol=1e-5, atol=1e-6 * max(1.0, float(want[k].abs().max())),
                                   msg=lambda m: f"{what}, {k}: {m}")


def _assert_oracle(prod, got, ref, keys=None, docs=None):
    """Gradients at the tolerances of test_producer_matches_oracle.  ref = _oracle(...)[1:]; docs: batch rows ref was computed on."""
    dctx, dnode, dtab, dsd = ref
    tol = lambda want: dict(rtol=1e-3, atol=1e-4 * max(1.0, want.abs().max().item()))
    sel = (lambda t: t) if docs is None else (lambda t: t[docs])
    if keys is None:
        for nm, g_, want in (("dctx", sel(got["dctx"]), dctx), ("dtable", got["dtable"], dtab)):
            torch.testing.assert_close(g_.cpu(), want, msg=lambda m: f"{nm}: {m}", **tol(want))
    want = dnode
    dn = sel(got["dnode"]).cpu()
    for b in range(want.shape[0]):          # per entity: a head-side term added to entity i instead of j shows up row by row
        for n in range(want.shape[1]):
            torch.testing.assert_close(dn[b, n], want[b, n], msg=lambda m: f"dnode[{b},{n}]: {m}", **tol(dnode))
    grads = P_.unpack_producer(got["dflat"].cpu(), prod.hidden, prod.dis_size)
    for k, want in dsd.items():
        if keys is None or k in keys:
            torch.testing.assert_close(grads[k], want, msg=lambda m: f"grad {k}: {m}", **tol(want))


@functools.lru_cache(maxsize=None)
def _shape_case(i):
    """Inputs, cotangent, producer and the oracle of shape i, computed once and shared (read-only) by tests 1-3."""
    B, N, S, T, Hd, P, dtype, ranges = SHAPES[i]
    inputs = synth_doc(B, N, S, T, Hd, P, seed=B * 100 + N, dtype=dtype, ranges=ranges)
    cot = torch.randn(B, N, N, Hd, generator=torch.Generator().manual_seed(1))      # random, asymmetric in (i, j)
    cot = cot * (~inputs[3][..., 0]).any(-1).unsqueeze(-1).float()                  # the 1e10-scaled pairs stay out of the loss
    dev = torch.device("cuda:0")
    prod = _producer(Hd, P, dev, seed=i)
    runs = [_run(prod, inputs, cot, True, dev) for _ in range(3)]
    default = _run(prod, inputs, cot, False, dev)
    ref = _oracle(prod, *inputs, cot)
    return prod, runs, default, ref


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=SHAPE_IDS)
def test_deterministic_backward_repeats_bitwise(gpu_device, i):
    _require_symbol()
    _, runs, _, _ = _shape_case(i)
    assert runs[0]["dflat"].abs().sum() > 0 and all(torch.isfinite(runs[0][k]).all() for k in GRADS)
    _assert_bitwise(runs[0], runs[1], "run 1 / run 2")
    _assert_bitwise(runs[0], runs[2], "run 1 / run 3")


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=SHAPE_IDS)
def test_deterministic_backward_matches_oracle(gpu_device, i):
    _require_symbol()
    prod, runs, _, ref = _shape_case(i)
    outs = ref[0]
    for b, o in enumerate(outs):
        scale = o.detach().abs().amax(dim=-1, keepdim=True).clamp_min(1.0)
        torch.testing.assert_close(runs[0]["E"][b].cpu() / scale, o.detach() / scale, rtol=1e-4, atol=1e-4)
    _assert_oracle(prod, runs[0], ref[1:])


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=SHAPE_IDS)
def test_deterministic_backward_matches_default(gpu_device, i):
    _require_symbol()
    _, runs, default, _ = _shape_case(i)
    assert torch.equal(runs[0]["E"], default["E"]), "the forward does not depend on the flag"
    _assert_repeat_tolerance(runs[0], default, "deterministic / default")


# ---- edges of the new kernels, each at one column chunk with idle lanes (Hd = 24) and at two chunks (Hd = 128) ---------------------
def _edge_inputs(B, N, S, T, Hd, P, seed, first_frac=0.6):
    inputs = synth_doc(B, N, S, T, Hd, P, seed=seed, first_frac=first_frac, dtype=torch.uint8)
    cot = torch.randn(B, N, N, Hd, generator=torch.Generator().manual_seed(seed + 1))
    cot = cot * (~inputs[3][..., 0]).any(-1).unsqueeze(-1).float()
    return inputs, cot


HDS = [(24, 7), (128, 20)]


@pytest.mark.parametrize("Hd,P", HDS)
@pytest.mark.parametrize("N", [1, 2])
def test_edges_one_and_two_entities(gpu_device, N, Hd, P):
    """N = 1: the only pair is (0, 0) -- entity 0 gets the head-side and the tail-side row of the same pair."""
    _require_symbol()
    B, S, T = 2, 3, 30
    inputs, cot = _edge_inputs(B, N, S, T, Hd, P, seed=40 + N, first_frac=0.9)
    sen = inputs[3]
    sen[:, :, :, 0, 0:5] = True                       # slot 0 of every pair is live ...
    sen[:, :, :, S - 1] = False
    sen[:, :, :, S - 1, 7:12] = True                   # ... and the last one is padded: the divisor stays O(1)
    cot = torch.randn(B, N, N, Hd, generator=torch.Generator().manual_seed(3))
    prod = _producer(Hd, P, gpu_device)
    a, b = (_run(prod, inputs, cot, True, gpu_device) for _ in range(2))
    assert a["counts"][1] == B * N * N and a["counts"][2] == 0
    _assert_bitwise(a, b, "repeat")
    _assert_oracle(prod, a, _oracle(prod, *inputs, cot)[1:])


@pytest.mark.parametrize("Hd,P", HDS)
def test_edges_ragged_batch_with_an_empty_document(gpu_device, Hd, P):
    """n_valid = [7, 0, 3] at N = 7: the gradients of an empty document and of padding entities are exactly zero."""
    _require_symbol()
    B, N, S, T = 3, 7, 3, 36
    inputs, cot = _edge_inputs(B, N, S, T, Hd, P, seed=50)
    nv = torch.tensor([7, 0, 3], dtype=torch.int32)
    prod = _producer(Hd, P, gpu_device)
    a, b = (_run(prod, inputs, cot, True, gpu_device, nv=nv) for _ in range(2))
    _assert_bitwise(a, b, "repeat")
    for k in GRADS:
        assert torch.isfinite(a[k]).all(), k
    assert (a["dnode"][1] == 0).all() and (a["dctx"][1] == 0).all() and (a["dnode"][2, 3:] == 0).all()
    real = [0, 2]                                      # the oracle runs on the documents that have entities
    ref = _oracle(prod, *(t[real] if t.dim() > 2 and t.shape[0] == B else t for t in inputs), cot[real], nv=nv[real])
    _assert_oracle(prod, a, ref[1:], docs=real)        # (the oracle's node gradient has zero rows for padding entities)
    _assert_repeat_tolerance(a, _run(prod, inputs, cot, False, gpu_device, nv=nv), "deterministic / default")


@pytest.mark.parametrize("Hd,P", HDS)
def test_edges_no_live_slot(gpu_device, Hd, P):
    """counts = 0: no wave owns a pair, no partial row is live -- the owners still write, and what they write is exactly zero."""
    _require_symbol()
    B, N, S, T = 2, 5, 2, 30
    inputs, _ = _edge_inputs(B, N, S, T, Hd, P, seed=60)
    inputs[3][..., 0] = False
    cot = torch.randn(B, N, N, Hd, generator=torch.Generator().manual_seed(4))
    prod = _producer(Hd, P, gpu_device)
    for caps in ((5, 3), (B * N * N * S, B * N * N)):
        a = _run(prod, inputs, cot, True, gpu_device, caps=caps)
        assert a["counts"][:3] == [0, 0, 0]
        grads = P_.unpack_producer(a["dflat"], Hd, P)
        assert (grads[VEC] == 0).all() and (grads[VEC_B] == 0).all() and (a["dnode"] == 0).all()
        assert all(torch.isfinite(a[k]).all() for k in GRADS)
        want = cot.sum(dim=(0, 1, 2))                  # every real pair of E is linear_sentence_att's bias
        torch.testing.assert_close(grads["linear_sentence_att.bias"].cpu(), want, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("Hd,P", HDS)
def test_edges_capacities_exactly_tight_and_over(gpu_device, Hd, P):
    _require_symbol()
    B, N, S, T = 2, 6, 3, 32
    inputs, cot = _edge_inputs(B, N, S, T, Hd, P, seed=70)
    prod = _producer(Hd, P, gpu_device)
    counted = _run(prod, inputs, cot, True, gpu_device)
    r, q = counted["counts"][:2]
    assert r > q > 0
    tight = _run(prod, inputs, cot, True, gpu_device, caps=(r, q))
    assert tight["counts"][:3] == [r, q, 0]
    _assert_bitwise(counted, tight, "capacities counted / given exactly")
    roomy = _run(prod, inputs, cot, True, gpu_device, caps=(B * N * N * S, B * N * N))
    torch.testing.assert_close(roomy["E"], counted["E"], rtol=1e-5, atol=1e-6)
    _assert_repeat_tolerance(roomy, counted, "capacities given generously / counted")   # (the GEMMs' split-K plans follow the capacity)
    # over capacity: nothing is computed (E is NaN: loud) -- and the owners write zeros instead of reading rows nobody wrote
    over = _run(prod, inputs, torch.zeros_like(cot), True, gpu_device, caps=(r, q - 1))
    assert over["counts"][2] == 1 and torch.isnan(over["E"]).any()
    grads = P_.unpack_producer(over["dflat"], Hd, P)
    assert (grads[VEC] == 0).all() and (grads[VEC_B] == 0).all() and (over["dnode"] == 0).all()


def test_edges_more_pairs_than_waves(gpu_device):
    """9800 live pairs > PGRID * PW = 8192: a wave owns two pairs and every workgroup writes a non-zero partial row.  Every pair's
    only slot is live, so the reference's divisor is 1e-10 (no padded slot): the cotangent carries the 1e-10 back."""
    _require_symbol()
    B, N, S, T, Hd, P = 2, 70, 1, 12, 64, 20
    g = torch.Generator().manual_seed(80)
    ctx = torch.tanh(torch.randn(B, T, Hd, generator=g))
    node = torch.rand(B, N, Hd, generator=g) * 2 - 1
    table = torch.randn(21, P, generator=g) * 0.5
    ln = torch.randint(3, T + 1, (B, N, N, S, 1), generator=g)
    sen = torch.arange(T).view(1, 1, 1, 1, T) < ln                                   # token 0 in every slot
    ph = torch.randint(0, 21, (B, N, N, S, T), generator=g).to(torch.uint8)
    pt = torch.randint(0, 21, (B, N, N, S, T), generator=g).to(torch.uint8)
    inputs = (ctx, node, table, sen, ph, pt)
    cot = torch.randn(B, N, N, Hd, generator=g) * 1e-10
    prod = _producer(Hd, P, gpu_device)
    a, b = (_run(prod, inputs, cot, True, gpu_device) for _ in range(2))
    assert a["counts"][:3] == [B * N * N, B * N * N, 0] and B * N * N > PGRID * PW
    _assert_bitwise(a, b, "repeat")
    _assert_oracle(prod, a, _oracle(prod, *inputs, cot)[1:], keys=(VEC,))


@pytest.mark.parametrize("Hd,P", HDS)
def test_edges_compact_rows(gpu_device, Hd, P):
    """compact=True hands the backward dEc instead of dE: the same prod_bwd, the same three kernels."""
    _require_symbol()
    B, N, S, T = 3, 7, 3, 36
    inputs, cot = _edge_inputs(B, N, S, T, Hd, P, seed=90)
    nv = torch.tensor([7, 4, 6], dtype=torch.int32)
    prod = _producer(Hd, P, gpu_device)
    dense = _run(prod, inputs, cot, True, gpu_device, nv=nv)
    a, b = (_run(prod, inputs, cot, True, gpu_device, nv=nv, compact=True) for _ in range(2))
    _assert_bitwise(a, b, "compact repeat")
    torch.testing.assert_close(a["E"], dense["E"], rtol=1e-5, atol=1e-6)
    _assert_repeat_tolerance(a, dense, "compact / dense")


def test_captured_graph_replays_the_eager_result(gpu_device):
    """Forward + backward under capture with capacities given; replays on NEW contents equal an eager deterministic run bitwise."""
    _require_symbol()
    B, N, S, T, Hd, P = 2, 6, 3, 40, 128, 20
    dev = gpu_device
    inputs, cot = _edge_inputs(B, N, S, T, Hd, P, seed=100)
    sen, ph, pt = (t.to(dev) for t in inputs[3:])
    r, q = F_.producer_live_counts(sen.view(torch.uint8))
    prod = _producer(Hd, P, dev)
    prod.deterministic = True
    ctx, node, table = (t.to(dev).requires_grad_() for t in inputs[:3])
    cot_s = cot.to(dev)
    out = {}

    def step():
        for t in (ctx, node, table, prod.flat):
            t.grad = None
        e = prod(ctx, sen, ph, pt, node, table, max_live_slots=r, max_live_pairs=q)
        (e * cot_s).sum().backward()
        out["E"] = e

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
    torch.cuda.synchronize()
    static = dict(E=out["E"], dctx=ctx.grad, dnode=node.grad, dtable=table.grad, dflat=prod.flat.grad)
    gen = torch.Generator().manual_seed(7)
    new = [torch.tanh(torch.randn(B, T, Hd, generator=gen)), torch.rand(B, N, Hd, generator=gen) * 2 - 1,
           torch.randn(B, N, N, Hd, generator=gen) * (cot != 0).float()]
    eager_prod = _producer(Hd, P, dev)
    want = _run(eager_prod, (new[0], new[1]) + tuple(inputs[2:]), new[2], True, dev, caps=(r, q))
    with torch.no_grad():
        ctx.copy_(new[0]), node.copy_(new[1]), cot_s.copy_(new[2])
    for rep in range(3):
        for v in static.values():
            v.detach().fill_(float("nan"))                # poison: a replay has to rewrite every result
        graph.replay()
        torch.cuda.synchronize()
        if rep in (0, 2):
            for k in ("E",) + GRADS:
                assert torch.equal(static[k].detach(), want[k]), f"replay {rep}: {k} is not bitwise the eager deterministic run's"


# ---- C ABI: the refusals answer before anything is launched ----------------------------------------------------------------------
def test_bwd_det_refuses_a_bad_workspace(gpu_device):
    _require_symbol()
    B, N, S, T, Hd, P, ND = 2, 4, 2, 16, 24, 7, 21
    dev = gpu_device
    inputs, _ = _edge_inputs(B, N, S, T, Hd, P, seed=110)
    ctx, node, table, sen, ph, pt = (t.to(dev) for t in inputs)
    sen = sen.view(torch.uint8)
    caps = (B * N * N * S, B * N * N)
    flat = _producer(Hd, P, dev).flat.detach()
    sizes = (ctypes.c_int64 * 7)()
    _lib.call("gcgcn_producer_sizes", B, N, S, T, Hd, P, ND, *caps, ctypes.cast(sizes, ctypes.c_void_p))
    ndet = ctypes.c_int64()
    _lib.call("gcgcn_producer_det_elems", B, N, Hd, caps[1], ctypes.cast(ctypes.pointer(ndet), ctypes.c_void_p))
    ndet = ndet.value
    ibuf, fbuf = torch.empty(sizes[0], dtype=torch.int32, device=dev), torch.empty(sizes[1], device=dev)
    E = torch.empty(B, N, N, Hd, device=dev)
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (B, N, S, T, Hd, P, ND, p(ctx), p(sen), p(ph), p(pt), 1, p(node), p(table), None, p(flat), *caps, p(ibuf), p(fbuf))
    _lib.call("gcgcn_producer_fwd", *head, None, 0, p(E), st)
    SENT = 12345.0
    bbuf = torch.full((int(sizes[2]),), SENT, device=dev)
    outs = [torch.full_like(t, SENT) for t in (ctx, node, table, flat)]
    detbuf = torch.full((ndet + 4,), SENT, device=dev)
    dE = torch.ones_like(E)
    h = _lib.lib()

    def bwd(det_ptr, det_elems):
        return h.gcgcn_producer_bwd_det(*head, p(bbuf), p(dE), None, *(p(o) for o in outs), det_ptr, det_elems, st)

    assert detbuf.data_ptr() % 16 == 0
    for det_ptr, det_elems, word in ((None, ndet, b"detbuf"), (ctypes.c_void_p(detbuf.data_ptr() + 4), ndet, b"detbuf"),
                                     (p(detbuf), ndet - 1, b"det_elems")):
        assert bwd(det_ptr, det_elems) != 0
        assert word in h.gcgcn_last_error(), h.gcgcn_last_error()
    torch.cuda.synchronize()
    for t in outs + [bbuf, detbuf]:
        assert (t == SENT).all(), "a refused call touched a buffer"
    assert bwd(p(detbuf), ndet) == 0, h.gcgcn_last_error()          # exactly enough: accepted, and everything is written
    torch.cuda.synchronize()
    assert all(torch.isfinite(o).all() and not (o == SENT).all() for o in outs[:2])
    assert (detbuf[ndet:] == SENT).all(), "the call wrote past det_elems"
