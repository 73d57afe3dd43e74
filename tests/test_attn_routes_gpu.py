"""MultiHeadAttention's core in each place it runs (csrc/attn_plan.hpp).  Every case first asks gcgcn_debug_attn_plan -- and
gcgcn_debug_chain_plan where a chain kernel hosts the core -- for the route it means to run: a shape that does not take its
route fails the case.  Then: the fused hop (functional.MaggcFn) equals MultiHeadAttention followed by MultiGraphConvolution bit
for bit, the core and the batched-GEMM route agree within the bound of test_hip_parity's mha_core A/B test, and padding rows
and columns are exact zeros."""
import ctypes

import numpy as np
import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib, functional as F_

pytestmark = pytest.mark.gpu
GEMM, CORE, CHAIN, GROUP, DONE = range(5)          # AttnPlan::Route
GENERIC, CHAIN_S, CHAIN_T = 1, 2, 3                # ChainPlan::Kind
AB_TOL = dict(rtol=2e-5, atol=2e-5)                # test_hip_parity.test_mha_core_and_generic_paths_agree


def attn_route(bwd, N, D, H, hook=0, chain_attends=0):
    out = np.full(4, -7, np.int32)
    _lib.call("gcgcn_debug_attn_plan", bwd, N, D, H, hook, chain_attends, 0, 0, out.ctypes.data_as(ctypes.c_void_p))
    assert out[3] == 0, f"N={N} D={D} H={H}: the hook is refused ({out[3]})"
    return int(out[0])


def chain_plan(bwd, B, N, D, L, H, ragged, hook):
    """(kind, attention) of a convolution call with workspace and no edge ride"""
    out = np.full(6, -7, np.int32)
    _lib.call("gcgcn_debug_chain_plan", bwd, B, N, D, L, H, int(ragged), 0, hook, 1, 0, out.ctypes.data_as(ctypes.c_void_p))
    return int(out[0]), int(out[4])


def inputs(B, N, D, n_valid, dev, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, D, generator=g) * 0.5
    nv = None
    if n_valid is not None:
        nv = torch.tensor(n_valid, dtype=torch.int32)
        x = x * (torch.arange(N)[None, :] < nv[:, None]).unsqueeze(-1).float()
        nv = nv.to(dev)
    return x.to(dev), nv, g


def assert_padding_is_zero(t, nv, what, square=False):
    """t[b, ..., i, :] == 0 for rows i >= n_valid[b] (square: columns too), exactly"""
    for b, n in enumerate(nv.tolist()):
        assert not t[b, ..., n:, :].any(), f"{what}: padding rows of document {b}"
        assert not (square and t[b, ..., :, n:].any()), f"{what}: padding columns of document {b}"


def run_mha(att, x, nv, cot, train, dev):
    att.train(train)
    att.zero_grad()
    gcgcn_amd.manual_seed(11, dev)
    xs = x.clone().requires_grad_()
    a, _ = F_.multi_head_adjacency(xs, att.flat, att.head_num, nv, att.p, train)
    torch.autograd.backward(a, cot)
    return a.detach(), xs.grad, att.flat.grad.clone()


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("N,D,H,n_valid,route", [(1, 64, 4, None, CORE), (17, 64, 4, (17, 9), CORE), (64, 64, 4, None, CORE),
                                                 (16, 64, 4, (16, 5), CORE),
                                                 (65, 64, 4, (65, 33), GEMM),     # one entity past the core's tile
                                                 (16, 24, 4, None, GEMM)])        # head width 6: no whole float4s
def test_standalone_attention_runs_where_the_plan_says(gpu_device, N, D, H, n_valid, route, train):
    """MhaFn forward and backward on `route`, then with option mha_core = 0 on the GEMMs whatever the shape: the two agree."""
    B = 2
    x, nv, g = inputs(B, N, D, n_valid, gpu_device, 100 * N + D)
    cot = torch.randn(B, H, N, N, generator=g).to(gpu_device)
    att = gcgcn_amd.MultiHeadAttention(H, D).to(gpu_device)
    res = []
    try:
        for core, want in ((1, route), (0, GEMM)):
            _lib.call("gcgcn_set_option", b"mha_core", core)
            assert attn_route(0, N, D, H) == want and attn_route(1, N, D, H) == want
            res.append(run_mha(att, x, nv, cot, train, gpu_device))
    finally:
        _lib.call("gcgcn_set_option", b"mha_core", 1)
    for a, dx, _ in res:
        if train:
            assert N == 1 or (a == 0).float().mean() > 0.02    # dropout was on
        else:
            rows = a if nv is None else torch.cat([a[b, :, :n] for b, n in enumerate(nv.tolist())], 1)
            torch.testing.assert_close(rows.sum(-1), torch.ones_like(rows[..., 0]), rtol=0, atol=1e-5)
        if nv is not None:
            assert_padding_is_zero(a, nv, "A", square=True)
            assert_padding_is_zero(dx, nv, "dX")
    for nm, p, q in zip(("A", "dX", "dflat"), *res):
        torch.testing.assert_close(p, q, **AB_TOL, msg=lambda m: f"{nm}: {m}")


# B, N, D, L, H, n_valid; the forward chain kernel, where the forward core runs, where the backward core runs
HOPS = {"generic chain, core launched inside the hook": (2, 16, 64, 4, 4, None, GENERIC, CORE, GROUP),
        "chain T prologue": (2, 16, 128, 2, 8, None, CHAIN_T, CHAIN, GROUP),
        "chain S prologue": (2, 64, 256, 2, 8, None, CHAIN_S, CHAIN, GROUP),
        "chain T with the row-block list": (3, 64, 256, 2, 8, (0, 17, 64), CHAIN_T, CHAIN, GROUP),
        # head width 68: the narrowest whose scratch the group launch's LDS does not hold (64 still rides: test_host_cpu)
        "backward core in front of the group": (2, 16, 136, 2, 2, None, GENERIC, CORE, CORE)}


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("case", list(HOPS))
def test_fused_hop_runs_where_the_plan_says_and_equals_the_two_modules(gpu_device, case, train):
    """MaggcFn against MhaFn + GcnFn under one manual_seed: out, A, dX, dEbar and both flat gradients, bit for bit.  The fused form
    parks the attention projection's weight gradient (functional.defer_fused_mha_weight_grads; MhaFn never parks it), and a parked
    product runs unsplit where the group launch splits K: that one tensor then differs in summation order (by up to 1.2e-7 on these shapes),
    so it is compared bit for bit with the switch off, and with it on at the tolerance of test_fused_maggc_hop_equals_separate_modules."""
    B, N, D, L, H, n_valid, kind, fwd_route, bwd_route = HOPS[case]
    got_kind, attends = chain_plan(0, B, N, D, L, H, n_valid is not None, 1)
    assert got_kind == kind and attends == (fwd_route == CHAIN), (got_kind, attends)
    assert attn_route(0, N, D, H, hook=1, chain_attends=attends) == fwd_route and attn_route(1, N, D, H, hook=1) == bwd_route
    assert bwd_route == GROUP or attn_route(1, N, D - 4 * H, H, hook=1) == GROUP      # (four features narrower still ride)
    x, nv, g = inputs(B, N, D, n_valid, gpu_device, 7 * N + D)
    ebar = (torch.randn(B, N, D, generator=g) * 0.5).to(gpu_device)
    cot = torch.randn(B, N, D, generator=g).to(gpu_device)
    att = gcgcn_amd.MultiHeadAttention(H, D).to(gpu_device).train(train)
    conv = gcgcn_amd.MultiGraphConvolution(L, H, D, D).to(gpu_device).train(train)
    assert F_.maggc_fusable(x, H)
    res = []
    try:
        for fused, park in ((True, True), (True, False), (False, True)):
            F_.defer_fused_mha_weight_grads = park
            att.zero_grad(), conv.zero_grad()
            gcgcn_amd.manual_seed(123, gpu_device)
            xs, es = x.clone().requires_grad_(), ebar.clone().requires_grad_()
            if fused:
                out = F_.maggc_hop(xs, es, att.flat, conv.flat, L, H, nv, att.p, conv.p, train)
                assert "Maggc" in type(out.grad_fn).__name__
                adj = out.grad_fn.saved_tensors[2]
            else:
                adj, xa = F_.multi_head_adjacency(xs, att.flat, H, nv, att.p, train)
                out = F_.gcn_stack(xa, es, adj, conv.flat, L, H, nv, conv.p, train)
            torch.autograd.backward(out, cot)
            res.append((out.detach(), adj.detach(), xs.grad, es.grad, att.flat.grad.clone(), conv.flat.grad.clone()))
    finally:
        F_.defer_fused_mha_weight_grads = True
    names = ("out", "A", "dX", "dEbar", "d flat (attention)", "d flat (convolution)")
    for nm, parked, unparked, sep in zip(names, *res):
        assert torch.equal(unparked, sep), f"{nm}: fused and separate differ by {(unparked - sep).abs().max().item():.3e}"
        if nm == "d flat (attention)":
            torch.testing.assert_close(parked, sep, rtol=1e-4, atol=1e-5 * max(1.0, sep.abs().max().item()), msg=lambda m: f"{nm}: {m}")
        else:
            assert torch.equal(parked, sep), f"{nm} (dWq parked): fused and separate differ by {(parked - sep).abs().max().item():.3e}"
    if nv is not None:
        out, adj, dx = res[0][:3]
        assert_padding_is_zero(adj, nv, "A", square=True)
        assert_padding_is_zero(dx, nv, "dX")
        assert_padding_is_zero(out, nv, "out")
