"""The output stage of the convolution's backward on each of its routes (csrc/gcn_plan.hpp: OutBwdPlan).  Every case first asks
gcgcn_debug_chain_plan and gcgcn_debug_out_bwd_plan for the route it means to run: a shape that does not take its route fails
the case.  Then one convolution block (functional.gcn_stack), forward and backward, against the CPU oracle per document: out, dX,
dEbar, dA and the flat gradient -- the output projection's dWlin and dblin named separately -- at the bounds test_hip_parity.py
uses for these tensors, in eval mode and in train mode (both dropouts on, their keep-masks replayed in the oracle); padding rows
of dX and dEbar are exact zeros where n_valid is given.  As in test_hip_parity's full-batch comparisons, the oracle replays the
HIP path's relu decisions (its saved Y > 0) and the decisions are checked on their own, at that file's bounds: two correct fp32
evaluations can put a pre-activation of 1e-8 on different sides of zero, and one such element moves a document's dX, dEbar and
dA by 1e-3 (seen at the two 16- and 17-document cases, once in four draws of the parameters; with the decisions replayed every
tensor agrees to 2e-6).  The parameters are drawn under a fixed seed.  Whether the group launch in front of the chain had a
reduce is the launcher's answer (gemm_group), which no test sees: only the first plan step (out_bwd_plan) is asserted."""
import ctypes

import numpy as np
import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib, functional as F_
from oracle import gcgcn_oracle as O

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-4)                   # test_hip_parity.close: outputs, dX, dE, dA
GRAD_TOL = dict(rtol=1e-3, atol=2e-4)              # test_hip_parity._check_stack_param_grads (atol x the tensor's largest entry)
NONE, LAUNCH, CHAIN = 0, 1, 2                      # OutBwdPlan::Mask; Col1's CHAIN is 0:
COL1_CHAIN, COL1_FRONT, COL1_BACK = 0, 1, 2
WSUM_NONE, WSUM_FORWARD, WSUM_HERE = 0, 1, 2
FOLD_NONE, FOLD_ONE_HEAD, FOLD_HEADS = 0, 1, 2
FRONT, BACK = 0, 1                                 # OutBwdPlan::DWlin
P_BLOCK, P_OUT = 0.2, 0.2

# B, N, D, L, H, n_valid, option chain, functional.head_sum_in_forward; then what out_bwd_plan must say: fuse, wsum, fold,
# head_sum_launch, dwlin, col1, chain_slices
ROUTES = {
    "fused, stage 1 in the chain": (2, 16, 64, 2, 4, None, 1, True, 1, WSUM_FORWARD, FOLD_NONE, 0, BACK, COL1_CHAIN, 4),
    "fused, 2B > 64: stage 1 in the back launch": (33, 16, 64, 2, 4, None, 1, True, 1, WSUM_FORWARD, FOLD_NONE, 0, BACK, COL1_BACK, 0),
    "fused, the head sum made here": (2, 16, 64, 2, 4, None, 1, False, 1, WSUM_HERE, FOLD_NONE, 0, BACK, COL1_CHAIN, 4),
    "not fused, one head: fold": (2, 16, 64, 2, 1, None, 0, True, 0, WSUM_NONE, FOLD_ONE_HEAD, 0, FRONT, COL1_FRONT, 0),
    "not fused, four heads, wsum from forward: fold": (2, 16, 64, 2, 4, None, 0, True, 0, WSUM_FORWARD, FOLD_HEADS, 0, FRONT, COL1_FRONT, 0),
    "not fused, no wsum: head_sum_drop_bwd": (2, 16, 64, 2, 4, None, 0, False, 0, WSUM_NONE, FOLD_NONE, 1, FRONT, COL1_FRONT, 0),
    "not fused, past the fold threshold": (17, 64, 256, 2, 8, None, 0, True, 0, WSUM_NONE, FOLD_NONE, 1, FRONT, COL1_FRONT, 0),
    "not fused, on the fold threshold": (16, 64, 256, 2, 8, None, 0, True, 0, WSUM_FORWARD, FOLD_HEADS, 0, FRONT, COL1_FRONT, 0),
    "fused, ragged": (2, 16, 64, 2, 4, (16, 5), 1, True, 1, WSUM_FORWARD, FOLD_NONE, 0, BACK, COL1_CHAIN, 4),
    "not fused, ragged": (2, 16, 64, 2, 4, (16, 5), 0, True, 0, WSUM_FORWARD, FOLD_HEADS, 0, FRONT, COL1_FRONT, 0),
}


def chain_fuses(B, N, D, L, H, ragged):
    """ChainPlan::fuse of a backward call with workspace, no edge ride and aligned operands"""
    out = np.full(6, -7, np.int32)
    _lib.call("gcgcn_debug_chain_plan", 1, B, N, D, L, H, int(ragged), 0, 0, 1, 0, out.ctypes.data_as(ctypes.c_void_p))
    return int(out[3])


def out_bwd_plan(fuse, B, N, D, H, wsum_fwd, ragged, odrop, drop):
    """OutBwdPlan of a call with workspace and an aligned dXres: mask, wsum, fold, fold_drop, head_sum_launch, dwlin, col1, slices"""
    out = np.full(10, -7, np.int32)
    _lib.call("gcgcn_debug_out_bwd_plan", fuse, B, N, D, H, 1, int(wsum_fwd), int(ragged), int(odrop), int(drop), 0, 0,
              out.ctypes.data_as(ctypes.c_void_p))
    return [int(v) for v in out[:8]]


def oracle_block(x, ebar, adj, sd, L, H, nv, keeps, cot, relus):
    """The CPU oracle, document by document on its real entities: the oracle takes an edge tensor [n, j, D] and means it over j
    after the projection, so Ebar is handed in as the edge tensor with one j.  keeps: None, or (block mask [B,N,H,L,gh], output mask
    [B,N,D]); relus [B,N,H,L,gh]: the HIP path's relu decisions, replayed (oracle._relu) and compared with the oracle's own
    pre-activations at the bounds of test_hip_parity._check_relu_decisions.  Returns outs and the leaves whose .grad hold dX,
    dEbar, dA per document, and the parameters' leaves."""
    B, N, D = x.shape
    sdl = {k: v.clone().requires_grad_() for k, v in sd.items()}
    outs, leaves = [], []
    total = flips = 0
    worst = 0.0
    for b in range(B):
        n = N if nv is None else int(nv[b])
        xb, eb, ab = (t.clone().requires_grad_() for t in (x[b, :n], ebar[b, :n], adj[b, :, :n, :n]))
        e = eb[:, None, :]
        kb = None if keeps is None else keeps[0][b, :n]
        rb = [[relus[b, :n, h, l] for l in range(L)] for h in range(H)]
        pre = []                                                  # the oracle's pre-activations, in (h, l) order
        if H == 1:
            out = O.graph_convolution(xb, e, ab[0], sdl, L, keep=None if kb is None else [kb[:, 0, l] for l in range(L)], p=P_BLOCK,
                                      relu_masks=rb[0], trace=pre)
        else:
            out = O.multi_graph_convolution(xb, e, list(ab.unbind(0)), sdl, L, H, p=P_BLOCK, relu_masks=rb, trace=pre,
                                            keep=None if kb is None else [[kb[:, h, l] for l in range(L)] for h in range(H)])
        for mask, t in zip((m for per_head in rb for m in per_head), pre):
            dis = (t > 0) != mask
            total += mask.numel()
            flips += int(dis.sum())
            if dis.any():
                worst = max(worst, t[dis].abs().max().item())
        if keeps is not None:
            out = out * keeps[1][b, :n].float() / (1.0 - P_OUT)
        outs.append(out)
        leaves.append((xb, eb, ab))
    assert worst < 1e-5, f"a relu decision differs from the oracle's at |pre-activation| = {worst:.3e}"
    assert flips <= max(16, int(2e-5 * total)), f"{flips} of {total} relu decisions differ from the oracle's"
    sum((o * cot[b, :o.shape[0]]).sum() for b, o in enumerate(outs)).backward()
    return outs, leaves, sdl


@pytest.mark.parametrize("train", [False, True])
@pytest.mark.parametrize("case", list(ROUTES))
def test_output_stage_runs_where_the_plan_says_and_matches_the_oracle(gpu_device, case, train):
    B, N, D, L, H, n_valid, chain, hsf, fuse, wsum, fold, hs_launch, dwlin, col1, slices = ROUTES[case]
    dev = gpu_device
    x, _, e2, adj = O.synth_docs(B, N, D, seed=31)
    g = torch.Generator().manual_seed(32)
    ebar = e2.mean(2)
    adj = (adj[:, None] * (torch.rand(B, H, N, N, generator=g) + 0.5)).contiguous()
    cot = torch.randn(B, N, D, generator=g)               # (also on padding rows: the block ignores what arrives there)
    nv = None
    if n_valid is not None:
        nv = torch.tensor(n_valid, dtype=torch.int32)
        live = torch.arange(N)[None, :] < nv[:, None]
        x, ebar = x * live[..., None], ebar * live[..., None]
        adj = adj * (live[:, None, :, None] & live[:, None, None, :])
    with torch.random.fork_rng(devices=[]):               # the parameters: the same draw wherever the case runs
        torch.manual_seed(33)
        conv = (gcgcn_amd.GraphConvolution(L, D, D) if H == 1 else gcgcn_amd.MultiGraphConvolution(L, H, D, D)).to(dev).train(train)
    sd = {k: v.detach().cpu() for k, v in conv.state_dict().items()}
    snaps, orig = [], F_.rng_snapshot

    def spy(d, lazy=False):
        snaps.append(orig(d, lazy))
        return snaps[-1]
    try:
        _lib.call("gcgcn_set_option", b"chain", chain)
        F_.head_sum_in_forward = hsf
        F_.rng_snapshot = spy
        # the route this case means to run
        assert chain_fuses(B, N, D, L, H, nv is not None) == fuse
        got = out_bwd_plan(fuse, B, N, D, H, hsf and H > 1, nv is not None, train, train)
        masked = nv is not None or train
        want = [(CHAIN if fuse else LAUNCH) if masked else NONE, wsum, fold, int(fold == FOLD_ONE_HEAD or (fold == FOLD_HEADS and train)),
                hs_launch, dwlin, col1, slices]
        assert got == want, f"{case}: out_bwd_plan gives {got}, the case means {want}"
        gcgcn_amd.manual_seed(77, dev)
        xs, es, as_ = (t.to(dev).requires_grad_() for t in (x, ebar, adj))
        out = F_.gcn_stack(xs, es, as_, conv.flat, L, H, None if nv is None else nv.to(dev), P_BLOCK, train, out_dropout=P_OUT)
        relus = out.grad_fn.saved_tensors[5].view(B, N, H, L, D // L).cpu() > 0      # save_for_backward(x, ebar, adj, flat, Pn, Y, ...)
        torch.autograd.backward(out, cot.to(dev))
    finally:
        _lib.call("gcgcn_set_option", b"chain", 1)
        F_.head_sum_in_forward = True
        F_.rng_snapshot = orig
    keeps = None
    if train:     # draw order: the block's dropout, then the output dropout (functional.gcn_stack)
        assert len(snaps) == 2
        keeps = (F_.dropout_keep_mask(snaps[0], _lib.SALT_GCN, P_BLOCK, B * N * H * D).view(B, N, H, L, D // L).cpu(),
                 F_.dropout_keep_mask(snaps[1], _lib.SALT_GLUE, P_OUT, B * N * D).view(B, N, D).cpu())
        assert all(abs(k.float().mean().item() - 0.8) < 0.03 for k in keeps), "keep rate off"
    outs, leaves, sdl = oracle_block(x, ebar, adj, sd, L, H, nv, keeps, cot, relus)
    for b, (o, (xb, eb, ab)) in enumerate(zip(outs, leaves)):
        n = o.shape[0]
        for nm, got_t, ref in (("out", out[b, :n], o), ("dX", xs.grad[b, :n], xb.grad), ("dEbar", es.grad[b, :n], eb.grad),
                               ("dA", as_.grad[b, :, :n, :n], ab.grad)):
            torch.testing.assert_close(got_t.detach().cpu(), ref.detach(), **TOL, msg=lambda m: f"{case}: {nm}[{b}]: {m}")
        assert not xs.grad[b, n:].any() and not es.grad[b, n:].any() and not out[b, n:].any(), f"{case}: padding rows of document {b}"
    grads = conv.named_grads()
    refs = {k: v.grad for k, v in sdl.items() if v.grad is not None}
    assert set(refs) <= set(grads) and {"linear_layer.weight", "linear_layer.bias"} <= set(refs)
    names = {"linear_layer.weight": "dWlin", "linear_layer.bias": "dblin"}
    for k, ref in refs.items():
        top = max(1.0, ref.abs().max().item())
        torch.testing.assert_close(grads[k].cpu(), ref, rtol=GRAD_TOL["rtol"], atol=GRAD_TOL["atol"] * top,
                                   msg=lambda m: f"{case}: {names.get(k, 'grad ' + k)}: {m}")
