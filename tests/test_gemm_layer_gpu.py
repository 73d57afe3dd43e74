"""The GEMM layer (csrc/gemm.hip, csrc/gemm_body.hpp) against float64, launcher by launcher, through gcgcn_debug_gemm_run: the fused
epilogue, both batch levels and every stride, split-K, the two row-block modes, group launches with their riding column sums, parked
problems and the three pairs on a device-side count.  Cases, restatement and bound: gemm_layer_cases.py.

Every case (1) asks gcgcn_debug_gemm_plan for the route it means to take and fails if the shape does not take it, (2) is compared
with the float64 restatement under the per-element bound, exact where the bound is zero (padding rows, zero-stored dead rows,
dropped elements), (3) must leave every element outside the window it may write as it was, bit for bit (SENTINEL, or an
accumulating problem's prior), and (4) runs twice with bitwise equal results."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_layer_cases as G
from gcgcn_amd import _lib

pytestmark = pytest.mark.gpu
CASES = G.all_cases()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def keep_masks(case, snap, dev):
    keeps = {}
    for i, q in enumerate(case.probs):
        if q.p > 0 and "C2" in q.ptr:
            n = G.keep_extent(q)
            k = torch.empty(n, dtype=torch.uint8, device=dev)
            _lib.call("gcgcn_dropout_keep", ptr(k), n, ptr(snap), q.salt, q.p, None)
            keeps[i] = k.cpu()
    return keeps


def launch(case, T, dev):
    """One run on fresh device copies -> (every buffer back on the CPU, the out row)"""
    D = {name: t.to(dev) for name, t in T.items()}
    cnt = torch.tensor([case.cnt or 0], dtype=torch.int32, device=dev)
    ints, scal, ptrs, ride, rptr = G.pack(case, lambda name: D[name].data_ptr())
    n = len(case.probs)
    out = np.full(2 + 2 * max(n, 1), -7, np.int32)
    as_p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    _lib.call("gcgcn_debug_gemm_run", case.form, n, as_p(ints), as_p(scal), as_p(ptrs), as_p(ride), as_p(rptr), case.tile, case.splits,
              ptr(cnt), case.cap, as_p(out), None)
    r = case.ride
    if r is not None and r.kind == 1 and out[1] == 1:          # col_later: the caller finishes stage 2 (col_sum_stage2_launch)
        ride2 = np.array([2, 0, r.ld, r.C, G.COL_RIDE_SLICES, 0], np.int64)
        out2 = np.full(2, -7, np.int32)
        _lib.call("gcgcn_debug_gemm_run", G.FORM_GROUP, 0, None, None, None, as_p(ride2), as_p(rptr), 0, 1, None, 0, as_p(out2), None)
    torch.cuda.synchronize()
    return {name: t.cpu() for name, t in D.items()}, out


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("group,case", CASES, ids=[f"{g}:{c.name}" for g, c in CASES])
def test_gemm_layer(gpu_device, group, case):
    plans = G.assert_routes(case, _lib.call)
    T = G.tensors_of(case)
    keeps = keep_masks(case, T["snap"].to(gpu_device), gpu_device)
    interior = {i: pl.get("interior") == 1 for i, pl in enumerate(plans)} if case.form >= G.FORM_PAIR_WX else None
    ref = G.reference(case, T, keeps, interior)
    got, out = launch(case, T, gpu_device)
    again, out_again = launch(case, T, gpu_device)
    n = len(case.probs)
    assert out[0] == 0 and (out == out_again).all()
    if case.form == G.FORM_PARK:                               # which problems gemm_defer took; a refused one ran through gemm()
        assert [int(out[2 + 2 * i]) for i in range(n)] == case.accepted
        assert all(out[3 + 2 * i] == (-1 if a else 0) for i, a in enumerate(case.accepted))
    if case.ride is not None and case.ride.kind == 1:
        assert out[1] == int(case.ride.later_expected), f"col_later {out[1]}"
    worst = 0.0
    ws_names = {q.ptr["ws"][0]: q for q in case.probs if "ws" in q.ptr}
    for name, (numel, kind) in case.buffers.items():
        g = got[name]
        assert torch.equal(bits(g), bits(again[name])), f"{name}: two runs differ"
        if kind != "out":
            assert torch.equal(bits(g), bits(T[name])), f"{name}: an input was written"
            continue
        if name in ref:
            exp, bound, written = ref[name]
            assert torch.equal(bits(g)[~written], bits(T[name])[~written]), \
                f"{name}: {(bits(g)[~written] != bits(T[name])[~written]).sum()} elements outside the window were written"
            err = (g.double() - exp).abs()[written]
            b = bound[written]
            exact = b == 0
            assert not err[exact].any(), f"{name}: {int((err[exact] != 0).sum())} elements that must be exact differ (max {err[exact].max()})"
            assert torch.isfinite(g[written]).all(), f"{name}: non-finite output"
            if (~exact).any():
                ratio = float((err[~exact] / b[~exact]).max())
                worst = max(worst, ratio)
        elif name in ws_names:                                 # a workspace: nothing in front of it, nothing behind its ws_elems
            q = ws_names[name]
            off = q.ptr["ws"][1]
            touched = bits(g) != bits(T[name])
            assert not touched[:off].any() and not touched[off + q.ws_elems:].any(), f"{name}: a store outside the workspace"
            if hasattr(case, "ws_split_members"):              # gemm_plan_slice: the members that stay split fill their slabs
                slab = 8 * 64 * 64
                assert int(touched.sum()) == case.ws_split_members * slab and touched[off:off + case.ws_split_members * slab].all()
        else:
            assert torch.equal(bits(g), bits(T[name])), f"{name}: written by a launch that has no business there"
    print(f"GEMM_LAYER_RATIO {group} {case.name} {worst:.4g}")
    assert worst <= 1.0, f"{case.name}: error / bound = {worst}"
