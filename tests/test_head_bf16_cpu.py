"""``classifier_head(..., matmul="bf16")`` without a GPU: the definition (gcgcn_amd.functional.Bf16HeadBilinearFn) against the oracle
head, how the bounds of tests/head_bf16_cases.py are set, the refusals and how the matmul argument reaches the C entry points."""
import ctypes

import pytest
import torch

import gcgcn_amd
import head_bf16_cases as C
from gcgcn_amd import _lib, functional as F_
from test_head_edges_gpu import reference as oracle_reference
from test_host_cpu import head_plan_table

SHAPES = [(1, 2, 97, 1), (2, 5, 33, 3), (1, 9, 96, 3), (2, 12, 97, 3), (1, 9, 1, 1)]
IDS = [f"B={s[0]} N={s[1]} R={s[2]} nf={s[3]}" for s in SHAPES]


@pytest.mark.parametrize("B,N,R,nf", SHAPES[:3], ids=IDS[:3])
def test_definition_without_rounding_is_the_oracle_head(B, N, R, nf):
    """Float64, the identity in place of bf16(.): logits and every gradient equal oracle.gcgcn_oracle.classifier_head's to 1e-12."""
    c = C.make_case(B, N, R, nv=[N] + [max(N // 2, 1)] * (B - 1), nf=nf)
    want = oracle_reference(c)
    got = C.reference(c, head=lambda *a: C.definition_head(*a, rnd=C.identity))
    for k, r in want.items():
        scale = max(1.0, r.abs().max().item())
        assert (got[k] - r).abs().max().item() <= 1e-12 * scale, k


def test_definition_rounds_what_it_says():
    """One pair, R = 1, operands chosen so that every rounding shows: the forward value and the five gradients by hand."""
    bf = F_._round_bf16
    g = torch.Generator().manual_seed(5)
    eh, et = (torch.rand(3, 128, generator=g, dtype=torch.float64) * 2 - 1 for _ in range(2))
    eh, et = eh.float().double().requires_grad_(), et.float().double().requires_grad_()
    wb = torch.randn(2, 128, 128, generator=g).double().requires_grad_()
    wc = torch.randn(2, 256, generator=g).double().requires_grad_()
    bias = torch.randn(2, generator=g).double().requires_grad_()
    dout = torch.randn(3, 2, generator=g).double()
    out = F_.Bf16HeadBilinearFn.apply(eh, et, wb, wc, bias)
    out.backward(dout)
    e, t, Wb, Wc = eh.detach(), et.detach(), bf(wb.detach()), bf(wc.detach())
    outer = bf((e.float()[:, :, None] * t.float()[:, None, :]).double())
    want = torch.einsum("pab,rab->pr", outer, Wb) + bf(torch.cat([e, t], 1)) @ Wc.t() + bias.detach()
    assert torch.allclose(out.detach(), want, rtol=1e-13, atol=1e-13)
    assert not torch.allclose(out.detach(), torch.einsum("pa,rab,pb->pr", e, wb.detach(), t) + torch.cat([e, t], 1) @ wc.detach().t()
                              + bias.detach(), rtol=1e-5, atol=1e-5)
    dr = bf(dout)
    de = bf((dout.float()[:, :, None] * t.float()[:, None, :]).double())
    assert torch.allclose(eh.grad, torch.einsum("prb,rab->pa", de, Wb) + dr @ Wc[:, :128], rtol=1e-13, atol=1e-13)
    dt = bf((dout.float()[:, :, None] * e.float()[:, None, :]).double())
    assert torch.allclose(et.grad, torch.einsum("pra,rab->pb", dt, Wb) + dr @ Wc[:, 128:], rtol=1e-13, atol=1e-13)
    assert torch.allclose(wb.grad, torch.einsum("pr,pab->rab", dr, outer), rtol=1e-13, atol=1e-13)
    assert torch.allclose(wc.grad, dr.t() @ bf(torch.cat([e, t], 1)), rtol=1e-13, atol=1e-13)
    assert torch.equal(bias.grad, dout.sum(0))                                  # the UNROUNDED cotangent


@pytest.mark.parametrize("B,N,R,nf", SHAPES, ids=IDS)
def test_float32_definition_is_well_inside_the_end_to_end_bound(B, N, R, nf):
    """How C_E2E is set: the float32 CPU run of the definition against its float64 run, under a quarter of the bound on every tensor."""
    c, ref = C.case_and_ref(B, N, R, nf=nf)
    res = C.e2e_fractions(C.reference(c, torch.float32), ref)
    print(f"[head-bf16] float32 definition {C.case_id(c)}: " + " ".join(f"{k}={v:.4f}" for k, v in res.items()))
    assert max(res.values()) < 0.25, res


@pytest.mark.parametrize("B,N,R,nf", SHAPES, ids=IDS)
def test_unrounded_head_violates_the_bound_where_it_separates(B, N, R, nf):
    """The per-pass bound tells a bf16 pass from an fp32 one: the float32 run of the definition (same operands, fp32 sums) meets it,
    the float32 head WITHOUT the rounding -- what an fp32 kernel behind the switch would compute -- breaks it on most elements of the
    two weight gradients and, at R = 1, of d eh and d et.  The shares of the other passes are printed (head_bf16_cases's docstring says why they are not asserted)."""
    c = C.make_case(B, N, R, nf=nf)
    b = 0
    eh, et = C.pair_features([f[b] for f in c.feats], c.ntype[b], c.rel[b], c.sd, c.dis_plus)
    eh, et, dout = eh.reshape(-1, C.HW), et.reshape(-1, C.HW), c.cot[b].reshape(-1, R)
    ref, mag = C.pass_reference(eh, et, c.sd, dout)
    bias = c.sd["bili_layer_01.bias"] + c.sd["classification_layer_01.bias"]
    for name, rnd in (("rounded", None), ("unrounded", C.identity)):
        e, t = eh.clone().requires_grad_(), et.clone().requires_grad_()
        wb, wc = c.sd["bili_layer_01.weight"].clone().requires_grad_(), c.sd["classification_layer_01.weight"].clone().requires_grad_()
        out = F_.Bf16HeadBilinearFn.apply(e, t, wb, wc, bias, rnd)
        out.backward(dout)
        got = {"logits": out.detach(), "d eh": e.grad, "d et": t.grad, "d bili_layer_01.weight": wb.grad,
               "d classification_layer_01.weight": wc.grad}
        res = C.pass_fractions(got, ref, mag, eh.shape[0], R)
        print(f"[head-bf16] float32 {name} {C.case_id(c)}: " + " ".join(f"{k}={v[0]:.3g} ({v[1]:.2f})" for k, v in res.items()))
        if rnd is None:
            assert max(v[0] for v in res.values()) <= 1.0, res
        else:
            assert all(res[k][1] > 0.5 for k in C.separating(R)), res


def test_refusals():
    """A matmul that is neither name is a ValueError before anything touches a device; the C entry points refuse other integers."""
    c = C.make_case(1, 2, 3)
    with pytest.raises(ValueError, match="matmul must be 'fp32' or 'bf16'"):
        F_.classifier_head(c.feats, c.ntype, c.rel, c.sd["ner_emb.weight"], c.sd["dis_embed.weight"], torch.zeros(8), 3, matmul="nonsense")
    with pytest.raises(ValueError, match="matmul must be 'fp32' or 'bf16'"):
        gcgcn_amd.ClassifierHead(matmul="nonsense")
    with pytest.raises(ValueError, match="matmul must be 'fp32' or 'bf16'"):
        gcgcn_amd.GraphModelTail(head_matmul="bf16 ")
    assert gcgcn_amd.GraphModelTail(head_matmul="bf16").head.matmul == "bf16" and gcgcn_amd.GraphModelTail().head.matmul == "fp32"
    h, out = _lib.lib(), (ctypes.c_int32 * 6)()
    null = ctypes.c_void_p()
    ptr = ctypes.byref(null)
    for bad in (-1, 2, 7):          # the call that takes the announcement refuses it before a launch -- and has taken it
        assert h.gcgcn_set_option(C.ANNOUNCE, bad) == 0
        assert h.gcgcn_debug_head_plan(2, 5, 97, 0, out) != 0 and b"head_matmul" in h.gcgcn_last_error()
        assert h.gcgcn_debug_head_plan(2, 5, 97, 0, out) == 0
        assert h.gcgcn_set_option(C.ANNOUNCE, bad) == 0
        assert h.gcgcn_head_fwd(1, 2, 128, 1, 20, 20, 97, 21, 10, ptr, ptr, ptr, ptr, ptr, None, ptr, ptr, None, ptr, None) != 0
        assert b"head_matmul" in h.gcgcn_last_error()
        assert h.gcgcn_debug_head_plan(2, 5, 97, 0, out) == 0
    assert int(h.gcgcn_version()) == 7


def test_the_announcement_is_per_call_and_per_thread(monkeypatch):
    """gcgcn_set_option("head_matmul", 1) reaches exactly the next head call of the thread that made it: the call after that, a call
    that fails on its arguments in between, and a call on another thread all see 0; the environment variable is not read."""
    import threading
    monkeypatch.setenv("GCGCN_HEAD_MATMUL", "1")
    h = _lib.lib()

    def plan():
        out = (ctypes.c_int32 * 6)()
        assert h.gcgcn_debug_head_plan(2, 5, 97, 0, out) == 0
        return list(out)
    fp32 = plan()
    assert fp32[1:4] != [3, 3, 2]
    assert h.gcgcn_set_option(C.ANNOUNCE, 1) == 0
    assert plan()[1:] == [3, 3, 2, 0, 0] and plan() == fp32              # taken by one call
    assert h.gcgcn_set_option(C.ANNOUNCE, 1) == 0
    assert h.gcgcn_debug_head_plan(0, 5, 97, 0, (ctypes.c_int32 * 6)()) != 0   # a call refused for its shape has taken it too
    assert plan() == fp32
    assert h.gcgcn_set_option(C.ANNOUNCE, 1) == 0
    seen = []
    t = threading.Thread(target=lambda: seen.append(plan()))
    t.start()
    t.join()
    assert seen == [fp32]                                                # another thread never sees it
    assert plan()[1:4] == [3, 3, 2] and plan() == fp32                   # and has not taken it


def test_state_dict_is_the_same_under_both_settings():
    a, b = gcgcn_amd.ClassifierHead(relation_num=5), gcgcn_amd.ClassifierHead(relation_num=5, matmul="bf16")
    assert list(a.state_dict()) == list(b.state_dict())
    for dst, src in ((a, b), (b, a)):
        res = dst.load_state_dict(src.state_dict(), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    assert all(v.dtype == torch.float32 for v in b.state_dict().values())


def test_plan_with_and_without_the_announcement():
    """gcgcn_debug_head_plan announced with matmul = 0 answers, over the option grid tests/test_host_cpu.py walks (1 728 plans), what
    it answers unannounced; announced with 1 every plan names the bf16 kernels (3, 3, 2), one launch per pass, and compacts
    exactly the shapes the fp32 plan compacts."""
    import numpy as np

    def plan(mm):
        def f(*args):
            out = np.zeros(6, np.int32)
            if mm is not None:
                _lib.call("gcgcn_set_option", C.ANNOUNCE, mm)
            _lib.call("gcgcn_debug_head_plan", *args, out.ctypes.data_as(ctypes.c_void_p))
            got = [int(v) for v in out]
            if mm == 1:
                assert got[1:] == [3, 3, 2, 0, 0], got
                got = [got[0], 0, 0, 0, 0, 0]
            return got
        return f

    set_option = lambda name, v: _lib.call("gcgcn_set_option", name.encode(), v)
    want = head_plan_table(plan(None), set_option)
    assert head_plan_table(plan(0), set_option) == want
    compact = lambda table: [[[code[0] for code in grp] for grp in line[1]] for line in table]
    assert compact(head_plan_table(plan(1), set_option)) == compact(want)
