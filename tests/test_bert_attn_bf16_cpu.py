"""attention="bf16" without a GPU: the definition (gcgcn_amd.bert.Bf16AttentionFn) against a hand-written restatement, the selectors
and their refusals, the new C symbols, and how the bounds of tests/bert_attn_bf16_cases.py are set."""
import math

import numpy as np
import pytest
import torch

from gcgcn_amd import _lib, functional as Fn, models as M
from gcgcn_amd import bert as bert_mod
from gcgcn_amd.bert import BertModel

import bert_attn_bf16_cases as C
from bert_cases import CONFIGS, MODEL_SWEEP, attn_case, attn_ref, config, model_case, state


def r(t):
    """One rounding to bfloat16, nearest even, back in the tensor's own dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def _restated(q, k, v, pen, m, dctx):
    """The issue's formulas as loops over (document, head) and explicit sums, float64: (ctx, lse, dq, dk, dv)."""
    B, H, T, dh = q.shape
    alpha = 1.0 / math.sqrt(dh)
    out = [torch.zeros_like(q) for _ in range(4)]
    ctx, dq, dk, dv = out
    lse = torch.zeros(B, H, T, dtype=q.dtype)
    for b in range(B):
        for h in range(H):
            qr, kr, vr, gr = r(q[b, h]), r(k[b, h]), r(v[b, h]), r(dctx[b, h])
            S = torch.zeros(T, T, dtype=q.dtype)
            for i in range(T):
                for j in range(T):
                    S[i, j] = alpha * (qr[i] * kr[j]).sum() + (0.0 if pen is None else pen[b, j])
            mx = S.max(1, keepdim=True).values
            E = torch.exp(S - mx)
            P = E / E.sum(1, keepdim=True)
            lse[b, h] = (mx + torch.log(E.sum(1, keepdim=True)))[:, 0]
            Pd = m[b, h] * P
            Pdr = r(Pd)
            for i in range(T):
                ctx[b, h, i] = (Pdr[i][:, None] * vr).sum(0)
            delta = (dctx[b, h] * ctx[b, h]).sum(1, keepdim=True)
            dPd = torch.zeros(T, T, dtype=q.dtype)
            for i in range(T):
                for j in range(T):
                    dPd[i, j] = (gr[i] * vr[j]).sum()
            dSr = r(P * (m[b, h] * dPd - delta))
            for j in range(T):
                dv[b, h, j] = (Pdr[:, j][:, None] * gr).sum(0)
                dk[b, h, j] = alpha * (dSr[:, j][:, None] * qr).sum(0)
            for i in range(T):
                dq[b, h, i] = alpha * (dSr[i][:, None] * kr).sum(0)
    return ctx, lse, dq, dk, dv


@pytest.mark.parametrize("penalty", [False, True])
@pytest.mark.parametrize("B,T,H", [(2, 5, 2), (2, 33, 2)])
def test_definition_against_a_restatement(B, T, H, penalty):
    g = torch.Generator().manual_seed(B + 3 * T + H + penalty)
    q, k, v, dctx = (torch.randn(B, H, T, 64, generator=g).double() for _ in range(4))
    pen = None
    if penalty:
        pen = torch.zeros(B, T, dtype=torch.float64)
        pen[0, 1::2] = -10000.0
        pen[1] = -10000.0          # every key masked: a finite softmax
    m = (torch.rand(B, H, T, T, generator=g) >= 0.3).double() / 0.7
    qa, ka, va = (t.clone().requires_grad_() for t in (q, k, v))
    ctx, lse = bert_mod.Bf16AttentionFn.apply(qa, ka, va, None if pen is None else pen[:, None, None, :], m)
    (ctx * dctx).sum().backward()
    want = _restated(q, k, v, pen, m, dctx)
    for name, a, b in zip(("ctx", "lse", "dq", "dk", "dv"), (ctx.detach(), lse, qa.grad, ka.grad, va.grad), want):
        err = (a - b).abs().max().item() / max(1.0, b.abs().max().item())
        assert err <= 1e-12, (name, err)
    assert not lse.requires_grad
    # m = None is m = ones
    c1, _ = bert_mod.Bf16AttentionFn.apply(q, k, v, None, None)
    c2, _ = bert_mod.Bf16AttentionFn.apply(q, k, v, None, torch.ones(B, H, T, T, dtype=torch.float64))
    assert torch.equal(c1, c2)


def test_the_rounding_is_really_there():
    """On the discriminating case the fp32 definition (bert_cases.attn_ref) lies outside the core bound around the bf16 definition on at
    least half the elements of ctx and of dqkv, and the float32 run of the bf16 definition inside it."""
    H = 2
    case = C.discriminating_case(H=H)
    ref = C.attn_def(case, H, torch.float64)
    fp = attn_ref(case, H, torch.float64)
    for k in ("ctx", "dqkv"):
        share = C.share_outside(fp[k], ref[k])
        print(f"fp32 definition: {share:.3f} of {k} outside the core bound")
        assert share >= 0.5, (k, share)
    fr = C.core_worst(C.attn_def(case, H, torch.float32), ref, "float32 run of the bf16 definition, discriminating case")
    assert max(fr.values()) <= 1.0, fr


def test_defaults_and_refusals():
    assert BertModel(config(128, 2)).attention == "fp32"
    with pytest.raises(ValueError, match="attention"):
        BertModel(config(128, 2), attention="fp16")
    with pytest.raises(ValueError, match="attention"):
        BertModel(config(128, 2), impl="hip", attention=1)
    x = torch.zeros(1, 4, 64)
    ps = [t.detach() for t in BertModel(config(64, 1)).encoder.layer[0].tensors()]
    with pytest.raises(ValueError, match="attention"):        # refused before anything else, CPU tensors included
        Fn.bert_layer(x, None, *ps, attention="fp16")
    with pytest.raises(ValueError, match="attention"):
        Fn.bert_attention(torch.zeros(1, 4, 192), None, 1, attention=1)
    import inspect
    assert inspect.signature(Fn.bert_layer).parameters["attention"].default == "fp32"
    assert inspect.signature(Fn.bert_attention).parameters["attention"].default == "fp32"
    sds = [list(BertModel(config(128, 2), matmul=mm, attention=at).state_dict()) for mm in ("fp32", "bf16") for at in ("fp32", "bf16")]
    assert all(s == sds[0] for s in sds)                     # one checkpoint for all four settings


class _Cfg:
    entity_type_size, coref_size, max_length, keep_prob, graph_hop = 20, 20, 512, 1.0, 2
    dis_size, dis_num, dis_plus, relation_num, alpha = 20, 21, 10, 97, 1.0

    def __init__(self, vocab, **kw):
        self.data_word_vec = np.zeros((vocab, 100), np.float32)
        self.__dict__.update(kw)


def test_model_config_selector():
    bc = config(128, 2)
    with pytest.raises(ValueError, match="bert_impl"):
        M.GraphCNN_multihead_bert_gate_cls(_Cfg(61, bert_attention="bf16", bert_config=bc), bert=BertModel(bc))
    with pytest.raises(ValueError, match="bert_attention"):
        M.GraphCNN_multihead_bert_gate_cls(_Cfg(61, bert_impl="torch", bert_attention="half", bert_config=bc))
    m = M.GraphCNN_multihead_bert_gate_cls(_Cfg(61, bert_impl="torch", bert_attention="bf16", bert_config=bc))
    assert m.bert.attention == "bf16" and m.bert.matmul == "fp32" and m.bert.impl == "torch"
    both = M.GraphCNN_multihead_bert_gate_cls(_Cfg(61, bert_impl="torch", bert_attention="bf16", bert_matmul="bf16", bert_config=bc))
    assert both.bert.attention == "bf16" and both.bert.matmul == "bf16"
    plain = M.GraphCNN_multihead_bert_gate_cls(_Cfg(61, bert_impl="torch", bert_config=bc))
    assert plain.bert.attention == "fp32"
    assert list(m.state_dict()) == list(plain.state_dict()) == list(both.state_dict())


def test_torch_model_with_both_settings_is_the_composition_of_the_two_definitions():
    """One layer of BertModel(impl="torch", matmul="bf16", attention="bf16"), float64, against a restatement: Bf16LinearFn for the six
    Linears, Bf16AttentionFn for the core, everything else written out."""
    D, H, B, T = 128, 2, 3, 33
    case = model_case(D, H, B, T, "holes")
    model = C.fresh_model(D, H, matmul="bf16")
    assert model.matmul == "bf16" and model.attention == "bf16"
    got = C.run_model(model, case)
    e = model.embeddings
    emb = e.word_embeddings(case["ids"]) + e.position_embeddings(torch.arange(T))[None] + e.token_type_embeddings(case["tt"])
    x = bert_mod.layer_norm(emb, e.LayerNorm.weight, e.LayerNorm.bias).detach()
    kb = (1.0 - case["mask"].double()) * -10000.0
    wq, bq, wk, bk, wv, bv, wo, bo, g1, b1, wi, bi, wo2, bo2, g2, b2 = (t.detach() for t in model.encoder.layer[0].tensors())
    lin = lambda t, w, b: r(t) @ r(w).t() + b
    split = lambda t: t.view(B, T, H, 64).permute(0, 2, 1, 3)
    q, k, v = split(lin(x, wq, bq)), split(lin(x, wk, bk)), split(lin(x, wv, bv))
    s = r(q) @ r(k).transpose(-1, -2) / 8.0 + kb[:, None, None, :]
    ctx = (r(torch.softmax(s, -1)) @ r(v)).permute(0, 2, 1, 3).reshape(B, T, D)
    a = bert_mod.layer_norm(lin(ctx, wo, bo) + x, g1, b1)
    y = bert_mod.layer_norm(lin(bert_mod.gelu(lin(a, wi, bi)), wo2, bo2) + a, g2, b2)
    err = (got["out0"] - y).abs().max().item() / max(1.0, y.abs().max().item())
    assert err <= 1e-12, err
    # and each selector alone changes the result
    for mm, at in (("fp32", "fp32"), ("bf16", "fp32"), ("fp32", "bf16")):
        other = C.run_model(C.fresh_model(D, H, matmul=mm, attention=at), case)
        assert not torch.equal(other["out0"], got["out0"]), (mm, at)


def test_new_symbols_are_declared_bound_and_exported():
    """The four _mx symbols against the header and the library: tests/test_abi_cpu.py.  Here: how their lists relate."""
    h = _lib.lib()
    for name in ("gcgcn_bert_attn_fwd", "gcgcn_bert_attn_bwd"):            # the _len argument list plus the selector
        assert _lib.SIGNATURES[name + "_mx"][1] == _lib.SIGNATURES[name + "_len"][1] + [_lib.I]
    for name in ("gcgcn_bert_layer_fwd", "gcgcn_bert_layer_bwd"):          # the _mm argument list plus the selector
        assert _lib.SIGNATURES[name + "_mx"][1] == _lib.SIGNATURES[name + "_mm"][1] + [_lib.I]
    assert _lib.ABI_VERSION == 7 and h.gcgcn_version() == 7


def _err():
    return _lib.lib().gcgcn_last_error().decode()


def test_refusals_through_mx_without_a_gpu():
    """Shape and selector checks come before anything touches the device: a non-null dummy address is never dereferenced."""
    h = _lib.lib()
    p = 4096                # a 16-byte aligned non-null address
    attn_fwd = lambda B, T, H, dh, attn: h.gcgcn_bert_attn_fwd_mx(B, T, H, dh, p, None, None, p, p, None, 0, 0.0, None, attn)
    attn_bwd = lambda B, T, H, dh, attn: h.gcgcn_bert_attn_bwd_mx(B, T, H, dh, p, None, None, p, p, p, p, p, None, 0, 0.0, None, attn)
    for f in (attn_fwd, attn_bwd):
        assert f(1, 16, 1, 64, 2) != 0
        assert "attn = 2" in _err()
        assert f(1, 16, 1, 64, -1) != 0
        assert "attn = -1" in _err()
        assert f(1, 513, 1, 64, 1) != 0
        assert "513" in _err()
        assert f(1, 16, 1, 32, 1) != 0
        assert "32" in _err()
    plist = (_lib.P * 12)(*([p] * 12))
    lf = lambda T, D, H, mm, attn: h.gcgcn_bert_layer_fwd_mx(1, T, D, H, 4 * D, p, None, None, None, plist, p, p, 1 << 40, None, 0.0, 0.0, None,
                                                             mm, attn)
    lb = lambda T, D, H, mm, attn: h.gcgcn_bert_layer_bwd_mx(1, T, D, H, 4 * D, p, None, None, None, plist, p, 1 << 40, p, 8192, plist, p,
                                                             1 << 40, None, 0.0, 0.0, None, mm, attn)
    for f in (lf, lb):
        assert f(16, 64, 1, 0, 2) != 0
        assert "attn = 2" in _err()
        assert f(16, 64, 1, 2, 0) != 0
        assert "matmul = 2" in _err()
        assert f(513, 64, 1, 0, 1) != 0
        assert "513" in _err()
        assert f(16, 64, 2, 0, 1) != 0                      # D = 64 with two heads: a head width of 32
        assert "head width" in _err()
    # _mm still refuses matmul = 2 with its message
    assert h.gcgcn_bert_layer_fwd_mm(1, 16, 64, 1, 256, p, None, None, None, plist, p, p, 1 << 40, None, 0.0, 0.0, None, 2) != 0
    assert "matmul = 2 (0: fp32, 1: bf16 operands)" in _err()


# ---- how the bounds are set -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matmul", ["fp32", "bf16"])
@pytest.mark.parametrize("D,H", sorted(CONFIGS))
@pytest.mark.parametrize("B,T", MODEL_SWEEP)
def test_float32_within_a_tenth_of_the_bound(D, H, B, T, matmul):
    """BOUNDS[matmul] of tests/bert_attn_bf16_cases.py: the float32 CPU run of impl="torch", attention="bf16" against its float64 run."""
    got = C.run_model(C.fresh_model(D, H, dtype=torch.float32, matmul=matmul), model_case(D, H, B, T))
    ref = C.model_reference(D, H, B, T, matmul)
    C.worst(got, ref, f"float32 CPU, attention=bf16 matmul={matmul}, D={D} H={H} ({B},{T}), at bert_bf16_cases' (4e-2, 4e-2)", matmul, atol=4e-2,
            rtol=4e-2)
    fr = C.worst(got, ref, f"float32 CPU, attention=bf16 matmul={matmul}, D={D} H={H} ({B},{T})", matmul)
    assert max(fr.values()) <= 0.1, fr


@pytest.mark.parametrize("B,T", C.ATTN_T)
def test_core_float32_within_a_tenth_of_the_core_bound(B, T):
    """CORE_ATOL / CORE_RTOL: the float32 CPU run of Bf16AttentionFn against its float64 run, every mask kind."""
    H = 2
    for kind in C.KINDS:
        got = C.attn_def(attn_case(B, T, H, kind), H, torch.float32)
        fr = C.core_worst(got, C.attn_reference(B, T, H, kind), f"float32 CPU, bf16 core B={B} T={T} {kind}")
        assert max(fr.values()) <= 0.1, fr
