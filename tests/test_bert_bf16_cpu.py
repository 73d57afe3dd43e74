"""matmul="bf16" without a GPU: the plain-PyTorch definition against a hand-written restatement, the selector's defaults and refusals,
the new symbols, and the two facts about chosen seeds and constants that the GPU tests rely on."""
import math

import numpy as np
import pytest
import torch

from gcgcn_amd import _lib, functional as Fn, models as M
from gcgcn_amd import bert as bert_mod
from gcgcn_amd.bert import BertModel

import bert_bf16_cases as C
from bert_cases import CONFIGS, MODEL_SWEEP, config, masks, model_case, state
from gemm_bf16_cases import case as gemm_case, reference as gemm_reference


def _r(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _by_hand(x, kb, params, H, dy):
    """Section 4 of the feature's definition written out, forward and backward, without autograd.Function: each Linear is
    bf16(x) bf16(W)^T + b; its backward dX = bf16(dY) bf16(W), dW = bf16(dY)^T bf16(X), db = sum of the unrounded dY.  Everything
    between the Linears goes through autograd on detached pieces."""
    wq, bq, wk, bk, wv, bv, wo, bo, g1, b1, wi, bi, wo2, bo2, g2, b2 = [t.double() for t in params]
    B, T, D = x.shape
    dh = D // H
    x = x.double()
    grads = {}

    def lin(inp, w, b):
        return _r(inp) @ _r(w).t() + b

    def lin_bwd(dout, inp, w):
        d2, i2 = dout.reshape(-1, dout.shape[-1]), inp.reshape(-1, inp.shape[-1])
        return (_r(dout) @ _r(w)), _r(d2).t() @ _r(i2), d2.sum(0)

    split = lambda t: t.view(B, T, H, dh).permute(0, 2, 1, 3)
    # forward, keeping a leaf at the output of every Linear
    q0, k0, v0 = (lin(x, w, b).detach().requires_grad_() for w, b in ((wq, bq), (wk, bk), (wv, bv)))
    s = split(q0) @ split(k0).transpose(-1, -2) / math.sqrt(dh)
    if kb is not None:
        s = s + kb.double()[:, None, None, :]
    ctx = (torch.softmax(s, -1) @ split(v0)).permute(0, 2, 1, 3).reshape(B, T, D)
    ctx_l = ctx.detach()
    ao = lin(ctx_l, wo, bo).detach().requires_grad_()
    x_l = x.detach().requires_grad_()
    g1l, b1l, g2l, b2l = (t.detach().requires_grad_() for t in (g1, b1, g2, b2))
    a = bert_mod.layer_norm(ao + x_l, g1l, b1l)
    a_l = a.detach().requires_grad_()
    z = lin(a_l.detach(), wi, bi).detach().requires_grad_()
    i_ = bert_mod.gelu(z)
    o2 = lin(i_.detach(), wo2, bo2).detach().requires_grad_()
    y = bert_mod.layer_norm(o2 + a_l, g2l, b2l)
    # backward, by hand across the Linears
    y.backward(dy.double())
    di, grads["wo2"], grads["bo2"] = lin_bwd(o2.grad, i_.detach(), wo2)
    i_.backward(di)
    da_lin, grads["wi"], grads["bi"] = lin_bwd(z.grad, a_l.detach(), wi)
    a.backward(a_l.grad + da_lin)
    dctx, grads["wo"], grads["bo"] = lin_bwd(ao.grad, ctx_l, wo)
    ctx.backward(dctx)
    dx = x_l.grad.clone()
    for leaf, w, n in ((q0, wq, "q"), (k0, wk, "k"), (v0, wv, "v")):
        d, grads["w" + n], grads["b" + n] = lin_bwd(leaf.grad, x, w)
        dx = dx + d
    order = [grads["wq"], grads["bq"], grads["wk"], grads["bk"], grads["wv"], grads["bv"], grads["wo"], grads["bo"], g1l.grad, b1l.grad,
             grads["wi"], grads["bi"], grads["wo2"], grads["bo2"], g2l.grad, b2l.grad]
    res = {"y": y.detach(), "dx": dx}
    res.update({f"d{i:02d}": t for i, t in enumerate(order)})
    return res


@pytest.mark.parametrize("kind", ["none", "holes"])
def test_definition_equals_its_restatement_by_hand(kind):
    """impl="torch", matmul="bf16" in float64: one layer's output and all 17 gradients at 1e-12 of the restatement; the model runs that
    layer (checked through its first layer's output)."""
    D, H, B, T = 128, 2, 3, 33
    g = torch.Generator().manual_seed(4)
    x, dy = torch.randn(B, T, D, generator=g), torch.randn(B, T, D, generator=g)
    m = masks(B, T, kind)
    kb = None if m is None else (1.0 - m) * -10000.0
    model = C.fresh_model(D, H)
    params = [t.detach() for t in model.encoder.layer[0].tensors()]
    got = C.layer_torch(x, kb, params, H, dy)
    want = _by_hand(x, kb, params, H, dy)
    for k in want:
        scale = max(1.0, want[k].abs().max().item())
        assert (got[k] - want[k]).abs().max().item() <= 1e-12 * scale, k
    # the rounding is really there: the fp32-matmul layer differs by far more than 1e-12
    plain = bert_mod.torch_layer(x.double(), None if kb is None else kb.double(), [t.double() for t in params], H, lambda s, t: t)
    assert (plain - want["y"]).abs().max().item() > 1e-4


def test_model_runs_the_definition_in_every_layer():
    D, H, B, T = 128, 2, 3, 33
    case = model_case(D, H, B, T)
    model = C.fresh_model(D, H)
    got = C.run_model(model, case)
    e = model.embeddings
    emb = e.word_embeddings(case["ids"]) + e.position_embeddings(torch.arange(T))[None] + e.token_type_embeddings(case["tt"])
    x = bert_mod.layer_norm(emb, e.LayerNorm.weight, e.LayerNorm.bias).detach()
    kb = (1.0 - case["mask"].double()) * -10000.0
    for li, layer in enumerate(model.encoder.layer):
        x = bert_mod.torch_layer(x, kb, [t.detach() for t in layer.tensors()], H, lambda s, t: t, bert_mod.bf16_linear)
        assert torch.equal(x, got[f"out{li}"])
    assert torch.equal(got["pooled"], torch.tanh(model.pooler.dense(x[:, 0])).detach())      # the pooler keeps its own arithmetic


def test_fp32_selector_and_no_selector_are_bitwise_equal():
    D, H, B, T = 128, 2, 3, 33
    case = model_case(D, H, B, T)
    plain = BertModel(config(D, H))
    plain.load_state_dict(state(D, H))
    a = C.run_model(plain.double(), case)
    b = C.run_model(C.fresh_model(D, H, matmul="fp32"), case)
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert BertModel(config(D, H)).matmul == "fp32"
    c = C.run_model(C.fresh_model(D, H, matmul="bf16"), case)
    assert not torch.equal(a["out1"], c["out1"])
    assert list(plain.state_dict()) == list(C.fresh_model(D, H, matmul="bf16").state_dict())   # one checkpoint for both settings


def test_unknown_values_are_refused():
    with pytest.raises(ValueError, match="matmul"):
        BertModel(config(128, 2), matmul="fp16")
    with pytest.raises(ValueError, match="matmul"):
        BertModel(config(128, 2), impl="hip", matmul=1)
    x = torch.zeros(1, 4, 64)
    ps = [t.detach() for t in BertModel(config(64, 1)).encoder.layer[0].tensors()]
    with pytest.raises(ValueError, match="matmul"):        # refused before anything else, CPU tensors included
        Fn.bert_layer(x, None, *ps, matmul="tf32")


class _Cfg:
    entity_type_size, coref_size, max_length, keep_prob, graph_hop = 20, 20, 512, 1.0, 2
    dis_size, dis_num, dis_plus, relation_num, alpha = 20, 21, 10, 97, 1.0

    def __init__(self, vocab, **kw):
        self.data_word_vec = np.zeros((vocab, 100), np.float32)
        self.__dict__.update(kw)


def test_model_config_selector():
    bc = config(128, 2)
    with pytest.raises(ValueError, match="bert_impl"):
        M.GraphCNN_multihead_bert_gate_cls(_Cfg(61, bert_matmul="bf16", bert_config=bc), bert=BertModel(bc))
    with pytest.raises(ValueError, match="bert_matmul"):
        M.GraphCNN_multihead_bert_gate_cls(_Cfg(61, bert_impl="torch", bert_matmul="half", bert_config=bc))
    m = M.GraphCNN_multihead_bert_gate_cls(_Cfg(61, bert_impl="torch", bert_matmul="bf16", bert_config=bc))
    assert m.bert.matmul == "bf16" and m.bert.impl == "torch"
    plain = M.GraphCNN_multihead_bert_gate_cls(_Cfg(61, bert_impl="torch", bert_config=bc))
    assert plain.bert.matmul == "fp32"
    assert list(m.state_dict()) == list(plain.state_dict())


def test_new_symbols_are_declared_bound_and_exported():
    """The four symbols against the header and the library: tests/test_abi_cpu.py.  Here: how their lists relate, and the sizes."""
    h = _lib.lib()
    for name in ("gcgcn_bert_layer_fwd", "gcgcn_bert_layer_bwd"):          # the _len argument list plus the selector
        assert _lib.SIGNATURES[name + "_mm"][1] == _lib.SIGNATURES[name + "_len"][1] + [_lib.I]
    assert h.gcgcn_version() == 7
    assert h.gcgcn_gemm_bf16_ws_bytes(64, 64, 64) == 0                      # one tile, one k-step: nothing to split
    assert h.gcgcn_gemm_bf16_ws_bytes(128, 128, 2048) > 0                   # the weight gradient's shape class: split K
    assert h.gcgcn_gemm_bf16_ws_bytes(0, 1, 1) == -1


def test_unrounded_product_violates_the_gemm_bound_for_the_chosen_seed():
    """What test_gemm_bf16_gpu.test_operands_are_really_rounded_to_bf16 relies on, with the emulation alone: at (64, 64, 32), NT, the
    float64 product of the UNROUNDED operands lies outside the bound around the rounded operands' product on at least half of the
    elements (operand rounding is about 2^-9 relative per factor; the bound is about 3e-4 there)."""
    c = gemm_case("nt", 64, 64, 32)
    ref, bound = gemm_reference(c, "nt")
    exact, _ = gemm_reference(c, "nt", rounded=False)
    out = ((exact - ref).abs() > bound).double().mean().item()
    print(f"unrounded product outside the bound on {out:.3f} of the elements; median bound {bound.median().item():.2e}")
    assert out >= 0.5
    # and the fp32 emulation of the path under test (rounded operands, fp32 accumulation) lies inside it everywhere
    emu = c["a"].to(torch.bfloat16).float() @ c["b"].to(torch.bfloat16).float().t()
    assert ((emu.double() - ref).abs() <= bound).all()


@pytest.mark.parametrize("D,H", sorted(CONFIGS))
@pytest.mark.parametrize("B,T", MODEL_SWEEP)
def test_float32_within_a_tenth_of_the_bound(D, H, B, T):
    """How ATOL / RTOL of tests/bert_bf16_cases.py are set: the float32 CPU run of the definition against its float64 run."""
    got = C.run_model(C.fresh_model(D, H, dtype=torch.float32), model_case(D, H, B, T))
    fr = C.worst(got, C.model_reference(D, H, B, T), f"float32 CPU, matmul=bf16, D={D} H={H} ({B},{T})")
    assert max(fr.values()) <= 0.1, fr
