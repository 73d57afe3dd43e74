"""The BERT encoder without a device: the ABI's additions, the state_dict contract, the plain-PyTorch implementation against torch's
own primitives and against float64, the refusals, and the model switch (config.bert_impl)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gcgcn_amd
from gcgcn_amd import _lib, models as M
from gcgcn_amd import bert as bert_mod
from gcgcn_amd.bert import BertConfig, BertModel

from bert_cases import (ATTN_TABLE, CONFIGS, MODEL_SWEEP, attn_case, attn_ref, attn_reference, config, model_case, model_reference,
                        run_model, state, worst)



def test_symbols_declared_bound_exported():
    """The ten C symbols against the header and the library: tests/test_abi_cpu.py.  Here: the ABI version and the Python names."""
    h = _lib.lib()                      # loading binds every declaration of the header and checks the ABI version
    assert _lib.ABI_VERSION == 7 and h.gcgcn_version() == 7
    for name in ("BertConfig", "BertModel", "load_pretrained_state_dict"):
        assert name in gcgcn_amd.__all__ and hasattr(gcgcn_amd, name)
    assert callable(gcgcn_amd.functional.bert_layer) and callable(gcgcn_amd.functional.res_layer_norm)


def _expected_keys(layers):
    keys = [f"embeddings.{n}.weight" for n in ("word_embeddings", "position_embeddings", "token_type_embeddings")]
    keys += ["embeddings.LayerNorm.weight", "embeddings.LayerNorm.bias"]
    for i in range(layers):
        p = f"encoder.layer.{i}."
        for lin in ("attention.self.query", "attention.self.key", "attention.self.value", "attention.output.dense", "attention.output.LayerNorm",
                    "intermediate.dense", "output.dense", "output.LayerNorm"):
            keys += [p + lin + ".weight", p + lin + ".bias"]
    return keys + ["pooler.dense.weight", "pooler.dense.bias"]


def test_state_dict_keys():
    for impl in ("torch", "hip"):
        assert set(BertModel(config(128, 2), impl=impl).state_dict().keys()) == set(_expected_keys(2))
    c = BertConfig()
    assert (c.vocab_size, c.hidden_size, c.num_hidden_layers, c.num_attention_heads, c.intermediate_size, c.max_position_embeddings,
            c.type_vocab_size, c.hidden_dropout_prob, c.attention_probs_dropout_prob) == (30522, 768, 12, 12, 3072, 512, 2, 0.1, 0.1)


def test_gamma_beta_checkpoint_round_trip(tmp_path):
    sd = state(128, 2)
    old = {}
    for k, v in sd.items():
        k = k.replace("LayerNorm.weight", "LayerNorm.gamma").replace("LayerNorm.bias", "LayerNorm.beta")
        old["bert." + k] = v
    assert any(k.endswith(".gamma") for k in old) and not any("LayerNorm.weight" in k for k in old)
    path = str(tmp_path / "ckpt.bin")
    torch.save(old, path)
    model = BertModel(config(128, 2))
    res = gcgcn_amd.load_pretrained_state_dict(model, path)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in model.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_torch_impl_agrees_with_torchs_primitives():
    """float64 round-off against code not written for this library: scaled_dot_product_attention with the additive mask,
    F.layer_norm(eps=1e-12), F.gelu."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(5, 7, 128, generator=g, dtype=torch.float64)
    w, b = torch.randn(128, generator=g, dtype=torch.float64), torch.randn(128, generator=g, dtype=torch.float64)
    torch.testing.assert_close(bert_mod.layer_norm(x, w, b), F.layer_norm(x, (128,), w, b, eps=1e-12), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(bert_mod.gelu(x * 3), F.gelu(x * 3), rtol=1e-12, atol=1e-13)
    # a whole layer, its attention through SDPA
    B, T, D, H = 3, 33, 128, 2
    case = model_case(D, H, B, T, "prefix")
    model = BertModel(config(D, H)).double()
    model.load_state_dict(state(D, H))
    layer = model.encoder.layer[0]
    xs = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    kb = (1.0 - case["mask"].double()) * -10000.0
    got = bert_mod.torch_layer(xs, kb, layer.tensors(), H, lambda s, t: t)
    a = layer.attention
    split = lambda t: t.view(B, T, H, D // H).transpose(1, 2)
    ctx = F.scaled_dot_product_attention(split(a.self.query(xs)), split(a.self.key(xs)), split(a.self.value(xs)),
                                         attn_mask=kb[:, None, None, :].expand(B, H, T, T))
    ctx = ctx.transpose(1, 2).reshape(B, T, D)
    h = F.layer_norm(a.output.dense(ctx) + xs, (D,), a.output.LayerNorm.weight, a.output.LayerNorm.bias, eps=1e-12)
    want = F.layer_norm(layer.output.dense(F.gelu(layer.intermediate.dense(h))) + h, (D,), layer.output.LayerNorm.weight,
                        layer.output.LayerNorm.bias, eps=1e-12)
    torch.testing.assert_close(got, want, rtol=1e-11, atol=1e-11)
    # the attention reference of the core's tests is the same arithmetic
    ac = attn_case(B, T, H, "holes")
    r = attn_ref(ac, H, torch.float64)
    q, k, v = (ac["qkv"].double()[..., i * D:(i + 1) * D].reshape(B, T, H, 64).transpose(1, 2) for i in range(3))
    want = F.scaled_dot_product_attention(q, k, v, attn_mask=ac["key_bias"].double()[:, None, None, :].expand(B, H, T, T))
    torch.testing.assert_close(r["ctx"], want.transpose(1, 2).reshape(B, T, D), rtol=1e-11, atol=1e-11)


def test_call_contract():
    model = BertModel(config(128, 2)).eval()
    ids = torch.randint(0, 61, (2, 9))
    with torch.no_grad():
        all_layers, pooled = model(ids)
        last, pooled2 = model(ids, torch.zeros_like(ids), torch.ones(2, 9), output_all_encoded_layers=False)
    assert isinstance(all_layers, list) and len(all_layers) == 2 and last.shape == (2, 9, 128) and pooled.shape == (2, 128)
    assert torch.equal(all_layers[-1], last) and torch.equal(pooled, pooled2)          # the defaults: zeros and ones
    assert torch.equal(pooled, torch.tanh(model.pooler.dense(last[:, 0])))
    dead = torch.ones(2, 9)
    dead[1] = 0                                                                          # every key masked: a finite softmax
    with torch.no_grad():
        out, _ = model(ids, attention_mask=dead, output_all_encoded_layers=False)
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("D,H", sorted(CONFIGS))
def test_float32_within_a_tenth_of_the_bound(D, H):
    """The bound's constants come from this run (tests/bert_cases.py): float32 impl="torch" on the CPU against float64."""
    worst_all = 0.0
    for B, T in MODEL_SWEEP:
        fr = worst(run_model(D, H, model_case(D, H, B, T), torch.float32), model_reference(D, H, B, T), f"float32 cpu D={D} H={H} ({B},{T})")
        worst_all = max(worst_all, max(fr.values()))
    if (D, H) == (128, 2):
        for B, T in ATTN_TABLE:
            for kind in ("none", "prefix"):
                fr = worst(attn_ref(attn_case(B, T, H, kind), H, torch.float32), attn_reference(B, T, H, kind), f"float32 cpu core ({B},{T}) {kind}")
                worst_all = max(worst_all, max(fr.values()))
    assert worst_all <= 0.1, worst_all


def test_hip_impl_refuses_cpu_tensors():
    model = BertModel(config(128, 2), impl="hip").eval()
    with pytest.raises(RuntimeError, match="MI355X only"):
        model(torch.randint(0, 61, (2, 9)))
    x = torch.zeros(2, 4, 128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gcgcn_amd.functional.res_layer_norm(x, torch.ones(128), torch.zeros(128))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gcgcn_amd.functional.bert_layer(x, None, *BertModel(config(128, 2)).encoder.layer[0].tensors())
    with pytest.raises(ValueError, match="head width of 64"):
        BertModel(BertConfig(hidden_size=128, num_attention_heads=4), impl="hip")


class _Cfg:
    entity_type_size, coref_size, max_length, keep_prob, graph_hop = 20, 20, 512, 0.8, 2
    dis_size, dis_num, dis_plus, relation_num, alpha = 20, 21, 10, 97, 1.0

    def __init__(self, **kw):
        self.data_word_vec = np.zeros((30, 100), np.float32)
        self.__dict__.update(kw)


def test_model_switch(tmp_path):
    """config.bert_impl builds the library's encoder (no third-party package); without it the constructor is what it was.  The graph
    blocks behind the encoder have no CPU path, so here the model is built and its encoder runs forward and backward on the CPU;
    tests/test_bert_gpu.py runs the whole model."""
    try:
        import pytorch_pretrained_bert  # noqa: F401
        have = True
    except ImportError:
        have = False
    if not have:
        with pytest.raises(ImportError, match="pytorch_pretrained_bert"):
            M.GraphCNN_multihead_bert_gate_cls(_Cfg())
    with pytest.raises(ValueError, match="bert_impl"):
        M.GraphCNN_multihead_bert_gate_cls(_Cfg(bert_impl="triton"))
    path = str(tmp_path / "w.bin")
    torch.save({k.replace("LayerNorm.weight", "LayerNorm.gamma"): v for k, v in state(128, 2).items()}, path)
    model = M.GraphCNN_multihead_bert_gate_cls(_Cfg(bert_impl="torch", bert_config=config(128, 2), bert_weights=path))
    assert isinstance(model.bert, BertModel) and model.bert.impl == "torch"
    assert model.linear_re.in_features == 128 + 20 + 20 and model.linear_cls.in_features == 128
    assert torch.equal(model.bert.embeddings.LayerNorm.weight, state(128, 2)["embeddings.LayerNorm.weight"])
    hip = M.GraphCNN_multihead_bert_gate_cls(_Cfg(bert_impl="hip", bert_config=config(128, 2)))
    assert list(hip.state_dict().keys()) == list(model.state_dict().keys())
    assert not hip.load_state_dict(model.state_dict(), strict=True).missing_keys
    ids = torch.randint(0, 61, (2, 11))
    mask = torch.arange(11)[None, :] < torch.tensor([11, 4])[:, None]
    model.train()
    doc, pooled = model.bert(ids, attention_mask=mask, output_all_encoded_layers=False)
    assert doc.shape == (2, 11, 128)
    (doc.sum() + pooled.sum()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.bert.parameters())


def test_sizes_and_refusals_without_a_device():
    h = _lib.lib()
    R, D, Hh, I = 4 * 512, 768, 12, 3072
    per_token = 7 * D + 2 * I + Hh + 4                       # DESIGN.md section 8.9 (+ D for the layer's input, the caller's)
    assert h.gcgcn_bert_layer_ws_bytes(4, 512, D, Hh, I, 0) == 4 * R * per_token
    assert h.gcgcn_bert_layer_ws_bytes(4, 512, D, Hh, I, 1) > 0 and h.gcgcn_res_ln_ws_bytes(768) > 0
    assert h.gcgcn_bert_layer_ws_bytes(4, 513, D, Hh, I, 0) == -1 and b"T = 513" in h.gcgcn_last_error()
    assert h.gcgcn_bert_layer_ws_bytes(4, 512, 768, 8, I, 0) == -1 and b"head width" in h.gcgcn_last_error()
    assert h.gcgcn_bert_layer_ws_bytes(4, 512, D, Hh, I, 2) == -1 and b"which" in h.gcgcn_last_error()
    assert h.gcgcn_bert_attn_fwd(2, 16, 2, 32, *([None] * 5), 0, 0.0, None) != 0 and b"head width 32" in h.gcgcn_last_error()
    assert h.gcgcn_bert_attn_fwd(2, 513, 2, 64, *([None] * 5), 0, 0.0, None) != 0 and b"T = 513" in h.gcgcn_last_error()
    assert h.gcgcn_bert_attn_bwd(2, 513, 2, 64, *([None] * 8), 0, 0.0, None) != 0 and b"T = 513" in h.gcgcn_last_error()
    assert h.gcgcn_bert_attn_bwd(2, 16, 2, 48, *([None] * 8), 0, 0.0, None) != 0 and b"head width 48" in h.gcgcn_last_error()
    assert h.gcgcn_bert_attn_fwd(2, 16, 2, 64, *([None] * 5), 0, 0.0, None) != 0 and b"null" in h.gcgcn_last_error()
    assert h.gcgcn_res_ln_fwd(4, 96, *([None] * 9), 0, 0.0, None) != 0 and b"multiple of 64" in h.gcgcn_last_error()
    assert h.gcgcn_res_ln_fwd(4, 1088, *([None] * 9), 0, 0.0, None) != 0 and b"at most 1024" in h.gcgcn_last_error()
    assert h.gcgcn_res_ln_ws_bytes(100) == -1
    assert h.gcgcn_bias_gelu_fwd(4, 6, None, None, None, None) != 0
