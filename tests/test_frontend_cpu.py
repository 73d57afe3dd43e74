"""The HIP token front end (csrc/frontend.hip, functional.token_embed / token_context, config.frontend_impl): what holds without
a GPU.  The ABI's five symbols are declared, bound and exported; the default models are the ones they were; CPU tensors are
refused; the host-side refusals answer before any pointer is looked at; and the bound of tests/test_frontend_gpu.py is one that
float32 arithmetic can meet: torch's own float32 CPU path meets it against float64 on every case of the GPU sweep."""

import numpy as np
import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib, models as M
from frontend_cases import SWEEP, inputs, reference, run_torch
from lstm_cases import worst



def test_symbols_are_declared_bound_and_exported():
    """The five C symbols against the header and the library: tests/test_abi_cpu.py.  Here: the ABI is the one it was and the package
    exports the two functions."""
    assert _lib.ABI_VERSION == 7 and _lib.lib().gcgcn_version() == 7                       # additive
    for name in ("token_embed", "token_context"):
        assert name in gcgcn_amd.__all__ and callable(getattr(gcgcn_amd, name))


def test_refusals_on_the_host():
    h = _lib.lib()
    ok = (2, 8, 30, 16, 7, 100, 20, 20)
    assert h.gcgcn_frontend_ws_bytes(*ok, 256) > 0 and h.gcgcn_frontend_ws_bytes(*ok, 0) > 0
    assert h.gcgcn_frontend_ws_bytes(2, 8, 0, 0, 0, 0, 0, 0, 808) > 0
    assert h.gcgcn_frontend_ws_bytes(2, 8, 0, 0, 0, 0, 0, 0, 0) == -1
    for i in range(8):                                                   # B, T, a table's rows or a width below 1
        bad = list(ok)
        bad[i] = 0 if i != 2 else -1
        assert h.gcgcn_frontend_ws_bytes(*bad, 0) == -1, i
        assert h.gcgcn_embed_fwd(*bad, *([None] * 9)) != 0, i              # the shape is refused before any pointer is looked at
        assert h.gcgcn_embed_bwd(*bad, *([None] * 5), 0, 0, *([None] * 4), 0, None) != 0, i
    assert h.gcgcn_embed_fwd(*ok, *([None] * 9)) != 0 and b"null" in h.gcgcn_last_error()
    assert h.gcgcn_embed_bwd(*ok, *([None] * 5), 0, 0, *([None] * 4), 0, None) != 0 and b"null" in h.gcgcn_last_error()
    for args in ((0, 8, 5, 256, 128), (2, 0, 5, 256, 128), (2, 8, 0, 256, 128), (2, 8, 5, 0, 128)):
        assert h.gcgcn_context_fwd(*args, *([None] * 8)) != 0 and b"bad shape" in h.gcgcn_last_error()
        assert h.gcgcn_context_bwd(*args, *([None] * 11), 0, None) != 0 and b"bad shape" in h.gcgcn_last_error()
    assert h.gcgcn_context_fwd(2, 8, 5, 256, 64, *([None] * 8)) != 0 and b"not served" in h.gcgcn_last_error()
    assert h.gcgcn_context_bwd(2, 8, 5, 256, 100, *([None] * 11), 0, None) != 0 and b"not served" in h.gcgcn_last_error()
    assert h.gcgcn_context_fwd(2, 8, 5, 256, 128, *([None] * 8)) != 0 and b"null" in h.gcgcn_last_error()
    assert h.gcgcn_context_bwd(2, 8, 5, 256, 128, *([None] * 11), 0, None) != 0 and b"null" in h.gcgcn_last_error()


class _Cfg:
    entity_type_size, coref_size, max_length, keep_prob, graph_hop = 20, 20, 512, 0.8, 2
    dis_size, dis_num, dis_plus, relation_num, alpha = 20, 21, 10, 97, 1.0

    def __init__(self, **kw):
        self.data_word_vec = np.zeros((30, 100), np.float32)
        self.__dict__.update(kw)


class _Bert(torch.nn.Module):
    def forward(self, document, output_all_encoded_layers=True):
        h = torch.zeros(*document.shape, 768)
        return h, h[:, 0]


def test_models_without_frontend_impl_are_unchanged():
    plain = M.GCGCN_glove(_Cfg())
    assert plain.frontend_impl == "torch" and plain.rnn.impl == "torch"
    for kw in (dict(frontend_impl="hip"), dict(frontend_impl="hip", encoder_impl="hip"), dict(encoder_impl="hip")):
        opted = M.GCGCN_glove(_Cfg(**kw))
        assert opted.frontend_impl == kw.get("frontend_impl", "torch") and opted.rnn.impl == kw.get("encoder_impl", "torch")   # independent
        assert list(plain.state_dict().keys()) == list(opted.state_dict().keys())
        assert not opted.load_state_dict(plain.state_dict(), strict=True).missing_keys
        assert not plain.load_state_dict(opted.state_dict(), strict=True).missing_keys
    with pytest.raises(ValueError, match="frontend_impl"):
        M.GCGCN_glove(_Cfg(frontend_impl="triton"))
    b0, b1 = (M.GraphCNN_multihead_bert_gate_cls(_Cfg(**kw), bert=_Bert()) for kw in ({}, dict(frontend_impl="hip")))
    assert (b0.frontend_impl, b1.frontend_impl) == ("torch", "hip") and list(b0.state_dict().keys()) == list(b1.state_dict().keys())
    # the default encode draws the locked-dropout mask as it always did: same seed, same output as the expression restated here
    plain.train()
    doc, z = torch.randint(0, 30, (2, 6)), torch.zeros(2, 6, dtype=torch.int64)
    torch.manual_seed(3)
    got = plain.encode(doc, z, z)
    torch.manual_seed(3)
    x = torch.cat([plain.word_emb(doc), plain.entity_embed(z), plain.ner_emb(z)], dim=-1)
    m = torch.empty(2, 1, 140).bernoulli_(0.8) / 0.8
    h0, c0 = (p.expand(-1, 2, -1).contiguous() for p in (plain.rnn.init_hidden[0], plain.rnn.init_c[0]))
    want = torch.tanh(plain.linear_re(plain.rnn.rnns[0](m.expand_as(x) * x, (h0, c0))[0]))
    assert torch.equal(got, want)


def test_cpu_tensors_are_refused():
    d = inputs(SWEEP[1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gcgcn_amd.token_embed(d["document"], d["document_pos"], d["document_ner"], d["word_w"], d["coref_w"], d["ner_w"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gcgcn_amd.token_context(torch.zeros(2, 2, 140), d["W"], d["b"], d["node_pos"])
    model = M.GCGCN_glove(_Cfg(frontend_impl="hip")).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.encode(d["document"], d["document_ner"], d["document_pos"])


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: c.label)
def test_float32_cpu_front_end_meets_the_bound(case):
    """The condition that keeps the GPU test's bound honest: torch's float32 CPU path against float64, same inputs, every tensor."""
    fr = worst(run_torch(case, inputs(case), torch.float32), reference(case), f"fp32 CPU {case.label}")
    assert max(fr.values()) <= 1.0, fr
