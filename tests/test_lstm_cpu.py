"""The HIP LSTM layer (csrc/lstm.hip, functional.lstm_layer, EncoderLSTM(impl="hip")): what holds without a GPU.  (The ABI's three
symbols against the header: tests/test_abi_cpu.py.)  The default encoder is the one it was; CPU tensors are refused; and the bound of
tests/test_lstm_gpu.py is one that float32 arithmetic can meet: torch's own float32 CPU LSTM meets it against float64 at every
shape of the GPU sweep."""
import numpy as np
import pytest
import torch
from torch import nn

import gcgcn_amd
from gcgcn_amd import _lib, models as M
from lstm_cases import H, SWEEP, TABLE, case, reference, run_torch, worst

def test_width_not_served_is_refused_on_the_host():
    h = _lib.lib()
    assert h.gcgcn_lstm_ws_bytes(4, 8, 140, 128, 2) > 0
    assert h.gcgcn_lstm_ws_bytes(4, 8, 140, 100, 2) == -1 and b"not served" in h.gcgcn_last_error()
    assert h.gcgcn_lstm_ws_bytes(4, 8, 140, 128, 3) == -1 and b"directions" in h.gcgcn_last_error()
    assert h.gcgcn_lstm_ws_bytes(4, 0, 140, 128, 2) == -1
    assert h.gcgcn_lstm_ws_bytes(0, 8, 140, 128, 2) == -1
    for args in ((4, 8, 140, 100, 2), (4, 8, 140, 128, 0), (4, 0, 140, 128, 1), (0, 8, 140, 128, 1)):
        assert h.gcgcn_lstm_fwd(*args, *([None] * 10)) != 0          # the shape is refused before any pointer is looked at
    assert h.gcgcn_lstm_fwd(4, 8, 140, 128, 2, *([None] * 10)) != 0 and b"null" in h.gcgcn_last_error()
    assert h.gcgcn_lstm_bwd(4, 8, 140, 128, 2, *([None] * 17), 0, None) != 0 and b"null" in h.gcgcn_last_error()


def _reference_encoder(input_size, num_units, nlayers, bidir):
    """The modules EncoderLSTM has always built, in its registration order (glove:377-400)."""
    m = nn.Module()
    m.rnns = nn.ModuleList(nn.LSTM(input_size if i == 0 else (num_units * 2 if bidir else num_units), num_units, 1, bidirectional=bidir,
                                   batch_first=True) for i in range(nlayers))
    nd = 2 if bidir else 1
    m.init_hidden = nn.ParameterList([nn.Parameter(torch.zeros(nd, 1, num_units)) for _ in range(nlayers)])
    m.init_c = nn.ParameterList([nn.Parameter(torch.zeros(nd, 1, num_units)) for _ in range(nlayers)])
    return m


@pytest.mark.parametrize("nlayers,bidir", [(1, True), (2, True), (1, False)])
def test_default_encoder_is_unchanged(nlayers, bidir):
    want = list(_reference_encoder(140, H, nlayers, bidir).state_dict().keys())
    for kw in ({}, {"impl": "torch"}, {"impl": "hip"}):
        enc = M.EncoderLSTM(140, H, nlayers, True, bidir, 0.2, False, **kw)
        assert list(enc.state_dict().keys()) == want, kw
        assert [type(m) for m in enc.rnns] == [nn.LSTM] * nlayers and isinstance(enc.dropout, M.LockedDropout)
    assert M.EncoderLSTM(140, H, 1, True, True, 0.2, False).impl == "torch"
    with pytest.raises(ValueError, match="impl"):
        M.EncoderLSTM(140, H, 1, True, True, 0.2, False, impl="miopen")
    # the default path computes what nn.LSTM computes on the same parameters
    enc = M.EncoderLSTM(140, H, nlayers, True, bidir, 0.0, False).eval()
    x = torch.randn(2, 5, 140, generator=torch.Generator().manual_seed(0))
    out, outs = x, []
    for i in range(nlayers):
        out, _ = enc.rnns[i](out, (enc.init_hidden[i].expand(-1, 2, -1).contiguous(), enc.init_c[i].expand(-1, 2, -1).contiguous()))
        outs.append(out)
    assert torch.equal(enc(x), torch.cat(outs, 2))


class _Cfg:
    entity_type_size, coref_size, max_length, keep_prob, graph_hop = 20, 20, 512, 1.0, 2
    dis_size, dis_num, dis_plus, relation_num, alpha = 20, 21, 10, 97, 1.0

    def __init__(self):
        self.data_word_vec = np.zeros((30, 100), np.float32)


def test_model_without_encoder_impl_is_unchanged():
    plain = M.GCGCN_glove(_Cfg())
    assert plain.rnn.impl == "torch"
    cfg = _Cfg()
    cfg.encoder_impl = "hip"
    opted = M.GCGCN_glove(cfg)
    assert opted.rnn.impl == "hip"
    assert list(plain.state_dict().keys()) == list(opted.state_dict().keys())
    rnn_keys = [k for k in plain.state_dict() if k.startswith("rnn.")]
    assert rnn_keys == ["rnn.rnns.0." + n for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse",
                                                     "weight_hh_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse")] + \
        ["rnn.init_hidden.0", "rnn.init_c.0"]
    assert not opted.load_state_dict(plain.state_dict(), strict=True).missing_keys
    assert not plain.load_state_dict(opted.state_dict(), strict=True).missing_keys
    assert "lstm_layer" in gcgcn_amd.__all__ and callable(gcgcn_amd.lstm_layer)


def test_cpu_tensors_are_refused():
    enc = M.EncoderLSTM(140, H, 1, True, True, 0.0, False, impl="hip")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        enc(torch.zeros(2, 3, 140))
    c = case(2, 3, 140)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gcgcn_amd.lstm_layer(c["x"], c["weight_ih_l0"], c["weight_hh_l0"], c["bias_ih_l0"], c["bias_hh_l0"], c["h0"][:1], c["c0"][:1])


@pytest.mark.parametrize("B,T,I", sorted(set(SWEEP) | set(TABLE)))
def test_float32_cpu_lstm_meets_the_bound(B, T, I):
    """The condition that keeps the GPU test's bound honest: torch's float32 CPU LSTM against float64, same inputs, every tensor."""
    fr = worst(run_torch(case(B, T, I), 2, torch.float32), reference(B, T, I), f"fp32 CPU (B,T,I)=({B},{T},{I})")
    assert max(fr.values()) <= 1.0, fr
