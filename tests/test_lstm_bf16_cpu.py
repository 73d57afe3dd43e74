"""recurrent="bf16" of the LSTM layer without a GPU: the definition (functional.lstm_layer_bf16_definition / Bf16RecurrentFn), the
rule that sets the bounds of tests/test_lstm_bf16_gpu.py, the discriminating case, EncoderLSTM(impl="torch", recurrent="bf16") and
the argument checks.  Cases, references and bounds: tests/lstm_bf16_cases.py."""
import pytest
import torch

from gcgcn_amd import functional as F_, models as M
from lstm_bf16_cases import (LEN_CASES, LOOSE, REPLAY_IDS, REPLAY_SHAPES, SWEEP, SWEEP_IDS, case, discriminating_case, frac_of_bound, param_names,
                             reference, replay, replay_fractions, representable_case, run_definition, worst)
from lstm_cases import Cfg, run_torch
from lstm_len_cases import IDS as LEN_IDS, padding_mask, run_torch_packed

SMALL = [(17, 3, 140, 2), (33, 37, 140, 2), (17, 3, 140, 1)]


@pytest.mark.parametrize("B,T,I,nd", SMALL + [(2, 512, 140, 2)])
def test_definition_without_rounding_is_the_float64_lstm(B, T, I, nd):
    c = case(B, T, I, nd)
    fr = worst(run_definition(c, nd, torch.float64, rounding=False), run_torch(c, nd, torch.float64), f"definition, rounding off ({B},{T},{I}) nd={nd}")
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize("B,T,I,lens,nd", [LEN_CASES[k] for k in (1, 3, 5, 8)], ids=[LEN_IDS[k] for k in (1, 3, 5, 8)])
def test_definition_without_rounding_is_the_packed_float64_lstm(B, T, I, lens, nd):
    c = case(B, T, I, nd)
    fr = worst(run_definition(c, nd, torch.float64, lens, rounding=False), run_torch_packed(c, nd, lens, torch.float64),
               f"definition, rounding off, lengths ({B},{T},{I}) nd={nd}")
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize("B,T,I,nd", SWEEP, ids=SWEEP_IDS)
def test_loose_bound_rule_on_the_sweep(B, T, I, nd):
    """The rule of lstm_bf16_cases (1): the float32 definition is within 0.1 of the LOOSE bound of its float64 run."""
    fr = worst(run_definition(case(B, T, I, nd), nd, torch.float32), reference(B, T, I, nd), f"float32 definition, loose bound ({B},{T},{I}) nd={nd}", LOOSE)
    assert max(fr.values()) <= 0.1, fr


@pytest.mark.parametrize("B,T,I,lens,nd", LEN_CASES, ids=LEN_IDS)
def test_loose_bound_rule_on_the_length_cases(B, T, I, lens, nd):
    fr = worst(run_definition(case(B, T, I, nd), nd, torch.float32, lens), reference(B, T, I, nd, lens),
               f"float32 definition, loose bound, lengths ({B},{T},{I}) nd={nd}", LOOSE)
    assert max(fr.values()) <= 0.1, fr


@pytest.mark.parametrize("B,T,I,lens", REPLAY_SHAPES, ids=REPLAY_IDS)
def test_replay_bound_rule(B, T, I, lens):
    """The rule of lstm_bf16_cases (2): the float32 CPU run of the recurrence, replayed step by step in float64 from its own
    buffers, is within 0.1 of the replay's bound."""
    c = case(B, T, I, 2)
    run32, _ = replay(c, 2, lens, None, torch.float32)
    exp, masks = replay(c, 2, lens, {k: run32[k] for k in ("out", "csave", "gates", "dgates")})
    fr = replay_fractions(run32, exp, masks, f"float32 recurrence replayed ({B},{T},{I}) {'lengths' if lens else 'full'}")
    assert max(fr.values()) <= 0.1, fr


def test_replay_feeding_itself_is_the_definition():
    """The replay's recurrence, run on its own in float64, is the definition's (a short case: no step for a rounding to flip at)."""
    B, T, I, lens = REPLAY_SHAPES[1]
    run, _ = replay(case(B, T, I, 2), 2, lens, None)
    ref = reference(B, T, I, 2, lens)
    assert frac_of_bound(run["out"], ref["out"]) <= 1.0
    assert frac_of_bound(run["dh0"].sum(1, keepdim=True), ref["dh0"]) <= 1.0 and frac_of_bound(run["dc0"].sum(1, keepdim=True), ref["dc0"]) <= 1.0


@pytest.mark.parametrize("nd", [1, 2])
def test_discriminating_case_separates_the_definition_from_the_fp32_layer(nd):
    """r(h0) r(W_hh)^T is 0 where h0 W_hh^T is 12: the definition is far outside the LOOSE bound of the fp32 layer, so a bf16 route
    that silently ran fp32 could not pass test_lstm_bf16_gpu's check at this case."""
    c = discriminating_case(nd)
    d, n = run_definition(c, nd, torch.float64), run_torch(c, nd, torch.float64)
    print(f"nd={nd}: |out| differs by up to {(d['out'] - n['out']).abs().max().item():.3f}")
    fr = worst(d, n, f"definition against float64 nn.LSTM, discriminating case nd={nd}, loose bound", LOOSE)
    assert max(fr.values()) >= 100.0 and fr["out"] >= 10.0, fr
    fr = worst(run_definition(c, nd, torch.float32), d, f"float32 definition, discriminating case nd={nd}")   # T = 1: no flip
    assert max(fr.values()) <= 0.1, fr


@pytest.mark.parametrize("B", [1, 17])
def test_representable_operands_need_no_rounding(B):
    c = representable_case(B, 2)
    d, n = run_definition(c, 2, torch.float64), run_torch(c, 2, torch.float64)
    assert frac_of_bound(d["out"], n["out"]) <= 1.0 and frac_of_bound(d["dc0"], n["dc0"]) <= 1.0


def test_bf16_recurrent_fn_is_the_documented_product():
    g = torch.Generator().manual_seed(5)
    a, w, dy = torch.randn(5, 128, generator=g), torch.randn(512, 128, generator=g), torch.randn(5, 512, generator=g)
    a.requires_grad_(), w.requires_grad_()
    y = F_.Bf16RecurrentFn.apply(a, w)
    r = lambda t: t.detach().to(torch.bfloat16).float()
    assert torch.equal(y, r(a) @ r(w).t())
    y.backward(dy)
    assert torch.equal(a.grad, r(dy) @ r(w)) and torch.equal(w.grad, dy.t() @ a.detach())
    a2, w2 = a.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    F_.Bf16RecurrentFn.apply(a2, w2, False).backward(dy)
    assert torch.equal(a2.grad, dy @ w.detach()) and torch.equal(w2.grad, dy.t() @ a.detach())


def _encoder(recurrent, nlayers=2, seed=0):
    torch.manual_seed(seed)
    enc = M.EncoderLSTM(20, 128, nlayers, True, True, 0.0, False, impl="torch", recurrent=recurrent)
    with torch.no_grad():
        for p in list(enc.init_hidden) + list(enc.init_c):
            p.normal_(0, 0.5)
    return enc


def test_torch_impl_with_bf16_honours_lengths():
    """Zeros at the padding, and every row of the batch is the one-document call at its own length; the gradient to the input is 0
    at the padding even with NaN in the cotangent there.  In float64: a product's last bits depend on the batch size, and in float32
    that can move an h across a bf16 boundary."""
    enc = _encoder("bf16").double()
    B, T, lens = 3, 6, (6, 2, 4)
    x = torch.randn(B, T, 20, generator=torch.Generator().manual_seed(1), dtype=torch.float64).requires_grad_()
    out = enc(x, torch.tensor(lens))
    pad = padding_mask(B, T, lens)
    assert out.shape == (B, T, 2 * 2 * 128) and not out[pad].any()
    for b, n in enumerate(lens):
        alone = enc(x[b:b + 1, :n].detach(), torch.tensor([n]))
        assert torch.allclose(out[b:b + 1, :n], alone, rtol=0, atol=1e-12), b
    dy = torch.randn(out.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    dy[pad] = float("nan")
    out.backward(dy)
    assert torch.isfinite(x.grad).all() and not x.grad[pad].any()
    for p in enc.parameters():
        assert torch.isfinite(p.grad).all()


def test_torch_impl_with_bf16_differs_from_fp32_and_shares_the_state_dict():
    a, b = _encoder("fp32"), _encoder("bf16")
    assert list(a.state_dict()) == list(b.state_dict())
    res = b.load_state_dict(a.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    x = torch.randn(2, 5, 20, generator=torch.Generator().manual_seed(3))
    ya, yb = a(x), b(x)
    assert ya.shape == yb.shape and not torch.equal(ya, yb) and torch.allclose(ya, yb, atol=5e-2)
    assert all(p.dtype == torch.float32 for p in b.parameters())


def test_arguments_are_validated():
    with pytest.raises(ValueError, match="recurrent"):
        M.EncoderLSTM(20, 128, 1, True, True, 0.0, False, recurrent="bf16 ")
    with pytest.raises(ValueError, match="recurrent"):
        M.EncoderLSTM(20, 128, 1, True, True, 0.0, False, impl="hip", recurrent="half")
    assert M.EncoderLSTM(20, 128, 1, True, True, 0.0, False).recurrent == "fp32"
    c = case(3, 5, 7)
    with pytest.raises(ValueError, match="recurrent"):
        F_.lstm_layer(c["x"], *(c[n] for n in param_names(2)[:4]), c["h0"], c["c0"], *(c[n] for n in param_names(2)[4:]), recurrent="fp16")


def test_encoder_recurrent_needs_encoder_impl():
    cfg = Cfg(50)
    cfg.encoder_recurrent = "bf16"
    with pytest.raises(ValueError, match="encoder_impl"):
        M.GCGCN_glove(cfg)
    for impl in ("torch", "hip"):
        cfg = Cfg(50, impl)
        cfg.encoder_recurrent = "bf16"
        assert M.GCGCN_glove(cfg).rnn.recurrent == "bf16"
    cfg = Cfg(50, "hip")
    cfg.encoder_recurrent = "half"
    with pytest.raises(ValueError, match="recurrent"):
        M.GCGCN_glove(cfg)
    assert M.GCGCN_glove(Cfg(50)).rnn.recurrent == "fp32"
