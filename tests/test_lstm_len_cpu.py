"""Per-row lengths through the HIP LSTM layer (csrc/lstm.hip, functional.lstm_layer(lengths=), EncoderLSTM(input_lengths=)): what
holds without a GPU.  The two additive symbols are declared and bound and refuse what the old ones refuse; the packed float64
reference of tests/lstm_len_cases.py is the per-document computation; float32 arithmetic can meet the bound against it; the torch
encoder with a lengths tensor is the per-document encoder; and the sweep can see the feature: the full-length LSTM is far outside
the bound wherever a row is shorter than T."""
import pytest
import torch
from torch import nn

from gcgcn_amd import _lib, models as M
from lstm_cases import reference as full_reference
from lstm_len_cases import CASES, H, IDS, case, frac_of_bound, param_names, padding_mask, reference, run_torch_packed, worst


def test_symbols_are_declared_and_bound():
    """Each is its plain twin's argument list with `const int* lens` in front of the stream: exactly one argument more.  (That the
    lists are the header's and the symbols the library's: tests/test_abi_cpu.py.)"""
    for name, old in (("gcgcn_lstm_fwd_len", "gcgcn_lstm_fwd"), ("gcgcn_lstm_bwd_len", "gcgcn_lstm_bwd")):
        plain = _lib.SIGNATURES[old][1]
        assert _lib.SIGNATURES[name][1] == plain[:-1] + [_lib.P] + plain[-1:]
        assert len(_lib.SIGNATURES[name][1]) == len(plain) + 1
    assert _lib.ABI_VERSION == 7 and _lib.lib().gcgcn_version() == 7          # additive


def test_refusals_on_the_host():
    """Shape first, then null pointers, then dout aliasing out -- with and without a lengths pointer (never dereferenced here)."""
    h = _lib.lib()
    lens = 0x1000
    for args in ((4, 8, 140, 100, 2), (4, 8, 140, 128, 0), (4, 0, 140, 128, 1), (0, 8, 140, 128, 1)):
        for ln in (None, lens):
            assert h.gcgcn_lstm_fwd_len(*args, *([None] * 9), ln, None) != 0 and b"null" not in h.gcgcn_last_error()
            assert h.gcgcn_lstm_bwd_len(*args, *([None] * 17), 0, ln, None) != 0 and b"null" not in h.gcgcn_last_error()
    assert h.gcgcn_lstm_fwd_len(4, 8, 140, 100, 2, *([None] * 9), lens, None) != 0 and b"not served" in h.gcgcn_last_error()
    for ln in (None, lens):
        assert h.gcgcn_lstm_fwd_len(4, 8, 140, 128, 2, *([None] * 9), ln, None) != 0 and b"null" in h.gcgcn_last_error()
        assert h.gcgcn_lstm_bwd_len(4, 8, 140, 128, 2, *([None] * 17), 0, ln, None) != 0 and b"null" in h.gcgcn_last_error()
    # every pointer given (fake, 16-byte aligned, distinct), dout == out: refused for the aliasing before anything is touched
    p = [0x10000 + 0x100 * i for i in range(17)]
    p[8] = p[5]                                                            # dout = out (x w_ih w_hh h0 c0 OUT gates csave DOUT ...)
    assert h.gcgcn_lstm_bwd_len(4, 8, 140, 128, 2, *p, 1 << 40, lens, None) != 0 and b"dout aliases the output" in h.gcgcn_last_error()


@pytest.mark.parametrize("B,T,I,lens,nd", CASES, ids=IDS)
def test_packed_reference_is_the_per_document_loop(B, T, I, lens, nd):
    """rnn(x[b:b+1, :len]) per document, float64, with the cotangent cut to the document: the packed reference's output and
    gradients, at a small fraction of the bound (two float64 computations)."""
    c = case(B, T, I, nd)
    ref = reference(B, T, I, lens, nd)
    rnn = nn.LSTM(I, H, 1, bidirectional=nd == 2, batch_first=True).double()
    with torch.no_grad():
        for n in param_names(nd):
            getattr(rnn, n).copy_(c[n])
    x, h0, c0 = (c[k].detach().double().requires_grad_() for k in ("x", "h0", "c0"))
    out = torch.zeros(B, T, nd * H, dtype=torch.float64)
    rows = []
    for b in range(B):
        rows.append(torch.cat([rnn(x[b:b + 1, :lens[b]], (h0, c0))[0], out[b:b + 1, lens[b]:]], 1))
    out = torch.cat(rows, 0)
    out.backward(c["dy"].double())
    got = {"out": out.detach(), "dx": x.grad, "dh0": h0.grad, "dc0": c0.grad}
    got.update({"d" + n: getattr(rnn, n).grad for n in param_names(nd)})
    fr = worst(got, ref, f"per-document loop (B,T,I)=({B},{T},{I}) nd={nd}")
    assert max(fr.values()) <= 1e-6, fr
    pad = padding_mask(B, T, lens)
    assert not ref["out"][pad].any() and not ref["dx"][pad].any()          # what the GPU test asks of the kernels' padding


@pytest.mark.parametrize("B,T,I,lens,nd", CASES, ids=IDS)
def test_float32_cpu_packed_lstm_meets_the_bound(B, T, I, lens, nd):
    """The condition that keeps the GPU test's bound honest: torch's float32 CPU LSTM over the same packed sequence."""
    fr = worst(run_torch_packed(case(B, T, I, nd), nd, lens, torch.float32), reference(B, T, I, lens, nd),
               f"fp32 CPU packed (B,T,I)=({B},{T},{I}) nd={nd}")
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize("B,T,I,lens,nd", [c for c in CASES if min(c[3]) < c[1]], ids=[i for i, c in zip(IDS, CASES) if min(c[3]) < c[1]])
def test_the_full_length_lstm_is_outside_the_bound(B, T, I, lens, nd):
    """What the batched call computes without lengths is NOT the lengths reference: the sweep can see the feature."""
    full, ref = full_reference(B, T, I, nd), reference(B, T, I, lens, nd)
    fr = worst({k: full[k] for k in ref}, ref, f"full length against lengths (B,T,I)=({B},{T},{I}) nd={nd}")
    assert fr["out"] > 1.0 and fr["dx"] > 1.0, fr
    if nd == 2:                                                             # the reverse direction of a shorter row starts elsewhere
        short = [b for b in range(B) if lens[b] < T]
        real = ~padding_mask(B, T, lens)
        got, want = full["out"][..., H:], ref["out"][..., H:]
        assert frac_of_bound(got[short][real[short]], want[short][real[short]]) > 1.0


@pytest.mark.parametrize("nlayers,bidir", [(1, True), (2, True), (1, False)])
def test_torch_encoder_with_lengths_is_the_per_document_encoder(nlayers, bidir):
    g = torch.Generator().manual_seed(5)
    enc = M.EncoderLSTM(140, H, nlayers, True, bidir, 0.2, False).eval().double()
    with torch.no_grad():
        for p in enc.parameters():
            p.copy_(torch.randn(p.shape, generator=g, dtype=torch.float64) * (0.5 if p.dim() == 3 else 0.1))
    B, T = 5, 9
    lens = torch.tensor([9, 1, 4, 7, 2])
    x = torch.randn(B, T, 140, generator=g, dtype=torch.float64)
    with torch.no_grad():
        got = enc(x, lens)
        assert got.shape == (B, T, nlayers * (2 if bidir else 1) * H)
        for b in range(B):
            want = enc(x[b:b + 1, :lens[b]])
            assert frac_of_bound(got[b:b + 1, :lens[b]], want) <= 1e-6
            assert not got[b, lens[b]:].any()
        assert torch.equal(enc(x, T), enc(x)) and torch.equal(enc(x, None), enc(x))     # a non-tensor is ignored, as before
        assert frac_of_bound(enc(x, torch.full((B,), T)), enc(x)) <= 1e-6


def test_cpu_tensors_are_refused_with_lengths_too():
    import gcgcn_amd
    c = case(2, 3, 140)
    args = (c["x"], c["weight_ih_l0"], c["weight_hh_l0"], c["bias_ih_l0"], c["bias_hh_l0"], c["h0"][:1], c["c0"][:1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gcgcn_amd.lstm_layer(*args, lengths=torch.tensor([3, 1]))
