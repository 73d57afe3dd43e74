"""recurrent="bf16" of the HIP LSTM layer (csrc/lstm.hip, the BF instantiations of the two recurrence kernels) on the GPU: through
lstm_layer, through the C ABI with the announcement gcgcn_set_option("lstm_recurrent", .), through EncoderLSTM and GCGCN_glove.
The reference is functional.lstm_layer_bf16_definition on the CPU in float64; the three bounds (LOOSE end to end, the flip-free step
replay, representable operands) and how they were set: tests/lstm_bf16_cases.py.  Every parity case prints its largest error as a
fraction of its bound."""
import pytest
import torch

from gcgcn_amd import _lib, functional as F_, models as M
from lstm_bf16_cases import (H, LEN_CASES, LOOSE, REPLAY_IDS, REPLAY_SHAPES, SWEEP, SWEEP_IDS, case, discriminating_case, frac_of_bound, param_names,
                             reference, replay, replay_fractions, representable_case, run_definition, run_hip, stacked, worst)
from lstm_cases import Cfg, doc_tensors, load_model, run_torch
from lstm_len_cases import IDS as LEN_IDS, padding_mask

pytestmark = pytest.mark.gpu

ANNOUNCE = b"lstm_recurrent"   # gcgcn_set_option(ANNOUNCE, v): the recurrent argument of this thread's next LSTM call (include/gcgcn.h)


# ---- end to end, the loose bound ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,I,nd", SWEEP, ids=SWEEP_IDS)
def test_layer_matches_the_float64_definition(gpu_device, B, T, I, nd):
    got = run_hip(case(B, T, I, nd), nd, gpu_device)
    fr = worst(got, reference(B, T, I, nd), f"hip bf16 (B,T,I)=({B},{T},{I}) nd={nd}, loose bound", LOOSE)
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize("B,T,I,lens,nd", LEN_CASES, ids=LEN_IDS)
def test_layer_with_lengths_matches_the_float64_definition(gpu_device, B, T, I, lens, nd):
    """Against the definition with the same lengths (which test_lstm_bf16_cpu shows to be the per-document truncated layer); out and
    dx exactly 0 at the padding, with a clean cotangent and with NaN in it there."""
    c, ref, pad = case(B, T, I, nd), reference(B, T, I, nd, lens), padding_mask(B, T, lens)
    dy = c["dy"].clone()
    dy[pad] = float("nan")
    for label, cot in (("", None),) + ((("NaN cotangent at padding, ", dy),) if bool(pad.any()) else ()):
        got = run_hip(c, nd, gpu_device, lens, dy=cot)
        fr = worst(got, ref, f"hip bf16 lengths, {label}(B,T,I)=({B},{T},{I}) nd={nd}, loose bound", LOOSE)
        assert max(fr.values()) <= 1.0, fr
        assert torch.equal(got["out"].cpu()[pad], torch.zeros(int(pad.sum()), nd * H)), "out is not exactly 0 at a padded position"
        assert torch.equal(got["dx"].cpu()[pad], torch.zeros(int(pad.sum()), I)), "dx is not exactly 0 at a padded position"


# ---- the C ABI: step replay, announcement -----------------------------------------------------------------------------------------------
def _raw(dev, c, nd, lens, announce_fwd, announce_bwd=None, backward=True):
    """gcgcn_lstm_fwd_len (+ _bwd_len) on NaN-filled buffers, each announced with the given value (None: no announcement)."""
    B, T, I = c["x"].shape
    st = {k: v.to(dev) for k, v in stacked(c, nd).items()}
    x, dy = c["x"].detach().to(dev), c["dy"].to(dev)
    ln = None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    b = dict(out=nan(B, T, nd * H), csave=nan(B, T, nd * H), gates=nan(B * T, nd * 4 * H), dgates=nan(B * T, nd * 4 * H), dx=nan(B, T, I),
             dh0=nan(nd, B, H), dc0=nan(nd, B, H), dw_ih=nan(nd * 4 * H, I), dw_hh=nan(nd * 4 * H, H), db=nan(nd * 4 * H))
    p, stream = F_._p, F_._stream
    if announce_fwd is not None:
        _lib.call("gcgcn_set_option", ANNOUNCE, announce_fwd)
    _lib.call("gcgcn_lstm_fwd_len", B, T, I, H, nd, p(x), p(st["w_ih"]), p(st["w_hh"]), p(st["bias"]), p(st["h0"]), p(st["c0"]), p(b["out"]),
              p(b["gates"]), p(b["csave"]), p(ln), stream())
    if backward:
        ws = torch.full((_lib.lib().gcgcn_lstm_ws_bytes(B, T, I, H, nd) // 4,), float("nan"), device=dev)
        if announce_bwd is not None:
            _lib.call("gcgcn_set_option", ANNOUNCE, announce_bwd)
        _lib.call("gcgcn_lstm_bwd_len", B, T, I, H, nd, p(x), p(st["w_ih"]), p(st["w_hh"]), p(st["h0"]), p(st["c0"]), p(b["out"]), p(b["gates"]),
                  p(b["csave"]), p(dy), p(b["dgates"]), p(b["dx"]), p(b["dw_ih"]), p(b["dw_hh"]), p(b["db"]), p(b["dh0"]), p(b["dc0"]), p(ws),
                  ws.numel() * 4, p(ln), stream())
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in b.items()}


@pytest.mark.parametrize("B,T,I,lens", REPLAY_SHAPES, ids=REPLAY_IDS)
def test_step_replay_from_the_kernels_own_buffers(gpu_device, B, T, I, lens):
    """Every step recomputed in float64 from what the kernels themselves wrote, so that no rounding can flip: the lane maps, the
    k-block order, the double buffers' parities and the length selects held to (a doubling of) the fp32 suite's bound."""
    c = case(B, T, I, 2)
    b = _raw(gpu_device, c, 2, lens, 1, 1)
    live = (torch.arange(T)[None, :] < (torch.full((B,), T) if lens is None else torch.tensor(lens))[:, None])[:, :, None]
    got = {k: b[k].view(B, T, -1) if k in ("gates", "dgates") else b[k] for k in ("out", "csave", "gates", "dgates", "dh0", "dc0")}
    for k in ("out", "dgates"):
        assert torch.isfinite(got[k]).all() and not got[k][~live.expand_as(got[k])].any(), f"{k}: not written, or not 0 at the padding"
    src = {k: torch.where(live, got[k], torch.zeros(())) for k in ("out", "csave", "gates", "dgates")}   # unwritten (NaN) where inactive
    exp, masks = replay(c, 2, lens, src)
    fr = replay_fractions(got, exp, masks, f"hip bf16 step replay (B,T,I)=({B},{T},{I}) {'lengths' if lens else 'full'}")
    assert max(fr.values()) <= 1.0, fr


def test_announcement_is_taken_by_the_next_call_only(gpu_device):
    """An announced call runs bf16; the call after it, unannounced, runs fp32 bit for bit; 2 is refused and consumed as well."""
    c = case(17, 3, 140)
    plain = _raw(gpu_device, c, 2, None, None)
    bf = _raw(gpu_device, c, 2, None, 1, 1)
    after = _raw(gpu_device, c, 2, None, None)
    zero = _raw(gpu_device, c, 2, None, 0, 0)
    for k in plain:
        assert torch.equal(plain[k], after[k]) and torch.equal(plain[k], zero[k]), k
    assert not torch.equal(plain["out"], bf["out"]) and not torch.equal(plain["dh0"], bf["dh0"])
    for backward in (False, True):
        with pytest.raises(RuntimeError, match="lstm_recurrent = 2"):
            _raw(gpu_device, c, 2, None, *((2,) if not backward else (None, 2)), backward=backward)
        again = _raw(gpu_device, c, 2, None, None)
        for k in plain:
            assert torch.equal(plain[k], again[k]), k
    mixed = _raw(gpu_device, c, 2, None, 1, None)             # the backward of a bf16 forward, unannounced: the fp32 kernel on its buffers
    assert torch.equal(mixed["out"], bf["out"]) and not torch.equal(mixed["dh0"], bf["dh0"])


# ---- precision where nothing is rounded, and where everything is ------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [1, 2])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
def test_representable_operands_meet_the_fp32_bound(gpu_device, B, nd):
    c = representable_case(B, nd)
    got, ref = run_hip(c, nd, gpu_device), run_torch(c, nd, torch.float64)
    fr = {k: frac_of_bound(got[k], ref[k]) for k in ("out", "dc0")}
    print(f"hip bf16, representable operands B={B} nd={nd}: out={fr['out']:.3f} dc0={fr['dc0']:.3f} of the fp32 bound")
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize("nd", [1, 2])
def test_discriminating_case(gpu_device, nd):
    """The rounded recurrent product is 0, the unrounded one 12 (lstm_bf16_cases.discriminating_case).  The bf16 route meets the
    definition at the fp32 suite's bound -- T = 1: nothing rounded depends on anything computed, except dh0 = r(dgates) r(W_hh), which
    is held to the loose bound -- and is far from the fp32 route."""
    c = discriminating_case(nd)
    got, ref, plain = run_hip(c, nd, gpu_device), run_definition(c, nd, torch.float64), run_hip(c, nd, gpu_device, recurrent="fp32")
    fr = worst(got, ref, f"hip bf16, discriminating case nd={nd}, fp32 bound")
    assert max(v for k, v in fr.items() if k != "dh0") <= 1.0 and fr["dh0"] <= LOOSE, fr
    far = worst(got, plain, f"hip bf16 against hip fp32, discriminating case nd={nd}, loose bound", LOOSE)
    assert max(far.values()) >= 100.0, far


# ---- bits -----------------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bitwise_equal(gpu_device):
    B, T, I, lens, nd = LEN_CASES[5]
    c = case(B, T, I, nd)
    for ln in (None, lens):
        a, b = run_hip(c, nd, gpu_device, ln), run_hip(c, nd, gpu_device, ln)
        for k in a:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("B,T,I,nd", [(16, 4, 140, 2), (33, 37, 140, 2), (17, 5, 140, 1)])
def test_lengths_all_T_equal_no_lengths_bitwise(gpu_device, B, T, I, nd):
    c = case(B, T, I, nd)
    a, b = run_hip(c, nd, gpu_device, None), run_hip(c, nd, gpu_device, (T,) * B)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _encoder(dev, recurrent, impl="hip", nlayers=1):
    enc = M.EncoderLSTM(140, H, nlayers, True, True, 0.0, False, impl=impl, recurrent=recurrent)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for p in enc.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.5 if p.dim() == 3 else 0.1))
    return enc.to(dev)


def test_no_grad_forward_equals_the_saving_forward(gpu_device):
    enc = _encoder(gpu_device, "bf16")
    x = case(17, 37, 140)["x"].to(gpu_device)
    for lengths in (None, torch.tensor([(7 * i) % 37 + 1 for i in range(17)], device=gpu_device)):
        with torch.no_grad():
            quiet = enc(x, lengths)
        loud = enc(x, lengths)
        assert loud.requires_grad and not quiet.requires_grad and torch.equal(quiet, loud.detach())


def test_graph_replay_on_new_contents_equals_eager(gpu_device):
    """Forward + backward of lstm_layer(lengths=, recurrent="bf16") captured in a hipGraph and replayed on NEW contents of every
    input, against the eager call, bit for bit: both announcements are made while capturing and belong to the captured calls."""
    B, T, I = 17, 5, 140
    lens0, lens1 = tuple((3 * i) % 5 + 1 for i in range(B)), tuple((2 * i + 1) % 5 + 1 for i in range(B))
    c0_, c1_ = case(B, T, I, seed=1), case(B, T, I, seed=2)
    t = {k: v.detach().to(gpu_device).requires_grad_() for k, v in c0_.items() if k != "dy"}
    dy = c0_["dy"].to(gpu_device)
    ln = torch.tensor(lens0, dtype=torch.int32, device=gpu_device)
    names = list(t)

    def step():
        out = F_.lstm_layer(t["x"], *(t[n] for n in param_names(2)[:4]), t["h0"], t["c0"], *(t[n] for n in param_names(2)[4:]), lengths=ln,
                            recurrent="bf16")
        return (out,) + torch.autograd.grad(out, [t[n] for n in names], dy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    with torch.no_grad():
        for n in names:
            t[n].copy_(c1_[n])
        dy.copy_(c1_["dy"])
        ln.copy_(torch.tensor(lens1, dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    for name, g, e in zip(["out"] + names, held, eager):
        assert torch.equal(g, e), name
    ref = reference(B, T, I, 2, lens1, seed=2)
    assert frac_of_bound(held[0], ref["out"], LOOSE) <= 1.0 and frac_of_bound(held[1 + names.index("x")], ref["dx"], LOOSE) <= 1.0
    plain = run_hip(c1_, 2, gpu_device, lens1, recurrent=None)
    assert not torch.equal(plain["out"], held[0]), "the captured calls ran fp32"


# ---- the default is untouched ---------------------------------------------------------------------------------------------------------
def test_fp32_keyword_and_no_keyword_are_bitwise_equal(gpu_device):
    B, T, I, lens, nd = LEN_CASES[5]
    c = case(B, T, I, nd)
    for ln in (None, lens):
        bf = run_hip(c, nd, gpu_device, ln)                      # an announced pair in front: nothing of it is left behind
        a, b = run_hip(c, nd, gpu_device, ln, recurrent=None), run_hip(c, nd, gpu_device, ln, recurrent="fp32")
        for k in a:
            assert torch.equal(a[k], b[k]), k
        assert not torch.equal(a["out"], bf["out"])


# ---- module and model -----------------------------------------------------------------------------------------------------------------
def test_two_stacked_layers_match_the_definition_on_the_device(gpu_device):
    hip, ref = _encoder(gpu_device, "bf16", nlayers=2), _encoder(gpu_device, "bf16", impl="torch", nlayers=2)
    ref.load_state_dict(hip.state_dict(), strict=True)
    x = torch.randn(17, 5, 140, generator=torch.Generator().manual_seed(12)).to(gpu_device)
    lengths = torch.tensor([(3 * i) % 5 + 1 for i in range(17)], device=gpu_device)
    for ln in (None, lengths):
        with torch.no_grad():
            want, got = ref(x, ln), hip(x, ln)
        assert got.shape == (17, 5, 4 * H)
        fr = frac_of_bound(got, want, LOOSE)
        print(f"two layers bf16, hip against the definition on the device ({'lengths' if ln is not None else 'full'}): {fr:.3f} of the loose bound")
        assert fr <= 1.0


def _model(g, sd, dev, impl, recurrent=None):
    cfg = Cfg(g["meta"]["vocab"], impl)
    if recurrent is not None:
        cfg.encoder_recurrent = recurrent
    model = M.GCGCN_glove(cfg).to(dev).eval()
    res = model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return model


def test_model_with_bf16_encoder_matches_the_definition_model(gpu_device):
    """GCGCN_glove at the model_step_c1 fixture's sizes, eval mode: encoder_impl = "hip" against encoder_impl = "torch", both with
    encoder_recurrent = "bf16", logits at the loose bound; the distance to the fp32 model is printed.  A checkpoint saved under one
    setting loads strictly under the other."""
    g, sd, plain = load_model(gpu_device, "hip")
    hip, ref = _model(g, sd, gpu_device, "hip", "bf16"), _model(g, sd, gpu_device, "torch", "bf16")
    assert hip.rnn.recurrent == "bf16" and hip.rnn.impl == "hip" and plain.rnn.recurrent == "fp32"
    for dst, src in ((hip, plain), (plain, hip)):
        res = dst.load_state_dict(src.state_dict(), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    assert all(v.dtype == torch.float32 for k, v in hip.state_dict().items() if k.startswith("rnn."))
    docs = [doc_tensors(g["raw"], di, gpu_device) for di in range(g["meta"]["docs"])]
    batch = {k: torch.stack([d[k] for d in docs]) for k in docs[0]}
    with torch.no_grad():
        want, got, fp32 = ref(**batch), hip(**batch), plain(**batch)
    fr = frac_of_bound(got, want, LOOSE)
    print(f"model logits, bf16 hip encoder against the bf16 definition: {fr:.3f} of the loose bound; against the fp32 model: "
          f"{frac_of_bound(got, fp32):.1f} of the fp32 bound")
    assert fr <= 1.0
