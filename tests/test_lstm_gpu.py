"""The HIP LSTM layer (csrc/lstm.hip: functional.lstm_layer, EncoderLSTM(impl="hip"), GCGCN_glove with config.encoder_impl = "hip")
against torch.nn.LSTM on the CPU in float64 (tests/lstm_cases.py: the reference, the sweep and the bound), at the edges of its
kernels: the 16-row batch tile, the ends and both parities of the time loop, the guarded and interior GEMM bodies.  Every case
prints its largest error as a fraction of the bound.  (tests/test_lstm_cpu.py shows torch's float32 CPU LSTM within 0.1 of the
same bound at the same shapes.)"""
import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib, functional as F_, models as M
from lstm_cases import Cfg, doc_tensors, load_model, H, SWEEP, case, frac_of_bound, param_names, reference, worst

pytestmark = pytest.mark.gpu


def _leaves(c, nd, dev):
    t = {k: v.to(dev).requires_grad_() for k, v in c.items() if k != "dy"}
    return t, c["dy"].to(dev)


def _layer(t, nd):
    rev = [t[n] for n in param_names(nd)[4:]]
    return gcgcn_amd.lstm_layer(t["x"], t["weight_ih_l0"], t["weight_hh_l0"], t["bias_ih_l0"], t["bias_hh_l0"], t["h0"], t["c0"], *rev)


def run_hip(c, nd, dev):
    t, dy = _leaves(c, nd, dev)
    out = _layer(t, nd)
    out.backward(dy)
    res = {"out": out.detach(), "dx": t["x"].grad, "dh0": t["h0"].grad, "dc0": t["c0"].grad}
    res.update({"d" + n: t[n].grad for n in param_names(nd)})
    return res


@pytest.mark.parametrize("B,T,I", SWEEP)
def test_layer_matches_float64(gpu_device, B, T, I):
    fr = worst(run_hip(case(B, T, I), 2, gpu_device), reference(B, T, I), f"hip (B,T,I)=({B},{T},{I})")
    assert max(fr.values()) <= 1.0, fr


def test_unidirectional_matches_float64(gpu_device):
    fr = worst(run_hip(case(17, 3, 140, nd=1), 1, gpu_device), reference(17, 3, 140, nd=1), "hip nd=1 (17,3,140)")
    assert max(fr.values()) <= 1.0, fr


def test_two_stacked_layers_match_the_torch_encoder(gpu_device):
    """EncoderLSTM(nlayers=2, concat=True) in eval mode, impl="hip" against impl="torch" on the same device and parameters, at the
    bound of every other case."""
    g = torch.Generator().manual_seed(11)
    ref = M.EncoderLSTM(140, H, 2, True, True, 0.2, False).eval()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * (0.5 if p.dim() == 3 else 0.1))
    hip = M.EncoderLSTM(140, H, 2, True, True, 0.2, False, impl="hip").eval()
    hip.load_state_dict(ref.state_dict(), strict=True)
    ref, hip = ref.to(gpu_device), hip.to(gpu_device)
    x = torch.randn(17, 5, 140, generator=g).to(gpu_device)
    with torch.no_grad():
        want, got = ref(x), hip(x)
    assert got.shape == (17, 5, 4 * H)
    fr = frac_of_bound(got, want)
    print(f"two layers, hip against torch on the device: {fr:.3f} of the bound")
    assert fr <= 1.0


def test_direction_of_time(gpu_device):
    """An input that is zero except at step k, zero biases and initial states: the forward half of the output is exactly zero before
    step k (and not from k on), the reverse half exactly zero after it (and not up to k)."""
    B, T, I, k = 3, 7, 5, 4
    c = {n: v.clone() for n, v in case(B, T, I).items()}
    for n in c:
        if "bias" in n or n in ("h0", "c0"):
            c[n].zero_()
    c["x"].zero_()
    c["x"][:, k] = 1.0
    t, _ = _leaves(c, 2, gpu_device)
    with torch.no_grad():
        out = _layer(t, 2).cpu()
    fwd, rev = out[..., :H], out[..., H:]
    assert not fwd[:, :k].any() and fwd[:, k:].abs().amin(dim=(0, 2)).gt(0).all()
    assert not rev[:, k + 1:].any() and rev[:, :k + 1].abs().amin(dim=(0, 2)).gt(0).all()


def _raw_call(dev, B, T, I, nd, alias_dout=False):
    """The C ABI on buffers with one NaN guard row (a whole batch entry) past B; everything NaN-filled before the calls."""
    c = case(B, T, I, nd)
    cat = lambda names: torch.cat([c[n] for n in names], 0).to(dev)
    pn = param_names(nd)
    w_ih, w_hh = cat(pn[0::4]), cat(pn[1::4])
    bias = torch.cat([c[pn[4 * d + 2]] + c[pn[4 * d + 3]] for d in range(nd)], 0).to(dev)
    x, dy = c["x"].to(dev), c["dy"].to(dev)
    h0, c0 = (c[k].expand(nd, B, H).contiguous().to(dev) for k in ("h0", "c0"))
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    out, csave, gates, dgates = nan(B + 1, T, nd * H), nan(B + 1, T, nd * H), nan((B + 1) * T, nd * 4 * H), nan((B + 1) * T, nd * 4 * H)
    dx, dh0, dc0 = nan(B + 1, T, I), nan(nd, B, H), nan(nd, B, H)
    dw_ih, dw_hh, db = nan(nd * 4 * H, I), nan(nd * 4 * H, H), nan(nd * 4 * H)
    p, st = F_._p, F_._stream
    _lib.call("gcgcn_lstm_fwd", B, T, I, H, nd, p(x), p(w_ih), p(w_hh), p(bias), p(h0), p(c0), p(out), p(gates), p(csave), st())
    ws = torch.full((_lib.lib().gcgcn_lstm_ws_bytes(B, T, I, H, nd) // 4,), float("nan"), device=dev)
    bufs = dict(out=out, csave=csave, gates=gates, dgates=dgates, dx=dx, dh0=dh0, dc0=dc0, dw_ih=dw_ih, dw_hh=dw_hh, db=db)
    _lib.call("gcgcn_lstm_bwd", B, T, I, H, nd, p(x), p(w_ih), p(w_hh), p(h0), p(c0), p(out), p(gates), p(csave), p(out if alias_dout else dy),
              p(dgates), p(dx), p(dw_ih), p(dw_hh), p(db), p(dh0), p(dc0), p(ws), ws.numel() * 4, st())
    torch.cuda.synchronize()
    return bufs


def test_padding_rows_are_neither_read_into_results_nor_written(gpu_device):
    B, T = 17, 3                                                         # the second tile holds one row and fifteen padding rows
    bufs = _raw_call(gpu_device, B, T, 140, 2)
    for k in ("out", "csave", "dx"):
        assert torch.isfinite(bufs[k][:B]).all(), k
        assert torch.isnan(bufs[k][B:]).all(), f"{k}: the guard row was written"
    for k in ("gates", "dgates"):
        assert torch.isfinite(bufs[k][:B * T]).all(), k
        assert torch.isnan(bufs[k][B * T:]).all(), f"{k}: the guard row was written"
    for k in ("dh0", "dc0", "dw_ih", "dw_hh", "db"):
        assert torch.isfinite(bufs[k]).all(), f"{k} holds NaN"
    ref = reference(B, T, 140)
    assert frac_of_bound(bufs["out"][:B], ref["out"]) <= 1.0 and frac_of_bound(bufs["dx"][:B], ref["dx"]) <= 1.0


def test_two_runs_are_bitwise_equal(gpu_device):
    c = case(33, 37, 140)
    a, b = run_hip(c, 2, gpu_device), run_hip(c, 2, gpu_device)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_graph_replay_equals_eager(gpu_device):
    """Forward + backward of lstm_layer captured in a hipGraph and replayed on NEW input contents, against the eager call, bit for bit."""
    B, T, I = 17, 5, 140
    c0_, c1_ = case(B, T, I, seed=1), case(B, T, I, seed=2)
    t, dy = _leaves(c0_, 2, gpu_device)
    names = list(t)

    def step():
        out = _layer(t, 2)
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
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    for name, g, e in zip(["out"] + names, held, eager):
        assert torch.equal(g, e), name
    fr = frac_of_bound(held[0], reference(B, T, I, seed=2)["out"])
    assert fr <= 1.0                                                     # ... and it is the new contents' result


def test_no_grad_forward_equals_the_training_forward(gpu_device):
    c = case(17, 37, 140)
    enc = M.EncoderLSTM(140, H, 1, True, True, 0.3, False, impl="hip").to(gpu_device)
    with torch.no_grad():
        for n in param_names(2):
            getattr(enc.rnns[0], n).copy_(c[n])
        enc.init_hidden[0].copy_(c["h0"])
        enc.init_c[0].copy_(c["c0"])
    x = c["x"].to(gpu_device)
    enc.eval()
    with torch.no_grad():
        quiet = enc(x)
    assert not quiet.requires_grad
    enc.train()
    enc.dropout.dropout = 0.0                                              # the same arithmetic, with the backward's tensors saved
    loud = enc(x)
    assert loud.requires_grad and torch.equal(quiet, loud.detach())


def test_model_with_hip_encoder_matches_the_default_model(gpu_device):
    """GCGCN_glove at the model_step_c1 fixture's sizes, eval mode, same state_dict and inputs: config.encoder_impl = "hip" against
    the default model; strict loads both ways."""
    g, sd, plain = load_model(gpu_device)
    plain.eval()
    cfg = Cfg(g["meta"]["vocab"])
    cfg.encoder_impl = "hip"
    opted = M.GCGCN_glove(cfg).to(gpu_device).eval()
    assert opted.rnn.impl == "hip" and plain.rnn.impl == "torch"
    for dst, src in ((opted, plain), (plain, opted)):
        res = dst.load_state_dict(src.state_dict(), strict=True)
        assert not res.missing_keys and not res.unexpected_keys
    docs = [doc_tensors(g["raw"], di, gpu_device) for di in range(g["meta"]["docs"])]
    batch = {k: torch.stack([d[k] for d in docs]) for k in docs[0]}
    with torch.no_grad():
        want, got = plain(**batch), opted(**batch)
    fr = frac_of_bound(got, want)
    print(f"model logits, hip encoder against the default: {fr:.3f} of the bound")
    assert fr <= 1.0


def test_refusals(gpu_device):
    dev = gpu_device
    g = torch.Generator().manual_seed(3)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.1).to(dev)
    with pytest.raises(RuntimeError, match="hidden width 100 is not served"):
        gcgcn_amd.lstm_layer(r(2, 3, 140), r(400, 140), r(400, 100), r(400), r(400), r(1, 1, 100), r(1, 1, 100))
    with pytest.raises(ValueError, match="reverse direction"):
        gcgcn_amd.lstm_layer(r(2, 3, 140), r(512, 140), r(512, 128), r(512), r(512), r(2, 1, 128), r(2, 1, 128), w_ih_r=r(512, 140))
    with pytest.raises(RuntimeError, match="dout aliases the output"):
        _raw_call(dev, 2, 3, 140, 2, alias_dout=True)
    torch.cuda.synchronize()
