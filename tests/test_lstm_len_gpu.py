"""Per-row lengths through the HIP LSTM layer (csrc/lstm.hip: lstm_layer(lengths=), EncoderLSTM(input_lengths=), GCGCN_glove and the
BERT model with t_valid) against torch.nn.LSTM over a packed sequence on the CPU in float64 (tests/lstm_len_cases.py), at the
project's bound, every element.  Every parity case prints its largest error as a fraction of the bound.  (tests/test_lstm_len_cpu.py
shows torch's float32 CPU packed LSTM within 0.05 of the same bound on the same cases, and the full-length LSTM 3e4 and more
outside it.)"""
import pytest
import torch
import torch.nn.functional as F

import gcgcn_amd
from gcgcn_amd import _lib, functional as F_, models as M
from lstm_cases import Cfg, doc_tensors, load_model
from lstm_len_cases import CASES, H, IDS, case, frac_of_bound, param_names, padding_mask, reference, worst

pytestmark = pytest.mark.gpu


def _leaves(c, dev):
    t = {k: v.detach().to(dev).requires_grad_() for k, v in c.items() if k != "dy"}
    return t, c["dy"].to(dev)


def _layer(t, nd, lengths):
    rev = [t[n] for n in param_names(nd)[4:]]
    return gcgcn_amd.lstm_layer(t["x"], t["weight_ih_l0"], t["weight_hh_l0"], t["bias_ih_l0"], t["bias_hh_l0"], t["h0"], t["c0"], *rev,
                                lengths=lengths)


def run_hip(c, nd, dev, lens, dy=None, dtype=torch.int32):
    t, dy_ = _leaves(c, dev)
    out = _layer(t, nd, None if lens is None else torch.tensor(lens, dtype=dtype, device=dev))
    out.backward(dy_ if dy is None else dy.to(dev))
    res = {"out": out.detach(), "dx": t["x"].grad, "dh0": t["h0"].grad, "dc0": t["c0"].grad}
    res.update({"d" + n: t[n].grad for n in param_names(nd)})
    return res


@pytest.mark.parametrize("B,T,I,lens,nd", CASES, ids=IDS)
def test_layer_with_lengths_matches_the_packed_float64_lstm(gpu_device, B, T, I, lens, nd):
    got = run_hip(case(B, T, I, nd), nd, gpu_device, lens, dtype=torch.int64 if B == 3 else torch.int32)
    fr = worst(got, reference(B, T, I, lens, nd), f"hip lengths (B,T,I)=({B},{T},{I}) nd={nd}")
    assert max(fr.values()) <= 1.0, fr
    pad = padding_mask(B, T, lens)
    assert torch.equal(got["out"].cpu()[pad], torch.zeros(int(pad.sum()), nd * H)), "out is not exactly 0 at a padded position"
    assert torch.equal(got["dx"].cpu()[pad], torch.zeros(int(pad.sum()), I)), "dx is not exactly 0 at a padded position"


@pytest.mark.parametrize("B,T,I,lens,nd", [c for c in CASES if min(c[3]) < c[1]], ids=[i for i, c in zip(IDS, CASES) if min(c[3]) < c[1]])
def test_nan_cotangent_at_padding_reaches_nothing(gpu_device, B, T, I, lens, nd):
    c = case(B, T, I, nd)
    dy = c["dy"].clone()
    dy[padding_mask(B, T, lens)] = float("nan")
    got = run_hip(c, nd, gpu_device, lens, dy=dy)
    for n, v in got.items():
        assert torch.isfinite(v).all(), f"{n} holds NaN / inf"
    fr = worst(got, reference(B, T, I, lens, nd), f"hip lengths, NaN cotangent at padding (B,T,I)=({B},{T},{I}) nd={nd}")
    assert max(fr.values()) <= 1.0, fr


def _raw_call(dev, B, T, I, nd, lens):
    """The C ABI (gcgcn_lstm_fwd_len / _bwd_len) on buffers with one NaN guard row (a whole batch entry) past B; everything the
    calls write NaN-filled before them, the workspace included; the cotangent NaN at the padded positions."""
    c = case(B, T, I, nd)
    cat = lambda names: torch.cat([c[n] for n in names], 0).to(dev)
    pn = param_names(nd)
    w_ih, w_hh = cat(pn[0::4]), cat(pn[1::4])
    bias = torch.cat([c[pn[4 * d + 2]] + c[pn[4 * d + 3]] for d in range(nd)], 0).to(dev)
    dy = c["dy"].clone()
    dy[padding_mask(B, T, lens)] = float("nan")
    x, dy = c["x"].detach().to(dev), dy.to(dev)
    h0, c0 = (c[k].detach().expand(nd, B, H).contiguous().to(dev) for k in ("h0", "c0"))
    ln = torch.tensor(lens, dtype=torch.int32, device=dev)
    nan = lambda *s: torch.full(s, float("nan"), device=dev)
    out, csave, gates, dgates = nan(B + 1, T, nd * H), nan(B + 1, T, nd * H), nan((B + 1) * T, nd * 4 * H), nan((B + 1) * T, nd * 4 * H)
    dx, dh0, dc0 = nan(B + 1, T, I), nan(nd, B, H), nan(nd, B, H)
    dw_ih, dw_hh, db = nan(nd * 4 * H, I), nan(nd * 4 * H, H), nan(nd * 4 * H)
    p, st = F_._p, F_._stream
    _lib.call("gcgcn_lstm_fwd_len", B, T, I, H, nd, p(x), p(w_ih), p(w_hh), p(bias), p(h0), p(c0), p(out), p(gates), p(csave), p(ln), st())
    ws = torch.full((_lib.lib().gcgcn_lstm_ws_bytes(B, T, I, H, nd) // 4,), float("nan"), device=dev)
    _lib.call("gcgcn_lstm_bwd_len", B, T, I, H, nd, p(x), p(w_ih), p(w_hh), p(h0), p(c0), p(out), p(gates), p(csave), p(dy), p(dgates), p(dx),
              p(dw_ih), p(dw_hh), p(db), p(dh0), p(dc0), p(ws), ws.numel() * 4, p(ln), st())
    torch.cuda.synchronize()
    return dict(out=out, csave=csave, gates=gates, dgates=dgates, dx=dx, dh0=dh0, dc0=dc0, dw_ih=dw_ih, dw_hh=dw_hh, db=db, ws=ws)


def test_c_abi_on_poisoned_buffers(gpu_device):
    """What the contract says is written comes out finite and right, the padding is zero, the guard row stays untouched; the saved
    gates and cell states are written at the active steps (and nothing is asked of them elsewhere)."""
    B, T, I, lens, nd = CASES[3]                                           # (17, 3, 140): the second tile holds one row of length 1
    bufs = _raw_call(gpu_device, B, T, I, nd, lens)
    pad = padding_mask(B, T, lens).to(gpu_device)
    for k in ("out", "dx"):
        assert torch.isfinite(bufs[k][:B]).all(), k
        assert not bufs[k][:B][pad].any(), f"{k}: not zero at the padding"
        assert torch.isnan(bufs[k][B:]).all(), f"{k}: the guard row was written"
    dg = bufs["dgates"][:B * T].view(B, T, -1)
    assert torch.isfinite(dg).all() and not dg[pad].any() and torch.isnan(bufs["dgates"][B * T:]).all()
    assert torch.isfinite(bufs["csave"][:B][~pad]).all() and torch.isfinite(bufs["gates"][:B * T].view(B, T, -1)[~pad]).all()
    assert torch.isnan(bufs["csave"][B:]).all() and torch.isnan(bufs["gates"][B * T:]).all()
    for k in ("dh0", "dc0", "dw_ih", "dw_hh", "db"):
        assert torch.isfinite(bufs[k]).all(), f"{k} holds NaN"
    assert torch.isfinite(bufs["ws"][:B * T * nd * H]).all(), "H_prev was left unwritten somewhere"
    ref = reference(B, T, I, lens, nd)
    assert frac_of_bound(bufs["out"][:B], ref["out"]) <= 1.0 and frac_of_bound(bufs["dx"][:B], ref["dx"]) <= 1.0
    assert frac_of_bound(bufs["dw_hh"][:4 * H], ref["dweight_hh_l0"]) <= 1.0
    assert frac_of_bound(bufs["dw_hh"][4 * H:], ref["dweight_hh_l0_reverse"]) <= 1.0
    assert frac_of_bound(bufs["dh0"].sum(1, keepdim=True), ref["dh0"]) <= 1.0


@pytest.mark.parametrize("B,T,I,nd", [(16, 4, 140, 2), (33, 37, 140, 2), (17, 5, 140, 1)])
def test_lengths_all_T_equal_no_lengths_bitwise(gpu_device, B, T, I, nd):
    c = case(B, T, I, nd)
    a, b = run_hip(c, nd, gpu_device, None), run_hip(c, nd, gpu_device, (T,) * B)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_two_runs_are_bitwise_equal(gpu_device):
    B, T, I, lens, nd = CASES[5]
    c = case(B, T, I, nd)
    a, b = run_hip(c, nd, gpu_device, lens), run_hip(c, nd, gpu_device, lens)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_graph_replay_on_new_input_and_new_lengths_equals_eager(gpu_device):
    """Forward + backward of lstm_layer(lengths=) captured in a hipGraph and replayed on NEW contents of x, the parameters, the
    cotangent AND the lengths tensor, against the eager call, bit for bit; and it is the new contents' result."""
    B, T, I = 17, 5, 140
    lens0, lens1 = tuple((3 * i) % 5 + 1 for i in range(B)), tuple((2 * i + 1) % 5 + 1 for i in range(B))
    c0_, c1_ = case(B, T, I, seed=1), case(B, T, I, seed=2)
    t, dy = _leaves(c0_, gpu_device)
    ln = torch.tensor(lens0, dtype=torch.int64, device=gpu_device)          # int64: the conversion is part of the capture
    names = list(t)

    def step():
        out = _layer(t, 2, ln)
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
        ln.copy_(torch.tensor(lens1))
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    for name, g, e in zip(["out"] + names, held, eager):
        assert torch.equal(g, e), name
    ref = reference(B, T, I, lens1, seed=2)
    assert frac_of_bound(held[0], ref["out"]) <= 1.0 and frac_of_bound(held[1 + names.index("x")], ref["dx"]) <= 1.0


def test_lengths_are_validated(gpu_device):
    dev = gpu_device
    c = case(3, 5, 7)
    t, _ = _leaves(c, dev)
    for bad in ([5, 0, 3], [5, 6, 3]):
        with pytest.raises(IndexError, match=r"lengths must lie in \[1, 5\]"):
            _layer(t, 2, torch.tensor(bad, device=dev))
    with pytest.raises(ValueError, match="lengths must be"):
        _layer(t, 2, torch.tensor([5, 1], device=dev))
    with pytest.raises(ValueError, match="lengths must be"):
        _layer(t, 2, torch.tensor([5.0, 1.0, 3.0], device=dev))
    with pytest.raises(ValueError, match="lengths must be"):
        _layer(t, 2, [5, 1, 3])
    torch.cuda.synchronize()


# ---- the models -----------------------------------------------------------------------------------------------------------------
EXTRA = 13
TOKEN_LAST = ("document", "document_ner", "document_pos", "sen_matrix", "pos_matrix_h", "pos_matrix_t", "node_pos")


def _pad_tokens(d, n):
    """The document with n more token positions that belong to no sentence and no mention: zeros in every tensor whose last axis is T."""
    return {k: F.pad(v, (0, n)) if k in TOKEN_LAST else v for k, v in d.items()}


def _mixed_batch(g, dev):
    """doc0 with 13 more (non-zero) words at its end, doc1 zero-padded to the same 53 tokens; t_valid = [53, 40]."""
    d0, d1 = (doc_tensors(g["raw"], di, dev) for di in range(2))
    T0 = d0["document"].shape[0]
    assert T0 == d1["document"].shape[0] == 40
    long0 = _pad_tokens(d0, EXTRA)
    long0["document"][T0:] = torch.arange(1, EXTRA + 1, device=dev) % (g["meta"]["vocab"] - 1) + 1
    assert bool((long0["document"][T0:] > 0).all())
    pad1 = _pad_tokens(d1, EXTRA)
    batch = {k: torch.stack([long0[k], pad1[k]]) for k in long0}
    return long0, d1, batch, torch.tensor([T0 + EXTRA, T0], dtype=torch.int32, device=dev)


@pytest.mark.parametrize("encoder_impl,frontend_impl", [("torch", None), ("hip", None), ("hip", "hip")])
def test_model_batch_of_mixed_lengths_is_the_per_document_model(gpu_device, encoder_impl, frontend_impl):
    g, sd, model = load_model(gpu_device, encoder_impl)
    if frontend_impl is not None:
        cfg = Cfg(g["meta"]["vocab"], encoder_impl)
        cfg.frontend_impl = frontend_impl
        model = M.GCGCN_glove(cfg).to(gpu_device).eval()
        model.load_state_dict(sd, strict=True)
    assert model.rnn.impl == encoder_impl and model.frontend_impl == (frontend_impl or "torch")
    long0, d1, batch, t_valid = _mixed_batch(g, gpu_device)
    want1 = torch.from_numpy(g["raw"]["doc1.logits"])
    with torch.no_grad():
        got = model(**batch, t_valid=t_valid)
        alone0 = model(**long0)
        blind = model(**batch)
    torch.testing.assert_close(got[1].cpu(), want1, rtol=1e-4, atol=1e-4)        # the tolerance of tests/test_model_gpu.py for this golden
    torch.testing.assert_close(got[0], alone0, rtol=1e-4, atol=1e-4)
    err = (blind[1].cpu() - want1).abs()
    print(f"{encoder_impl}/{frontend_impl}: without t_valid row 1 is off by up to {err.max().item():.3e}")
    assert bool((err > 1e-4 + 1e-4 * want1.abs()).any()), "the batch without t_valid is inside the tolerance: the test sees nothing"


@pytest.mark.parametrize("encoder_impl", ["torch", "hip"])
def test_model_encoder_gradients_of_a_mixed_batch_are_the_per_document_sum(gpu_device, encoder_impl):
    g, sd, model = load_model(gpu_device, encoder_impl)
    model.rnn.train()                # MIOpen's LSTM backward wants training mode; keep_prob = 1, so the encoder's dropout is the identity
    long0, d1, batch, t_valid = _mixed_batch(g, gpu_device)
    labels = [torch.from_numpy(g["raw"][f"doc{di}.labels"]).float().to(gpu_device) for di in range(2)]
    enc = dict(model.rnn.named_parameters())

    def grads(loss):
        model.zero_grad()
        loss.backward()
        return {k: p.grad.clone() for k, p in enc.items()}

    both = grads(gcgcn_amd.pair_bce_loss(model(**batch, t_valid=t_valid), torch.stack(labels)).sum())
    one = [grads(gcgcn_amd.pair_bce_loss(model(**d), lb)) for d, lb in zip((long0, d1), labels)]
    fr = {k: frac_of_bound(both[k], one[0][k] + one[1][k]) for k in both}
    print(f"{encoder_impl}: encoder gradients, batch against the per-document sum: " + " ".join(f"{k}={v:.3f}" for k, v in fr.items()))
    assert max(fr.values()) <= 1.0, fr


class _StubBert(torch.nn.Module):
    """Stands in for pytorch_pretrained_bert.BertModel (third-party): ``bert(document, token_type_ids=None, attention_mask=None,
    output_all_encoded_layers=True) -> (states [B,T,768], pooled)``.  Records the keywords of every call."""

    def __init__(self, vocab):
        super().__init__()
        self.emb = torch.nn.Embedding(vocab, 768)
        self.seen = []

    def forward(self, document, token_type_ids=None, **kw):
        assert set(kw) <= {"attention_mask", "output_all_encoded_layers"}, kw
        self.seen.append(dict(kw))
        h = torch.tanh(self.emb(document))
        return h, h[:, 0]


def test_bert_model_hands_the_mask_to_its_encoder(gpu_device):
    g, _, _ = load_model(gpu_device)
    long0, d1, batch, t_valid = _mixed_batch(g, gpu_device)
    stub = _StubBert(g["meta"]["vocab"])
    model = M.GraphCNN_multihead_bert_gate_cls(Cfg(g["meta"]["vocab"]), bert=stub).to(gpu_device).eval()
    with torch.no_grad():
        a = model(**batch, t_valid=t_valid)
        b = model(**batch)
    assert a.shape == b.shape and torch.isfinite(a).all()
    with_mask, without = stub.seen
    assert set(with_mask) == {"attention_mask", "output_all_encoded_layers"} and with_mask["output_all_encoded_layers"] is False
    T = batch["document"].shape[1]
    want = torch.arange(T, device=gpu_device)[None, :] < t_valid[:, None]
    mask = with_mask["attention_mask"]
    assert mask.shape == (2, T) and mask.device == want.device and torch.equal(mask.bool(), want)
    assert int(mask[0].sum()) == 53 and int(mask[1].sum()) == 40
    assert without == {"output_all_encoded_layers": False}                 # without t_valid: exactly the call it has always made
