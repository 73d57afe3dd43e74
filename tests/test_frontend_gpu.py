"""The HIP token front end on the GPU (csrc/frontend.hip through functional.token_embed / token_context and config.frontend_impl).

The sweep (frontend_cases.SWEEP) is the smallest shapes at which each kernel can go wrong:
  (B,T) in {(1,1), (2,2), (3,37), (2,512)} at widths 100/20/20    the model's length, a T that is no multiple of a tile or a chunk
  widths (3,1,5) at (3,37)                                        unaligned parts
  V = 1, and all ids equal, at (2,512)                            one run of 1 024 tokens: four chunks of eight pieces each
  V = 1000 random at (2,512)                                      many duplicated ids
  all ids distinct, V = B T                                       singleton runs, the last table row
  V = 200 000 with 74 tokens                                      the table-sized passes, untouched rows exactly zero
  N in {1, 5, 42}, K in {256, 808}                                the pooling and the context pair
Bound: lstm_cases.frac_of_bound, |got - ref| <= 1e-5 * max(1, max|ref|) + 1e-4 * |ref| on every element, against float64."""
import functools

import pytest
import torch
import torch.nn.functional as F

import gcgcn_amd
from gcgcn_amd import _lib, models as M
from frontend_cases import DETERMINISM, HD, OUTPUTS, SWEEP, Case, inputs, reference
from lstm_cases import Cfg, doc_tensors, frac_of_bound, load_model, worst

pytestmark = pytest.mark.gpu
ORDER = ("document", "document_ner", "document_pos", "adj_matrix", "sen_matrix", "pos_matrix_h", "pos_matrix_t", "node_pos", "node_type",
         "node_relative_pos")
LEAVES = ("word_w", "coref_w", "ner_w", "W", "b")


def _dev(d, dev):
    return {k: None if v is None else v.to(dev) for k, v in d.items()}


def _run_hip(c: Case, t):
    """Forward + backward of the case through the two HIP functions on the device tensors `t`: {name: tensor} over OUTPUTS."""
    leaves = {k: t[k].detach().clone().requires_grad_() for k in LEAVES}
    x = gcgcn_amd.token_embed(t["document"], t["document_pos"], t["document_ner"], leaves["word_w"], leaves["coref_w"], leaves["ner_w"],
                              scale=t["scale"])
    h = x if c.K is None else t["h"].detach().clone().requires_grad_()
    ctx, node_feat = gcgcn_amd.token_context(h, leaves["W"], leaves["b"], t["node_pos"])
    outs, cots = [ctx, node_feat], [t["dctx"], t["dnode"]]
    if c.K is not None:
        outs.append(x), cots.append(t["dx"])
    grads = torch.autograd.grad(outs, [leaves[k] for k in LEAVES] + [h], cots)
    res = {"x": x.detach(), "ctx": ctx.detach(), "node_feat": node_feat.detach()}
    res.update(zip(("dword", "dcoref", "dner", "dW", "db", "dh"), grads))
    return res


@functools.lru_cache(maxsize=None)
def _hip(c: Case):
    return _run_hip(c, _dev(inputs(c), torch.device("cuda")))


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: c.label)
def test_embedding_forward_is_a_bitwise_copy(gpu_device, case):
    t = _dev(inputs(case), gpu_device)
    want = torch.cat([F.embedding(t["document"], t["word_w"]), F.embedding(t["document_pos"], t["coref_w"], padding_idx=0),
                      F.embedding(t["document_ner"], t["ner_w"], padding_idx=0)], dim=-1)
    ids = (t["document"], t["document_pos"], t["document_ner"])
    tabs = (t["word_w"], t["coref_w"], t["ner_w"])
    with torch.no_grad():
        got = gcgcn_amd.token_embed(*ids, *tabs)
        assert not got.requires_grad and torch.equal(got, want)
        g = torch.Generator().manual_seed(1)
        scale = (torch.empty(case.B, 1, want.shape[2]).bernoulli_(0.8, generator=g) / 0.8).to(gpu_device)
        assert torch.equal(gcgcn_amd.token_embed(*ids, *tabs, scale=scale), scale.expand_as(want) * want)


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: c.label)
def test_against_float64(gpu_device, case):
    got, ref = _hip(case), reference(case)
    fr = worst({k: got[k] for k in OUTPUTS}, ref, f"hip {case.label}")
    assert max(fr.values()) <= 1.0, fr
    # the padding rows of the two small tables are exactly zero; the word table has none: row 0 collects its tokens' gradient
    assert not got["dcoref"][0].any() and not got["dner"][0].any()
    if case.V == 1:
        assert got["dword"][0].abs().max() > 0
    untouched = torch.ones(case.V, dtype=torch.bool)
    untouched[inputs(case)["document"].view(-1)] = False
    assert not got["dword"][untouched.to(gpu_device)].any()                       # written, and exactly zero


@pytest.mark.parametrize("case", DETERMINISM, ids=lambda c: c.label)
def test_two_runs_are_bitwise_equal(gpu_device, case):
    t = _dev(inputs(case), gpu_device)
    a, b = _run_hip(case, t), _run_hip(case, t)
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["dword"], _hip(case)["dword"])


def test_no_grad_saves_nothing_and_equals_the_training_forward(gpu_device):
    case = SWEEP[2]
    t = _dev(inputs(case), gpu_device)
    with torch.no_grad():
        x = gcgcn_amd.token_embed(t["document"], t["document_pos"], t["document_ner"], t["word_w"], t["coref_w"], t["ner_w"], scale=t["scale"])
        ctx, node_feat = gcgcn_amd.token_context(x, t["W"], t["b"], t["node_pos"])
    assert x.grad_fn is None and ctx.grad_fn is None and node_feat.grad_fn is None
    got = _hip(case)
    assert torch.equal(x, got["x"]) and torch.equal(ctx, got["ctx"]) and torch.equal(node_feat, got["node_feat"])


def test_graph_replay_equals_eager(gpu_device):
    """Forward + backward of both functions captured in a hipGraph and replayed on NEW contents (ids included), against the eager
    call on those contents, bit for bit."""
    case = Case(3, 37, 50, N=5, scaled=True)
    first, second = _dev(inputs(case, seed=1), gpu_device), _dev(inputs(case, seed=2), gpu_device)
    t = {k: v.clone() for k, v in first.items()}
    for k in LEAVES:
        t[k].requires_grad_()

    def step():
        x = gcgcn_amd.token_embed(t["document"], t["document_pos"], t["document_ner"], t["word_w"], t["coref_w"], t["ner_w"], scale=t["scale"])
        ctx, node_feat = gcgcn_amd.token_context(x, t["W"], t["b"], t["node_pos"])
        return (x, ctx, node_feat) + torch.autograd.grad([ctx, node_feat], [t[k] for k in LEAVES], [t["dctx"], t["dnode"]])

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
        for k, v in second.items():
            t[k].copy_(v)
    graph.replay()
    torch.cuda.synchronize()
    eager = step()
    names = ("x", "ctx", "node_feat", "dword", "dcoref", "dner", "dW", "db")
    for name, g, e in zip(names, held, eager):
        assert torch.equal(g, e), name
    ref = reference(case, seed=2)
    fr = worst(dict(zip(names, held)), {k: ref[k] for k in names}, "replayed")
    assert max(fr.values()) <= 1.0, fr                                        # ... and it is the new contents' result


def _hip_twin(base, vocab, dev, encoder_impl, keep_prob=1.0):
    cfg = Cfg(vocab, encoder_impl)
    cfg.frontend_impl, cfg.keep_prob = "hip", keep_prob
    twin = M.GCGCN_glove(cfg).to(dev).eval()
    res = twin.load_state_dict(base.state_dict(), strict=True)                 # strict, one way ...
    assert not res.missing_keys and not res.unexpected_keys
    res = base.load_state_dict(twin.state_dict(), strict=True)                 # ... and the other
    assert not res.missing_keys and not res.unexpected_keys
    return twin


@pytest.mark.parametrize("encoder_impl", [None, "hip"], ids=["lstm-torch", "lstm-hip"])
def test_model_eval_logits(gpu_device, encoder_impl):
    g, _, base = load_model(gpu_device, encoder_impl)
    twin = _hip_twin(base, g["meta"]["vocab"], gpu_device, encoder_impl)
    assert twin.frontend_impl == "hip" and base.frontend_impl == "torch" and twin.rnn.impl == base.rnn.impl
    docs = [doc_tensors(g["raw"], di, gpu_device) for di in range(g["meta"]["docs"])]
    with torch.no_grad():
        for di, d in enumerate(docs):                                            # the reference's one-document call
            want, got = base(*[d[k] for k in ORDER]), twin(*[d[k] for k in ORDER])
            fr = frac_of_bound(got, want)
            print(f"doc {di}: logits at {fr:.3f} of the bound")
            assert got.shape == want.shape and fr <= 1.0
        batch = {k: torch.stack([d[k] for d in docs]) for k in ORDER}
        want, got = base(**batch), twin(**batch)
        fr = frac_of_bound(got, want)
        print(f"batch: logits at {fr:.3f} of the bound")
        assert fr <= 1.0


def test_model_train_mode_draws_the_same_mask(gpu_device):
    """keep_prob = 0.8, the same torch seed and library seed on both sides: the hip front end draws the locked-dropout mask with the
    same torch call at the same point, so encode's output and word_emb.weight.grad agree within the bound."""
    g, sd, _ = load_model(gpu_device)
    vocab = g["meta"]["vocab"]
    cfg = Cfg(vocab)
    cfg.keep_prob = 0.8
    base = M.GCGCN_glove(cfg).to(gpu_device)
    base.load_state_dict(sd, strict=True)
    twin = _hip_twin(base, vocab, gpu_device, None, keep_prob=0.8)
    docs = [doc_tensors(g["raw"], di, gpu_device) for di in range(g["meta"]["docs"])]
    batch = {k: torch.stack([d[k] for d in docs]) for k in ORDER}
    labels = torch.stack([torch.from_numpy(g["raw"][f"doc{di}.labels"]) for di in range(len(docs))]).to(gpu_device).float()
    res = {}
    for name, model in (("torch", base), ("hip", twin)):
        model.train()
        torch.manual_seed(11)
        with torch.no_grad():
            enc = model.encode(batch["document"], batch["document_ner"], batch["document_pos"])
        torch.manual_seed(12)
        gcgcn_amd.manual_seed(13)
        model.zero_grad(set_to_none=True)
        gcgcn_amd.pair_bce_loss(model(**batch), labels).sum().backward()
        res[name] = {"encode": enc, "word_emb.weight.grad": model.word_emb.weight.grad.clone(),
                     "entity_embed.weight.grad": model.entity_embed.weight.grad.clone()}
    torch.manual_seed(11)
    eval_enc = twin.eval().encode(batch["document"], batch["document_ner"], batch["document_pos"])
    assert not torch.equal(eval_enc, res["hip"]["encode"])                      # the mask was drawn at all
    fr = worst(res["hip"], res["torch"], "train mode, hip vs torch front end")
    assert max(fr.values()) <= 1.0, fr


class _StubBert(torch.nn.Module):
    """Stands in for pytorch_pretrained_bert.BertModel, as in tests/test_model_gpu.py: ``(states[B,T,768], pooled[B,768])``."""

    def __init__(self, vocab):
        super().__init__()
        self.emb = torch.nn.Embedding(vocab, 768)
        self.mix = torch.nn.Linear(768, 768)

    def forward(self, document, output_all_encoded_layers=True):
        h = torch.tanh(self.mix(self.emb(document)))
        return h, h[:, 0]


def test_bert_model_logits(gpu_device):
    from conftest import golden_files, load_golden
    g = load_golden(golden_files("model_step")[0])
    vocab = g["meta"]["vocab"]
    torch.manual_seed(5)
    base = M.GraphCNN_multihead_bert_gate_cls(Cfg(vocab), bert=_StubBert(vocab)).to(gpu_device).eval()
    cfg = Cfg(vocab)
    cfg.frontend_impl = "hip"
    twin = M.GraphCNN_multihead_bert_gate_cls(cfg, bert=_StubBert(vocab)).to(gpu_device).eval()
    with torch.no_grad():
        for n, p in base.named_parameters():
            if n.endswith("attention_all.bias"):
                p.fill_(0.4)
    assert not twin.load_state_dict(base.state_dict(), strict=True).missing_keys
    docs = [doc_tensors(g["raw"], di, gpu_device) for di in range(g["meta"]["docs"])]
    with torch.no_grad():
        d = docs[0]
        fr1 = frac_of_bound(twin(*[d[k] for k in ORDER]), base(*[d[k] for k in ORDER]))
        batch = {k: torch.stack([d[k] for d in docs]) for k in ORDER}
        frb = frac_of_bound(twin(**batch), base(**batch))
    print(f"bert model, hip vs torch front end: one document {fr1:.3f}, batch {frb:.3f} of the bound")
    assert fr1 <= 1.0 and frb <= 1.0


def test_refusals_launch_nothing(gpu_device):
    """Every refusal answers with its message and leaves the outputs as they were."""
    h = _lib.lib()
    B, T, N, K = 2, 8, 3, 16
    dims = (B, T, 30, 16, 7, 100, 20, 20)
    dev = gpu_device
    ids = [torch.zeros(B, T, dtype=torch.int64, device=dev) for _ in range(3)]
    tabs = [torch.ones(r, w, device=dev) for r, w in ((30, 100), (16, 20), (7, 20))]
    x = torch.full((B, T, 140), 7.0, device=dev)
    grads = [torch.full_like(w, 7.0) for w in tabs]
    ws = torch.empty(h.gcgcn_frontend_ws_bytes(*dims, K) // 4 + 8, device=dev)
    hh, w, b, npos = torch.ones(B, T, K, device=dev), torch.ones(HD, K, device=dev), torch.ones(HD, device=dev), torch.ones(B, N, T, device=dev)
    pre, ctx, nf = (torch.full(s, 7.0, device=dev) for s in ((B, T, HD), (B, T, HD), (B, N, HD)))
    dpre, dh, dw, db = (torch.full(s, 7.0, device=dev) for s in ((B, T, HD), (B, T, K), (HD, K), (HD,)))
    p = lambda t: t.data_ptr()
    S = None                                                                  # the null stream

    def refused(rc, word):
        assert rc != 0 and word in h.gcgcn_last_error(), h.gcgcn_last_error()

    eb = lambda ws_ptr, nbytes, dx=p(x): h.gcgcn_embed_bwd(*dims, *map(p, ids), dx, None, 0, 0, *map(p, grads), ws_ptr, nbytes, S)
    refused(eb(p(ws), 16), b"workspace")
    refused(eb(p(ws) + 4, ws.numel() * 4 - 4), b"aligned")
    refused(eb(None, ws.numel() * 4), b"null")
    refused(eb(p(ws), ws.numel() * 4, dx=None), b"null")
    refused(h.gcgcn_embed_fwd(*dims, *map(p, ids), *map(p, tabs), None, None, S), b"null")
    refused(h.gcgcn_embed_fwd(0, *dims[1:], *map(p, ids), *map(p, tabs), None, p(x), S), b"bad shape")
    refused(h.gcgcn_embed_fwd(*dims[:5], 0, 20, 20, *map(p, ids), *map(p, tabs), None, p(x), S), b"width")
    cf = lambda *a: h.gcgcn_context_fwd(*a, p(hh), p(w), p(b), p(npos), p(pre), p(ctx), p(nf), S)
    refused(cf(B, T, N, K, 64), b"not served")
    refused(cf(B, T, 0, K, HD), b"bad shape")
    refused(h.gcgcn_context_fwd(B, T, N, K, HD, p(hh), p(w), p(b), p(npos), p(pre), None, p(nf), S), b"null")
    refused(h.gcgcn_context_fwd(B, T, N, K, HD, p(hh), p(w), p(b), p(npos), p(pre) + 4, p(ctx), p(nf), S), b"aligned")
    cb = lambda hd, ws_ptr, nbytes: h.gcgcn_context_bwd(B, T, N, K, hd, p(hh), p(w), p(npos), p(ctx), p(pre), p(nf), p(dpre), p(dh), p(dw),
                                                        p(db), ws_ptr, nbytes, S)
    refused(cb(100, p(ws), ws.numel() * 4), b"not served")
    refused(cb(HD, p(ws), 16), b"workspace")
    refused(cb(HD, p(ws) + 4, ws.numel() * 4 - 4), b"aligned")
    refused(cb(HD, None, ws.numel() * 4), b"null")
    torch.cuda.synchronize()
    for t in [x, pre, ctx, nf, dpre, dh, dw, db] + grads:
        assert bool((t == 7.0).all())
    with pytest.raises(IndexError, match="document_ner"):                        # ids are checked on the Python side
        gcgcn_amd.token_embed(ids[0], ids[1], ids[2] + 7, *tabs)
    with pytest.raises(ValueError, match="int64"):
        gcgcn_amd.token_embed(ids[0].int(), ids[1], ids[2], *tabs)
