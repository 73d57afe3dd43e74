"""The BERT graph model's folded front end and [CLS] logit tail on the GPU (csrc/bert_frontend.hip through
functional.bert_token_context / pair_logit_bias and config.bert_frontend).  Cases, reference and bound: tests/bert_frontend_cases.py
(the definition in float64; lstm_cases.frac_of_bound, |got - ref| <= 1e-5 * max(1, max|ref|) + 1e-4 * |ref| on every element)."""
import functools

import pytest
import torch

import gcgcn_amd
from gcgcn_amd import functional as Fn, models as M
from gcgcn_amd.bert import BertConfig
import bert_frontend_cases as C
from lstm_cases import Cfg, doc_tensors, frac_of_bound, worst

pytestmark = pytest.mark.gpu
LEAVES = ("states", "coref_w", "ner_w", "W", "b")
GRADS = ("dstates", "dcoref_w", "dner_w", "dweight", "dbias")
ORDER = ("document", "document_ner", "document_pos", "adj_matrix", "sen_matrix", "pos_matrix_h", "pos_matrix_t", "node_pos", "node_type",
         "node_relative_pos")


def _dev(d, dev):
    return {k: None if v is None else v.to(dev) for k, v in d.items()}


def _step(t):
    """Forward + backward through the HIP function on the device tensors `t` (leaves require grad): the seven outputs in OUTPUTS' terms."""
    ctx, node_feat = Fn.bert_token_context(t["states"], t["document_pos"], t["document_ner"], t["coref_w"], t["ner_w"], t["W"], t["b"],
                                           t["node_pos"])
    grads = torch.autograd.grad([ctx, node_feat], [t[k] for k in LEAVES], [t["dctx"], t["dnode"]])
    res = {"ctx": ctx.detach(), "node_feat": node_feat.detach()}
    res.update(zip(GRADS, grads))
    return res


def _leaves(t):
    return {k: (v.detach().clone().requires_grad_() if k in LEAVES else v) for k, v in t.items()}


@functools.lru_cache(maxsize=None)
def _hip(c):
    return _step(_leaves(_dev(C.inputs(c), torch.device("cuda"))))


@pytest.mark.parametrize("case", C.SWEEP, ids=lambda c: c.label)
def test_context_pair_against_float64(gpu_device, case):
    got, ref = _hip(case), C.reference(case)
    fr = worst({k: got[k] for k in C.OUTPUTS}, ref, f"hip {case.label}")
    assert max(fr.values()) <= 1.0, fr
    assert not got["dcoref_w"][0].any() and not got["dner_w"][0].any()             # the padding rows: written, and exactly zero
    d = C.inputs(case)
    untouched = torch.ones(case.P, dtype=torch.bool)
    untouched[d["document_pos"].view(-1)] = False
    assert not got["dcoref_w"][untouched.to(gpu_device)].any()                      # rows nobody refers to as well


def test_no_padding_index_keeps_the_row(gpu_device):
    """padding index None: row 0 of both table gradients is what autograd gives without one."""
    case = C.SWEEP[2]
    t = _leaves(_dev(C.inputs(case), gpu_device))
    ctx, node_feat = Fn.bert_token_context(t["states"], t["document_pos"], t["document_ner"], t["coref_w"], t["ner_w"], t["W"], t["b"],
                                           t["node_pos"], coref_padding_idx=None, ner_padding_idx=None)
    dcoref, dner = torch.autograd.grad([ctx, node_feat], [t["coref_w"], t["ner_w"]], [t["dctx"], t["dnode"]])
    want = C.run_folded(case, C.inputs(case), torch.float64, coref_pad=None, ner_pad=None)
    assert want["dcoref_w"][0].abs().max() > 0 and want["dner_w"][0].abs().max() > 0
    assert frac_of_bound(dcoref, want["dcoref_w"]) <= 1.0 and frac_of_bound(dner, want["dner_w"]) <= 1.0
    rest = _hip(case)
    assert torch.equal(dcoref[1:], rest["dcoref_w"][1:]) and torch.equal(dner[1:], rest["dner_w"][1:])


@pytest.mark.parametrize("case", C.DETERMINISM, ids=lambda c: c.label)
def test_context_pair_two_runs_are_bitwise_equal(gpu_device, case):
    t = _leaves(_dev(C.inputs(case), gpu_device))
    a, b = _step(t), _step(t)
    for k in C.OUTPUTS:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], _hip(case)[k]), k


def test_no_grad_saves_nothing_and_equals_the_training_forward(gpu_device):
    case = C.SWEEP[3]
    t = _dev(C.inputs(case), gpu_device)
    with torch.no_grad():
        ctx, node_feat = Fn.bert_token_context(t["states"], t["document_pos"], t["document_ner"], t["coref_w"], t["ner_w"], t["W"], t["b"],
                                               t["node_pos"])
    assert ctx.grad_fn is None and node_feat.grad_fn is None
    assert torch.equal(ctx, _hip(case)["ctx"]) and torch.equal(node_feat, _hip(case)["node_feat"])


# ---- the [CLS] logit tail ----------------------------------------------------------------------------------------------------
def _tail_step(t):
    out = Fn.pair_logit_bias(t["logits"], t["cls"], t["n_valid"])
    dlogits, dcls = torch.autograd.grad(out, [t["logits"], t["cls"]], t["dout"])
    return out.detach(), dlogits, dcls


@pytest.mark.parametrize("case", C.TAIL_CASES, ids=lambda c: "B{}-N{}-R{}-{}".format(*c))
def test_tail_forward_is_the_models_expression_and_dcls_is_within_the_bound(gpu_device, case):
    t = _dev(C.tail_inputs(*case), gpu_device)
    t["logits"], t["cls"] = t["logits"].clone().requires_grad_(), t["cls"].clone().requires_grad_()
    out, dlogits, dcls = _tail_step(t)
    assert torch.equal(out, C.tail_expression(t["logits"].detach(), t["cls"].detach(), t["n_valid"]))
    assert dlogits.data_ptr() == t["dout"].data_ptr()                               # the incoming gradient itself: no copy
    ref = C.tail_reference(*case)
    fr = worst({"out": out, "dcls": dcls}, {"out": ref["out"], "dcls": ref["dcls"]}, "tail B{}-N{}-R{}-{}".format(*case))
    assert max(fr.values()) <= 1.0, fr
    out2, _, dcls2 = _tail_step(t)                                                   # two runs: bitwise
    assert torch.equal(out, out2) and torch.equal(dcls, dcls2)
    if case[3] == "mixed":                                                           # a document without entities gets exact zeros
        assert not dcls[0].any() and torch.equal(out[0], t["logits"][0].detach())
    with torch.no_grad():                                                            # the unaligned start takes the scalar path
        flat = torch.empty(t["logits"].numel() + 1, device=gpu_device)
        view = flat[1:].view_as(t["logits"]).copy_(t["logits"])
        assert torch.equal(Fn.pair_logit_bias(view, t["cls"], t["n_valid"]), out)


# ---- hipGraph ------------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager(gpu_device):
    """Forward + backward of both functions captured in a hipGraph and replayed twice, on the captured contents and on NEW ones (ids
    and n_valid included), against the eager step on the same contents, bit for bit."""
    case, tail = C.GRAPH_CASE, (3, 5, 97, "mixed")
    first = {**_dev(C.inputs(case, seed=1), gpu_device), **_dev(C.tail_inputs(*tail, seed=1), gpu_device)}
    second = {**_dev(C.inputs(case, seed=2), gpu_device), **_dev(C.tail_inputs(*tail, seed=2), gpu_device)}
    second["n_valid"] = second["n_valid"].flip(0).contiguous()
    t = {k: v.clone() for k, v in first.items()}
    for k in LEAVES + ("logits", "cls"):
        t[k].requires_grad_()

    def step():
        r = _step(t)
        return tuple(r[k] for k in C.OUTPUTS) + _tail_step(t)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        held = step()
    names = C.OUTPUTS + ("out", "dlogits", "dcls")
    for contents, seed in ((first, 1), (second, 2)):
        with torch.no_grad():
            for k, v in contents.items():
                t[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [h.clone() for h in held]
        eager = step()
        for name, g, e in zip(names, replayed, eager):
            assert torch.equal(g, e), (name, seed)
        ref = C.reference(case, seed=seed)
        fr = worst(dict(zip(C.OUTPUTS, replayed)), ref, f"replayed, seed {seed}")
        assert max(fr.values()) <= 1.0, fr                                        # ... and it is those contents' result


# ---- the model switch ----------------------------------------------------------------------------------------------------------
class _StubBert(torch.nn.Module):
    """Stands in for pytorch_pretrained_bert.BertModel, as in tests/test_frontend_gpu.py: ``(states[B,T,768], pooled[B,768])``."""

    def __init__(self, vocab):
        super().__init__()
        self.emb = torch.nn.Embedding(vocab, 768)
        self.mix = torch.nn.Linear(768, 768)

    def forward(self, document, output_all_encoded_layers=True):
        h = torch.tanh(self.mix(self.emb(document)))
        return h, h[:, 0]


def _fixture(dev):
    from conftest import golden_files, load_golden
    g = load_golden(golden_files("model_step")[0])
    docs = [doc_tensors(g["raw"], di, dev) for di in range(g["meta"]["docs"])]
    labels = [torch.from_numpy(g["raw"][f"doc{di}.labels"]).to(dev).float() for di in range(len(docs))]
    return g["meta"]["vocab"], docs, labels


def _ragged(docs, labels, dev):
    """A batch of three documents (the fixture's two and the first again) with entity counts below the padded N."""
    pick = (0, 1, 0)
    batch = {k: torch.stack([docs[i][k] for i in pick]) for k in ORDER}
    N = batch["node_type"].shape[1]
    return batch, torch.stack([labels[i] for i in pick]), torch.tensor([N, N - 3, 4], device=dev)


def test_model_folded_agrees_with_cat(gpu_device):
    """A stub encoder, frontend_impl = "hip" on both sides: logits and every parameter gradient under bert_frontend = "folded" agree
    with "cat" within the bound -- the one-document call, and a ragged batch with n_valid."""
    dev = gpu_device
    vocab, docs, labels = _fixture(dev)
    torch.manual_seed(5)
    cfg = Cfg(vocab)
    cfg.frontend_impl = "hip"
    base = M.GraphCNN_multihead_bert_gate_cls(cfg, bert=_StubBert(vocab)).to(dev).eval()
    cfg = Cfg(vocab)
    cfg.frontend_impl, cfg.bert_frontend = "hip", "folded"
    twin = M.GraphCNN_multihead_bert_gate_cls(cfg, bert=_StubBert(vocab)).to(dev).eval()
    assert base.bert_frontend == "cat" and twin.bert_frontend == "folded"
    with torch.no_grad():
        for n, p in base.named_parameters():
            if n.endswith("attention_all.bias"):
                p.fill_(0.4)
            if n == "linear_cls.bias":
                p.normal_()
    res = twin.load_state_dict(base.state_dict(), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    batch, blabels, nv = _ragged(docs, labels, dev)
    for label, args, kw, lab in (("one document", [docs[0][k] for k in ORDER], {}, labels[0][None]),
                                 ("ragged batch", [batch[k] for k in ORDER], {"n_valid": nv}, blabels)):
        got = {}
        for name, model in (("cat", base), ("folded", twin)):
            model.zero_grad(set_to_none=True)
            logits = model(*args, **kw)
            lg = logits if logits.dim() == 4 else logits[None]
            gcgcn_amd.pair_bce_loss(lg, lab, n_valid=kw.get("n_valid")).sum().backward()
            got[name] = {"logits": logits.detach()}
            got[name].update({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
        assert got["cat"].keys() == got["folded"].keys() and {"linear_re.weight", "entity_embed.weight", "ner_emb.weight",
                                                              "linear_cls.bias", "bert.emb.weight"} <= set(got["cat"])
        fr = worst(got["folded"], got["cat"], f"bert model, folded vs cat, {label}")
        assert max(fr.values()) <= 1.0, fr
        assert not got["folded"]["entity_embed.weight"][0].any() and not got["folded"]["ner_emb.weight"][0].any()


def test_model_folded_train_step_repeats_bitwise(gpu_device):
    """This library's own encoder (impl "hip", fused embeddings), the folded front end, config.deterministic, train mode: two steps from
    one seed give every parameter gradient to the last bit -- the one-document call, and a ragged batch of three with n_valid."""
    dev = gpu_device
    vocab, docs, labels = _fixture(dev)
    cfg = Cfg(vocab)
    cfg.frontend_impl, cfg.bert_frontend, cfg.deterministic = "hip", "folded", True
    cfg.bert_impl, cfg.bert_embeddings = "hip", "fused"
    cfg.bert_config = BertConfig(vocab_size=vocab, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=128,
                                 max_position_embeddings=64)
    torch.manual_seed(9)
    model = M.GraphCNN_multihead_bert_gate_cls(cfg).to(dev).train()
    assert model.bert_frontend == "folded" and model.deterministic is True and model.linear_re.weight.shape[1] == 64 + 20 + 20
    batch, blabels, nv = _ragged(docs, labels, dev)
    T = batch["document"].shape[1]
    tv = torch.tensor([T, T - 7, T - 1], device=dev)
    for label, args, kw, lab in (("one document", [docs[0][k] for k in ORDER], {}, labels[0][None]),
                                 ("ragged batch", [batch[k] for k in ORDER], {"n_valid": nv, "t_valid": tv}, blabels)):
        runs = []
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            torch.manual_seed(12)
            gcgcn_amd.manual_seed(13)
            logits = model(*args, **kw)
            lg = logits if logits.dim() == 4 else logits[None]
            loss = gcgcn_amd.pair_bce_loss(lg, lab, n_valid=kw.get("n_valid")).sum()
            loss.backward()
            grads = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
            grads["logits"], grads["loss"] = logits.detach(), loss.detach()
            runs.append(grads)
        a, b = runs
        assert a.keys() == b.keys() and len(a) > 10 and all(torch.isfinite(v).all() for v in a.values()), label
        assert {"linear_re.weight", "entity_embed.weight", "ner_emb.weight", "linear_cls.weight"} <= set(a)
        bad = [k for k in a if not torch.equal(a[k], b[k])]
        assert not bad, f"{label}: gradients that differ between two runs: " + ", ".join(
            f"{k} ({(a[k] - b[k]).abs().max().item():.3e})" for k in bad)
