"""The fused embeddings stage of the HIP BERT encoder on the device (csrc/bert_embed.hip; functional.bert_embeddings;
BertModel(embeddings="fused")): against float64 with the device's mask replayed, bit for bit against the unfused HIP path, the exact
zeros of the contract, determinism and graph capture, the model-level wiring, the host wrapper's refusals.  Cases, runner and
reference: tests/bert_embed_cases.py; the bound is tests/bert_cases.py's, nothing new."""
import numpy as np
import pytest
import torch

import gcgcn_amd
from gcgcn_amd import functional as Fn, models as M
from gcgcn_amd.bert import BertModel

import bert_cases as BC
import bert_embed_cases as C

pytestmark = pytest.mark.gpu


def _pad(inp, T):
    return None if inp["lengths"] is None else torch.arange(T)[None, :] >= inp["lengths"][:, None]


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_against_float64(gpu_device, case):
    """y and the five gradients within the BERT bound of impl="torch" in float64 on the CPU, in train mode (where the case has p > 0,
    the device's mask replayed) and in eval mode."""
    D, B, T, extra, tt_kind, len_kind, p = case
    inp = C.inputs(D, B, T, tt_kind, len_kind)
    model = C.build(D, T + extra, p, device=gpu_device, impl="hip", embeddings="fused")
    for train in ((True, False) if p > 0 else (False,)):
        gcgcn_amd.manual_seed(17)
        got = C.run_stage(model, inp, train=train)
        override = None
        if train:
            assert model.last_rng_snaps is not None and len(model.last_rng_snaps) == 1
            override = C.replay(model.last_rng_snaps[0], p)
        ref = C.reference(case, override=override, train=train)
        for k, t in got.items():
            assert torch.isfinite(t).all(), k
        fr = BC.worst(got, ref, f"bert_embeddings {C.case_id(case)} train={train}")
        assert max(fr.values()) <= 1.0, fr
    if p > 0:
        assert not torch.equal(got["y"], C.run_stage(model, inp, train=True, backward=False)["y"])     # masks were drawn at all


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_forward_equals_the_unfused_hip_path_bit_for_bit(gpu_device, case):
    """Same process, parameters and rng snapshot, eval and train mode: the sum is the same two fp32 adds and the LayerNorm row body is
    shared, so the bits agree.  The gradients (another summation order for the tables) agree within the bound."""
    D, B, T, extra, tt_kind, len_kind, p = case
    inp = C.inputs(D, B, T, tt_kind, len_kind)
    res = {}
    for emb in ("fused", "torch"):
        model = C.build(D, T + extra, p, device=gpu_device, impl="hip", embeddings=emb)
        for train in (False, True):
            gcgcn_amd.manual_seed(23)
            res[emb, train] = C.run_stage(model, inp, train=train)
    for train in (False, True):
        assert torch.equal(res["fused", train]["y"], res["torch", train]["y"]), train
        fr = BC.worst(res["fused", train], res["torch", train], f"fused vs unfused {C.case_id(case)} train={train}")
        assert max(fr.values()) <= 1.0, fr
    if p > 0:
        assert not torch.equal(res["fused", True]["y"], res["fused", False]["y"])


@pytest.mark.parametrize("case", [c for c in C.CASES if c[5] == "ragged"], ids=C.case_id)
def test_exact_zeros(gpu_device, case):
    D, B, T, extra, tt_kind, len_kind, p = case
    inp = C.inputs(D, B, T, tt_kind, len_kind)
    model = C.build(D, T + extra, p, device=gpu_device, impl="hip", embeddings="fused")
    gcgcn_amd.manual_seed(3)
    got = {k: v.cpu() for k, v in C.run_stage(model, inp, train=p > 0).items()}
    pad = _pad(inp, T)
    assert pad.any() and (got["y"][pad] == 0).all() and (got["y"][~pad] != 0).any()
    live_ids = set(inp["ids"][~pad].tolist())
    dead = [v for v in range(C.V) if v not in live_ids]
    assert set(C.NEVER_LIVE) <= set(dead) and set(inp["ids"][pad].tolist()) <= set(C.NEVER_LIVE)     # they sit on padding only
    assert (got["dW"][dead] == 0).all() and all((got["dW"][v] != 0).any() for v in live_ids)
    longest = int(inp["lengths"].max())
    assert longest == T and (got["dP"][T:] == 0).all() and got["dP"].shape[0] == T + extra
    # no document reaches past `cut`: the position rows from there on are zero too
    short = dict(inp, lengths=torch.clamp(inp["lengths"], max=max(1, T // 2)))
    cut = int(short["lengths"].max())
    g2 = C.run_stage(model, short, train=False)
    assert (g2["dP"][cut:] == 0).all() and (cut == 0 or (g2["dP"][:cut] != 0).any())
    # every document empty: nothing reaches any gradient, and nothing is NaN although the whole cotangent is
    empty = dict(inp, lengths=torch.zeros(B, dtype=torch.int64), dy=torch.full_like(inp["dy"], float("nan")))
    g0 = C.run_stage(model, empty, train=p > 0)
    for k, t in g0.items():
        assert (t == 0).all(), k


def test_two_backward_passes_are_bitwise_equal(gpu_device):
    case = C.CASES[-1]                                                     # (4, 128): two chunks of the word table's scheme
    D, B, T, extra, tt_kind, len_kind, p = case
    inp = C.inputs(D, B, T, tt_kind, len_kind)
    runs = []
    for _ in range(2):
        gcgcn_amd.manual_seed(31)
        model = C.build(D, T + extra, p, device=gpu_device, impl="hip", embeddings="fused")
        runs.append(C.run_stage(model, inp, train=True))
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_graph_replay_matches_eager_and_follows_new_ids_and_lengths(gpu_device):
    """A captured forward + backward (train mode, p = 0.1) replayed twice equals two eager steps from the same generator state, bit
    for bit; one more replay after new ids, token types and lengths were written into the static buffers equals the eager step on
    those inputs."""
    D, B, T, extra, p = 128, 3, 33, 3, 0.1
    a, b = C.inputs(D, B, T, "mixed", "ragged"), C.inputs(D, B, T, "mixed", "ragged", seed=1)
    b = dict(b, lengths=torch.tensor([5, T, 0]))
    model = C.build(D, T + extra, p, device=gpu_device, impl="hip", embeddings="fused").train()
    ids, tt = a["ids"].to(gpu_device), a["tt"].to(gpu_device)
    lens = a["lengths"].to(device=gpu_device, dtype=torch.int32)
    dy = torch.nan_to_num(a["dy"]).to(gpu_device)                           # one cotangent for both inputs: their padding differs
    out = {}

    def load(inp):
        ids.copy_(inp["ids"]), tt.copy_(inp["tt"]), lens.copy_(inp["lengths"])

    def step():
        model.zero_grad(set_to_none=True)
        y, _ = model(ids, tt, output_all_encoded_layers=False, lengths=lens)
        y.backward(dy)
        out["y"] = y

    def results():
        params = dict(model.named_parameters())
        r = {"y": out["y"]}
        r.update({k: params[n].grad for k, n in C.GRADS.items()})
        return r

    gcgcn_amd.manual_seed(9)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    torch.cuda.synchronize()
    live = results()
    rng = Fn._state(torch.device(gpu_device))
    start = rng.clone()
    replays = []
    for i in range(3):
        if i == 2:
            load(b)
        graph.replay()
        torch.cuda.synchronize()
        replays.append({k: v.detach().clone() for k, v in live.items()})
    rng.copy_(start)
    load(a)
    for i in range(3):
        if i == 2:
            load(b)
        step()
        torch.cuda.synchronize()
        for k, v in results().items():
            assert torch.equal(v, replays[i][k]), (i, k)
    assert not torch.equal(replays[0]["y"], replays[1]["y"])                # a fresh mask at every replay
    assert not torch.equal(replays[1]["dW"], replays[2]["dW"])              # the new ids were followed
    pad_b = torch.arange(T)[None, :] >= b["lengths"][:, None]
    assert (replays[2]["y"].cpu()[pad_b] == 0).all() and (replays[2]["y"].cpu()[~pad_b] != 0).any()


def test_two_layer_model_fused_against_unfused(gpu_device):
    """BertModel(impl="hip") with two layers: embeddings="fused" against "torch" -- every output bitwise equal in eval mode, every
    parameter gradient within the bound of the float64 reference (tests/bert_cases.py's, computed once there)."""
    D, H, B, T = 128, 2, 3, 33
    case = BC.model_case(D, H, B, T)
    res = {}
    for emb in ("torch", "fused"):
        model = BertModel(BC.config(D, H), impl="hip", embeddings=emb)
        model.load_state_dict(BC.state(D, H))
        res[emb] = BC.run_model(D, H, case, torch.float32, device=gpu_device, model=model.to(gpu_device))
    for k in ("out0", "out1", "pooled"):
        assert torch.equal(res["fused"][k], res["torch"][k]), k
    fr = BC.worst(res["fused"], BC.model_reference(D, H, B, T), "2-layer model, embeddings='fused'")
    assert max(fr.values()) <= 1.0, fr
    fr = BC.worst({k: v for k, v in res["fused"].items() if k.startswith("d")}, {k: v for k, v in res["torch"].items() if k.startswith("d")},
                  "2-layer model, fused vs unfused gradients")
    assert max(fr.values()) <= 1.0, fr


class _Cfg:
    entity_type_size, coref_size, max_length, keep_prob, graph_hop = 20, 20, 512, 1.0, 2
    dis_size, dis_num, dis_plus, relation_num, alpha = 20, 21, 10, 97, 1.0

    def __init__(self, vocab, **kw):
        self.data_word_vec = np.zeros((vocab, 100), np.float32)
        self.__dict__.update(kw)


def test_model_wiring_one_training_step_with_lengths(gpu_device):
    """GraphCNN_multihead_bert_gate_cls with config.bert_embeddings = "fused" against the same model without it: one state_dict, one
    seed, a ragged two-document batch with t_valid, train mode with dropout in the encoder; the logits are bitwise equal and the
    backward fills finite gradients, the word table's included."""
    from conftest import golden_files, load_golden
    from lstm_cases import doc_tensors
    g = load_golden(golden_files("model_step")[0])
    vocab = g["meta"]["vocab"]
    bc = BC.config(128, 2, p=0.1)
    bc.vocab_size = vocab
    torch.manual_seed(5)
    base = M.GraphCNN_multihead_bert_gate_cls(_Cfg(vocab, bert_impl="hip", bert_config=bc)).to(gpu_device).train()
    twin = M.GraphCNN_multihead_bert_gate_cls(_Cfg(vocab, bert_impl="hip", bert_config=bc, bert_embeddings="fused")).to(gpu_device).train()
    assert (base.bert.embeddings_impl, twin.bert.embeddings_impl) == ("torch", "fused")
    with torch.no_grad():
        sd = BC.state(128, 2)
        for n, q in base.bert.named_parameters():
            if "word_embeddings" not in n:
                q.copy_(sd[n])
            else:
                q.normal_(0, 0.5)
    assert not twin.load_state_dict(base.state_dict(), strict=True).missing_keys
    docs = [doc_tensors(g["raw"], di, gpu_device) for di in range(2)]
    batch = {k: torch.stack([d[k] for d in docs]) for k in docs[0]}
    T = batch["document"].shape[1]
    t_valid = torch.tensor([T, max(1, T - 13)], device=gpu_device)
    logits = {}
    for name, m in (("base", base), ("twin", twin)):
        gcgcn_amd.manual_seed(41), torch.manual_seed(41)
        logits[name] = m(**batch, t_valid=t_valid)
        logits[name].square().mean().backward()
    assert torch.isfinite(logits["twin"]).all() and torch.equal(logits["twin"], logits["base"])
    for (n, q), (_, r) in zip(twin.named_parameters(), base.named_parameters()):
        assert (q.grad is None) == (r.grad is None), n
        assert q.grad is None or torch.isfinite(q.grad).all(), n
    gw = twin.bert.embeddings.word_embeddings.weight.grad
    assert gw is not None and (gw != 0).any()


def test_host_wrapper_refusals(gpu_device):
    """An out-of-range id, T > Pmax and D = 96 raise in the host wrapper: no launch is made (the kernels never see such input)."""
    dev = gpu_device
    D, B, T = 64, 2, 5
    tabs = lambda d=D, pmax=8: (torch.zeros(C.V, d, device=dev), torch.zeros(pmax, d, device=dev), torch.zeros(C.TY, d, device=dev),
                                torch.ones(d, device=dev), torch.zeros(d, device=dev))
    ids, tt = torch.zeros(B, T, dtype=torch.int64, device=dev), torch.zeros(B, T, dtype=torch.int64, device=dev)
    assert Fn.bert_embeddings(ids, tt, *tabs()).shape == (B, T, D)          # the inputs below differ from a valid call in one thing
    assert Fn.bert_embeddings(ids, None, *tabs()).shape == (B, T, D)
    for bad_ids, bad_tt, who in ((ids + C.V, tt, "input_ids"), (ids - 1, tt, "input_ids"), (ids, tt + C.TY, "token_type_ids")):
        with pytest.raises(IndexError, match=who):
            Fn.bert_embeddings(bad_ids, bad_tt, *tabs())
    with pytest.raises(ValueError, match="exceed the position table"):
        Fn.bert_embeddings(ids, tt, *tabs(pmax=T - 1))
    with pytest.raises(ValueError, match="multiple of 64"):
        Fn.bert_embeddings(ids, tt, *tabs(d=96))
    with pytest.raises(ValueError, match="int64"):
        Fn.bert_embeddings(ids.int(), tt, *tabs())
    with pytest.raises(RuntimeError, match="MI355X only"):
        Fn.bert_embeddings(ids, tt, *(t.cpu() for t in tabs()))
