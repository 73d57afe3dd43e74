"""matmul="bf16" on the device: the HIP encoder with its twelve Linear products on the bf16 matrix cores (csrc/gemm_bf16.hip) against
the float64 CPU run of the definition, ``BertModel(impl="torch", matmul="bf16")``, under the bound of tests/bert_bf16_cases.py.
Shapes, masks, parameters and inputs are those of tests/test_bert_gpu.py and tests/test_bert_lengths_gpu.py; the suite runs on
NaN-poisoned free memory (conftest.py), so the saved state and the workspaces of every call start as NaN."""
import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib, functional as Fn, models as M
from gcgcn_amd.bert import BertModel

import bert_bf16_cases as C
from bert_cases import CONFIGS, MODEL_SWEEP, config, model_case, state
from bert_length_cases import NAN, layer_len_case, pad_mask, run_with_lengths

pytestmark = pytest.mark.gpu


def _layer_inputs(D, H, B, T, kind):
    case = model_case(D, H, B, T, kind)
    g = torch.Generator().manual_seed(B + T + D)
    x = torch.randn(B, T, D, generator=g)
    model = BertModel(config(D, H))
    model.load_state_dict(state(D, H))
    params = [t.detach() for t in model.encoder.layer[0].tensors()]
    kb = None if case["mask"] is None else (1.0 - case["mask"]) * -10000.0
    return case, x, params, kb


def _layer_hip(x, kb, params, dy, dev, **kw):
    x = x.to(dev).requires_grad_()
    ps = [t.to(dev).requires_grad_() for t in params]
    y = Fn.bert_layer(x, None if kb is None else kb.to(dev), *ps, matmul="bf16", **kw)
    y.backward(dy.to(dev))
    res = {"y": y.detach(), "dx": x.grad}
    res.update({f"d{i:02d}": t.grad for i, t in enumerate(ps)})
    return res


@pytest.mark.parametrize("kind", ["none", "prefix", "holes"])
@pytest.mark.parametrize("D,H,B,T", [(128, 2, 3, 33), (192, 3, 2, 130)])
def test_layer_against_float64_definition(gpu_device, D, H, B, T, kind):
    """functional.bert_layer(matmul="bf16"): the output and all 17 gradients.  (3, 33): 99 rows, every tile guarded; (2, 130): 260 rows,
    interior tiles and a guarded edge; the weight gradients (K = 99 / 260) through the guarded k tail."""
    case, x, params, kb = _layer_inputs(D, H, B, T, kind)
    ref = C.layer_torch(x, kb, params, H, case["dy"])
    got = _layer_hip(x, kb, params, case["dy"], gpu_device)
    fr = C.worst(got, ref, f"layer bf16 D={D} H={H} ({B},{T}) {kind}")
    assert max(fr.values()) <= 1.0, fr


def test_layer_really_takes_the_bf16_products(gpu_device):
    """The bf16 layer's output differs from the fp32 layer's by more than the fp32 tests' bound allows: the selector is not ignored."""
    D, H, B, T = 128, 2, 3, 33
    case, x, params, kb = _layer_inputs(D, H, B, T, "prefix")
    bf = _layer_hip(x, kb, params, case["dy"], gpu_device)["y"]
    ps = [t.to(gpu_device) for t in params]
    fp = Fn.bert_layer(x.to(gpu_device), kb.to(gpu_device), *ps)
    assert torch.equal(fp, Fn.bert_layer(x.to(gpu_device), kb.to(gpu_device), *ps, matmul="fp32"))
    assert (bf - fp).abs().max().item() > 1e-3


@pytest.mark.parametrize("D,H", sorted(CONFIGS))
@pytest.mark.parametrize("B,T", MODEL_SWEEP)
def test_model_eval_against_float64_definition(gpu_device, D, H, B, T):
    """The 2-layer BertModel(impl="hip", matmul="bf16"), eval mode: every layer's output, pooled and every parameter gradient."""
    model = C.fresh_model(D, H, impl="hip", dtype=torch.float32, device=gpu_device)
    got = C.run_model(model, model_case(D, H, B, T))
    fr = C.worst(got, C.model_reference(D, H, B, T), f"model bf16 D={D} H={H} ({B},{T})")
    assert max(fr.values()) <= 1.0, fr


def _replay(model, p):
    """dropout_override for the float64 reference: the masks the device drew, from the snapshots the hip model used."""
    snaps = model.last_rng_snaps
    scale = 1.0 / (1.0 - p)

    def keep(layer, site, t):
        snap = snaps[0] if layer < 0 else snaps[1 + layer]
        salt = {"emb": _lib.SALT_BERT_EMB, "attn": _lib.SALT_BERT_ATTN, "ao": _lib.SALT_BERT_AO, "out": _lib.SALT_BERT_OUT}[site]
        m = Fn.dropout_keep_mask(snap, salt, p, t.numel()).view(t.shape).cpu()
        return t * m.to(t.dtype) * scale
    return keep


def test_model_train_mode_with_replayed_masks(gpu_device):
    D, H, B, T, p = 128, 2, 3, 33, 0.1
    case = model_case(D, H, B, T)
    gcgcn_amd.manual_seed(5)
    model = C.fresh_model(D, H, impl="hip", dtype=torch.float32, device=gpu_device, p=p)
    got = C.run_model(model, case, train=True)
    assert model.last_rng_snaps is not None and len(model.last_rng_snaps) == 3
    ref = C.run_model(C.fresh_model(D, H, p=p), case, train=True, override=_replay(model, p))
    assert not torch.equal(C.run_model(model, case)["out1"], got["out1"])              # masks were drawn at all
    fr = C.worst(got, ref, f"model bf16 train p={p}")
    assert max(fr.values()) <= 1.0, fr


def test_two_runs_from_one_seed_are_bitwise_equal(gpu_device):
    D, H, B, T = 192, 3, 2, 130
    case = model_case(D, H, B, T)
    runs = []
    for _ in range(2):
        gcgcn_amd.manual_seed(21)
        runs.append(C.run_model(C.fresh_model(D, H, impl="hip", dtype=torch.float32, device=gpu_device, p=0.1), case, train=True))
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_graph_replay_matches_eager(gpu_device):
    """A captured forward + backward (train mode, p = 0.1) replayed twice equals two eager steps from the same generator state, bit for
    bit: the bf16 products allocate nothing, read nothing back and run on the capturing stream."""
    D, H, B, T = 128, 2, 3, 33
    case = model_case(D, H, B, T)
    model = C.fresh_model(D, H, impl="hip", dtype=torch.float32, device=gpu_device, p=0.1).train()
    ids, tt, mask = case["ids"].to(gpu_device), case["tt"].to(gpu_device), case["mask"].to(gpu_device)
    dy, dp = case["dy"].to(gpu_device), case["dp"].to(gpu_device)
    out = {}

    def step():
        model.zero_grad(set_to_none=True)
        last, pooled = model(ids, tt, mask, output_all_encoded_layers=False)
        ((last * dy).sum() + (pooled * dp).sum()).backward()
        out["last"], out["pooled"] = last, pooled

    def results():
        r = {"last": out["last"], "pooled": out["pooled"]}
        r.update({n: q.grad for n, q in model.named_parameters()})
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
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append({k: v.detach().clone() for k, v in live.items()})
    rng.copy_(start)
    for i in range(2):
        step()
        torch.cuda.synchronize()
        for k, v in results().items():
            assert torch.equal(v, replays[i][k]), (i, k)
    assert not torch.equal(replays[0]["last"], replays[1]["last"])                     # a fresh mask at every replay


def _zeros_on(t, pad, name):
    rows = t[pad.to(t.device)]
    assert torch.equal(rows, torch.zeros_like(rows)), f"{name}: padding rows are not exactly zero"


@pytest.mark.parametrize("B,T,lengths,rowblk", [(3, 48, (48, 0, 17), False), (4, 64, (64, 33, 16, 0), True)])
def test_layer_lengths_against_per_document_float64(gpu_device, B, T, lengths, rowblk):
    """t_valid with the bf16 products (always dense; a row-block list is accepted and ignored): live rows against the definition run on
    every document alone, the output and dx exactly zero on padding rows, a NaN cotangent there ignored."""
    D, H = 128, 2
    c = layer_len_case(D, H, B, T, lengths)
    tv = torch.tensor(lengths, dtype=torch.int32, device=gpu_device)
    dy = c["dy"].clone()
    pad = pad_mask(lengths, T)
    dy[pad] = NAN
    got = _layer_hip(c["x"], None, c["params"], dy, gpu_device, t_valid=tv, rowblk=Fn.row_blocks(tv, B, T) if rowblk else None)
    _zeros_on(got["y"], pad, "y")
    _zeros_on(got["dx"], pad, "dx")
    fr = C.worst(got, C.layer_len_reference(D, H, B, T, lengths), f"layer bf16, lengths {lengths} of T={T}")
    assert max(fr.values()) <= 1.0, fr
    if rowblk:      # the list changes nothing, bit for bit
        dense = _layer_hip(c["x"], None, c["params"], dy, gpu_device, t_valid=tv)
        for k in got:
            assert torch.equal(got[k], dense[k]), k


@pytest.mark.parametrize("B,T,lengths", [(3, 48, (48, 0, 17)), (4, 64, (64, 33, 16, 0))])
def test_model_lengths_against_per_document_float64(gpu_device, B, T, lengths):
    """BertModel(impl="hip", matmul="bf16") with lengths= (it builds the row-block list at T % 16 == 0): NaN cotangent and other token
    ids on the padding rows."""
    D, H = 128, 2
    case = dict(model_case(D, H, B, T))
    pad = pad_mask(lengths, T)
    case["ids"] = torch.where(pad, (case["ids"] + 7) % 61, case["ids"])
    model = C.fresh_model(D, H, impl="hip", dtype=torch.float32, device=gpu_device)
    got = run_with_lengths(model, case, lengths)
    for k in ("out0", "out1"):
        _zeros_on(got[k], pad, k)
    b = lengths.index(0)
    assert torch.equal(got["pooled"][b], torch.tanh(model.pooler.dense.bias.detach()))
    fr = C.worst(got, C.model_len_reference(D, H, B, T, lengths), f"model bf16, lengths {lengths} of T={T}")
    assert max(fr.values()) <= 1.0, fr


class _Cfg:
    entity_type_size, coref_size, max_length, keep_prob, graph_hop = 20, 20, 512, 1.0, 2
    dis_size, dis_num, dis_plus, relation_num, alpha = 20, 21, 10, 97, 1.0

    def __init__(self, vocab, **kw):
        import numpy as np
        self.data_word_vec = np.zeros((vocab, 100), np.float32)
        self.__dict__.update(kw)


def test_graph_model_hip_against_torch_definition(gpu_device):
    """GraphCNN_multihead_bert_gate_cls with bert_impl="hip", bert_matmul="bf16": one forward + backward at the config of
    test_bert_gpu.test_model_wiring_hip_against_torch; the logits against bert_impl="torch", bert_matmul="bf16" on the device under
    the bound; every parameter of the hip twin gets a finite gradient."""
    from conftest import golden_files, load_golden
    from lstm_cases import doc_tensors
    g = load_golden(golden_files("model_step")[0])
    vocab = g["meta"]["vocab"]
    bc = config(128, 2)
    bc.vocab_size = vocab
    torch.manual_seed(5)
    base = M.GraphCNN_multihead_bert_gate_cls(_Cfg(vocab, bert_impl="torch", bert_matmul="bf16", bert_config=bc)).to(gpu_device).eval()
    twin = M.GraphCNN_multihead_bert_gate_cls(_Cfg(vocab, bert_impl="hip", bert_matmul="bf16", bert_config=bc)).to(gpu_device).eval()
    assert twin.bert.matmul == "bf16" and twin.bert.impl == "hip"
    with torch.no_grad():
        sd = state(128, 2)
        for n, q in base.bert.named_parameters():
            if "word_embeddings" not in n:
                q.copy_(sd[n])
            else:
                q.normal_(0, 0.5)
        for n, q in base.named_parameters():
            if n.endswith("attention_all.bias"):
                q.fill_(0.4)
    assert not twin.load_state_dict(base.state_dict(), strict=True).missing_keys
    docs = [doc_tensors(g["raw"], di, gpu_device) for di in range(2)]
    batch = {k: torch.stack([d[k] for d in docs]) for k in docs[0]}
    T = batch["document"].shape[1]
    t_valid = torch.tensor([T, max(1, T - 13)], device=gpu_device)
    want = base(**batch, t_valid=t_valid)
    got = twin(**batch, t_valid=t_valid)
    got.square().mean().backward()
    assert torch.isfinite(got).all()
    print(f"bert graph model, bf16: hip vs torch {C.frac_of_bound(got, want):.3f} of the bound, max |logit| {want.abs().max().item():.3e}")
    assert C.frac_of_bound(got, want) <= 1.0
    grads = [q.grad for q in twin.bert.encoder.parameters()]
    assert all(t is not None and torch.isfinite(t).all() for t in grads)
