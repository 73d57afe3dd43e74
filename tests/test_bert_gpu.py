"""The HIP BERT encoder on the device against the float64 CPU reference of tests/bert_cases.py (bound and constants there).

Block edges of the attention kernels (csrc/bert.hip): a workgroup owns 16 rows (queries in the forward and the dq kernel, keys in
the dk / dv kernel) and streams the other side in blocks of 64.  ATTN_T: 1 (one row of one block), 15 / 16 / 17 (either side of the
owner block's edge: one workgroup, exactly one, two), 33 (three owner blocks, the last with one row; inside the first streamed
block), 63 / 64 / 65 (either side of the streamed block's edge), 130 (three streamed blocks, the last with two rows), 512 (the
largest T served: eight streamed blocks, the whole LDS score row)."""
import ctypes

import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib, functional as Fn, models as M
from gcgcn_amd import bert as bert_mod
from gcgcn_amd.bert import BertModel

from bert_cases import (CONFIGS, MODEL_SWEEP, attn_case, attn_ref, attn_reference, config, frac_of_bound, model_case, model_reference,
                        run_model, state, worst)

pytestmark = pytest.mark.gpu

ATTN_T = [(3, 1), (3, 15), (3, 16), (3, 17), (3, 33), (3, 63), (3, 64), (3, 65), (3, 130), (1, 512)]
NAN = float("nan")


def _p(t):
    return None if t is None else t.data_ptr()


def _attn_device(case, H, dev, snap=None, salt=0, p=0.0, guard=NAN):
    """The core through the C ABI.  Every buffer carries one guard document past its end, filled with `guard`; the outputs are
    NaN-filled before the call.  Returns ({"ctx", "lse", "dqkv"}, the guards of the outputs)."""
    B, T, D3 = case["qkv"].shape
    D = D3 // 3

    def padded(t, fill):
        buf = torch.full((B + 1,) + tuple(t.shape[1:]), fill, device=dev)
        buf[:B] = t.to(dev)
        return buf

    qkv, dctx = padded(case["qkv"], guard), padded(case["dctx"], guard)
    kb = None if case["key_bias"] is None else padded(case["key_bias"], guard)
    ctx, dqkv = torch.full((B + 1, T, D), NAN, device=dev), torch.full((B + 1, T, 3 * D), NAN, device=dev)
    lse, delta = torch.full((B + 1, H, T), NAN, device=dev), torch.full((B + 1, H, T), NAN, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("gcgcn_bert_attn_fwd", B, T, H, 64, _p(qkv), _p(kb), _p(ctx), _p(lse), _p(snap), salt, p, st)
    _lib.call("gcgcn_bert_attn_bwd", B, T, H, 64, _p(qkv), _p(kb), _p(ctx), _p(lse), _p(dctx), _p(dqkv), _p(delta), _p(snap), salt, p, st)
    torch.cuda.synchronize()
    # the kernels store lse relative to the document's largest penalty c_b (include/gcgcn.h): the row's log-sum-exp is lse + c_b
    cb = 0.0 if kb is None else kb[:B].max(dim=1).values.double()[:, None, None]
    return {"ctx": ctx[:B], "lse": lse[:B].double() + cb, "dqkv": dqkv[:B]}, (ctx[B], lse[B], dqkv[B], delta[B])


@pytest.mark.parametrize("kind", ["none", "prefix", "holes", "dead"])
@pytest.mark.parametrize("B,T", ATTN_T)
def test_attention_core_against_float64(gpu_device, B, T, kind):
    """ctx, lse, dq | dk | dv within the bound; the guard document behind every output stays NaN, everything inside is finite, and the
    results do not depend on what lies behind the inputs' end (NaN or 1.0 behind the last block's rows)."""
    H = 2
    case = attn_case(B, T, H, kind)
    got, guards = _attn_device(case, H, gpu_device)
    for g in guards:
        assert torch.isnan(g).all()
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
    fr = worst(got, attn_reference(B, T, H, kind), f"attention core B={B} T={T} {kind}")
    assert max(fr.values()) <= 1.0, fr
    again, _ = _attn_device(case, H, gpu_device, guard=1.0)
    for k in got:
        assert torch.equal(got[k], again[k]), k


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_core_dropout_replays_the_mask(gpu_device, p):
    B, T, H = 3, 65, 3
    case = attn_case(B, T, H, "prefix")
    gcgcn_amd.manual_seed(11)
    snap = Fn.rng_snapshot(gpu_device)
    got, _ = _attn_device(case, H, gpu_device, snap=snap, salt=_lib.SALT_BERT_ATTN, p=p)
    keep = Fn.dropout_keep_mask(snap, _lib.SALT_BERT_ATTN, p, B * H * T * T).view(B, H, T, T).cpu()
    assert 0.6 * (1 - p) < keep.float().mean().item() < min(1.0, 1.4 * (1 - p))
    fr = worst(got, attn_ref(case, H, torch.float64, keep=keep, scale=1.0 / (1.0 - p)), f"attention core, dropout p={p}")
    assert max(fr.values()) <= 1.0, fr


def _layer_inputs(D, H, B, T, dev, kind="prefix"):
    case = model_case(D, H, B, T, kind)
    g = torch.Generator().manual_seed(B + T + D)
    x = torch.randn(B, T, D, generator=g)
    names = [k[len("encoder.layer.0."):] for k in state(D, H) if k.startswith("encoder.layer.0.")]
    model = BertModel(config(D, H))
    model.load_state_dict(state(D, H))
    params = [t.detach() for t in model.encoder.layer[0].tensors()]
    kb = None if case["mask"] is None else (1.0 - case["mask"]) * -10000.0
    return case, x, params, kb, names


def _layer_torch(x, kb, params, H, dy, dtype, drop=lambda s, t: t):
    x = x.to(dtype).clone().requires_grad_()
    ps = [t.to(dtype).clone().requires_grad_() for t in params]
    y = bert_mod.torch_layer(x, None if kb is None else kb.to(dtype), ps, H, drop)
    (y * dy.to(dtype)).sum().backward()
    res = {"y": y.detach(), "dx": x.grad}
    res.update({f"d{i:02d}": t.grad for i, t in enumerate(ps)})
    return res


def _layer_hip(x, kb, params, dy, dev, **kw):
    x = x.to(dev).requires_grad_()
    ps = [t.to(dev).requires_grad_() for t in params]
    y = Fn.bert_layer(x, None if kb is None else kb.to(dev), *ps, **kw)
    (y * dy.to(dev)).sum().backward()
    res = {"y": y.detach(), "dx": x.grad}
    res.update({f"d{i:02d}": t.grad for i, t in enumerate(ps)})
    return res


@pytest.mark.parametrize("D,H", sorted(CONFIGS))
@pytest.mark.parametrize("B,T", MODEL_SWEEP)
def test_layer_eval_against_float64(gpu_device, D, H, B, T):
    """functional.bert_layer: output, input gradient and the gradient of all 16 tensors.  (3, 33): 99 rows, the guarded GEMM body;
    (2, 130): 260 rows with D = 128 / 192 and 4 D columns, interior tiles and a guarded edge."""
    case, x, params, kb, _ = _layer_inputs(D, H, B, T, gpu_device)
    ref = _layer_torch(x, kb, params, H, case["dy"], torch.float64)
    got = _layer_hip(x, kb, params, case["dy"], gpu_device)
    fr = worst(got, ref, f"layer eval D={D} H={H} ({B},{T})")
    assert max(fr.values()) <= 1.0, fr
    got2 = _layer_hip(x, None, params, case["dy"], gpu_device)              # without key_bias
    fr = worst(got2, _layer_torch(x, None, params, H, case["dy"], torch.float64), f"layer eval, no mask D={D} H={H} ({B},{T})")
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize("D,H", sorted(CONFIGS))
@pytest.mark.parametrize("B,T", MODEL_SWEEP)
def test_model_eval_against_float64(gpu_device, D, H, B, T):
    """The 2-layer BertModel(impl="hip"): every layer's output, the pooled output and every parameter gradient (the embedding tables'
    gradients are the model's input gradient)."""
    got = run_model(D, H, model_case(D, H, B, T), torch.float32, device=gpu_device, impl="hip")
    fr = worst(got, model_reference(D, H, B, T), f"model eval D={D} H={H} ({B},{T})")
    assert max(fr.values()) <= 1.0, fr


def _replay(model, dev, B, H, T, D, p):
    """dropout_override for the float64 reference: the masks the device drew, from the snapshots the hip model used."""
    snaps = model.last_rng_snaps
    scale = 1.0 / (1.0 - p)

    def keep(layer, site, t):
        snap = snaps[0] if layer < 0 else snaps[1 + layer]
        salt = {"emb": _lib.SALT_BERT_EMB, "attn": _lib.SALT_BERT_ATTN, "ao": _lib.SALT_BERT_AO, "out": _lib.SALT_BERT_OUT}[site]
        m = Fn.dropout_keep_mask(snap, salt, p, t.numel()).view(t.shape).cpu()
        return t * m.to(t.dtype) * scale
    return keep


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_model_train_mode_against_float64_with_replayed_masks(gpu_device, p):
    D, H, B, T = 128, 2, 3, 33
    case = model_case(D, H, B, T)
    gcgcn_amd.manual_seed(5)
    model = BertModel(config(D, H, 2, p), impl="hip")
    model.load_state_dict(state(D, H))
    model = model.to(gpu_device)
    got = run_model(D, H, case, torch.float32, device=gpu_device, train=True, model=model)
    assert model.last_rng_snaps is not None and len(model.last_rng_snaps) == 3
    ref = run_model(D, H, case, torch.float64, p=p, train=True, override=_replay(model, gpu_device, B, H, T, D, p))
    eval_out = run_model(D, H, case, torch.float32, device=gpu_device, impl="hip")["out1"]
    assert not torch.equal(eval_out, got["out1"])                                     # masks were drawn at all
    fr = worst(got, ref, f"model train p={p}")
    assert max(fr.values()) <= 1.0, fr


def test_two_runs_from_one_seed_are_bitwise_equal(gpu_device):
    D, H, B, T = 192, 3, 2, 130
    case = model_case(D, H, B, T)
    runs = []
    for _ in range(2):
        gcgcn_amd.manual_seed(21)
        model = BertModel(config(D, H, 2, 0.1), impl="hip")
        model.load_state_dict(state(D, H))
        runs.append(run_model(D, H, case, torch.float32, device=gpu_device, train=True, model=model.to(gpu_device)))
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_graph_replay_matches_eager(gpu_device):
    """A captured forward + backward (train mode, p = 0.1) replayed twice equals two eager steps from the same generator state, bit for
    bit: nothing is allocated or read back inside the calls, and the dropout counter advances on the device."""
    D, H, B, T = 128, 2, 3, 33
    case = model_case(D, H, B, T)
    model = BertModel(config(D, H, 2, 0.1), impl="hip")
    model.load_state_dict(state(D, H))
    model = model.to(gpu_device).train()
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


@pytest.mark.parametrize("rows", [1, 17])
@pytest.mark.parametrize("D", [64, 192, 768])
def test_res_layer_norm_alone(gpu_device, D, rows):
    """Each optional operand on and off, training dropout with the replayed mask, a constant row (variance 0)."""
    g = torch.Generator().manual_seed(D + rows)
    x, res, dy = (torch.randn(rows, D, generator=g) for _ in range(3))
    x[0] = 0.75                                                                         # constant where nothing is added
    lb, w, b = 0.3 * torch.randn(D, generator=g), 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    gcgcn_amd.manual_seed(3)
    for use_bias, use_res, p in [(False, False, 0.0), (True, False, 0.0), (False, True, 0.0), (True, True, 0.0), (True, True, 0.5), (False, False, 0.1)]:
        snap = Fn.rng_snapshot(gpu_device) if p > 0 else None
        leaves = [t.to(gpu_device).requires_grad_() for t in (x, res, lb, w, b)]
        y = Fn.res_layer_norm(leaves[0], leaves[3], leaves[4], lin_bias=leaves[2] if use_bias else None, res=leaves[1] if use_res else None,
                              p=p, training=p > 0, snap=snap, salt=_lib.SALT_BERT_EMB)
        (y * dy.to(gpu_device)).sum().backward()
        got = {"y": y.detach(), "dx": leaves[0].grad, "dw": leaves[3].grad, "db": leaves[4].grad}
        r = [t.double().clone().requires_grad_() for t in (x, res, lb, w, b)]
        v = r[0] + r[2] if use_bias else r[0]
        if p > 0:
            v = v * Fn.dropout_keep_mask(snap, _lib.SALT_BERT_EMB, p, rows * D).view(rows, D).cpu().double() / (1.0 - p)
        v = v + r[1] if use_res else v
        yr = bert_mod.layer_norm(v, r[3], r[4])
        (yr * dy.double()).sum().backward()
        ref = {"y": yr.detach(), "dx": r[0].grad, "dw": r[3].grad, "db": r[4].grad}
        if use_bias:
            got["dlb"], ref["dlb"] = leaves[2].grad, r[2].grad
        if use_res:
            got["dres"], ref["dres"] = leaves[1].grad, r[1].grad
        for k, t in got.items():
            assert torch.isfinite(t).all(), (k, use_bias, use_res, p)
        if not (use_bias or use_res or p > 0):
            # the constant row: y = bias exactly, and no gradient passes a normalisation of a constant
            assert torch.equal(got["y"][0].cpu(), b)
            got = {k: (t[1:] if k in ("y", "dx") else t) for k, t in got.items()}
            ref = {k: (t[1:] if k in ("y", "dx") else t) for k, t in ref.items()}
            if rows == 1:
                continue
        fr = worst(got, ref, f"res_layer_norm D={D} rows={rows} bias={use_bias} res={use_res} p={p}")
        assert max(fr.values()) <= 1.0, fr


class _Cfg:
    entity_type_size, coref_size, max_length, keep_prob, graph_hop = 20, 20, 512, 1.0, 2
    dis_size, dis_num, dis_plus, relation_num, alpha = 20, 21, 10, 97, 1.0

    def __init__(self, vocab, **kw):
        import numpy as np
        self.data_word_vec = np.zeros((vocab, 100), np.float32)
        self.__dict__.update(kw)


def test_model_wiring_hip_against_torch(gpu_device):
    """GraphCNN_multihead_bert_gate_cls with bert_impl="hip" against bert_impl="torch" on the device: one state_dict, loaded strict both
    ways; a ragged two-document batch with t_valid, eval mode; logits within the bound the model tests use (rtol 1e-4, atol 2e-4)."""
    from conftest import golden_files, load_golden
    from lstm_cases import doc_tensors
    g = load_golden(golden_files("model_step")[0])
    vocab = g["meta"]["vocab"]
    bc = config(128, 2)
    bc.vocab_size = vocab
    torch.manual_seed(5)
    base = M.GraphCNN_multihead_bert_gate_cls(_Cfg(vocab, bert_impl="torch", bert_config=bc)).to(gpu_device).eval()
    twin = M.GraphCNN_multihead_bert_gate_cls(_Cfg(vocab, bert_impl="hip", bert_config=bc)).to(gpu_device).eval()
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
    assert not base.load_state_dict(twin.state_dict(), strict=True).missing_keys
    docs = [doc_tensors(g["raw"], di, gpu_device) for di in range(2)]
    batch = {k: torch.stack([d[k] for d in docs]) for k in docs[0]}
    T = batch["document"].shape[1]
    t_valid = torch.tensor([T, max(1, T - 13)], device=gpu_device)
    with torch.no_grad():
        want = base(**batch, t_valid=t_valid)
        got = twin(**batch, t_valid=t_valid)
    assert torch.isfinite(got).all()
    err = (got - want).abs()
    print(f"bert model, hip vs torch encoder: max |diff| {err.max().item():.3e}, max |logit| {want.abs().max().item():.3e}")
    torch.testing.assert_close(got, want, rtol=1e-4, atol=2e-4)
