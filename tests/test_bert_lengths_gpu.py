"""Per-document token lengths of the HIP BERT encoder (t_valid; DESIGN.md section 8.9, include/gcgcn.h) on the device.

Reference and bound: tests/bert_length_cases.py -- float64 ``impl="torch"`` on every document ALONE, truncated to its length, no mask --
and ``bert_cases.frac_of_bound(got, ref) <= 1``.  Padding rows are compared with ``torch.equal`` against zeros.  The cotangents are
NaN on padding rows unless a test says otherwise, and the suite runs on NaN-poisoned free memory (conftest.py).

Shapes.  The attention kernels own 16 rows and stream blocks of 64: (4, 160) with (160, 65, 16, 0) has the streamed block's edge on
either side (64 | 65), a document that is one whole owner block, an empty one; (3, 48) with (48, 17, 1) a partly live owner block and a
single token; (2, 512) with (512, 449) the largest T and a last streamed block of one key.  The layer's products: (3, 48) and (3, 33)
are 144 and 99 rows, no whole 64-row tiles, so the GEMM launcher drops the row-block list (33: there is none) and every product runs
dense; (4, 64) is 256 rows of whole tiles, where the backward's group launches keep the list (data gradients compute, weight
gradients sum over the live blocks); (8, 512) with D = 128 has 384 and 512 tiles in the qkv and intermediate products, above the
launcher's threshold for a stand-alone row-block launch, so the forward walks the list too and leaves the dead blocks of qkv and z
UNWRITTEN; (17, 512) is 8704 rows, more than the 512 blocks a weight gradient's list may hold: data gradients on the list, weight
gradients dense, in one call."""
import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib, functional as Fn, models as M

from bert_cases import CONFIGS, config, model_case, state, worst
from bert_length_cases import (NAN, attn_len_case, attn_len_reference, fresh_model, layer_len_case, layer_len_reference, model_len_reference,
                               pad_mask, run_with_lengths)

pytestmark = pytest.mark.gpu

ATTN_CASES = [(4, 160, (160, 65, 16, 0)), (3, 48, (48, 17, 1)), (2, 512, (512, 449))]
LAYER_CASES = [(3, 48, (48, 17, 1)), (3, 33, (33, 20, 0))]
ROWBLK_CASE = (4, 64, (64, 33, 16, 0))


def _p(t):
    return None if t is None else t.data_ptr()


def _zeros_on(t, pad, name):
    rows = t[pad.to(t.device)]
    assert torch.equal(rows, torch.zeros_like(rows)), f"{name}: padding rows are not exactly zero"


def _attn_len_device(case, H, lengths, dev, nan_dctx=False, nan_qkv=False, snap=None, salt=0, p=0.0):
    """The core through gcgcn_bert_attn_fwd_len / _bwd_len; outputs NaN-filled before the call."""
    B, T, D3 = case["qkv"].shape
    D = D3 // 3
    pad = pad_mask(lengths, T)
    qkv, dctx = case["qkv"].clone(), case["dctx"].clone()
    if nan_dctx:
        dctx[pad] = NAN
    if nan_qkv:
        qkv[pad] = NAN
    qkv, dctx = qkv.to(dev), dctx.to(dev)
    kb = None if case["key_bias"] is None else case["key_bias"].to(dev)
    tv = torch.tensor(lengths, dtype=torch.int32, device=dev)
    ctx, dqkv = torch.full((B, T, D), NAN, device=dev), torch.full((B, T, 3 * D), NAN, device=dev)
    lse, delta = torch.full((B, H, T), NAN, device=dev), torch.full((B, H, T), NAN, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("gcgcn_bert_attn_fwd_len", B, T, H, 64, _p(qkv), _p(kb), _p(tv), _p(ctx), _p(lse), _p(snap), salt, p, st)
    _lib.call("gcgcn_bert_attn_bwd_len", B, T, H, 64, _p(qkv), _p(kb), _p(tv), _p(ctx), _p(lse), _p(dctx), _p(dqkv), _p(delta), _p(snap), salt,
              p, st)
    torch.cuda.synchronize()
    return {"ctx": ctx, "lse": lse, "dqkv": dqkv}


def _check_attn(got, ref, case, lengths, label):
    B, T, _ = case["qkv"].shape
    pad = pad_mask(lengths, T)
    _zeros_on(got["ctx"], pad, "ctx")
    _zeros_on(got["dqkv"], pad, "dqkv")
    _zeros_on(got["lse"].transpose(1, 2), pad, "lse")
    # the kernels store lse relative to c_b, the largest penalty of the document's LIVE keys (include/gcgcn.h)
    lse = got["lse"].double().cpu()
    if case["key_bias"] is not None:
        for b, n in enumerate(lengths):
            if n:
                lse[b, :, :n] += case["key_bias"][b, :n].max().double()
    fr = worst({"ctx": got["ctx"], "lse": lse, "dqkv": got["dqkv"]}, ref, label)
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize("B,T,lengths", ATTN_CASES)
def test_attention_core_lengths_against_per_document_float64(gpu_device, B, T, lengths):
    H = 2
    case = attn_len_case(B, T, H)
    got = _attn_len_device(case, H, lengths, gpu_device)
    _check_attn(got, attn_len_reference(B, T, H, lengths), case, lengths, f"attention core, lengths {lengths} of T={T}")
    # what sits on padding rows is not read: dctx = NaN there (the contract), and qkv too
    for kw in (dict(nan_dctx=True), dict(nan_dctx=True, nan_qkv=True)):
        again = _attn_len_device(case, H, lengths, gpu_device, **kw)
        for k in got:
            assert torch.equal(got[k], again[k]), (k, kw)


def test_attention_core_lengths_with_key_bias_holes(gpu_device):
    B, T, lengths, H = 3, 48, (48, 17, 1), 2
    case = attn_len_case(B, T, H, holes=True)
    got = _attn_len_device(case, H, lengths, gpu_device, nan_dctx=True)
    _check_attn(got, attn_len_reference(B, T, H, lengths, True), case, lengths, "attention core, lengths + key_bias holes")


def _layer_len_hip(c, lengths, dev, rowblk=True, nan_pad=True, **kw):
    B, T, D = c["x"].shape
    tv = torch.tensor(lengths, dtype=torch.int32, device=dev)
    x = c["x"].to(dev).requires_grad_()
    ps = [t.to(dev).requires_grad_() for t in c["params"]]
    dy = c["dy"].clone()
    if nan_pad:
        dy[pad_mask(lengths, T)] = NAN
    y = Fn.bert_layer(x, None, *ps, t_valid=tv, rowblk=Fn.row_blocks(tv, B, T) if rowblk else None, **kw)
    # y * dy would turn 0 * NaN into a NaN loss; hand the cotangent over as it is
    y.backward(dy.to(dev))
    res = {"y": y.detach(), "dx": x.grad}
    res.update({f"d{i:02d}": t.grad for i, t in enumerate(ps)})
    return res


def _check_layer(got, ref, lengths, T, label):
    pad = pad_mask(lengths, T)
    _zeros_on(got["y"], pad, "y")
    _zeros_on(got["dx"], pad, "dx")
    fr = worst(got, ref, label)
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize("D,H", sorted(CONFIGS))
@pytest.mark.parametrize("B,T,lengths", LAYER_CASES + [ROWBLK_CASE])
def test_layer_lengths_against_per_document_float64(gpu_device, D, H, B, T, lengths):
    c = layer_len_case(D, H, B, T, lengths)
    got = _layer_len_hip(c, lengths, gpu_device)
    _check_layer(got, layer_len_reference(D, H, B, T, lengths), lengths, T, f"layer, lengths {lengths} of T={T} D={D}")
    dense = _layer_len_hip(c, lengths, gpu_device, rowblk=False)               # rowblk = None: every product dense, the same contract
    _check_layer(dense, layer_len_reference(D, H, B, T, lengths), lengths, T, f"layer, lengths {lengths} of T={T} D={D}, no row blocks")


@pytest.mark.parametrize("B,T,lengths", [(8, 512, (512, 449, 130, 64, 17, 1, 0, 300)),
                                         (17, 512, (512, 200, 64, 16, 1, 0) + tuple(range(5, 16)))])
def test_layer_lengths_where_the_forward_walks_row_blocks(gpu_device, B, T, lengths):
    """(8, 512): the stand-alone forward products keep the list and leave dead blocks unwritten.  (17, 512): B T > 8192, the weight
    gradients run dense beside data gradients on the list."""
    D, H = 128, 2
    c = layer_len_case(D, H, B, T, lengths)
    got = _layer_len_hip(c, lengths, gpu_device)
    _check_layer(got, layer_len_reference(D, H, B, T, lengths), lengths, T, f"layer, lengths of ({B},{T}) D={D}")


@pytest.mark.parametrize("D,H", sorted(CONFIGS))
@pytest.mark.parametrize("B,T,lengths", LAYER_CASES + [ROWBLK_CASE])
def test_model_lengths_against_per_document_float64(gpu_device, D, H, B, T, lengths):
    """The 2-layer BertModel(impl="hip") with lengths=: every layer's output, pooled, every parameter gradient; other token ids on the
    padding rows than the reference ever saw (it never sees them)."""
    case = dict(model_case(D, H, B, T))
    pad = pad_mask(lengths, T)
    case["ids"] = torch.where(pad, (case["ids"] + 7) % 61, case["ids"])
    model = fresh_model(D, H, impl="hip", dtype=torch.float32, device=gpu_device)
    got = run_with_lengths(model, case, lengths)
    for k in ("out0", "out1"):
        _zeros_on(got[k], pad, k)
    if 0 in lengths:
        b = lengths.index(0)
        assert torch.equal(got["pooled"][b], torch.tanh(model.pooler.dense.bias.detach()))
    fr = worst(got, model_len_reference(D, H, B, T, lengths), f"model, lengths {lengths} of T={T} D={D}")
    assert max(fr.values()) <= 1.0, fr


def _replay(model, p):
    """dropout_override for the float64 reference: the masks the device drew, from the snapshots the hip model used (indices of the PADDED
    tensors)."""
    snaps = model.last_rng_snaps
    scale = 1.0 / (1.0 - p)

    def keep(layer, site, t):
        snap = snaps[0] if layer < 0 else snaps[1 + layer]
        salt = {"emb": _lib.SALT_BERT_EMB, "attn": _lib.SALT_BERT_ATTN, "ao": _lib.SALT_BERT_AO, "out": _lib.SALT_BERT_OUT}[site]
        m = Fn.dropout_keep_mask(snap, salt, p, t.numel()).view(t.shape).cpu()
        return t * m.to(t.dtype) * scale
    return keep


def test_model_lengths_train_mode_with_replayed_masks(gpu_device):
    """Train mode, p = 0.1, lengths (48, 17, 1).  (1) Against the float64 impl="torch" model with the same lengths and the device's masks
    replayed (tests/test_bert_lengths_cpu.py ties that model to the per-document runs).  (2) From the same seed the prefix-mask path
    draws the same snapshots; on live rows and in every gradient (cotangent zero on padding rows for both) it agrees with the length
    path within the bound: the dropout indices did not move."""
    D, H, B, T, lengths, p = 128, 2, 3, 48, (48, 17, 1), 0.1
    case = model_case(D, H, B, T)
    pad = pad_mask(lengths, T)
    gcgcn_amd.manual_seed(5)
    model = fresh_model(D, H, impl="hip", dtype=torch.float32, device=gpu_device, p=p)
    got = run_with_lengths(model, case, lengths, train=True)
    assert model.last_rng_snaps is not None and len(model.last_rng_snaps) == 3
    ref = run_with_lengths(fresh_model(D, H, p=p), case, lengths, train=True, override=_replay(model, p))
    for k in ("out0", "out1"):
        _zeros_on(got[k], pad, k)
    eval_out = run_with_lengths(model, case, lengths)["out1"]
    assert not torch.equal(eval_out, got["out1"])                                     # masks were drawn at all
    fr = worst(got, ref, f"model, lengths, train p={p}")
    assert max(fr.values()) <= 1.0, fr

    gcgcn_amd.manual_seed(5)
    a = run_with_lengths(model, case, lengths, nan_pad=False, train=True)
    gcgcn_amd.manual_seed(5)
    b = run_with_lengths(model, case, lengths, nan_pad=False, train=True, mask=(~pad).float(), lengths_arg=False)
    for k in ("out0", "out1"):
        b[k] = torch.where(pad.to(gpu_device)[:, :, None], torch.zeros_like(b[k]), b[k])
    fr = worst(a, b, "length path against prefix-mask path, one snapshot")
    assert max(fr.values()) <= 1.0, fr


def test_lengths_two_runs_from_one_seed_are_bitwise_equal(gpu_device):
    D, H = 192, 3
    B, T, lengths = ROWBLK_CASE
    case = model_case(D, H, B, T)
    runs = []
    for _ in range(2):
        gcgcn_amd.manual_seed(21)
        model = fresh_model(D, H, impl="hip", dtype=torch.float32, device=gpu_device, p=0.1)
        runs.append(run_with_lengths(model, case, lengths, train=True))
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_lengths_graph_replays_on_new_lengths(gpu_device):
    """One hipGraph captured with a t_valid tensor, replayed after t_valid.copy_(other): bitwise the eager run on `other`.  Nothing is
    read on the host, the grids do not depend on the lengths, the row-block list is rebuilt on the device inside the graph."""
    D, H = 128, 2
    B, T, lengths = ROWBLK_CASE
    others = [(16, 64, 0, 49), (1, 1, 64, 32), lengths]
    case = model_case(D, H, B, T)
    model = fresh_model(D, H, impl="hip", dtype=torch.float32, device=gpu_device).eval()
    ids, tt = case["ids"].to(gpu_device), case["tt"].to(gpu_device)
    dy, dp = case["dy"].to(gpu_device), case["dp"].to(gpu_device)
    tv = torch.tensor(lengths, dtype=torch.int32, device=gpu_device)
    out = {}

    def step(t_valid):
        model.zero_grad(set_to_none=True)
        last, pooled = model(ids, tt, output_all_encoded_layers=False, lengths=t_valid)
        torch.autograd.backward([last, pooled], [dy, dp])
        out["last"], out["pooled"] = last, pooled

    def results():
        r = {"last": out["last"], "pooled": out["pooled"]}
        r.update({n: q.grad for n, q in model.named_parameters()})
        return r

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(tv)
        step(tv)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(tv)
    torch.cuda.synchronize()
    live = results()
    replays = []
    for other in others:
        tv.copy_(torch.tensor(other, dtype=torch.int32, device=gpu_device))
        graph.replay()
        torch.cuda.synchronize()
        replays.append({k: v.detach().clone() for k, v in live.items()})
    for other, rep in zip(others, replays):
        step(torch.tensor(other, dtype=torch.int32, device=gpu_device))
        torch.cuda.synchronize()
        for k, v in results().items():
            assert torch.equal(v, rep[k]), (other, k)
        _zeros_on(rep["last"], pad_mask(other, T), "last")
    assert not torch.equal(replays[0]["last"], replays[1]["last"])


@pytest.mark.parametrize("B,T", [(3, 48), (3, 33)])
def test_lengths_all_equal_to_T_match_the_path_without_lengths(gpu_device, B, T):
    D, H = 128, 2
    case = model_case(D, H, B, T)
    model = fresh_model(D, H, impl="hip", dtype=torch.float32, device=gpu_device)
    got = run_with_lengths(model, case, (T,) * B)
    model.zero_grad(set_to_none=True)
    outs, pooled = model(case["ids"].to(gpu_device), case["tt"].to(gpu_device))
    torch.autograd.backward([outs[-1], pooled], [case["dy"].to(gpu_device), case["dp"].to(gpu_device)])
    ref = {f"out{i}": t.detach() for i, t in enumerate(outs)}
    ref["pooled"] = pooled.detach()
    ref.update({"d" + k: q.grad for k, q in model.named_parameters()})
    fr = worst(got, ref, f"lengths = T against lengths = None ({B},{T})")
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize("D", [64, 192])
def test_res_layer_norm_and_gelu_with_lengths(gpu_device, D):
    """The row kernels alone: NaN in every input on padding rows, zeros out; live rows and the parameter gradients as without lengths
    on the live rows alone."""
    B, T, lengths = 3, 7, (7, 3, 0)
    pad = pad_mask(lengths, T)
    g = torch.Generator().manual_seed(D)
    x, res, dy = (torch.randn(B, T, D, generator=g) for _ in range(3))
    lb, w, b = 0.3 * torch.randn(D, generator=g), 1 + 0.1 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    tv = torch.tensor(lengths, dtype=torch.int32, device=gpu_device)
    poisoned = [t.clone() for t in (x, res, dy)]
    for t in poisoned:
        t[pad] = NAN
    leaves = [t.to(gpu_device).requires_grad_() for t in (poisoned[0], poisoned[1], lb, w, b)]
    y = Fn.res_layer_norm(leaves[0], leaves[3], leaves[4], lin_bias=leaves[2], res=leaves[1], t_valid=tv)
    y.backward(poisoned[2].to(gpu_device))
    got = {"y": y.detach(), "dx": leaves[0].grad, "dres": leaves[1].grad, "dlb": leaves[2].grad, "dw": leaves[3].grad, "db": leaves[4].grad}
    for k in ("y", "dx", "dres"):
        _zeros_on(got[k], pad, k)
    r = [t.double().clone().requires_grad_() for t in (x, res, lb, w, b)]
    from gcgcn_amd import bert as bert_mod
    yr = torch.where(pad[:, :, None], torch.zeros((), dtype=torch.float64), bert_mod.layer_norm(r[0] + r[2] + r[1], r[3], r[4]))
    (yr * dy.double()).sum().backward()
    ref = {"y": yr.detach(), "dx": r[0].grad, "dres": r[1].grad, "dlb": r[2].grad, "dw": r[3].grad, "db": r[4].grad}
    fr = worst(got, ref, f"res_layer_norm with lengths D={D}")
    assert max(fr.values()) <= 1.0, fr

    C = 4 * D
    z, dz = torch.randn(B, T, C, generator=g), torch.randn(B, T, C, generator=g)
    bi = 0.1 * torch.randn(C, generator=g)
    zp, dzp = z.clone(), dz.clone()
    zp[pad], dzp[pad] = NAN, NAN
    zd, dzd, bid = zp.to(gpu_device), dzp.to(gpu_device), bi.to(gpu_device)
    out, dout = torch.full_like(zd, NAN), torch.full_like(zd, NAN)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("gcgcn_bias_gelu_fwd_len", B * T, C, _p(zd), _p(bid), _p(tv), T, _p(out), st)
    _lib.call("gcgcn_bias_gelu_bwd_len", B * T, C, _p(dzd), _p(zd), _p(bid), _p(tv), T, _p(dout), st)
    torch.cuda.synchronize()
    _zeros_on(out, pad, "gelu")
    _zeros_on(dout, pad, "gelu backward")
    zr = (z.double() + bi.double()).requires_grad_()
    gr = torch.where(pad[:, :, None], torch.zeros((), dtype=torch.float64), bert_mod.gelu(zr))
    (gr * dz.double()).sum().backward()
    fr = worst({"g": out, "dz": dout}, {"g": gr.detach(), "dz": zr.grad}, f"bias_gelu with lengths C={C}")
    assert max(fr.values()) <= 1.0, fr


class _Cfg:
    entity_type_size, coref_size, max_length, keep_prob, graph_hop = 20, 20, 512, 1.0, 2
    dis_size, dis_num, dis_plus, relation_num, alpha = 20, 21, 10, 97, 1.0

    def __init__(self, vocab, **kw):
        import numpy as np
        self.data_word_vec = np.zeros((vocab, 100), np.float32)
        self.__dict__.update(kw)


def test_model_wiring_lengths_hip_against_torch(gpu_device):
    """GraphCNN_multihead_bert_gate_cls with t_valid: bert_impl="hip" hands it to the kernels as lengths, bert_impl="torch" computes the
    same contract in plain PyTorch.  The shape, the state and the tolerance of test_bert_gpu.test_model_wiring_hip_against_torch."""
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
    docs = [doc_tensors(g["raw"], di, gpu_device) for di in range(2)]
    batch = {k: torch.stack([d[k] for d in docs]) for k in docs[0]}
    T = batch["document"].shape[1]
    t_valid = torch.tensor([T, max(1, T - 13)], device=gpu_device)
    # (the golden documents fill all T tokens: their sentence and mention matrices point at the second document's last 13 rows too, so
    # the logits agree only if BOTH encoders leave exactly zeros there)
    seen = {}
    hook = twin.bert.register_forward_hook(lambda m, args, kwargs, out: seen.update(kwargs, doc=out[0]), with_kwargs=True)
    with torch.no_grad():
        want = base(**batch, t_valid=t_valid)
        got = twin(**batch, t_valid=t_valid)
    hook.remove()
    assert seen.get("lengths") is t_valid and seen.get("attention_mask") is None       # the lengths went to the kernels
    assert torch.equal(seen["doc"][1, T - 13:], torch.zeros_like(seen["doc"][1, T - 13:]))
    assert torch.isfinite(got).all()
    err = (got - want).abs()
    print(f"bert model with t_valid, hip lengths vs torch mask: max |diff| {err.max().item():.3e}, max |logit| {want.abs().max().item():.3e}")
    torch.testing.assert_close(got, want, rtol=1e-4, atol=2e-4)
