"""attention="bf16" on the device: the attention core of csrc/bert_attn_bf16.hip (the four products on v_mfma_f32_16x16x32_bf16) against
the float64 CPU run of the definition, ``gcgcn_amd.bert.Bf16AttentionFn``, under the bounds of tests/bert_attn_bf16_cases.py.

Block edges of the kernels: a workgroup owns 64 rows, one wave 16 of them, and streams the other side in blocks of 64.  ATTN_T: 1, 15 /
16 / 17 (either side of a wave's edge), 33 (three waves, the last with one row), 63 / 64 / 65 (either side of the workgroup's and the
streamed block's edge), 130 (three blocks, the last with two rows), 512 (the largest T served).  The suite runs on NaN-poisoned free
memory (conftest.py)."""
import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib, functional as Fn, models as M
from gcgcn_amd.bert import BertModel

import bert_attn_bf16_cases as C
from bert_cases import CONFIGS, MODEL_SWEEP, attn_case, attn_ref, config, model_case, state
from bert_length_cases import NAN, attn_len_case, layer_len_case, pad_mask, run_with_lengths

pytestmark = pytest.mark.gpu


def _p(t):
    return None if t is None else t.data_ptr()


def _core(case, H, dev, attn, snap=None, p=0.0, guard=NAN, lengths=None, nan_dctx=False):
    """The core through gcgcn_bert_attn_fwd_mx / _bwd_mx.  Every buffer carries one guard document past its end, filled with `guard`;
    the outputs are NaN-filled before the call.  Returns ({"ctx", "lse" (as stored, relative to c_b), "dqkv"}, the outputs' guards)."""
    B, T, D3 = case["qkv"].shape
    D = D3 // 3

    def padded(t, fill):
        buf = torch.full((B + 1,) + tuple(t.shape[1:]), fill, device=dev)
        buf[:B] = t.to(dev)
        return buf

    dctx = case["dctx"].clone()
    if nan_dctx:
        dctx[pad_mask(lengths, T)] = NAN
    qkv, dctx = padded(case["qkv"], guard), padded(dctx, guard)
    kb = None if case["key_bias"] is None else padded(case["key_bias"], guard)
    tv = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    ctx, dqkv = torch.full((B + 1, T, D), NAN, device=dev), torch.full((B + 1, T, 3 * D), NAN, device=dev)
    lse, delta = torch.full((B + 1, H, T), NAN, device=dev), torch.full((B + 1, H, T), NAN, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    salt = _lib.SALT_BERT_ATTN
    _lib.call("gcgcn_bert_attn_fwd_mx", B, T, H, 64, _p(qkv), _p(kb), _p(tv), _p(ctx), _p(lse), _p(snap), salt, p, st, attn)
    _lib.call("gcgcn_bert_attn_bwd_mx", B, T, H, 64, _p(qkv), _p(kb), _p(tv), _p(ctx), _p(lse), _p(dctx), _p(dqkv), _p(delta), _p(snap), salt,
              p, st, attn)
    torch.cuda.synchronize()
    return {"ctx": ctx[:B], "lse": lse[:B], "dqkv": dqkv[:B]}, (ctx[B], lse[B], dqkv[B], delta[B])


def _full_lse(got, case, lengths=None):
    """The kernels store lse relative to c_b, the largest penalty of the document's (live) keys: the row's log-sum-exp is lse + c_b."""
    out = dict(got)
    lse = got["lse"].double().cpu()
    kb = case["key_bias"]
    if kb is not None:
        for b in range(kb.shape[0]):
            n = kb.shape[1] if lengths is None else lengths[b]
            if n:
                lse[b, :, :n] += kb[b, :n].max().double()
    out["lse"] = lse
    return out


# ---- 1. the core against the float64 definition ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", C.KINDS)
@pytest.mark.parametrize("B,T", C.ATTN_T)
def test_core_against_float64_definition(gpu_device, B, T, kind):
    """ctx, lse, dq | dk | dv within the core bound; the guard document behind every output stays NaN, everything inside is finite, and
    the results do not depend on what lies behind the inputs' end (NaN or 1.0)."""
    H = 2
    case = attn_case(B, T, H, kind)
    got, guards = _core(case, H, gpu_device, 1)
    for g in guards:
        assert torch.isnan(g).all()
    for k, v in got.items():
        assert torch.isfinite(v).all(), k
    fr = C.core_worst(_full_lse(got, case), C.attn_reference(B, T, H, kind), f"bf16 core B={B} T={T} {kind}")
    assert max(fr.values()) <= 1.0, fr
    again, _ = _core(case, H, gpu_device, 1, guard=1.0)
    for k in got:
        assert torch.equal(got[k], again[k]), k


# ---- 2. the discriminating case ----------------------------------------------------------------------------------------------------------
def test_discriminating_case_on_the_device(gpu_device):
    """Inputs on which bf16 and fp32 operands differ at order one: attn = 1 is inside the core bound, attn = 0 of the same call outside
    it on at least half the elements of ctx and of dqkv."""
    H = 2
    case = C.discriminating_case(H=H)
    ref = C.attn_def(case, H, torch.float64)
    got, _ = _core(case, H, gpu_device, 1)
    fr = C.core_worst(got, ref, "discriminating case, attn = 1")
    assert max(fr.values()) <= 1.0, fr
    fp, _ = _core(case, H, gpu_device, 0)
    for k in ("ctx", "dqkv"):
        share = C.share_outside(fp[k], ref[k])
        print(f"discriminating case, attn = 0: {share:.3f} of {k} outside the core bound")
        assert share >= 0.5, (k, share)


# ---- 3. dropout --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_core_dropout_replays_the_mask(gpu_device, p):
    """The keep mask regenerated from the snapshot and replayed in the float64 definition matches the device run; attn = 0 draws the
    same mask (its run matches the fp32 definition with that mask under the fp32 tests' bound)."""
    from bert_cases import worst as fp32_worst
    B, T, H = 3, 65, 3
    case = attn_case(B, T, H, "prefix")
    gcgcn_amd.manual_seed(11)
    snap = Fn.rng_snapshot(gpu_device)
    keep = Fn.dropout_keep_mask(snap, _lib.SALT_BERT_ATTN, p, B * H * T * T).view(B, H, T, T).cpu()
    assert 0.6 * (1 - p) < keep.float().mean().item() < min(1.0, 1.4 * (1 - p))
    got, _ = _core(case, H, gpu_device, 1, snap=snap, p=p)
    fr = C.core_worst(_full_lse(got, case), C.attn_def(case, H, torch.float64, keep=keep, scale=1.0 / (1.0 - p)), f"bf16 core, dropout p={p}")
    assert max(fr.values()) <= 1.0, fr
    fp, _ = _core(case, H, gpu_device, 0, snap=snap, p=p)
    fr = fp32_worst(_full_lse(fp, case), attn_ref(case, H, torch.float64, keep=keep, scale=1.0 / (1.0 - p)), f"fp32 core, same mask p={p}")
    assert max(fr.values()) <= 1.0, fr


# ---- 4. token lengths, core ------------------------------------------------------------------------------------------------------------
def _zeros_on(t, pad, name):
    rows = t[pad.to(t.device)]
    assert torch.equal(rows, torch.zeros_like(rows)), f"{name}: padding rows are not exactly zero"


@pytest.mark.parametrize("B,T,lengths,holes", C.LEN_CASES)
def test_core_lengths_against_per_document_float64(gpu_device, B, T, lengths, holes):
    H = 2
    case = attn_len_case(B, T, H, holes)
    got, guards = _core(case, H, gpu_device, 1, lengths=lengths, nan_dctx=True)
    for g in guards:
        assert torch.isnan(g).all()
    pad = pad_mask(lengths, T)
    _zeros_on(got["ctx"], pad, "ctx")
    _zeros_on(got["dqkv"], pad, "dqkv")
    _zeros_on(got["lse"].transpose(1, 2), pad, "lse")
    fr = C.core_worst(_full_lse(got, case, lengths), C.attn_len_reference(B, T, H, lengths, holes), f"bf16 core, lengths {lengths} of T={T}")
    assert max(fr.values()) <= 1.0, fr


# ---- 5. one layer ----------------------------------------------------------------------------------------------------------------------
def _layer_inputs(D, H, B, T, kind):
    case = model_case(D, H, B, T, kind)
    g = torch.Generator().manual_seed(B + T + D)
    x = torch.randn(B, T, D, generator=g)
    model = BertModel(config(D, H))
    model.load_state_dict(state(D, H))
    params = [t.detach() for t in model.encoder.layer[0].tensors()]
    kb = None if case["mask"] is None else (1.0 - case["mask"]) * -10000.0
    return case, x, params, kb


def _layer_hip(x, kb, params, dy, dev, matmul, **kw):
    x = x.to(dev).requires_grad_()
    ps = [t.to(dev).requires_grad_() for t in params]
    y = Fn.bert_layer(x, None if kb is None else kb.to(dev), *ps, matmul=matmul, attention="bf16", **kw)
    y.backward(dy.to(dev))
    res = {"y": y.detach(), "dx": x.grad}
    res.update({f"d{i:02d}": t.grad for i, t in enumerate(ps)})
    return res


@pytest.mark.parametrize("matmul", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["none", "prefix", "holes"])
@pytest.mark.parametrize("D,H,B,T", [(128, 2, 3, 33), (192, 3, 2, 130)])
def test_layer_against_float64_definition(gpu_device, D, H, B, T, kind, matmul):
    case, x, params, kb = _layer_inputs(D, H, B, T, kind)
    ref = C.layer_torch(x, kb, params, H, case["dy"], matmul)
    got = _layer_hip(x, kb, params, case["dy"], gpu_device, matmul)
    fr = C.worst(got, ref, f"layer attention=bf16 matmul={matmul} D={D} H={H} ({B},{T}) {kind}", matmul)
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize("matmul", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,lengths,rowblk", [(3, 48, (48, 0, 17), False), (3, 48, (48, 0, 17), True), (4, 64, (64, 33, 16, 0), False),
                                                (4, 64, (64, 33, 16, 0), True)])
def test_layer_lengths_against_per_document_float64(gpu_device, B, T, lengths, rowblk, matmul):
    D, H = 128, 2
    c = layer_len_case(D, H, B, T, lengths)
    tv = torch.tensor(lengths, dtype=torch.int32, device=gpu_device)
    dy = c["dy"].clone()
    pad = pad_mask(lengths, T)
    dy[pad] = NAN
    got = _layer_hip(c["x"], None, c["params"], dy, gpu_device, matmul, t_valid=tv, rowblk=Fn.row_blocks(tv, B, T) if rowblk else None)
    _zeros_on(got["y"], pad, "y")
    _zeros_on(got["dx"], pad, "dx")
    fr = C.worst(got, C.layer_len_reference(D, H, B, T, lengths, matmul), f"layer attention=bf16 matmul={matmul}, lengths {lengths} of T={T}",
                 matmul)
    assert max(fr.values()) <= 1.0, fr


# ---- 6. the 2-layer model ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matmul", ["fp32", "bf16"])
@pytest.mark.parametrize("D,H", sorted(CONFIGS))
@pytest.mark.parametrize("B,T", MODEL_SWEEP)
def test_model_eval_against_float64_definition(gpu_device, D, H, B, T, matmul):
    model = C.fresh_model(D, H, impl="hip", dtype=torch.float32, device=gpu_device, matmul=matmul)
    got = C.run_model(model, model_case(D, H, B, T))
    fr = C.worst(got, C.model_reference(D, H, B, T, matmul), f"model attention=bf16 matmul={matmul} D={D} H={H} ({B},{T})", matmul)
    assert max(fr.values()) <= 1.0, fr


def _replay(model, p):
    """dropout_override for the float64 reference: the masks the device drew (multiplicative, as attention="bf16" requires)."""
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
    fr = C.worst(got, ref, f"model attention=bf16 train p={p}", "fp32")
    assert max(fr.values()) <= 1.0, fr


def test_model_lengths_against_per_document_float64(gpu_device):
    D, H, B, T, lengths = 128, 2, 4, 64, (64, 33, 16, 0)
    case = dict(model_case(D, H, B, T))
    pad = pad_mask(lengths, T)
    case["ids"] = torch.where(pad, (case["ids"] + 7) % 61, case["ids"])
    model = C.fresh_model(D, H, impl="hip", dtype=torch.float32, device=gpu_device)
    got = run_with_lengths(model, case, lengths)
    for k in ("out0", "out1"):
        _zeros_on(got[k], pad, k)
    fr = C.worst(got, C.model_len_reference(D, H, B, T, lengths, "fp32"), f"model attention=bf16, lengths {lengths} of T={T}", "fp32")
    assert max(fr.values()) <= 1.0, fr


class _Cfg:
    entity_type_size, coref_size, max_length, keep_prob, graph_hop = 20, 20, 512, 1.0, 2
    dis_size, dis_num, dis_plus, relation_num, alpha = 20, 21, 10, 97, 1.0

    def __init__(self, vocab, **kw):
        import numpy as np
        self.data_word_vec = np.zeros((vocab, 100), np.float32)
        self.__dict__.update(kw)


def test_graph_model_hip_against_torch_definition(gpu_device):
    """GraphCNN_multihead_bert_gate_cls with bert_impl="hip" against "torch", both with bert_attention="bf16", on the device."""
    from conftest import golden_files, load_golden
    from lstm_cases import doc_tensors
    g = load_golden(golden_files("model_step")[0])
    vocab = g["meta"]["vocab"]
    bc = config(128, 2)
    bc.vocab_size = vocab
    torch.manual_seed(5)
    base = M.GraphCNN_multihead_bert_gate_cls(_Cfg(vocab, bert_impl="torch", bert_attention="bf16", bert_config=bc)).to(gpu_device).eval()
    twin = M.GraphCNN_multihead_bert_gate_cls(_Cfg(vocab, bert_impl="hip", bert_attention="bf16", bert_config=bc)).to(gpu_device).eval()
    assert twin.bert.attention == "bf16" and twin.bert.matmul == "fp32" and twin.bert.impl == "hip"
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
    print(f"bert graph model, attention=bf16: hip vs torch {C.frac_of_bound(got, want, 'fp32'):.3f} of the bound")
    assert C.frac_of_bound(got, want, "fp32") <= 1.0
    grads = [q.grad for q in twin.bert.encoder.parameters()]
    assert all(t is not None and torch.isfinite(t).all() for t in grads)


# ---- 7. determinism and capture ------------------------------------------------------------------------------------------------------
def test_two_runs_from_one_seed_are_bitwise_equal(gpu_device):
    D, H, B, T = 192, 3, 2, 130
    case = model_case(D, H, B, T)
    runs = []
    for _ in range(2):
        gcgcn_amd.manual_seed(21)
        runs.append(C.run_model(C.fresh_model(D, H, impl="hip", dtype=torch.float32, device=gpu_device, p=0.1), case, train=True))
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def _capture(step):
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
    return graph


def test_graph_replay_matches_eager(gpu_device):
    """A captured forward + backward (train mode, p = 0.1) replayed twice equals two eager steps from the same generator state."""
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
    graph = _capture(step)
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


def test_captured_step_replays_on_new_lengths(gpu_device):
    """A captured core step (functional.bert_attention, forward + backward) replayed after t_valid.copy_(other) equals the eager run
    on `other`: the grids do not depend on the lengths and nothing is read on the host."""
    B, T, H = 4, 64, 2
    case = attn_len_case(B, T, H)
    qkv = case["qkv"].to(gpu_device).requires_grad_()
    dctx = case["dctx"].to(gpu_device)
    tv = torch.tensor((64, 33, 16, 0), dtype=torch.int32, device=gpu_device)
    other = torch.tensor((17, 64, 0, 48), dtype=torch.int32, device=gpu_device)
    out = {}

    def step():
        qkv.grad = None
        y = Fn.bert_attention(qkv, None, H, t_valid=tv, attention="bf16")
        y.backward(dctx)
        out["y"] = y

    graph = _capture(step)
    live_y, live_g = out["y"], qkv.grad
    tv.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    ry, rg = live_y.detach().clone(), live_g.detach().clone()
    step()
    torch.cuda.synchronize()
    assert torch.equal(out["y"], ry) and torch.equal(qkv.grad, rg)
    assert not torch.equal(ry[0, 17:], torch.ones_like(ry[0, 17:])) and torch.equal(ry[0, 17:], torch.zeros_like(ry[0, 17:]))


# ---- 8. attn = 0 is the code that was there ----------------------------------------------------------------------------------------------
def test_attn_0_through_mx_is_bitwise_the_older_symbols(gpu_device):
    B, T, H, lengths = 3, 48, 2, (48, 17, 1)
    case = attn_len_case(B, T, H, True)
    dev = gpu_device
    got, _ = _core(case, H, dev, 0, lengths=lengths)
    qkv, dctx, kb = case["qkv"].to(dev), case["dctx"].to(dev), case["key_bias"].to(dev)
    tv = torch.tensor(lengths, dtype=torch.int32, device=dev)
    ctx, dqkv = torch.full((B, T, H * 64), NAN, device=dev), torch.full((B, T, 3 * H * 64), NAN, device=dev)
    lse, delta = torch.full((B, H, T), NAN, device=dev), torch.full((B, H, T), NAN, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("gcgcn_bert_attn_fwd_len", B, T, H, 64, _p(qkv), _p(kb), _p(tv), _p(ctx), _p(lse), None, 0, 0.0, st)
    _lib.call("gcgcn_bert_attn_bwd_len", B, T, H, 64, _p(qkv), _p(kb), _p(tv), _p(ctx), _p(lse), _p(dctx), _p(dqkv), _p(delta), None, 0, 0.0, st)
    torch.cuda.synchronize()
    assert torch.equal(got["ctx"], ctx) and torch.equal(got["lse"], lse) and torch.equal(got["dqkv"], dqkv)
    # the layer: _mx with attn = 0 against _mm, both matmul settings, through the autograd function's two calls
    D, Hh, Bl, Tl = 128, 2, 3, 33
    cs, x, params, kbl = _layer_inputs(D, Hh, Bl, Tl, "holes")
    ps = [t.to(dev) for t in params]
    wqkv, bqkv = torch.cat([ps[0], ps[2], ps[4]], 0), torch.cat([ps[1], ps[3], ps[5]], 0)
    plist = [wqkv, bqkv] + ps[6:]
    xd, kbd, dy = x.to(dev), kbl.to(dev), cs["dy"].to(dev)
    dims = (Bl, Tl, D, Hh, 4 * D)
    for mm in (0, 1):
        outs = []
        for name, extra in (("mm", (mm,)), ("mx", (mm, 0))):
            saved = Fn._f32_buf(Fn._bytes_or_raise("gcgcn_bert_layer_ws_bytes", *dims, 0), dev)
            ws = Fn._f32_buf(Fn._bytes_or_raise("gcgcn_bert_layer_ws_bytes", *dims, 1), dev)
            y, dx = torch.empty_like(xd), torch.empty_like(xd)
            grads = [torch.empty_like(t) for t in plist]
            _lib.call(f"gcgcn_bert_layer_fwd_{name}", *dims, _p(xd), _p(kbd), None, None, Fn._ptr_array(plist), _p(y), _p(saved),
                      saved.numel() * 4, None, 0.0, 0.0, st, *extra)
            _lib.call(f"gcgcn_bert_layer_bwd_{name}", *dims, _p(xd), _p(kbd), None, None, Fn._ptr_array(plist), _p(saved), saved.numel() * 4,
                      _p(dy), _p(dx), Fn._ptr_array(grads), _p(ws), ws.numel() * 4, None, 0.0, 0.0, st, *extra)
            torch.cuda.synchronize()
            outs.append([y, dx] + grads)
        for a, b in zip(*outs):
            assert torch.equal(a, b)


# ---- 9. functional.bert_attention ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("attention", ["fp32", "bf16"])
@pytest.mark.parametrize("B,T,kind", [(3, 33, "holes"), (3, 130, "prefix")])
def test_functional_bert_attention_agrees_with_the_c_abi(gpu_device, B, T, kind, attention):
    H = 2
    case = attn_case(B, T, H, kind)
    want, _ = _core(case, H, gpu_device, Fn.BERT_ATTENTIONS.index(attention))
    qkv = case["qkv"].to(gpu_device).requires_grad_()
    kb = None if case["key_bias"] is None else case["key_bias"].to(gpu_device)
    y = Fn.bert_attention(qkv, kb, H, attention=attention)
    y.backward(case["dctx"].to(gpu_device))
    assert torch.equal(y, want["ctx"]) and torch.equal(qkv.grad, want["dqkv"])
