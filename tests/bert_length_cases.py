"""What tests/test_bert_lengths_cpu.py and tests/test_bert_lengths_gpu.py share: the per-document reference of the token-length
contract and the runs it is compared with.  Configs, seeded parameters, inputs and the bound are
tests/bert_cases.py's.

Reference: the float64 ``impl="torch"`` model, layer or attention core on the CPU, run on each document ALONE, truncated to
``lengths[b]`` tokens, with no mask; outputs scattered into zero tensors of the padded shape, parameter gradients summed over the
documents.  A document of length 0 has no token to run: its rows are zeros, ``pooled = tanh(pooler bias)``, and only that bias takes
a gradient from it.  Computed once per case (lru_cache); nobody writes to it."""
import functools

import torch

from gcgcn_amd import bert as bert_mod
from gcgcn_amd.bert import BertModel

from bert_cases import attn_ref, config, model_case, state

NAN = float("nan")


def pad_mask(lengths, T):
    """[B,T] bool, True on padding rows."""
    return torch.arange(T)[None, :] >= torch.tensor(lengths)[:, None]


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def fresh_model(D, H, impl="torch", dtype=torch.float64, device="cpu", p=0.0):
    m = BertModel(config(D, H, 2, p), impl=impl)
    m.load_state_dict(state(D, H))
    return m.to(device=device, dtype=dtype)


def per_document(model, case, lengths):
    """{"out0", "out1", "pooled", "d<name>"} of ``model`` (float64, eval) on every document alone at its own length."""
    B, T = case["ids"].shape
    D = case["dy"].shape[-1]
    outs = [torch.zeros(B, T, D, dtype=torch.float64) for _ in model.encoder.layer]
    pooled = torch.zeros(B, D, dtype=torch.float64)
    model.eval()
    model.zero_grad(set_to_none=True)
    for b, n in enumerate(lengths):
        if n == 0:      # no token to encode: the pooler sees a zero row, so only its bias takes a gradient from this document
            p = torch.tanh(model.pooler.dense.bias)
            (p * case["dp"][b].double()).sum().backward()
            pooled[b] = p.detach()
            continue
        o, p = model(case["ids"][b:b + 1, :n], case["tt"][b:b + 1, :n])
        ((o[-1] * case["dy"][b:b + 1, :n].double()).sum() + (p * case["dp"][b:b + 1].double()).sum()).backward()   # gradients accumulate
        for i, t in enumerate(o):
            outs[i][b, :n] = t[0].detach()
        pooled[b] = p[0].detach()
    res = {f"out{i}": t for i, t in enumerate(outs)}
    res["pooled"] = pooled
    res.update({"d" + k: (q.grad.clone() if q.grad is not None else torch.zeros_like(q)) for k, q in model.named_parameters()})
    return res


@functools.lru_cache(maxsize=None)
def model_len_reference(D, H, B, T, lengths):
    return per_document(fresh_model(D, H), model_case(D, H, B, T), lengths)


def run_with_lengths(model, case, lengths, nan_pad=True, train=False, override=None, mask=None, lengths_arg=True):
    """Forward + backward of ``model`` on its own device and dtype with ``lengths=`` (or, lengths_arg=False, with ``attention_mask=mask``).
    nan_pad: the cotangent of the last layer's output is NaN on every padding row; otherwise zero there."""
    q = next(model.parameters())
    dev, dtype = q.device, q.dtype
    B, T = case["ids"].shape
    pad = pad_mask(lengths, T)
    dy = case["dy"].to(dtype).clone()
    dy[pad] = NAN if nan_pad else 0.0
    model.train(train)
    model.dropout_override = override
    model.zero_grad(set_to_none=True)
    ids, tt = case["ids"].to(dev), case["tt"].to(dev)
    if lengths_arg:
        outs, pooled = model(ids, tt, None if mask is None else mask.to(dev), lengths=torch.tensor(lengths, dtype=torch.int32, device=dev))
    else:
        outs, pooled = model(ids, tt, mask.to(dev))
    ((outs[-1] * dy.to(dev)).sum() + (pooled * case["dp"].to(device=dev, dtype=dtype)).sum()).backward()
    res = {f"out{i}": t.detach() for i, t in enumerate(outs)}
    res["pooled"] = pooled.detach()
    res.update({"d" + k: p.grad for k, p in model.named_parameters()})
    return res


# ---- one layer ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layer_len_case(D, H, B, T, lengths):
    """x (zero on padding rows: the layer's contract), the cotangent dy, the layer's 16 tensors."""
    g = torch.Generator().manual_seed(3 * B + 5 * T + D + sum(lengths))
    x, dy = torch.randn(B, T, D, generator=g), torch.randn(B, T, D, generator=g)
    x[pad_mask(lengths, T)] = 0.0
    model = BertModel(config(D, H))
    model.load_state_dict(state(D, H))
    return {"x": x, "dy": dy, "params": [t.detach() for t in model.encoder.layer[0].tensors()]}


@functools.lru_cache(maxsize=None)
def layer_len_reference(D, H, B, T, lengths):
    c = layer_len_case(D, H, B, T, lengths)
    ps = [t.double().clone().requires_grad_() for t in c["params"]]
    y, dx = torch.zeros(B, T, D, dtype=torch.float64), torch.zeros(B, T, D, dtype=torch.float64)
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        x = c["x"][b:b + 1, :n].double().clone().requires_grad_()
        yb = bert_mod.torch_layer(x, None, ps, H, lambda s, t: t)
        (yb * c["dy"][b:b + 1, :n].double()).sum().backward()
        y[b, :n], dx[b, :n] = yb[0].detach(), x.grad[0]
    res = {"y": y, "dx": dx}
    res.update({f"d{i:02d}": (t.grad if t.grad is not None else torch.zeros_like(t)) for i, t in enumerate(ps)})
    return res


# ---- the attention core ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def attn_len_case(B, T, H, holes=False):
    g = torch.Generator().manual_seed(77 + 7 * B + 13 * T + H)
    c = {"qkv": torch.randn(B, T, 3 * H * 64, generator=g), "dctx": torch.randn(B, T, H * 64, generator=g), "key_bias": None}
    if holes:   # masked keys INSIDE the live prefixes: every third key of document 0 from key 1 on, one key of document 1
        kb = torch.zeros(B, T)
        kb[0, 1::3] = -10000.0
        kb[1, 5] = -10000.0
        c["key_bias"] = kb
    return c


@functools.lru_cache(maxsize=None)
def attn_len_reference(B, T, H, lengths, holes=False):
    """{"ctx", "lse", "dqkv"} float64 in the padded shapes, zeros on padding rows; lse is the row's full log-sum-exp."""
    c = attn_len_case(B, T, H, holes)
    D = H * 64
    ref = {"ctx": torch.zeros(B, T, D, dtype=torch.float64), "lse": torch.zeros(B, H, T, dtype=torch.float64),
           "dqkv": torch.zeros(B, T, 3 * D, dtype=torch.float64)}
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        sub = {k: (None if v is None else v[b:b + 1, :n]) for k, v in c.items()}
        r = attn_ref(sub, H, torch.float64)
        ref["ctx"][b, :n], ref["lse"][b, :, :n], ref["dqkv"][b, :n] = r["ctx"][0], r["lse"][0], r["dqkv"][0]
    return ref
