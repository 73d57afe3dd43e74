"""What tests/test_bert_bf16_cpu.py and tests/test_bert_bf16_gpu.py share: the reference of ``matmul="bf16"`` and its bound.  Configs,
seeded parameters, inputs, masks and the bound's FORM are tests/bert_cases.py's and tests/bert_length_cases.py's.

Reference: ``gcgcn_amd.BertModel(impl="torch", matmul="bf16").double()`` on the CPU (one layer: ``bert.torch_layer`` with
``bert.bf16_linear``): every Linear's operands rounded to bfloat16, everything else float64.  Computed once per case (lru_cache);
nobody writes to it.

Bound: |got - ref| <= ATOL * max(1, max|ref|) + RTOL * |ref|, every element.  The constants of bert_cases.py (2e-5, 2e-4) cannot be
taken over: an operand that sits near a bf16 rounding boundary in the float64 run rounds the other way in a float32 run, and that
step is 2^-9 of the element, not 2^-24.  They are set the way bert_cases.py sets its own: the float32 CPU run of ``impl="torch",
matmul="bf16"`` against its float64 run at the sweep's shapes (MODEL_SWEEP x CONFIGS, eval mode, outputs and every gradient) has to
sit at or below 0.1 of the bound -- a tenfold allowance for another summation order on the device, which moves other operands
across their boundaries.  Measured fractions of the bound with ATOL = 4e-2, RTOL = 4e-2
(test_bert_bf16_cpu.test_float32_within_a_tenth_of_the_bound prints them):
  model  D=128 H=2 (3,33): 0.068   (2,130): 0.095      D=192 H=3 (3,33): 0.081   (2,130): 0.071
With (2e-2, 2e-2) the same run sits at 0.14 .. 0.19, above the tenth; with (5e-3, 5e-3) at 0.54 .. 0.76.  The worst tensors are the
gradients of layer 0's query / key / value weights and the pooled output: one flipped rounding in layer 0 is a relative step of
2^-9 .. 2^-8 in one operand element, which the softmax and two LayerNorms behind it spread over whole rows.  A wrong lane map, a
dropped k-step or a missing bias is an error of order one and does not fit in 4e-2 of the tensor's largest element.
The bound is never derived from the HIP path's output."""
import functools

import torch

from gcgcn_amd import bert as bert_mod
from gcgcn_amd.bert import BertModel

from bert_cases import config, model_case, state
from bert_length_cases import layer_len_case, per_document

RTOL, ATOL = 4e-2, 4e-2


def fresh_model(D, H, impl="torch", dtype=torch.float64, device="cpu", p=0.0, matmul="bf16"):
    m = BertModel(config(D, H, 2, p), impl=impl, matmul=matmul)
    m.load_state_dict(state(D, H))
    return m.to(device=device, dtype=dtype)


def run_model(model, case, train=False, override=None):
    """Forward + backward of the 2-layer model on its own device and dtype: {"out0", "out1", "pooled", "d<param name>"...}."""
    q = next(model.parameters())
    dev, dtype = q.device, q.dtype
    model.train(train)
    model.dropout_override = override
    model.zero_grad(set_to_none=True)
    mask = None if case["mask"] is None else case["mask"].to(dev)
    outs, pooled = model(case["ids"].to(dev), case["tt"].to(dev), mask, output_all_encoded_layers=True)
    ((outs[-1] * case["dy"].to(device=dev, dtype=dtype)).sum() + (pooled * case["dp"].to(device=dev, dtype=dtype)).sum()).backward()
    res = {f"out{i}": o.detach() for i, o in enumerate(outs)}
    res["pooled"] = pooled.detach()
    res.update({"d" + n: q.grad for n, q in model.named_parameters()})
    return res


@functools.lru_cache(maxsize=None)
def model_reference(D, H, B, T, kind="prefix"):
    return run_model(fresh_model(D, H), model_case(D, H, B, T, kind))


@functools.lru_cache(maxsize=None)
def model_len_reference(D, H, B, T, lengths):
    """Every document alone at its own length (bert_length_cases.per_document) with the bf16 Linears."""
    return per_document(fresh_model(D, H), model_case(D, H, B, T), lengths)


def layer_torch(x, kb, params, H, dy, dtype=torch.float64, drop=lambda s, t: t):
    """One layer of the definition: {"y", "dx", "d00" .. "d15"}."""
    x = x.to(dtype).clone().requires_grad_()
    ps = [t.to(dtype).clone().requires_grad_() for t in params]
    y = bert_mod.torch_layer(x, None if kb is None else kb.to(dtype), ps, H, drop, bert_mod.bf16_linear)
    (y * dy.to(dtype)).sum().backward()
    res = {"y": y.detach(), "dx": x.grad}
    res.update({f"d{i:02d}": t.grad for i, t in enumerate(ps)})
    return res


@functools.lru_cache(maxsize=None)
def layer_len_reference(D, H, B, T, lengths):
    """bert_length_cases.layer_len_reference with the bf16 Linears: every document alone, truncated, no mask."""
    c = layer_len_case(D, H, B, T, lengths)
    ps = [t.double().clone().requires_grad_() for t in c["params"]]
    y, dx = torch.zeros(B, T, D, dtype=torch.float64), torch.zeros(B, T, D, dtype=torch.float64)
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        x = c["x"][b:b + 1, :n].double().clone().requires_grad_()
        yb = bert_mod.torch_layer(x, None, ps, H, lambda s, t: t, bert_mod.bf16_linear)
        (yb * c["dy"][b:b + 1, :n].double()).sum().backward()
        y[b, :n], dx[b, :n] = yb[0].detach(), x.grad[0]
    res = {"y": y, "dx": dx}
    res.update({f"d{i:02d}": (t.grad if t.grad is not None else torch.zeros_like(t)) for i, t in enumerate(ps)})
    return res


def frac_of_bound(got, ref):
    """Largest |got - ref| as a fraction of the bound (<= 1 passes); NaN / inf anywhere gives inf."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if not torch.isfinite(got).all():
        return float("inf")
    bound = ATOL * max(1.0, ref.abs().max().item()) + RTOL * ref.abs()
    return ((got - ref).abs() / bound).max().item()


def worst(got, ref, label):
    """Prints the case's largest error as a fraction of the bound, per tensor, and returns {name: fraction}."""
    fr = {k: frac_of_bound(got[k], ref[k]) for k in ref}
    k = max(fr, key=fr.get)
    print(f"{label}: worst {fr[k]:.3f} of the bound ({k}); " + " ".join(f"{n}={v:.3f}" for n, v in sorted(fr.items(), key=lambda kv: -kv[1])[:6]))
    return fr
