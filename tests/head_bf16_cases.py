"""What tests/test_head_bf16_cpu.py and tests/test_head_bf16_gpu.py share about ``classifier_head(..., matmul="bf16")`` (csrc/head_bf16.hip):
the float64 reference built on the definition ``gcgcn_amd.functional.Bf16HeadBilinearFn``, the derived per-pass bound, the end-to-end
bound and the C-ABI harness.  Inputs are tests/test_head_edges_gpu.make_case's (float32 masters on the CPU).

PER PASS.  A pass is a sum of K exact products of bf16 operands, accumulated in fp32 in some order, so against the float64 sum of the
SAME rounded operands its error is at most ``2^-23 (K + 2) (sum |A^||B^| + |bias|)`` per element (gemm_bf16_cases.py has the argument;
the two extra roundings are the bias add and the store).  K = 128^2 + 256 forward, 128 R + R for d eh / d et, P (the pairs) for the
weight gradients.  The operands must be the device's own: eh / et are read back from the forward workspace (a tanh that differs in
the last bit would flip bf16 roundings, 2^-9 of a term each), dout is the test's cotangent.  d eh / d et are observable only after the
fp32 tanh backward, in place: ``g = fl(d * fl(1 - h^2))``; with ``f = 1 - h^2`` exact, ``|fl-factor - f| <= 2^-23`` whether or not the
compiler contracts the factor, so ``|g - ref f| <= bound |f| + 2^-22 (bound + |ref|)`` -- that is what pass_fractions applies.

THE UNROUNDED HEAD MUST FAIL.  The same operands multiplied WITHOUT the rounding (the fp32 head) differ from the reference by about
2^-9 of a term, summed like a random walk: about ``2^-9 sqrt(sum (a b)^2)`` against a bound of ``2^-23 (K + 2) sum |a b|``.  Where K is
small the bound is far smaller and nearly every element violates it: the weight gradients (K = P <= 432 here).  Where K = 16 642 (the
forward pass) the bound is as large as the rounding itself and the fp32 head passes it -- no per-pass bound of this form can tell
the two apart there, and the same holds for d eh / d et at R = 33 and more (K >= 4 257).  So the share is asserted where the bound
separates (``separating``): on d bili_layer_01.weight and d classification_layer_01.weight at every shape, and on d eh / d et at
R = 1 (K = 129).  Measured on the CPU (test_head_bf16_cpu.test_unrounded_head_violates_the_bound_where_it_separates): >= 0.95 of
the elements wherever it is asserted; asserted > 0.5.  The other shares are printed.

END TO END (logits and every gradient of the whole head against the per-document float64 definition): ``c max(1, max|ref|) + c |ref|``
with ``C_E2E`` below.  Not derived: the device's eh / et differ from the reference's in the last bits, which flips bf16 roundings, so
the bound is set from the float32 CPU run of the definition against its float64 run (test_head_bf16_cpu prints the fractions;
DESIGN.md section 8.3 records them next to the device's).
"""
import ctypes
import functools

import torch

from gcgcn_amd import _lib, functional as F_, params as P_
from test_head_edges_gpu import HW, case_id, make_case   # noqa: F401  (re-exported)

U23 = 2.0 ** -23
# The float32 CPU run of the definition sits at 0.16 of this bound at worst (d bili_layer_01.weight at B, N, R = 1, 9, 96; logits
# and the feature gradients below 0.02) -- test_head_bf16_cpu.test_float32_definition_is_well_inside_the_end_to_end_bound asserts
# a quarter.  The BERT bf16 suite's constant for the same form is 4e-2: this one is eight times tighter.
C_E2E = 5e-3
NAN = float("nan")
ANNOUNCE = b"head_matmul"   # gcgcn_set_option(ANNOUNCE, v): the matmul argument of this thread's next head call (include/gcgcn.h)
PARAM_KEYS = tuple(P_.HEAD_STATE_ORDER)
BIL_KEYS = ("bili_layer_01.weight", "classification_layer_01.weight")


def separating(R):
    """The passes whose derived bound the unrounded fp32 head must break at this R (the module docstring has the reason)."""
    return tuple("d " + k for k in BIL_KEYS) + (("d eh", "d et") if R == 1 else ())


def identity(t):
    return t


# ------------------------------------------------------------------------------------------------------
# the definition as a whole head
# ------------------------------------------------------------------------------------------------------
def pair_features(node_feats, node_type, rel, sd, dis_plus):
    """eh, et [n, n, 128] of one document: the unchanged part of the head (GCGCN_glove.py:306-307, 344-355)."""
    n = node_type.shape[0]
    x = torch.cat(list(node_feats) + [torch.nn.functional.embedding(node_type, sd["ner_emb.weight"], padding_idx=0)], 1)
    dis = sd["dis_embed.weight"]
    w, b = sd["dense_layer.weight"], sd["dense_layer.bias"]
    eh = torch.tanh(torch.cat([x.unsqueeze(0).expand(n, -1, -1), dis[dis_plus + rel]], -1) @ w.t() + b)
    et = torch.tanh(torch.cat([x.unsqueeze(1).expand(-1, n, -1), dis[dis_plus - rel]], -1) @ w.t() + b)
    return eh, et


def definition_head(node_feats, node_type, rel, sd, dis_plus, rnd=None):
    """One document's logits [n, n, R] with the bilinear passes of Bf16HeadBilinearFn (rnd = identity: the exact head)."""
    n = node_type.shape[0]
    eh, et = pair_features(node_feats, node_type, rel, sd, dis_plus)
    bias = sd["bili_layer_01.bias"] + sd["classification_layer_01.bias"]
    out = F_.Bf16HeadBilinearFn.apply(eh.reshape(n * n, HW), et.reshape(n * n, HW), sd["bili_layer_01.weight"],
                                      sd["classification_layer_01.weight"], bias, rnd)
    return out.reshape(n, n, -1)


def reference(c, dtype=torch.float64, head=definition_head):
    """-> {"logits" (zero on padding pairs), "d f<k>", "d <parameter / table>"}, per document on the real slices, gradients by
    autograd with the case's cotangent (the layout of tests/test_head_edges_gpu.reference)."""
    cast = lambda t: t.detach().to(dtype)
    sd = {k: cast(v).requires_grad_() for k, v in c.sd.items()}
    feats = [cast(f).requires_grad_() for f in c.feats]
    cot = cast(c.cot)
    logits = torch.zeros(c.B, c.N, c.N, c.R, dtype=dtype)
    for b, n in enumerate(c.ns):
        if n == 0:
            continue
        out = head([f[b, :n] for f in feats], c.ntype[b, :n], c.rel[b, :n, :n], sd, c.dis_plus)
        (out * cot[b, :n, :n]).sum().backward()
        logits[b, :n, :n] = out.detach()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    ref = {"logits": logits}
    ref.update({f"d f{k}": zero(f) for k, f in enumerate(feats)})
    ref.update({"d " + k: zero(v) for k, v in sd.items()})
    return ref


@functools.lru_cache(maxsize=None)
def _cached(key):
    c = make_case(*key[:3], nv=key[3], nf=key[4])
    return c, reference(c)


def case_and_ref(B, N, R, nv=None, nf=3):
    """One case and its float64 reference, computed once and shared (never modified)."""
    return _cached((B, N, R, None if nv is None else tuple(nv), nf))


def e2e_fractions(got, ref, c=C_E2E):
    """Per tensor: the largest |got - ref| / (c max(1, max|ref|) + c |ref|); a NaN counts as infinite."""
    res = {}
    for k, r in ref.items():
        r = r.detach().double()
        a = got[k].detach().cpu().double()
        assert a.shape == r.shape, f"{k}: shape {tuple(a.shape)} != {tuple(r.shape)}"
        bound = c * max(1.0, r.abs().max().item()) + c * r.abs()
        res[k] = torch.nan_to_num((a - r).abs() / bound, nan=float("inf")).max().item() if r.numel() else 0.0
    return res


# ------------------------------------------------------------------------------------------------------
# the passes, from the operands the device used
# ------------------------------------------------------------------------------------------------------
def pass_reference(eh, et, sd, dout):
    """The four passes in float64 over the rounded operands, and sum |A^||B^| (+ |bias|) of every element: two runs of the definition,
    the second with |bf16(.)| for the rounding.  eh, et [P,128], dout [P,R]: float32, what the device multiplied.
    -> (ref, mag), dicts over "logits", "d eh", "d et", "d bili_layer_01.weight", "d classification_layer_01.weight"."""
    bias = (sd["bili_layer_01.bias"] + sd["classification_layer_01.bias"]).double()   # the fp32 sum head_node_kernel forms
    res = []
    for rnd in (None, lambda t: F_._round_bf16(t).abs()):
        e, t = eh.double().requires_grad_(), et.double().requires_grad_()
        wb, wc = sd["bili_layer_01.weight"].double().requires_grad_(), sd["classification_layer_01.weight"].double().requires_grad_()
        out = F_.Bf16HeadBilinearFn.apply(e, t, wb, wc, bias if rnd is None else bias.abs(), rnd)
        out.backward(dout.double())
        res.append({"logits": out.detach(), "d eh": e.grad, "d et": t.grad, "d bili_layer_01.weight": wb.grad,
                    "d classification_layer_01.weight": wc.grad})
    return res[0], res[1]


def pass_K(name, P, R):
    return HW * HW + 2 * HW if name == "logits" else HW * R + R if name in ("d eh", "d et") else P


def pass_fractions(got, ref, mag, P, R, factor=None):
    """Per pass: (the worst |got - ref| / bound, the share of elements past the bound).  factor: {"d eh": 1 - eh^2, "d et": 1 - et^2}
    in float64 when got holds the entity gradients AFTER the tanh backward (the module docstring has the bound)."""
    res = {}
    for k, r in ref.items():
        bound = U23 * (pass_K(k, P, R) + 2) * mag[k]
        if factor is not None and k in factor:
            f = factor[k]
            bound = bound * f.abs() + 2.0 ** -22 * (bound + r.abs())
            r = r * f
        q = torch.nan_to_num((got[k].detach().cpu().double() - r).abs() / bound.clamp_min(1e-300), nan=float("inf"))
        res[k] = (q.max().item(), (q > 1.0).double().mean().item()) if q.numel() else (0.0, 0.0)
    return res


# ------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def run_abi(c, dev, matmul, cot=None, nv=None):
    """gcgcn_head_fwd + gcgcn_head_bwd, each announced with matmul (gcgcn_set_option("head_matmul", .) right before), on NaN-filled buffers.  -> (got, ws): got as reference() lays it out; ws the pair rows the
    passes worked on, in row order (every pair slot, or the live pairs of a compacted batch): "eh", "et" from the forward workspace,
    "g eh", "g et" (the entity gradients after the tanh backward) from the backward one."""
    dims = (c.Hd, c.nf, c.Pt, c.Pr, c.R)
    flat = torch.zeros(P_.head_layout(*dims)[-1])
    P_.pack_head(c.sd, *dims, flat)
    flat = flat.to(dev)
    feats = [f.to(dev).contiguous() for f in c.feats]
    ner, dis = c.sd["ner_emb.weight"].to(dev), c.sd["dis_embed.weight"].to(dev)
    ntype, rel = c.ntype.to(dev), c.rel.to(dev)
    nvd = (c.nv if nv is None else nv)
    nvd = None if nvd is None else nvd.to(dev)
    sizes = (ctypes.c_int64 * 3)()
    _lib.call("gcgcn_head_sizes", c.B, c.N, c.R, c.ND, ctypes.cast(sizes, ctypes.c_void_p))
    fbuf, bbuf = torch.full((sizes[0],), NAN, device=dev), torch.full((sizes[1],), NAN, device=dev)
    ibuf = torch.full((sizes[2],), -1, dtype=torch.int32, device=dev) if nvd is not None else None
    logits = torch.full((c.B, c.N, c.N, c.R), NAN, device=dev)
    fp = (ctypes.c_void_p * c.nf)(*[f.data_ptr() for f in feats])
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    head = (c.B, c.N, c.Hd, c.nf, c.Pt, c.Pr, c.R, c.ND, c.dis_plus, ctypes.cast(fp, ctypes.c_void_p), _p(ntype), _p(rel), _p(ner), _p(dis),
            _p(nvd), _p(flat), _p(fbuf), _p(ibuf))
    F_._head_call(matmul, "gcgcn_head_fwd", *head, _p(logits), st)
    dl = (c.cot if cot is None else cot).to(dev).contiguous()
    dfeats = [torch.full_like(f, NAN) for f in feats]
    dner, dtab, dflat = torch.full_like(ner, NAN), torch.full_like(dis, NAN), torch.zeros_like(flat)
    dp = (ctypes.c_void_p * c.nf)(*[f.data_ptr() for f in dfeats])
    F_._head_call(matmul, "gcgcn_head_bwd", *head, _p(bbuf), _p(dl), ctypes.cast(dp, ctypes.c_void_p), _p(dner), _p(dtab), _p(dflat), st)
    torch.cuda.synchronize()
    got = {"logits": logits}
    got.update({f"d f{k}": f for k, f in enumerate(dfeats)})
    got.update({"d " + k: v for k, v in P_.unpack_head(dflat, *dims).items()})
    got["d ner_emb.weight"], got["d dis_embed.weight"] = dner, dtab
    # head_bind's layout (csrc/head.hip): forward [U | Tt | Rt | UT | bsum | EH | ET | ..], backward [doutp | dEH | dET | ..], the pair
    # tensors padded to whole 128-row tiles
    BN, pairs = c.B * c.N, c.B * c.N * c.N
    pp = (pairs + 127) // 128 * 128
    at = (BN + 7 + c.ND + BN + 1) * HW
    rows = c.count if nvd is not None else pairs
    take = lambda buf, o: buf[o:o + rows * HW].view(rows, HW).cpu()
    ws = {"eh": take(fbuf, at), "et": take(fbuf, at + pp * HW), "g eh": take(bbuf, pp * HW), "g et": take(bbuf, 2 * pp * HW)}
    return got, ws


def run_fn(c, dev, matmul=None, cot=None):
    """The same through functional.classifier_head and autograd (matmul None: the argument is not passed at all)."""
    dims = (c.Hd, c.nf, c.Pt, c.Pr, c.R)
    flat = torch.zeros(P_.head_layout(*dims)[-1])
    P_.pack_head(c.sd, *dims, flat)
    flat = flat.to(dev).requires_grad_()
    fg = [f.to(dev).requires_grad_() for f in c.feats]
    ner, dis = c.sd["ner_emb.weight"].to(dev).requires_grad_(), c.sd["dis_embed.weight"].to(dev).requires_grad_()
    kw = {} if matmul is None else {"matmul": matmul}
    out = F_.classifier_head(fg, c.ntype.to(dev), c.rel.to(dev), ner, dis, flat, c.R, None if c.nv is None else c.nv.to(dev), c.dis_plus, **kw)
    out.backward((c.cot if cot is None else cot).to(dev))
    got = {"logits": out.detach()}
    got.update({f"d f{k}": f.grad for k, f in enumerate(fg)})
    got.update({"d " + k: v for k, v in P_.unpack_head(flat.grad, *dims).items()})
    got["d ner_emb.weight"], got["d dis_embed.weight"] = ner.grad, dis.grad
    return got
