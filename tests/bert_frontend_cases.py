"""What tests/test_bert_frontend_cpu.py and tests/test_bert_frontend_gpu.py share: the cases, the float64 reference, the plain-PyTorch
restatement of the folded algebra, and the [CLS] logit tail's cases and reference.

The context pair.  The reference is the definition, in float64 on the CPU::

    ctx = tanh(F.linear(cat([states, coref_w[document_pos], ner_w[document_ner]], -1), weight, bias));  node_feat = bmm(node_pos, ctx)

with ``padding_idx`` 0 in both tables and gradients from autograd with random cotangents on ``ctx`` and ``node_feat``.  Input
distributions are those of tests/frontend_cases.py: table values and ``states`` N(0, 1), ``weight`` and ``bias`` N(0, 0.1^2), ids 0
(the padding id) on about 70 % of the tokens in the "random" cases, ``node_pos`` from its generator.  Computed once per case and shared
(lru_cache); nobody writes to it.  The bound is the project's own (lstm_cases.frac_of_bound):
|got - ref| <= 1e-5 * max(1, max|ref|) + 1e-4 * |ref| on every element.

The cases are the smallest shapes at which each kernel can go wrong:

  B  T    N   widths        P     ids
  1  1    1   768/20/20     512   random                 one token, one entity
  2  2    5   768/20/20     512   random
  3  37   42  64/1/5        9     "third"                unaligned fold widths (K = 70: the guarded GEMM body, W2 / W3 at unaligned
                                                         offsets); every third token carries the padding id, the others a non-zero one
  3  37   5   768/20/20     111   "distinct"             document_pos a permutation of all 111 rows: singleton runs, the last table row
  2  512  42  768/20/20     512   random                 the model's own sizes; many duplicated ids; four chunks of the sorted scheme
  2  512  5   768/20/20     512   "equal"                every token the same non-zero id: one run of 1 024 into one fold row -- the
                                                         7-row ner table's regime

The tail.  Reference: the model's own expression (``tail_expression``: models.py's ``logits + cls[:, None, None, :] * mask``) in
float64, ``dcls`` from autograd with a random cotangent.  Cases (B, N, R): (1, 1, 97), (2, 5, 97), (3, 64, 97) -- R = 97 rows are not
16-byte aligned, 64 entities are the model's padded count -- and (2, 5, 4) for a tensor whose every row is; ``n_valid`` None, all-full,
and mixed (0, 1, N) cycled over the batch."""
import functools
from typing import NamedTuple, Tuple

import torch
import torch.nn.functional as F

from frontend_cases import NER_ROWS, _node_pos

HD = 128
OUTPUTS = ("ctx", "node_feat", "dstates", "dweight", "dbias", "dcoref_w", "dner_w")


class Case(NamedTuple):
    B: int
    T: int
    N: int
    widths: Tuple[int, int, int] = (768, 20, 20)
    P: int = 512
    ids: str = "random"            # "random" | "third" | "distinct" | "equal"

    @property
    def label(self):
        return f"B{self.B}-T{self.T}-N{self.N}-w{'x'.join(map(str, self.widths))}-P{self.P}-{self.ids}"


SWEEP = [
    Case(1, 1, 1),
    Case(2, 2, 5),
    Case(3, 37, 42, widths=(64, 1, 5), P=9, ids="third"),
    Case(3, 37, 5, P=111, ids="distinct"),
    Case(2, 512, 42),
    Case(2, 512, 5, ids="equal"),
]
DETERMINISM = [SWEEP[2], SWEEP[4], SWEEP[5]]
GRAPH_CASE = Case(3, 37, 5, P=64)


@functools.lru_cache(maxsize=None)
def inputs(c: Case, seed=0):
    """float32 / int64 CPU tensors of the case."""
    g = torch.Generator().manual_seed(1409 * seed + 31 * c.B + 7 * c.T + c.N + c.P + sum(c.widths) + len(c.ids))
    n = c.B * c.T
    Dw, Dc, Dn = c.widths
    if c.ids == "equal":
        pos, ner = torch.full((c.B, c.T), min(7, c.P - 1), dtype=torch.int64), torch.full((c.B, c.T), 3, dtype=torch.int64)
    elif c.ids == "distinct":
        assert c.P == n
        pos = torch.randperm(n, generator=g).view(c.B, c.T)
        ner = torch.randint(0, NER_ROWS, (c.B, c.T), generator=g)
    elif c.ids == "third":
        live = (torch.arange(n) % 3 != 0).view(c.B, c.T)
        pos = torch.randint(1, c.P, (c.B, c.T), generator=g) * live
        ner = torch.randint(1, NER_ROWS, (c.B, c.T), generator=g) * live
        pos.view(-1)[1] = c.P - 1
    else:
        keep = torch.rand(c.B, c.T, generator=g) < 0.3                           # most tokens are no mention: padding id 0
        pos = torch.randint(0, c.P, (c.B, c.T), generator=g) * keep
        ner = torch.randint(0, NER_ROWS, (c.B, c.T), generator=g) * keep
        pos.view(-1)[n // 2] = c.P - 1                                           # the last row is always touched
    return {"states": torch.randn(c.B, c.T, Dw, generator=g), "document_pos": pos, "document_ner": ner,
            "coref_w": torch.randn(c.P, Dc, generator=g), "ner_w": torch.randn(NER_ROWS, Dn, generator=g),
            "W": torch.randn(HD, Dw + Dc + Dn, generator=g) * 0.1, "b": torch.randn(HD, generator=g) * 0.1,
            "node_pos": _node_pos(c, g),
            "dctx": torch.randn(c.B, c.T, HD, generator=g), "dnode": torch.randn(c.B, c.N, HD, generator=g)}


def run_definition(c: Case, d, dtype, device="cpu"):
    """The definition in plain torch in `dtype`, gradients by autograd: {name: tensor} over OUTPUTS."""
    fl = lambda k: d[k].to(device=device, dtype=dtype)
    st, cw, nw, W, b = (fl(k).requires_grad_() for k in ("states", "coref_w", "ner_w", "W", "b"))
    x = torch.cat([st, F.embedding(d["document_pos"].to(device), cw, padding_idx=0),
                   F.embedding(d["document_ner"].to(device), nw, padding_idx=0)], dim=-1)
    ctx = torch.tanh(F.linear(x, W, b))
    node_feat = torch.bmm(fl("node_pos"), ctx)
    ((ctx * fl("dctx")).sum() + (node_feat * fl("dnode")).sum()).backward()
    return {"ctx": ctx.detach(), "node_feat": node_feat.detach(), "dstates": st.grad, "dweight": W.grad, "dbias": b.grad,
            "dcoref_w": cw.grad, "dner_w": nw.grad}


@functools.lru_cache(maxsize=None)
def reference(c: Case, seed=0):
    return run_definition(c, inputs(c, seed), torch.float64)


def run_folded(c: Case, d, dtype, coref_pad=0, ner_pad=0):
    """The folded algebra restated in plain torch in `dtype`, forward and backward written out (no autograd): what
    csrc/bert_frontend.hip computes, launch by launch, without its orders of summation."""
    fl = lambda k: d[k].to(dtype)
    Dw, Dc, Dn = c.widths
    st, cw, nw, W, b, npos = fl("states"), fl("coref_w"), fl("ner_w"), fl("W"), fl("b"), fl("node_pos")
    pos, ner = d["document_pos"].reshape(-1), d["document_ner"].reshape(-1)
    W1, W2, W3 = W[:, :Dw], W[:, Dw:Dw + Dc], W[:, Dw + Dc:]
    F2, F3 = cw @ W2.T, nw @ W3.T                                                 # the two fold products
    pre = st @ W1.T + b                                                           # the large product at K = Dw
    ctx = torch.tanh((pre + F2[pos].view(c.B, c.T, HD)) + F3[ner].view(c.B, c.T, HD))
    node_feat = torch.bmm(npos, ctx)
    dpre = (fl("dctx") + torch.bmm(npos.transpose(1, 2), fl("dnode"))) * (1 - ctx * ctx)
    dp = dpre.reshape(-1, HD)
    dF2 = torch.zeros(c.P, HD, dtype=dtype).index_add_(0, pos, dp)                # every token, the padding ids included
    dF3 = torch.zeros(NER_ROWS, HD, dtype=dtype).index_add_(0, ner, dp)
    dweight = torch.cat([dp.T @ st.reshape(-1, Dw), dF2.T @ cw, dF3.T @ nw], dim=1)
    dcoref, dner = dF2 @ W2, dF3 @ W3
    if coref_pad is not None:
        dcoref[coref_pad] = 0
    if ner_pad is not None:
        dner[ner_pad] = 0
    return {"ctx": ctx, "node_feat": node_feat, "dstates": dpre @ W1, "dweight": dweight, "dbias": dp.sum(0), "dcoref_w": dcoref,
            "dner_w": dner}


# ---- the [CLS] logit tail ----------------------------------------------------------------------------------------------------
TAIL_SHAPES = [(1, 1, 97), (2, 5, 97), (3, 64, 97), (2, 5, 4)]
NV_KINDS = ("none", "full", "mixed")
TAIL_CASES = [(B, N, R, kind) for (B, N, R) in TAIL_SHAPES for kind in NV_KINDS]


def tail_n_valid(B, N, kind):
    if kind == "none":
        return None
    if kind == "full":
        return torch.full((B,), N, dtype=torch.int64)
    return torch.tensor([(0, 1, N)[b % 3] for b in range(B)], dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def tail_inputs(B, N, R, kind, seed=0):
    g = torch.Generator().manual_seed(211 * seed + 5 * B + 3 * N + R + len(kind))
    return {"logits": torch.randn(B, N, N, R, generator=g), "cls": torch.randn(B, R, generator=g), "n_valid": tail_n_valid(B, N, kind),
            "dout": torch.randn(B, N, N, R, generator=g)}


def tail_expression(logits, cls, n_valid):
    """gcgcn_amd/models.py's own lines for a batch."""
    add = cls[:, None, None, :]
    if n_valid is not None:
        ok = torch.arange(logits.shape[1], device=logits.device)[None, :] < n_valid[:, None]
        add = add * (ok[:, :, None] & ok[:, None, :]).unsqueeze(-1).to(add.dtype)
    return logits + add


@functools.lru_cache(maxsize=None)
def tail_reference(B, N, R, kind, seed=0):
    d = tail_inputs(B, N, R, kind, seed)
    logits, cls = d["logits"].double().requires_grad_(), d["cls"].double().requires_grad_()
    out = tail_expression(logits, cls, d["n_valid"])
    out.backward(d["dout"].double())
    return {"out": out.detach(), "dcls": cls.grad, "dlogits": logits.grad}
