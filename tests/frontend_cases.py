"""What tests/test_frontend_cpu.py and tests/test_frontend_gpu.py share: the case generator, the float64 reference and the sweep.

A case is the token front end either side of the encoder: three embedding gathers (``padding_idx`` 0 in the two small tables, none
in the word table), ``cat``, the locked-dropout factor ``scale[B,I]`` where the case has one, then ``F.linear`` + ``tanh`` and the
entity pooling ``bmm(node_pos, ctx)``.  With ``K=None`` the projection reads the embeddings themselves (K = I: the table gradients
flow through it); with ``K`` given it reads an independent ``h[B,T,K]`` (the context pair at the models' inner widths) and the
embeddings get a random cotangent of their own.  Table values are N(0, 1), ``W`` and ``b`` N(0, 0.1^2); ``node_pos`` rows are 1/len
over a span of 1-3 tokens, every fourth entity has no mention, entity 0 starts at t = 0, entity 1 ends at t = T - 1 and entity 2
shares entity 0's first token.  Gradients come from autograd with random cotangents on ``ctx`` and ``node_feat``.

The reference is computed once per case in float64 on the CPU and shared (lru_cache); nobody writes to it.  The bound is the
project's own (lstm_cases.frac_of_bound): |got - ref| <= 1e-5 * max(1, max|ref|) + 1e-4 * |ref| on every element."""
import functools
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

HD = 128
NER_ROWS = 7
OUTPUTS = ("x", "ctx", "node_feat", "dword", "dcoref", "dner", "dW", "db", "dh")


class Case(NamedTuple):
    B: int
    T: int
    V: int
    widths: Tuple[int, int, int] = (100, 20, 20)
    N: int = 5
    ids: str = "random"            # "random" | "equal" (every token the same id) | "distinct" (a permutation of V = B * T ids)
    K: Optional[int] = None        # None: the projection reads the embeddings
    scaled: bool = False
    P: int = 512                   # rows of the coreference table (max_length)

    @property
    def label(self):
        return f"B{self.B}-T{self.T}-V{self.V}-w{'x'.join(map(str, self.widths))}-N{self.N}-{self.ids}-K{self.K}-{'scale' if self.scaled else 'plain'}"


# the smallest shapes at which each kernel can go wrong (the table of the test module's docstring)
SWEEP = [
    Case(1, 1, 50, N=1),
    Case(2, 2, 50, N=5),
    Case(3, 37, 50, N=5, scaled=True),
    Case(2, 512, 1000, N=42, scaled=True),                   # the model's length; many duplicated ids; three tiles of node_pos
    Case(3, 37, 7, widths=(3, 1, 5), N=42, P=9),             # unaligned parts
    Case(2, 512, 1, N=5),                                    # one run of 1 024 tokens
    Case(2, 512, 1000, N=5, ids="equal", scaled=True),       # the same with an id other than 0
    Case(3, 37, 111, N=5, ids="distinct"),                   # singleton runs, the last table row
    Case(2, 37, 200000, N=5),                                # the table-sized passes; untouched rows
    Case(2, 37, 50, N=1, K=256),                             # the context pair at the models' inner widths
    Case(3, 37, 50, N=42, K=808),
    Case(2, 512, 50, N=5, K=256),
]
DETERMINISM = [SWEEP[6], SWEEP[3]]


def _node_pos(c: Case, g):
    pos = torch.zeros(c.B, c.N, c.T)
    for b in range(c.B):
        for n in range(c.N):
            if n % 4 == 3:
                continue
            ln = min(c.T, 1 + int(torch.randint(0, 3, (1,), generator=g)))
            if n == 0 or n == 2:
                s = 0
            elif n == 1:
                s = c.T - ln
            else:
                s = int(torch.randint(0, c.T - ln + 1, (1,), generator=g))
            pos[b, n, s:s + ln] = 1.0 / ln
    return pos


@functools.lru_cache(maxsize=None)
def inputs(c: Case, seed=0):
    """float32 / int64 CPU tensors of the case."""
    g = torch.Generator().manual_seed(977 * seed + 31 * c.B + 7 * c.T + c.V + c.N + sum(c.widths) + (c.K or 0))
    n = c.B * c.T
    Dw, Dc, Dn = c.widths
    I = Dw + Dc + Dn
    if c.ids == "equal":
        doc = torch.full((c.B, c.T), min(7, c.V - 1), dtype=torch.int64)
    elif c.ids == "distinct":
        assert c.V == n
        doc = torch.randperm(n, generator=g).view(c.B, c.T)
    else:
        doc = torch.randint(0, c.V, (c.B, c.T), generator=g)
        doc.view(-1)[n // 2] = c.V - 1                                           # the last row is always touched
    keep = torch.rand(c.B, c.T, generator=g) < 0.3                               # most tokens are no mention: padding id 0
    d = {"document": doc,
         "document_pos": torch.randint(0, c.P, (c.B, c.T), generator=g) * keep,
         "document_ner": torch.randint(0, NER_ROWS, (c.B, c.T), generator=g) * keep,
         "word_w": torch.randn(c.V, Dw, generator=g), "coref_w": torch.randn(c.P, Dc, generator=g),
         "ner_w": torch.randn(NER_ROWS, Dn, generator=g),
         "scale": ((torch.rand(c.B, I, generator=g) < 0.8).float() / 0.8) if c.scaled else None,
         "W": torch.randn(HD, c.K or I, generator=g) * 0.1, "b": torch.randn(HD, generator=g) * 0.1,
         "node_pos": _node_pos(c, g),
         "dctx": torch.randn(c.B, c.T, HD, generator=g), "dnode": torch.randn(c.B, c.N, HD, generator=g)}
    if c.K is not None:
        d["h"] = torch.randn(c.B, c.T, c.K, generator=g)
        d["dx"] = torch.randn(c.B, c.T, I, generator=g)
    return d


def run_torch(c: Case, d, dtype, device="cpu"):
    """The front end in plain torch in `dtype`: {name: tensor} over OUTPUTS."""
    fl = lambda k: d[k].to(device=device, dtype=dtype)
    ix = lambda k: d[k].to(device)
    ww, cw, nw, W, b = (fl(k).requires_grad_() for k in ("word_w", "coref_w", "ner_w", "W", "b"))
    x = torch.cat([F.embedding(ix("document"), ww), F.embedding(ix("document_pos"), cw, padding_idx=0),
                   F.embedding(ix("document_ner"), nw, padding_idx=0)], dim=-1)
    if c.scaled:
        x = fl("scale")[:, None, :].expand_as(x) * x
    if c.K is None:
        h = x
        h.retain_grad()
    else:
        h = fl("h").requires_grad_()
    ctx = torch.tanh(F.linear(h, W, b))
    node_feat = torch.bmm(fl("node_pos"), ctx)
    loss = (ctx * fl("dctx")).sum() + (node_feat * fl("dnode")).sum()
    if c.K is not None:
        loss = loss + (x * fl("dx")).sum()
    loss.backward()
    return {"x": x.detach(), "ctx": ctx.detach(), "node_feat": node_feat.detach(), "dword": ww.grad, "dcoref": cw.grad, "dner": nw.grad,
            "dW": W.grad, "db": b.grad, "dh": h.grad}


@functools.lru_cache(maxsize=None)
def reference(c: Case, seed=0):
    return run_torch(c, inputs(c, seed), torch.float64)
