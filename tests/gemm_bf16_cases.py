"""What tests/test_gemm_bf16_gpu.py and tests/test_bert_bf16_cpu.py share about the stand-alone bf16-operand product (gcgcn_gemm_bf16,
csrc/gemm_bf16.hip): shapes, seeded operands, the float64 reference and the bound.

Reference: the float64 product of the bf16-ROUNDED operands -- ``A.to(bfloat16).double()``, likewise B -- plus bias and add in float64.

Bound, derived and not measured, for every element:
    |got - ref| <= 2^-23 (K + 2) (|A^| |B^| + |bias| + |add|)_ij
the forward error of an fp32 sum of K exact products (a product of two bf16 numbers has 16 significant bits: exact in fp32) and two
more terms, in any order, with a factor 2 over the unit round-off 2^-24 so that it does not depend on how the matrix instruction
rounds its partial sums.

Operands are N(0, 1), seeded per (shape, form).  Shapes (M, N, K) against the kernel's 64 x 64 x 64 tile:
    (1, 1, 1)          the smallest problem
    (64, 64, 32)       one tile, one (partial) k-step
    (65, 63, 33)       every edge at once
    (130, 192, 100)    several tiles with edges
    (99, 384, 128)     the small model's own product shape
    (128, 128, 2048)   the weight gradient's split-K route (4 tiles, 32 k-steps)"""
import functools

import torch

SHAPES = [(1, 1, 1), (64, 64, 32), (65, 63, 33), (130, 192, 100), (99, 384, 128), (128, 128, 2048)]
FORMS = ("nn", "nt", "tn")
NAN = float("nan")


def stored_shapes(form, M, N, K):
    """Shapes of a and b as STORED."""
    return ((M, K) if form != "tn" else (K, M)), ((N, K) if form == "nt" else (K, N))


@functools.lru_cache(maxsize=None)
def case(form, M, N, K, seed=0):
    g = torch.Generator().manual_seed(1 + seed + 3 * FORMS.index(form) + 7 * M + 11 * N + 13 * K)
    sa, sb = stored_shapes(form, M, N, K)
    return {"a": torch.randn(sa, generator=g), "b": torch.randn(sb, generator=g), "bias": torch.randn(N, generator=g),
            "add": torch.randn(M, N, generator=g)}


def _ops(c, form, rounded):
    cast = (lambda t: t.to(torch.bfloat16).double()) if rounded else (lambda t: t.double())
    a, b = cast(c["a"]), cast(c["b"])
    return (a if form != "tn" else a.t()), (b.t() if form == "nt" else b)


def reference(c, form, bias=False, add=False, rounded=True):
    """(ref, bound) in float64; rounded=False: the product of the UNROUNDED operands (what a path that skipped the rounding computes)."""
    a, b = _ops(c, form, rounded)
    ar, br = _ops(c, form, True)
    K = a.shape[1]
    ref, mag = a @ b, ar.abs() @ br.abs()
    if bias:
        ref, mag = ref + c["bias"].double(), mag + c["bias"].double().abs()
    if add:
        ref, mag = ref + c["add"].double(), mag + c["add"].double().abs()
    return ref, 2.0 ** -23 * (K + 2) * mag


def violations(got, ref, bound):
    """Fraction of elements outside the bound (NaN counts as outside)."""
    return (~((got.double().cpu() - ref).abs() <= bound)).double().mean().item()
