"""The bf16-operand product on the device, through the C ABI (gcgcn_gemm_bf16), against the float64 product of the bf16-rounded operands
under the derived bound of tests/gemm_bf16_cases.py.  Every buffer of every call is followed by a NaN guard region that must come
back untouched, and C is NaN-filled before the call."""
import pytest
import torch

from gcgcn_amd import _lib, functional as Fn

from gemm_bf16_cases import FORMS, NAN, SHAPES, case, reference, violations

pytestmark = pytest.mark.gpu

GUARD = 256


def _p(t):
    return None if t is None else t.data_ptr()


def _buffer(t, ld, dev, fill=NAN):
    """t [rows][cols] laid out with row pitch ld in a flat NaN buffer with GUARD floats behind it -> (flat buffer, the view's size)."""
    rows, cols = t.shape
    n = (rows - 1) * ld + cols
    flat = torch.full((n + GUARD,), fill, device=dev)
    torch.as_strided(flat, (rows, cols), (ld, 1)).copy_(t.to(dev))
    return flat, n


def _device(c, form, M, N, K, dev, bias=False, add=False, pad=0):
    """One call.  pad: extra floats of row pitch on a, b, c and add (NaN in the padding).  -> (C [M][N], {name: (flat, n, image before the call)})."""
    a, b = c["a"], c["b"]
    lda, ldb, ldc, ldadd = a.shape[1] + pad, b.shape[1] + pad, N + pad, N + pad
    bufs = {"a": _buffer(a, lda, dev), "b": _buffer(b, ldb, dev), "c": _buffer(torch.full((M, N), NAN), ldc, dev)}
    if bias:
        bufs["bias"] = _buffer(c["bias"][None, :], N, dev)
    if add:
        bufs["add"] = _buffer(c["add"], ldadd, dev)
    need = int(_lib.lib().gcgcn_gemm_bf16_ws_bytes(M, N, K))
    assert need >= 0
    ws = torch.full((need // 4 + GUARD,), NAN, device=dev)
    before = {k: f.clone() for k, (f, _) in bufs.items() if k != "c"}
    _lib.call("gcgcn_gemm_bf16", int(form != "tn"), int(form == "nt"), _p(bufs["a"][0]), lda, _p(bufs["b"][0]), ldb, _p(bufs["c"][0]), ldc, M, N, K,
              _p(bufs["bias"][0]) if bias else None, _p(bufs["add"][0]) if add else None, ldadd if add else 0, _p(ws) if need else None, need,
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for k, f in before.items():                                                       # inputs, their padding and their guards: as they were
        assert torch.equal(torch.nan_to_num(bufs[k][0], nan=12345.0), torch.nan_to_num(f, nan=12345.0)), f"{k} was written"
    flat, n = bufs["c"]
    assert torch.isnan(flat[n:]).all(), "the guard behind C was written"
    assert torch.isnan(ws[need // 4:]).all(), "the guard behind the workspace was written"
    out = torch.as_strided(flat, (M, N), (ldc, 1))
    if pad:
        assert torch.isnan(torch.as_strided(flat, (M - 1, pad), (ldc, 1), N)).all() if M > 1 else True, "C's ld padding was written"
    return out.clone()


@pytest.mark.parametrize("epi", ["none", "bias", "add", "both"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_product_against_float64_of_rounded_operands(gpu_device, M, N, K, form, epi):
    bias, add = epi in ("bias", "both"), epi in ("add", "both")
    c = case(form, M, N, K)
    got = _device(c, form, M, N, K, gpu_device, bias, add)
    ref, bound = reference(c, form, bias, add)
    err = ((got.double().cpu() - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"gemm_bf16 {form} ({M},{N},{K}) {epi}: worst {err:.3f} of the bound")
    assert torch.isfinite(got).all()
    assert violations(got, ref, bound) == 0.0, err
    again = _device(c, form, M, N, K, gpu_device, bias, add)
    assert torch.equal(got, again), "two calls differ"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("M,N,K,pad", [(130, 192, 100, 3), (128, 128, 2048, 4), (64, 64, 64, 8)])
def test_row_pitch_larger_than_the_width(gpu_device, M, N, K, pad, form):
    """ld > width with NaN in the padding: pad = 3 breaks the 16-byte alignment of every row (the guarded body), pad = 4 and 8 keep it
    (the unguarded body; (128, 128, 2048) through the split workspace).  Nothing of the padding is read (the result is finite and
    within the bound) or written."""
    c = case(form, M, N, K)
    got = _device(c, form, M, N, K, gpu_device, True, True, pad=pad)
    ref, bound = reference(c, form, True, True)
    assert torch.isfinite(got).all()
    assert violations(got, ref, bound) == 0.0
    assert torch.equal(got, _device(c, form, M, N, K, gpu_device, True, True, pad=pad))


def test_operands_are_really_rounded_to_bf16(gpu_device):
    """(64, 64, 32), NT: the result is within the bound of the ROUNDED operands' product, and the float64 product of the UNROUNDED
    operands violates that bound on at least half of the elements (test_bert_bf16_cpu.py checks the latter for this seed with the
    emulation alone) -- so an fp32-operand path could not pass."""
    M, N, K = 64, 64, 32
    c = case("nt", M, N, K)
    got = Fn.gemm_bf16(c["a"].to(gpu_device), c["b"].to(gpu_device), form="nt")
    ref, bound = reference(c, "nt")
    assert violations(got, ref, bound) == 0.0
    exact, _ = reference(c, "nt", rounded=False)
    assert violations(got, exact, bound) >= 0.5


@pytest.mark.parametrize("form", FORMS)
def test_python_binding(gpu_device, form):
    """functional.gemm_bf16: strided views, bias and add, the three forms."""
    M, N, K = 65, 63, 33
    c = case(form, M, N, K)
    wide = lambda t: torch.cat([t, torch.full((t.shape[0], 5), NAN)], 1).to(gpu_device)[:, :t.shape[1]]
    got = Fn.gemm_bf16(wide(c["a"]), wide(c["b"]), form=form, bias=c["bias"].to(gpu_device), add=wide(c["add"]))
    ref, bound = reference(c, form, True, True)
    assert violations(got, ref, bound) == 0.0
    with pytest.raises(ValueError):
        Fn.gemm_bf16(c["a"].to(gpu_device), c["b"].to(gpu_device), form="tt")
    with pytest.raises(RuntimeError):
        Fn.gemm_bf16(c["a"], c["b"], form=form)
