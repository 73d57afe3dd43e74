"""Per-document token lengths of the BERT encoder, the checks that need no device: the contract in plain
PyTorch (``BertModel(impl="torch")(..., lengths=)``) against per-document truncated runs, and the new symbols.

Reference: the float64 ``impl="torch"`` model on each document ALONE, truncated to ``lengths[b]`` tokens, with no mask; parameter
gradients summed over the documents.  Both sides are float64 on the CPU and differ only in the order of a few sums (a softmax over T
keys of which T - lengths[b] are exactly 0, against one over lengths[b] keys), so the bound is round-off: 1e-12 relative and
absolute on values of order 1 to 10."""
import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib
from gcgcn_amd.bert import BertModel

from bert_cases import config, model_case
from bert_length_cases import fresh_model, model_len_reference, pad_mask, run_with_lengths


def _model(D, H, dtype=torch.float64):
    return fresh_model(D, H, dtype=dtype).eval()


@pytest.mark.parametrize("B,T,lengths", [(3, 48, (48, 17, 1)), (3, 33, (33, 20, 0))])
def test_torch_lengths_equal_per_document_runs(B, T, lengths):
    D, H = 128, 2
    model = _model(D, H)
    case = model_case(D, H, B, T)
    got = run_with_lengths(model, case, lengths)
    ref = model_len_reference(D, H, B, T, lengths)
    pad = pad_mask(lengths, T)
    for k, r in ref.items():
        assert torch.isfinite(got[k]).all(), k
        torch.testing.assert_close(got[k], r, rtol=1e-12, atol=1e-12, msg=lambda m: f"{k}: {m}")
    for k in ("out0", "out1"):
        assert torch.equal(got[k][pad], torch.zeros_like(got[k][pad])), k
    if 0 in lengths:
        b = lengths.index(0)
        assert torch.equal(got["pooled"][b], torch.tanh(model.pooler.dense.bias.detach()))


def test_torch_lengths_ignore_what_sits_on_padding_rows():
    """Other token ids on the padding rows and NaN cotangents there change nothing, bit for bit."""
    D, H, B, T, lengths = 128, 2, 3, 33, (33, 20, 0)
    model = _model(D, H)
    case = model_case(D, H, B, T)
    a = run_with_lengths(model, case, lengths, nan_pad=False)
    other = dict(case)
    pad = pad_mask(lengths, T)
    other["ids"] = torch.where(pad, (case["ids"] + 7) % 61, case["ids"])
    b = run_with_lengths(model, other, lengths, nan_pad=True)
    for k in a:
        if k == "dembeddings.word_embeddings.weight":
            continue   # zero rows either way, but the zeros land on other vocabulary rows' sums: equal in value, checked below
        assert torch.equal(a[k], b[k]), k
    torch.testing.assert_close(a["dembeddings.word_embeddings.weight"], b["dembeddings.word_embeddings.weight"], rtol=0, atol=0)


def test_lengths_none_is_bitwise_the_old_result():
    D, H, B, T = 128, 2, 3, 33
    case = model_case(D, H, B, T)
    for dtype in (torch.float32, torch.float64):
        model = _model(D, H, dtype)
        with torch.no_grad():
            a, pa = model(case["ids"], case["tt"], case["mask"])
            b, pb = model(case["ids"], case["tt"], case["mask"], True, None)
            c, pc = model(case["ids"], case["tt"], case["mask"], lengths=None)
        for x, y, z in zip(a + [pa], b + [pb], c + [pc]):
            assert torch.equal(x, y) and torch.equal(x, z)
    # lengths all equal to T: the same function (no key is masked, no row is padding)
    model = _model(D, H)
    with torch.no_grad():
        a, pa = model(case["ids"], case["tt"])
        b, pb = model(case["ids"], case["tt"], lengths=torch.full((B,), T))
    for x, y in zip(a + [pa], b + [pb]):
        torch.testing.assert_close(x, y, rtol=1e-13, atol=1e-13)


def test_lengths_shape_is_checked():
    model = _model(128, 2)
    with pytest.raises(ValueError, match="lengths"):
        model(torch.randint(0, 61, (2, 9)), lengths=torch.tensor([9, 9, 9]))


def test_hip_impl_still_refuses_cpu_tensors():
    model = BertModel(config(128, 2), impl="hip").eval()
    with pytest.raises(RuntimeError, match="MI355X only"):
        model(torch.randint(0, 61, (2, 9)), lengths=torch.tensor([9, 4]))
    x = torch.zeros(2, 4, 128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gcgcn_amd.functional.res_layer_norm(x, torch.ones(128), torch.zeros(128), t_valid=torch.tensor([4, 2]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gcgcn_amd.functional.bert_layer(x, None, *[torch.zeros(1)] * 16, t_valid=torch.tensor([4, 2]))


def test_symbols_declared_bound_exported():
    """The eight _len symbols against the header and the library: tests/test_abi_cpu.py.  Here: the ABI version and the Python
    signatures that carry the lengths."""
    h = _lib.lib()                      # loading binds every declaration of the header and checks the ABI version
    assert _lib.ABI_VERSION == 7 and h.gcgcn_version() == 7
    import inspect
    assert "lengths" in inspect.signature(BertModel.forward).parameters
    assert list(inspect.signature(BertModel.forward).parameters)[-1] == "lengths"
    for fn, names in ((gcgcn_amd.functional.bert_layer, ("t_valid", "rowblk")), (gcgcn_amd.functional.res_layer_norm, ("t_valid",))):
        for n in names:
            assert inspect.signature(fn).parameters[n].default is None


def test_refusals_without_a_device():
    """Argument checks of the new entry points come before any launch."""
    h = _lib.lib()
    assert h.gcgcn_res_ln_fwd_len(10, 128, 1, None, None, 1, 1, None, 5, 1, None, None, None, 0, 0.0, None) != 0
    assert b"t_valid is null" in h.gcgcn_last_error()
    assert h.gcgcn_res_ln_fwd_len(10, 128, 1, None, None, 1, 1, 1, 4, 1, None, None, None, 0, 0.0, None) != 0
    assert b"no whole documents" in h.gcgcn_last_error()
    assert h.gcgcn_bert_attn_fwd_len(2, 513, 2, 64, 16, None, 16, 16, 16, None, 0, 0.0, None) != 0
    assert b"T = 513" in h.gcgcn_last_error()
    assert h.gcgcn_bias_gelu_fwd_len(10, 128, 16, None, None, 5, 16, None) != 0
    assert b"t_valid is null" in h.gcgcn_last_error()
