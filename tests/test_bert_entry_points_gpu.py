"""The BERT section's exported symbols forward to one body per operation (csrc/api.hip): the older symbols must compute, bit for bit,
what gcgcn_bert_layer_fwd_mm / _bwd_mm compute from the arguments the forwarders stand for.

One shape, B = 2, T = 32, D = 128 (two heads), Dff = 256: two 16-row blocks per document, and lengths (32, 9) give one full block,
one partly live block and one dead block.  Inputs and parameters are bert_cases'.  Every output is NaN-filled before the call and
compared as bit patterns, so a buffer one side leaves unwritten shows.  The plain row operations against their _len forms with
t_valid = (T, T) at bert_cases' RTOL / ATOL (test_lengths_all_equal_to_T_match_the_path_without_lengths: these need not be
bitwise equal), and bitwise against themselves across two calls."""
import ctypes

import pytest
import torch

from gcgcn_amd import _lib, functional as Fn
from gcgcn_amd.bert import BertModel

from bert_cases import ATOL, RTOL, attn_case, config, model_case, state

pytestmark = pytest.mark.gpu

B, T, D, H, DFF = 2, 32, 128, 2, 256
DIMS = (B, T, D, H, DFF)
NAN = float("nan")


def _p(t):
    return None if t is None else t.data_ptr()


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _nan(*shape, dev):
    return torch.full(shape, NAN, device=dev)


def _params(dev):
    """The 12 tensors of the C parameter list: query | key | value stacked, as functional.bert_layer does.  bert_cases' layer has an
    intermediate size of 4 D; its first DFF units are this test's."""
    model = BertModel(config(D, H))
    model.load_state_dict(state(D, H))
    ts = [t.detach() for t in model.encoder.layer[0].tensors()]
    ts[10], ts[11], ts[12] = ts[10][:DFF], ts[11][:DFF], ts[12][:, :DFF]
    ts = [torch.cat([ts[0], ts[2], ts[4]], 0), torch.cat([ts[1], ts[3], ts[5]], 0)] + ts[6:]
    ts = [t.contiguous().to(dev) for t in ts]
    assert ts[6].shape == (DFF, D) and ts[8].shape == (D, DFF)
    return ts


def _ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*(t.data_ptr() for t in ts))


def _layer(suffix, dev, params, lengths=None, rowblk=False, matmul=None):
    """Forward + backward through gcgcn_bert_layer_fwd<suffix> / _bwd<suffix>: [y, saved, dx, the 12 gradients]."""
    x = attn_case(B, T, H, "none")["dctx"].clone()
    tv = rb = None
    if lengths is not None:
        x[torch.arange(T)[None, :] >= torch.tensor(lengths)[:, None]] = 0.0      # the layer's contract
        tv = torch.tensor(lengths, dtype=torch.int32, device=dev)
        rb = Fn.row_blocks(tv, B, T) if rowblk else None
    x, dy = x.to(dev), model_case(D, H, B, T)["dy"].to(dev)
    lib = _lib.lib()
    saved = _nan(lib.gcgcn_bert_layer_ws_bytes(*DIMS, 0) // 4, dev=dev)
    ws = _nan(lib.gcgcn_bert_layer_ws_bytes(*DIMS, 1) // 4, dev=dev)
    y, dx = _nan(B, T, D, dev=dev), _nan(B, T, D, dev=dev)
    grads = [torch.full_like(t, NAN) for t in params]
    lens = () if suffix == "" else (_p(tv), _p(rb))
    tail = () if matmul is None else (matmul,)
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("gcgcn_bert_layer_fwd" + suffix, *DIMS, _p(x), None, *lens, _ptr_array(params), _p(y), _p(saved), saved.numel() * 4, None,
              0.0, 0.0, st, *tail)
    _lib.call("gcgcn_bert_layer_bwd" + suffix, *DIMS, _p(x), None, *lens, _ptr_array(params), _p(saved), saved.numel() * 4, _p(dy), _p(dx),
              _ptr_array(grads), _p(ws), ws.numel() * 4, None, 0.0, 0.0, st, *tail)
    torch.cuda.synchronize()
    return [y, saved, dx] + grads


def _assert_same(a, b, label):
    names = ["y", "saved", "dx"] + [f"grad{i:02d}" for i in range(12)]
    assert len(a) == len(b) == len(names)
    for n, s, t in zip(names, a, b):
        assert _same_bits(s, t), f"{label}: {n} differs"
    for n, s in zip(names, a):
        if n != "saved":      # a product on the row-block list may leave dead blocks of the saved state unwritten
            assert torch.isfinite(s).all(), f"{label}: {n} is not finite"


def test_plain_layer_symbols_are_mm_without_lengths(gpu_device):
    params = _params(gpu_device)
    _assert_same(_layer("", gpu_device, params), _layer("_mm", gpu_device, params, matmul=0), "plain against _mm")


@pytest.mark.parametrize("rowblk", [True, False])
def test_len_layer_symbols_are_mm_with_fp32_products(gpu_device, rowblk):
    params = _params(gpu_device)
    a = _layer("_len", gpu_device, params, (32, 9), rowblk)
    b = _layer("_mm", gpu_device, params, (32, 9), rowblk, matmul=0)
    _assert_same(a, b, f"_len against _mm, rowblk = {rowblk}")
    pad = slice(9, T)
    assert not a[0][1, pad].any() and not a[2][1, pad].any()      # y and dx on the padding rows: exactly zero


def _close(got, want, label):
    torch.testing.assert_close(got, want, rtol=RTOL, atol=ATOL, msg=lambda m: f"{label}: {m}")


def test_plain_row_operations_against_their_len_forms(gpu_device):
    dev = gpu_device
    c = attn_case(B, T, H, "none")
    params = _params(dev)
    tv = torch.full((B,), T, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    qkv = c["qkv"].to(dev)

    def attn(name, *lens):
        ctx, lse = _nan(B, T, D, dev=dev), _nan(B, H, T, dev=dev)
        _lib.call(name, B, T, H, 64, _p(qkv), None, *lens, _p(ctx), _p(lse), None, 0, 0.0, st)
        return ctx, lse

    x, res = c["dctx"].to(dev), model_case(D, H, B, T)["dy"].to(dev)
    bo, ln1w, ln1b, bi = params[3], params[4], params[5], params[7]

    def res_ln(name, *lens):
        y, mean, rstd = _nan(B, T, D, dev=dev), _nan(B * T, dev=dev), _nan(B * T, dev=dev)
        _lib.call(name, B * T, D, _p(x), _p(bo), _p(res), _p(ln1w), _p(ln1b), *lens, _p(y), _p(mean), _p(rstd), None, 0, 0.0, st)
        return y, mean, rstd

    z = qkv[..., :DFF].contiguous()

    def gelu(name, *lens):
        out = _nan(B, T, DFF, dev=dev)
        _lib.call(name, B * T, DFF, _p(z), _p(bi), *lens, _p(out), st)
        return (out,)

    for fn, name, lens in ((attn, "gcgcn_bert_attn_fwd", (_p(tv),)), (res_ln, "gcgcn_res_ln_fwd", (_p(tv), T)),
                           (gelu, "gcgcn_bias_gelu_fwd", (_p(tv), T))):
        plain, again, with_len, with_len_again = fn(name), fn(name), fn(name + "_len", *lens), fn(name + "_len", *lens)
        torch.cuda.synchronize()
        for i, (a, a2, b, b2) in enumerate(zip(plain, again, with_len, with_len_again)):
            assert _same_bits(a, a2), f"{name}: output {i} differs between two calls"
            assert _same_bits(b, b2), f"{name}_len: output {i} differs between two calls"
            _close(b, a, f"{name}_len against {name}, output {i}")
