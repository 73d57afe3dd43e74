"""matmul="bf16" with a row-block list: the twelve Linear products of a layer walk the live 16-row blocks (csrc/gemm_bf16.hip, launches
timed as ``gemm_bf16_rb``) and give, bit for bit, what the dense launches give (option ``bf16_rows`` = 0: one process runs both sides).
Harness and bounds are tests/bert_bf16_cases.py's, tests/bert_attn_bf16_cases.py's and tests/bert_length_cases.py's; the suite runs
on NaN-poisoned free memory (conftest.py), so every output, workspace and saved buffer of a call starts as NaN; the cotangent is NaN
on padding rows and ``t_valid`` lives on the device."""
import ctypes

import pytest
import torch

from gcgcn_amd import _lib, functional as Fn

import bert_attn_bf16_cases as A
import bert_bf16_cases as C
from bert_cases import model_case
from bert_length_cases import NAN, layer_len_case, pad_mask, run_with_lengths

pytestmark = pytest.mark.gpu

OPTION = b"bf16_rows"      # 1 (default): the bf16 products take the row-block list; 0: they ignore it


class _rows:
    """``with _rows(0):`` the bf16 route ignores the list; the default (1) is restored on the way out."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        _lib.call("gcgcn_set_option", OPTION, self.value)

    def __exit__(self, *exc):
        _lib.call("gcgcn_set_option", OPTION, 1)


def _layer_hip(c, dy, dev, tv, rb, attention="fp32"):
    x = c["x"].to(dev).requires_grad_()
    ps = [t.to(dev).requires_grad_() for t in c["params"]]
    y = Fn.bert_layer(x, None, *ps, matmul="bf16", attention=attention, t_valid=tv, rowblk=rb)
    y.backward(dy.to(dev))
    res = {"y": y.detach(), "dx": x.grad}
    res.update({f"d{i:02d}": t.grad for i, t in enumerate(ps)})
    return res


def _inputs(D, H, B, T, lengths, dev):
    c = layer_len_case(D, H, B, T, lengths)
    tv = torch.tensor(lengths, dtype=torch.int32, device=dev)
    dy = c["dy"].clone()
    pad = pad_mask(lengths, T)
    dy[pad] = NAN
    return c, tv, dy, pad


def _zeros_on(t, pad, name):
    rows = t[pad.to(t.device)]
    assert torch.equal(rows, torch.zeros_like(rows)), f"{name}: padding rows are not exactly zero"


def kept_products(B, T, D, Dff):
    """How many of a layer's twelve bf16 products keep the list, by the rule gemm_bf16.hpp states (every buffer of the layer is 16-byte
    aligned and every leading dimension a multiple of 4, so the rule is one of shapes): M and N multiples of 64, K a multiple of 64.
    Forward y[R, N] = x[R, K] w^T, data gradient dx[R, K] = dy[R, N] w (list on M = R), weight gradient dw[N, K] over K = R rows."""
    R, n = B * T, 0
    for N, K in ((3 * D, D), (D, D), (Dff, D), (D, Dff)):
        n += R % 64 == 0 and N % 64 == 0 and K % 64 == 0          # forward: M = R, N, K
        n += R % 64 == 0 and K % 64 == 0 and N % 64 == 0          # data gradient: M = R, N = K, K = N
        n += N % 64 == 0 and K % 64 == 0 and R % 64 == 0          # weight gradient: M = N, N = K, K = R
    return int(n) if T % 16 == 0 else 0


def _count_rb_launches(fn):
    ms, n, w = ctypes.c_double(), ctypes.c_int(), ctypes.c_double()
    _lib.call("gcgcn_prof_start", b"gemm_bf16_rb", 64)
    try:
        fn()
    finally:
        _lib.call("gcgcn_prof_stop", ctypes.byref(ms), ctypes.byref(n), ctypes.byref(w))
    return n.value


def test_route_the_products_take_the_list(gpu_device):
    """One layer, forward + backward, at (8, 64), D = 128: all twelve products keep the list and are launched as gemm_bf16_rb; none
    is with bf16_rows = 0 or without a list."""
    D, H, B, T = 128, 2, 8, 64
    lengths = (64, 33, 16, 0, 0, 0, 0, 0)
    c, tv, dy, _ = _inputs(D, H, B, T, lengths, gpu_device)
    rb = Fn.row_blocks(tv, B, T)
    want = kept_products(B, T, D, c["params"][10].shape[0])
    assert want == 12
    assert _count_rb_launches(lambda: _layer_hip(c, dy, gpu_device, tv, rb)) == want
    with _rows(0):
        assert _count_rb_launches(lambda: _layer_hip(c, dy, gpu_device, tv, rb)) == 0
    assert _count_rb_launches(lambda: _layer_hip(c, dy, gpu_device, tv, None)) == 0
    assert kept_products(3, 48, D, 4 * D) == 0          # 144 rows: no whole 64-row tiles, every product runs dense
    assert _count_rb_launches(lambda: _rb_layer(3, 48, (48, 0, 17), gpu_device)) == 0


def _rb_layer(B, T, lengths, dev, D=128, H=2):
    c, tv, dy, _ = _inputs(D, H, B, T, lengths, dev)
    return _layer_hip(c, dy, dev, tv, Fn.row_blocks(tv, B, T))


CASES = [
    (4, 64, 128, 2, (64, 33, 16, 0)),                   # a partly live block, a dead document, one tile spanning documents
    (8, 64, 128, 2, (64, 33, 16, 0, 0, 0, 0, 0)),       # weight gradients split K two ways (8 steps); the second run has no live step
    (8, 64, 128, 2, (64, 1, 0, 17, 48, 64, 16, 33)),    # live and dead steps interleaved in both runs
    (1, 512, 128, 2, (88,)),                            # a long document: two live steps of eight
    (2, 128, 256, 4, (128, 19)),                        # the data gradient over K = 3 D = 768 splits: list-aware reduce, rb_zero on NaN dx
    (3, 48, 128, 2, (48, 0, 17)),                       # T % 64 != 0 and B T % 64 != 0: steps straddle documents
    (2, 64, 128, 2, (64, 64)),                          # every block is live
    (2, 64, 128, 2, (0, 0)),                            # nothing is live: all gradients exactly zero
]


@pytest.mark.parametrize("B,T,D,H,lengths", CASES)
def test_list_is_bitwise_the_dense_route_and_within_the_bound(gpu_device, B, T, D, H, lengths):
    c, tv, dy, pad = _inputs(D, H, B, T, lengths, gpu_device)
    rb = Fn.row_blocks(tv, B, T)
    got = _layer_hip(c, dy, gpu_device, tv, rb)
    with _rows(0):
        dense = _layer_hip(c, dy, gpu_device, tv, rb)
    assert len(got) == 18
    for k in got:
        assert not torch.isnan(got[k]).any(), k
        assert torch.equal(got[k], dense[k]), k
    _zeros_on(got["y"], pad, "y")
    _zeros_on(got["dx"], pad, "dx")
    fr = C.worst(got, C.layer_len_reference(D, H, B, T, lengths), f"layer bf16 on row blocks, lengths {lengths} of T={T}")
    assert max(fr.values()) <= 1.0, fr
    if not any(lengths):
        for k in got:
            assert torch.equal(got[k], torch.zeros_like(got[k])), k


@pytest.mark.parametrize("attention", ["fp32", "bf16"])
def test_model_is_bitwise_the_dense_route_and_within_the_bound(gpu_device, attention):
    """The 2-layer BertModel(impl="hip", matmul="bf16") with lengths= at (4, 64): it builds the list itself."""
    D, H, B, T, lengths = 128, 2, 4, 64, (64, 33, 16, 0)
    case = model_case(D, H, B, T)
    model = A.fresh_model(D, H, impl="hip", dtype=torch.float32, device=gpu_device, matmul="bf16", attention=attention)
    got = {k: v.detach().clone() for k, v in run_with_lengths(model, case, lengths).items()}
    with _rows(0):
        dense = run_with_lengths(model, case, lengths)
    for k in got:
        assert torch.equal(got[k], dense[k]), k
    if attention == "fp32":
        fr = C.worst(got, C.model_len_reference(D, H, B, T, lengths), f"model bf16 on row blocks, lengths {lengths}")
    else:
        fr = A.worst(got, A.model_len_reference(D, H, B, T, lengths, "bf16"), f"model bf16 + bf16 core on row blocks, lengths {lengths}", "bf16")
    assert max(fr.values()) <= 1.0, fr


def test_graph_replays_on_new_lengths(gpu_device):
    """A captured forward + backward of one layer, replayed after t_valid.copy_(b) and after gcgcn_row_blocks rebuilt the list in place
    on the same stream: bitwise the eager run on b.  b has more live blocks than a in document 0 and fewer in document 1."""
    D, H, B, T = 128, 2, 4, 64
    a, b = (16, 64, 33, 0), (49, 17, 33, 64)
    c = layer_len_case(D, H, B, T, a)
    x = c["x"].clone()
    x[pad_mask(a, T) & pad_mask(b, T)] = 0.0
    xa, xb = x.clone(), x.clone()
    xa[pad_mask(a, T)] = 0.0
    xb[pad_mask(b, T)] = 0.0
    dy = c["dy"].clone()
    dy[pad_mask(a, T) & pad_mask(b, T)] = NAN          # rows that are padding under both sets of lengths
    dy = dy.to(gpu_device)
    xin =xa.to(gpu_device).requires_grad_()
    ps = [t.to(gpu_device).requires_grad_() for t in c["params"]]
    tv = torch.tensor(a, dtype=torch.int32, device=gpu_device)
    rb = Fn.row_blocks(tv, B, T)
    out = {}

    def step(t_valid, rowblk):
        xin.grad = None
        for t in ps:
            t.grad = None
        y = Fn.bert_layer(xin, None, *ps, matmul="bf16", t_valid=t_valid, rowblk=rowblk)
        y.backward(dy)
        out["y"] = y

    def results():
        r = {"y": out["y"].detach(), "dx": xin.grad}
        r.update({f"d{i:02d}": t.grad for i, t in enumerate(ps)})
        return r

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(tv, rb)
        step(tv, rb)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(tv, rb)
    torch.cuda.synchronize()
    live = results()
    with torch.no_grad():
        xin.copy_(xb.to(gpu_device))
    tv.copy_(torch.tensor(b, dtype=torch.int32, device=gpu_device))
    _lib.call("gcgcn_row_blocks", B, T, tv.data_ptr(), rb.data_ptr(), torch.cuda.current_stream().cuda_stream)
    replays = []
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        replays.append({k: v.detach().clone() for k, v in live.items()})
    tvb = torch.tensor(b, dtype=torch.int32, device=gpu_device)
    step(tvb, Fn.row_blocks(tvb, B, T))
    torch.cuda.synchronize()
    for k, v in results().items():
        assert torch.equal(v, replays[0][k]), k
        assert torch.equal(replays[0][k], replays[1][k]), k
    _zeros_on(replays[0]["y"], pad_mask(b, T), "y")
