"""Host side of the bf16 Linears on row blocks (tests/test_bert_bf16_rows_gpu.py has the device side): the run-time switch exists, no
symbol or workspace size moved.  The launcher's keep-or-drop rule (gemm_bf16.hpp) is not exposed to the host; the GPU route test counts
its launches instead."""
from gcgcn_amd import _lib


def test_option_bf16_rows_is_known():
    """gcgcn_set_option(b"bf16_rows", v) returns 0 for both values; the default (1) is put back."""
    h = _lib.lib()
    try:
        assert h.gcgcn_set_option(b"bf16_rows", 0) == 0
    finally:
        assert h.gcgcn_set_option(b"bf16_rows", 1) == 0
    assert h.gcgcn_set_option(b"bf16_row", 1) != 0          # a near miss stays unknown


def test_no_symbol_and_no_workspace_moved():
    """ABI 7 as it was: the layer's entry points already carry rowblk, and the row-block route uses the backward's existing split region."""
    h = _lib.lib()
    assert h.gcgcn_version() == 7
    B, T, D, H, Dff = 8, 256, 768, 12, 3072
    R, W = B * T, 3072
    up4 = lambda n: (n + 3) & ~3
    split = min(16 * W * D, 16 << 20)
    res_ln = h.gcgcn_res_ln_ws_bytes(D) // 4
    want = 3 * up4(R * D) + up4(R * W) + up4(B * H * T) + up4(split) + up4(128 * W) + up4(res_ln)
    assert h.gcgcn_bert_layer_ws_bytes(B, T, D, H, Dff, 1) == 4 * want
