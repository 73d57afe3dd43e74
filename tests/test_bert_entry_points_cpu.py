"""The BERT section's exported symbols are forwarders to one checked body per operation (csrc/api.hip).  What that must keep, checked
without a device (the library refuses before any launch): every message names the symbol that was CALLED, the _len entries
require t_valid where _mm does not, and the row-block list's rules."""
import ctypes

import pytest

from gcgcn_amd import _lib

PTR = 16          # a non-null, 16-byte aligned dummy: every call below is refused before anything is dereferenced on the device
LAYER = (2, 32, 128, 2, 256)

# symbol -> leading shape arguments that its first check refuses (T = 513 > 512; D = 96 is no multiple of 64; C = 6 none of 4)
REFUSED_SHAPES = {
    "gcgcn_bert_attn_fwd": (2, 513, 2, 64), "gcgcn_bert_attn_bwd": (2, 513, 2, 64),
    "gcgcn_bert_attn_fwd_len": (2, 513, 2, 64), "gcgcn_bert_attn_bwd_len": (2, 513, 2, 64),
    "gcgcn_res_ln_ws_bytes": (96,),
    "gcgcn_res_ln_fwd": (10, 96), "gcgcn_res_ln_bwd": (10, 96), "gcgcn_res_ln_fwd_len": (10, 96), "gcgcn_res_ln_bwd_len": (10, 96),
    "gcgcn_bias_gelu_fwd": (10, 6), "gcgcn_bias_gelu_bwd": (10, 6), "gcgcn_bias_gelu_fwd_len": (10, 6), "gcgcn_bias_gelu_bwd_len": (10, 6),
    "gcgcn_bert_layer_ws_bytes": (2, 513, 128, 2, 256, 0),
    "gcgcn_bert_layer_fwd": (2, 513, 128, 2, 256), "gcgcn_bert_layer_bwd": (2, 513, 128, 2, 256),
    "gcgcn_bert_layer_fwd_len": (2, 513, 128, 2, 256), "gcgcn_bert_layer_bwd_len": (2, 513, 128, 2, 256),
    "gcgcn_bert_layer_fwd_mm": (2, 513, 128, 2, 256), "gcgcn_bert_layer_bwd_mm": (2, 513, 128, 2, 256),
}


def _fill(name, head):
    """head, then a dummy per remaining argument of the symbol's declared signature."""
    dummy = {_lib.P: PTR, _lib.F: 0.0}
    return tuple(head) + tuple(dummy.get(t, 0) for t in _lib.SIGNATURES[name][1][len(head):])


@pytest.mark.parametrize("name", sorted(REFUSED_SHAPES))
def test_a_refusal_names_the_symbol_that_was_called(name):
    h = _lib.lib()
    assert len(REFUSED_SHAPES) == 20
    assert getattr(h, name)(*_fill(name, REFUSED_SHAPES[name])) != 0
    err = h.gcgcn_last_error().decode()
    assert err.startswith(name[len("gcgcn_"):] + ":"), err


def _ptrs():
    return (ctypes.c_void_p * 12)(*[PTR] * 12)


def _layer_args(direction, t_valid, rowblk, dims=LAYER):
    """The _len argument list with a saved buffer of 0 bytes: the refusal behind the checks of t_valid and rowblk."""
    if direction == "fwd":
        return dims + (PTR, None, t_valid, rowblk, _ptrs(), PTR, PTR, 0, None, 0.0, 0.0, None)
    return dims + (PTR, None, t_valid, rowblk, _ptrs(), PTR, 0, PTR, 2 * PTR, _ptrs(), PTR, 0, None, 0.0, 0.0, None)


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_len_requires_t_valid_and_mm_does_not(direction):
    h = _lib.lib()
    args = _layer_args(direction, None, None)
    assert getattr(h, f"gcgcn_bert_layer_{direction}_len")(*args) != 0
    err = h.gcgcn_last_error().decode()
    assert err.startswith(f"bert_layer_{direction}_len:") and "t_valid is null" in err, err
    assert getattr(h, f"gcgcn_bert_layer_{direction}_mm")(*args, 0) != 0
    err = h.gcgcn_last_error().decode()
    assert err.startswith(f"bert_layer_{direction}_mm:") and "saved activations needed" in err and "which = 0" in err, err
    # and with lengths both get as far
    assert getattr(h, f"gcgcn_bert_layer_{direction}_len")(*_layer_args(direction, PTR, None)) != 0
    err = h.gcgcn_last_error().decode()
    assert err.startswith(f"bert_layer_{direction}_len:") and "saved activations needed" in err, err


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_row_block_rules_of_mm(direction):
    h = _lib.lib()
    fn = getattr(h, f"gcgcn_bert_layer_{direction}_mm")
    assert fn(*_layer_args(direction, None, PTR), 0) != 0
    err = h.gcgcn_last_error().decode()
    assert err.startswith(f"bert_layer_{direction}_mm:") and "without t_valid" in err, err
    assert fn(*_layer_args(direction, PTR, PTR, (2, 24, 128, 2, 256)), 0) != 0
    err = h.gcgcn_last_error().decode()
    assert "multiple of 16" in err and "T = 24" in err, err
    assert fn(*_layer_args(direction, PTR, PTR), 0) != 0       # T = 32 with both: on to the next check
    assert "saved activations needed" in h.gcgcn_last_error().decode()
    assert fn(*_layer_args(direction, PTR, PTR), 2) != 0
    assert "matmul = 2" in h.gcgcn_last_error().decode()
