"""The bit-reproducible producer backward (csrc/producer.hip: prod_sent_bwd_det / prod_nterm_owner / prod_dwb_fin behind
gcgcn_producer_bwd_det): what holds without a GPU.  The two additive symbols are declared, bound and exported; the workspace size
is the documented formula and its refusals answer on the host; every switch defaults to off and a model's config reaches its tail."""
import ctypes

import numpy as np
import pytest

import gcgcn_amd
from gcgcn_amd import _lib, models as M

PGRID = 2048                      # workgroups of the producer's row kernels (csrc/producer.hip): one partial row each


def _det_elems(Hd, cap_pairs):
    """include/gcgcn.h: rows of Ec (the capacity rounded up to 64) x 2 x Hd, plus PGRID x (Hd + 1), each rounded to 16 bytes."""
    up4 = lambda v: (v + 3) & ~3
    return up4(((cap_pairs + 63) & ~63) * 2 * Hd) + up4(PGRID * (Hd + 1))


def test_symbols_are_declared_bound_and_exported():
    """The deterministic entry is the default entry's argument list with (detbuf, det_elems) in front of the stream.  (That the two
    lists are the header's and the symbols the library's: tests/test_abi_cpu.py.)"""
    base, det = _lib.SIGNATURES["gcgcn_producer_bwd"][1], _lib.SIGNATURES["gcgcn_producer_bwd_det"][1]
    assert det == base[:-1] + [_lib.P, _lib.L] + base[-1:]
    assert _lib.ABI_VERSION == 7 and _lib.lib().gcgcn_version() == 7                       # additive


@pytest.mark.parametrize("B,N,Hd,cap", [(2, 6, 64, 10), (1, 42, 128, 1764)])
def test_det_elems_is_the_documented_formula(B, N, Hd, cap):
    out = ctypes.c_int64(-1)
    _lib.call("gcgcn_producer_det_elems", B, N, Hd, cap, ctypes.cast(ctypes.pointer(out), ctypes.c_void_p))
    assert out.value == _det_elems(Hd, cap)
    assert out.value % 4 == 0


def test_det_elems_refusals():
    h = _lib.lib()
    out = ctypes.c_int64(-1)
    po = ctypes.cast(ctypes.pointer(out), ctypes.c_void_p)
    assert h.gcgcn_producer_det_elems(2, 6, 0, 10, po) != 0 and b"Hd" in h.gcgcn_last_error()
    assert h.gcgcn_producer_det_elems(2, 6, -3, 10, po) != 0 and b"Hd" in h.gcgcn_last_error()
    assert h.gcgcn_producer_det_elems(2, 6, 64, -1, po) != 0 and b"cap_pairs" in h.gcgcn_last_error()
    assert h.gcgcn_producer_det_elems(2, 6, 64, 10, None) != 0
    assert out.value == -1                                                # a refused call writes nothing
    with pytest.raises(RuntimeError, match="cap_pairs"):
        _lib.call("gcgcn_producer_det_elems", 2, 6, 64, -1, po)


class _Cfg:
    entity_type_size, coref_size, max_length, keep_prob, graph_hop = 20, 20, 512, 0.8, 2
    dis_size, dis_num, dis_plus, relation_num, alpha = 20, 21, 10, 97, 1.0

    def __init__(self, **kw):
        self.data_word_vec = np.zeros((30, 100), np.float32)
        self.__dict__.update(kw)


def test_every_switch_defaults_to_off():
    assert gcgcn_amd.EdgeFeatureProducer.deterministic is False and gcgcn_amd.GraphModelTail.deterministic is False
    assert gcgcn_amd.EdgeFeatureProducer(24, 7).deterministic is False
    tail = gcgcn_amd.GraphModelTail()
    assert tail.deterministic is False and all(p.deterministic is False for p in tail.producers)
    plain = M.GCGCN_glove(_Cfg())
    assert plain.deterministic is False and not hasattr(plain.config, "deterministic")


def test_config_reaches_the_tail():
    opted = M.GCGCN_glove(_Cfg(deterministic=True))
    assert isinstance(opted, gcgcn_amd.GraphModelTail) and opted.deterministic is True
    assert M.GCGCN_glove(_Cfg(deterministic=0)).deterministic is False
    # an instance override, as with check_capacity: the class default is untouched
    prod = gcgcn_amd.EdgeFeatureProducer(24, 7)
    prod.deterministic = True
    assert prod.deterministic is True and gcgcn_amd.EdgeFeatureProducer.deterministic is False
    assert list(opted.state_dict().keys()) == list(M.GCGCN_glove(_Cfg()).state_dict().keys())
