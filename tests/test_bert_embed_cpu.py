"""The fused embeddings stage of the HIP BERT encoder, everything that needs no GPU: the extension header's symbol table (declared ==
recorded == exported), the C entries' refusals (made before any launch, so they run here), the switch's validation in BertModel and in
GraphCNN_multihead_bert_gate_cls, and impl="torch" computing one contract under both settings.  Cases: tests/bert_embed_cases.py."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from gcgcn_amd import _lib, models as M
from gcgcn_amd.bert import BertConfig, BertModel

from conftest import GOLDEN
import bert_embed_cases as C


def test_the_extensions_symbols_declared_recorded_exported():
    """include/gcgcn_bert_embed.h (symbols gcbe_*) is held the way tests/test_optim_decay_cpu.py holds include/gcgcn_optim.h: the
    parsed table equals the hand-written tests/golden/abi_signatures_bert_embed.json entry by entry, every declared symbol resolves
    in the library, and the library exports no gcbe_* symbol that the header does not declare.  The core table is not touched."""
    sig = _lib.BERT_EMBED_SIGNATURES
    names = {ctypes.c_int: "c_int", ctypes.c_int64: "c_int64", ctypes.c_float: "c_float", ctypes.c_void_p: "c_void_p"}
    with open(os.path.join(GOLDEN, "abi_signatures_bert_embed.json")) as f:
        recorded = json.load(f)
    assert list(sig) == list(recorded) == ["gcbe_ws_bytes", "gcbe_fwd", "gcbe_bwd"]
    for name, (res, args) in sig.items():
        assert {"restype": names[res], "argtypes": [names[a] for a in args]} == recorded[name], name
    assert not set(sig) & (set(_lib.SIGNATURES) | set(_lib.OPTIM_SIGNATURES)) and all(n.startswith("gcgcn_") for n in _lib.SIGNATURES)
    assert _lib.ABI_VERSION == 7 and _lib.lib().gcgcn_version() == 7
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in sig:
        assert hasattr(handle, name), f"{name} is declared in include/gcgcn_bert_embed.h but missing from the library"
    if shutil.which("nm") is not None:
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        assert {line.split()[-1] for line in out.splitlines() if re.fullmatch(r"gcbe_\w+", line.split()[-1])} == set(sig)
    with pytest.raises(RuntimeError, match="not a declaration"):           # a gcgcn_* declaration does not belong in that header
        _lib._parse_header("int gcgcn_x(int n);", _lib._DECL_BERT_EMBED)


def _call(name, *args):
    h = _lib.lib()
    rc = getattr(h, name)(*args)
    return rc, h.gcgcn_last_error().decode()


def test_the_c_entries_refuse_before_any_launch():
    """Bad shapes, a null pointer, dropout without a snapshot, a short / null / misaligned workspace: status 1 and a message, checked
    before anything is launched (the dummy pointers below are never dereferenced; this machine may have no GPU at all)."""
    h = _lib.lib()
    B, T, D, Pmax = 2, 5, 64, 8
    assert h.gcbe_ws_bytes(B, T, D, C.V, Pmax, C.TY) > 4 * B * T * D
    for bad, what in (((B, T, 96, C.V, Pmax, C.TY), "multiple of 64"), ((B, T, 1088, C.V, Pmax, C.TY), "at most 1024"),
                      ((B, 9, D, C.V, Pmax, C.TY), "exceeds the position table"), ((0, T, D, C.V, Pmax, C.TY), "bad shape"),
                      ((B, T, D, 0, Pmax, C.TY), "bad tables")):
        assert h.gcbe_ws_bytes(*bad) == -1 and what in h.gcgcn_last_error().decode(), (bad, h.gcgcn_last_error())
    q = 4096                                                               # a non-null, 16-byte aligned dummy address
    fwd = [q] * 7 + [None] + [q] * 3
    for bad, what in (((B, T, 96, C.V, Pmax, C.TY), "multiple of 64"), ((B, 9, D, C.V, Pmax, C.TY), "exceeds the position table")):
        rc, msg = _call("gcbe_fwd", *bad, *fwd, None, 0.0, None)
        assert rc == 1 and what in msg, msg
    rc, msg = _call("gcbe_fwd", B, T, D, C.V, Pmax, C.TY, *fwd, None, 0.1, None)
    assert rc == 1 and "without an rng snapshot" in msg
    rc, msg = _call("gcbe_fwd", B, T, D, C.V, Pmax, C.TY, None, *fwd[1:], None, 0.0, None)
    assert rc == 1 and "null pointer" in msg
    need = h.gcbe_ws_bytes(B, T, D, C.V, Pmax, C.TY)
    bwd = [q] * 6 + [None] + [q] * 8
    for ws, nbytes in ((None, need), (q, need - 1), (q + 4, need)):
        rc, msg = _call("gcbe_bwd", B, T, D, C.V, Pmax, C.TY, *bwd, ws, nbytes, None, 0.0, None)
        assert rc == 1 and "workspace" in msg, (ws, nbytes, msg)
    rc, msg = _call("gcbe_bwd", B, T, 96, C.V, Pmax, C.TY, *bwd, q, need, None, 0.0, None)
    assert rc == 1 and "multiple of 64" in msg


def test_constructor_validation():
    c = C.config(64, 8)
    for impl in ("torch", "hip"):
        for emb in ("torch", "fused"):
            assert BertModel(c, impl=impl, embeddings=emb).embeddings_impl == emb
        for bad in ("hip", "Fused", None, 1):
            with pytest.raises(ValueError, match="embeddings must be 'torch' or 'fused'"):
                BertModel(c, impl=impl, embeddings=bad)
    assert BertModel(c).embeddings_impl == "torch"                         # the default
    # the switch leaves the parameters' names alone: a checkpoint moves freely between the settings
    assert list(BertModel(c, embeddings="fused").state_dict()) == list(BertModel(c).state_dict())


class _Cfg:
    entity_type_size, coref_size, max_length, keep_prob, graph_hop = 20, 20, 512, 0.8, 2
    dis_size, dis_num, dis_plus, relation_num, alpha = 20, 21, 10, 97, 1.0

    def __init__(self, **kw):
        self.data_word_vec = np.zeros((30, 100), np.float32)
        self.__dict__.update(kw)


def test_config_validation():
    bc = BertConfig(vocab_size=30, hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=128,
                    max_position_embeddings=16)
    with pytest.raises(ValueError, match="set config.bert_impl too"):
        M.GraphCNN_multihead_bert_gate_cls(_Cfg(bert_embeddings="fused"), bert=torch.nn.Identity())
    with pytest.raises(ValueError, match="bert_embeddings must be 'torch' or 'fused'"):
        M.GraphCNN_multihead_bert_gate_cls(_Cfg(bert_impl="hip", bert_config=bc, bert_embeddings="hip"))
    for impl in ("torch", "hip"):                                          # independent of bert_matmul / bert_attention
        for extra in ({}, {"bert_matmul": "bf16"}, {"bert_attention": "bf16"}):
            m = M.GraphCNN_multihead_bert_gate_cls(_Cfg(bert_impl=impl, bert_config=bc, bert_embeddings="fused", **extra))
            assert m.bert.embeddings_impl == "fused" and m.bert.impl == impl
    m = M.GraphCNN_multihead_bert_gate_cls(_Cfg(bert_impl="hip", bert_config=bc))
    assert m.bert.embeddings_impl == "torch"
    assert list(m.state_dict()) == list(M.GraphCNN_multihead_bert_gate_cls(_Cfg(bert_impl="hip", bert_config=bc,
                                                                                 bert_embeddings="fused")).state_dict())


@pytest.mark.parametrize("case", [C.CASES[1], C.CASES[3], C.CASES[6]], ids=C.case_id)
def test_impl_torch_computes_one_contract_under_both_settings(case):
    """impl="torch" in float64: embeddings="fused" and "torch" give the same output and gradients, bit for bit (it is one code path),
    and with lengths the padding rows of the output and the gradient rows of ids that occur on padding only are exactly zero."""
    D, B, T, extra, tt_kind, len_kind, p = case
    inp = C.inputs(D, B, T, tt_kind, len_kind)
    a = C.run_stage(C.build(D, T + extra, 0.0, torch.float64, embeddings="fused"), inp)
    b = C.run_stage(C.build(D, T + extra, 0.0, torch.float64, embeddings="torch"), inp)
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.isfinite(a[k]).all(), k
    if inp["lengths"] is not None:
        pad = torch.arange(T)[None, :] >= inp["lengths"][:, None]
        assert pad.any() and (a["y"][pad] == 0).all()
        assert (a["dW"][list(C.NEVER_LIVE)] == 0).all() and (a["dP"][int(inp["lengths"].max()):] == 0).all()


def test_the_hip_model_refuses_cpu_tensors_under_both_settings():
    for emb in ("torch", "fused"):
        model = C.build(64, 8, 0.0, impl="hip", embeddings=emb)
        with pytest.raises(RuntimeError, match="runs on MI355X only"):
            model(torch.zeros(1, 3, dtype=torch.int64))
