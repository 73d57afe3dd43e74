"""The BERT graph model's folded front end and [CLS] logit tail, everything that needs no GPU: the folded algebra restated in plain
PyTorch against the float64 definition, the padding rows, the extension header's symbol table (declared == recorded == exported), the
C entries' refusals (made before any launch), and the model switch's validation.  Cases: tests/bert_frontend_cases.py."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from gcgcn_amd import _lib, functional as Fn, models as M

from conftest import GOLDEN
import bert_frontend_cases as C
from lstm_cases import worst


@pytest.mark.parametrize("case", C.SWEEP, ids=lambda c: c.label)
def test_folded_algebra_in_fp32_stays_within_the_bound(case):
    """The restatement (bert_frontend_cases.run_folded) in float32 against the definition in float64, on every case."""
    fr = worst(C.run_folded(case, C.inputs(case), torch.float32), C.reference(case), f"fp32 restatement {case.label}")
    assert max(fr.values()) <= 1.0, fr


@pytest.mark.parametrize("case", [C.SWEEP[2], C.SWEEP[4]], ids=lambda c: c.label)
def test_padding_rows_are_zero_and_dweight_still_sees_the_padding_tokens(case):
    """Gradient rows at both padding indices are exactly 0 -- while the weight's gradient counts the padding tokens: in float64 the
    restatement equals the definition to rounding, and leaving the padding tokens out of dF2 / dF3 moves it far outside the bound."""
    d, ref = C.inputs(case), C.reference(case)
    assert (d["document_pos"] == 0).any() and (d["document_ner"] == 0).any()
    got = C.run_folded(case, d, torch.float64)
    assert not got["dcoref_w"][0].any() and not got["dner_w"][0].any()
    assert not ref["dcoref_w"][0].any() and not ref["dner_w"][0].any()
    assert got["dcoref_w"][1:].abs().max() > 0 and got["dner_w"][1:].abs().max() > 0
    fr = worst(got, ref, f"fp64 restatement {case.label}")
    assert max(fr.values()) <= 1e-3, fr
    # the same with the padding tokens dropped from the per-id sums: the columns of W2 / W3 are wrong
    Dw = case.widths[0]
    dp = (d["dctx"].double() + torch.bmm(d["node_pos"].double().transpose(1, 2), d["dnode"].double())) * (1 - ref["ctx"] ** 2)
    live = (d["document_pos"].reshape(-1) != 0)
    dF2 = torch.zeros(case.P, C.HD, dtype=torch.float64).index_add_(0, d["document_pos"].reshape(-1)[live], dp.reshape(-1, C.HD)[live])
    wrong = dF2.T @ d["coref_w"].double()
    right = ref["dweight"][:, Dw:Dw + case.widths[1]]
    if d["coref_w"][0].abs().max() > 0:
        assert (wrong - right).abs().max() > 1e-2 * right.abs().max()


def test_the_extensions_symbols_declared_recorded_exported():
    """include/gcgcn_bert_frontend.h (symbols gcbf_*) is held the way the other extension headers are: the parsed table equals
    tests/golden/abi_signatures_bert_frontend.json entry by entry, every declared symbol resolves in the library, and the library
    exports no gcbf_* symbol that the header does not declare.  The core table and its version are not touched."""
    sig = _lib.BERT_FRONTEND_SIGNATURES
    names = {ctypes.c_int: "c_int", ctypes.c_int64: "c_int64", ctypes.c_float: "c_float", ctypes.c_void_p: "c_void_p"}
    with open(os.path.join(GOLDEN, "abi_signatures_bert_frontend.json")) as f:
        recorded = json.load(f)
    assert list(sig) == list(recorded) == ["gcbf_context_ws_bytes", "gcbf_context_fwd", "gcbf_context_bwd", "gcbf_logit_bias_ws_bytes",
                                           "gcbf_logit_bias_fwd", "gcbf_logit_bias_bwd"]
    for name, (res, args) in sig.items():
        assert {"restype": names[res], "argtypes": [names[a] for a in args]} == recorded[name], name
    others = set(_lib.SIGNATURES) | set(_lib.OPTIM_SIGNATURES) | set(_lib.BERT_EMBED_SIGNATURES) | set(_lib.PRODUCER_REC_SIGNATURES)
    assert not set(sig) & others and all(n.startswith("gcgcn_") for n in _lib.SIGNATURES)
    assert _lib.ABI_VERSION == 7 and _lib.lib().gcgcn_version() == 7
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in sig:
        assert hasattr(handle, name), f"{name} is declared in include/gcgcn_bert_frontend.h but missing from the library"
    if shutil.which("nm") is not None:
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        assert {line.split()[-1] for line in out.splitlines() if re.fullmatch(r"gcbf_\w+", line.split()[-1])} == set(sig)
    with pytest.raises(RuntimeError, match="not a declaration"):           # a gcgcn_* declaration does not belong in that header
        _lib._parse_header("int gcgcn_x(int n);", _lib._DECL_BERT_FRONTEND)


def _call(name, *args):
    h = _lib.lib()
    rc = getattr(h, name)(*args)
    return rc, h.gcgcn_last_error().decode()


def test_the_c_entries_refuse_before_any_launch():
    """Bad shapes, a null pointer, a padding index outside its table, a short / null / misaligned workspace: status 1 and a message,
    checked before anything is launched (the dummy pointers below are never dereferenced; this machine may have no GPU at all)."""
    h = _lib.lib()
    dims = (2, 5, 3, 64, 20, 20, 16, 7)
    need = h.gcbf_context_ws_bytes(*dims)
    assert need > 4 * 2 * 5 * 128
    for bad, what in (((0,) + dims[1:], "bad shape"), (dims[:4] + (0,) + dims[5:], "width below 1"), (dims[:6] + (0, 7), "bad tables"),
                      ((70000,) + dims[1:], "bad shape")):
        assert h.gcbf_context_ws_bytes(*bad) == -1 and what in h.gcgcn_last_error().decode(), (bad, h.gcgcn_last_error())
    q = 4096                                                               # a non-null, 16-byte aligned dummy address
    rc, msg = _call("gcbf_context_fwd", 0, *dims[1:], *([q] * 12), None)
    assert rc == 1 and "bad shape" in msg
    rc, msg = _call("gcbf_context_fwd", *dims, None, *([q] * 11), None)
    assert rc == 1 and "null pointer" in msg
    rc, msg = _call("gcbf_context_fwd", *dims, *([q] * 9), q + 4, q, q, None)
    assert rc == 1 and "aligned" in msg
    rc, msg = _call("gcbf_context_fwd", *dims, *([q] * 9), q, q, q, None)
    assert rc == 1 and "aliases" in msg
    bwd = lambda cpad, npad, ws, nbytes: _call("gcbf_context_bwd", *dims, *([q] * 10), cpad, npad, *([q] * 5), ws, nbytes, None)
    for ws, nbytes in ((None, need), (q, need - 1), (q + 4, need)):
        rc, msg = bwd(0, 0, ws, nbytes)
        assert rc == 1 and "workspace" in msg, (ws, nbytes, msg)
    rc, msg = bwd(16, 0, q, need)
    assert rc == 1 and "padding index" in msg
    rc, msg = _call("gcbf_context_bwd", *dims, *([q] * 9), None, 0, 0, *([q] * 5), q, need, None)
    assert rc == 1 and "null pointer" in msg
    # the tail
    assert h.gcbf_logit_bias_ws_bytes(2, 5, 97) == 4 * 2 * 5 * 97
    for bad, what in (((0, 5, 97), "bad shape"), ((2, 5, 0), "bad shape"), ((64, 1024, 97), "too large")):
        assert h.gcbf_logit_bias_ws_bytes(*bad) == -1 and what in h.gcgcn_last_error().decode(), bad
    rc, msg = _call("gcbf_logit_bias_fwd", 2, 5, 97, q, None, None, q, None)
    assert rc == 1 and "null pointer" in msg
    rc, msg = _call("gcbf_logit_bias_fwd", 64, 1024, 97, q, q, None, q, None)
    assert rc == 1 and "too large" in msg
    for ws, nbytes in ((None, 3880), (q, 3879), (q + 4, 3880)):
        rc, msg = _call("gcbf_logit_bias_bwd", 2, 5, 97, q, None, q, ws, nbytes, None)
        assert rc == 1 and "workspace" in msg, (ws, nbytes, msg)


def test_the_functions_refuse_cpu_tensors():
    c = C.SWEEP[1]
    d = C.inputs(c)
    with pytest.raises(RuntimeError, match="runs on MI355X only"):
        Fn.bert_token_context(d["states"], d["document_pos"], d["document_ner"], d["coref_w"], d["ner_w"], d["W"], d["b"], d["node_pos"])
    t = C.tail_inputs(2, 5, 97, "none")
    with pytest.raises(RuntimeError, match="runs on MI355X only"):
        Fn.pair_logit_bias(t["logits"], t["cls"])


class _Cfg:
    entity_type_size, coref_size, max_length, keep_prob, graph_hop = 20, 20, 512, 0.8, 2
    dis_size, dis_num, dis_plus, relation_num, alpha = 20, 21, 10, 97, 1.0

    def __init__(self, **kw):
        self.data_word_vec = np.zeros((30, 100), np.float32)
        self.__dict__.update(kw)


def test_config_validation_and_the_state_dict():
    enc = torch.nn.Identity
    with pytest.raises(ValueError, match="set config.frontend_impl='hip' too"):
        M.GraphCNN_multihead_bert_gate_cls(_Cfg(bert_frontend="folded"), bert=enc())
    with pytest.raises(ValueError, match="set config.frontend_impl='hip' too"):
        M.GraphCNN_multihead_bert_gate_cls(_Cfg(bert_frontend="folded", frontend_impl="torch"), bert=enc())
    for bad in ("hip", "Folded", None, 1):
        with pytest.raises(ValueError, match="bert_frontend must be 'cat' or 'folded'"):
            M.GraphCNN_multihead_bert_gate_cls(_Cfg(bert_frontend=bad, frontend_impl="hip"), bert=enc())
    default = M.GraphCNN_multihead_bert_gate_cls(_Cfg(), bert=enc())
    assert default.bert_frontend == "cat"
    assert M.GraphCNN_multihead_bert_gate_cls(_Cfg(bert_frontend="cat"), bert=enc()).bert_frontend == "cat"      # "cat" needs nothing
    folded = M.GraphCNN_multihead_bert_gate_cls(_Cfg(bert_frontend="folded", frontend_impl="hip"), bert=enc())
    assert folded.bert_frontend == "folded"
    # the switch leaves parameters and keys alone: a checkpoint moves freely between the settings
    keys = list(default.state_dict())
    assert keys == list(folded.state_dict()) == list(M.GraphCNN_multihead_bert_gate_cls(_Cfg(frontend_impl="hip"), bert=enc()).state_dict())
    assert [n for n, _ in default.named_parameters()] == [n for n, _ in folded.named_parameters()]
    assert not folded.load_state_dict(default.state_dict(), strict=True).missing_keys
    assert {"linear_re.weight", "linear_cls.weight", "entity_embed.weight", "ner_emb.weight"} <= set(keys)
    assert tuple(default.linear_re.weight.shape) == (128, 808)
