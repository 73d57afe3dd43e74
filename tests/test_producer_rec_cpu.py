"""The record route of the edge-feature producer, everything that needs no GPU: the extension header's symbol table (declared ==
recorded == exported), the C entries' refusals (made before any launch), data.live_counts against a numpy restatement of the dense
tensors on hand-made documents, and the ValueError paths of functional.edge_features / EdgeFeatureProducer."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib, data as D, functional as F_

from conftest import GOLDEN
import producer_rec_cases as C


def test_the_extensions_symbols_declared_recorded_exported():
    """include/gcgcn_producer_rec.h (symbols gcpr_*) is held the way the other extension headers are: the parsed table equals the
    hand-written tests/golden/abi_signatures_producer_rec.json entry by entry, every declared symbol resolves in the library, and the
    library exports no gcpr_* symbol that the header does not declare.  The core table and its version are not touched."""
    sig = _lib.PRODUCER_REC_SIGNATURES
    names = {ctypes.c_int: "c_int", ctypes.c_int64: "c_int64", ctypes.c_float: "c_float", ctypes.c_void_p: "c_void_p"}
    with open(os.path.join(GOLDEN, "abi_signatures_producer_rec.json")) as f:
        recorded = json.load(f)
    assert list(sig) == list(recorded) == ["gcpr_producer_fwd", "gcpr_producer_bwd", "gcpr_producer_bwd_det"]
    for name, (res, args) in sig.items():
        assert {"restype": names[res], "argtypes": [names[a] for a in args]} == recorded[name], name
    others = set(_lib.SIGNATURES) | set(_lib.OPTIM_SIGNATURES) | set(_lib.BERT_EMBED_SIGNATURES)
    assert not set(sig) & others and all(n.startswith("gcgcn_") for n in _lib.SIGNATURES)
    assert _lib.ABI_VERSION == 7 and _lib.lib().gcgcn_version() == 7
    # the dense entries' arguments with (sen, pos_h, pos_t, pos_bytes) replaced by (n_records, records, dis_plus)
    for dense, rec in (("gcgcn_producer_fwd", "gcpr_producer_fwd"), ("gcgcn_producer_bwd", "gcpr_producer_bwd"),
                       ("gcgcn_producer_bwd_det", "gcpr_producer_bwd_det")):
        d, r = _lib.SIGNATURES[dense][1], sig[rec][1]
        assert r == d[:8] + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int] + d[12:], rec
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in sig:
        assert hasattr(handle, name), f"{name} is declared in include/gcgcn_producer_rec.h but missing from the library"
    if shutil.which("nm") is not None:
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
        assert {line.split()[-1] for line in out.splitlines() if re.fullmatch(r"gcpr_\w+", line.split()[-1])} == set(sig)
    with pytest.raises(RuntimeError, match="not a declaration"):           # a gcgcn_* declaration does not belong in that header
        _lib._parse_header("int gcgcn_x(int n);", _lib._DECL_PRODUCER_REC)


def test_the_c_entries_refuse_before_any_launch():
    """A null pointer, a negative count, T > 2048, a short workspace: status 1 and a message, checked before anything is launched
    (the dummy pointers below are never dereferenced; this machine may have no GPU at all)."""
    h = _lib.lib()
    q = 4096                                                               # a non-null, 16-byte aligned dummy address
    B, N, S, T, Hd, P, ND = 2, 3, 2, 8, 64, 5, 21
    need = ctypes.c_int64()
    assert h.gcgcn_producer_det_elems(B, N, Hd, 4, ctypes.cast(ctypes.pointer(need), ctypes.c_void_p)) == 0

    def fwd(shape=(B, N, S, T, Hd, P, ND), ctx=q, n=3, rec=q, ibuf=q, scratch=None, se=0, caps=(4, 4)):
        rc = h.gcpr_producer_fwd(*shape, ctx, n, rec, 10, q, q, None, q, *caps, ibuf, q, scratch, se, q, None)
        return rc, h.gcgcn_last_error().decode()

    def bwd(name, shape=(B, N, S, T, Hd, P, ND), n=3, rec=q, dE=q, tail=()):
        rc = getattr(h, name)(*shape, q, n, rec, 10, q, q, None, q, 4, 4, q, q, q, dE, None, q, q, q, q, *tail, None)
        return rc, h.gcgcn_last_error().decode()

    for kw, what in ((dict(ctx=None), "null pointer"), (dict(rec=None), "null pointer records"), (dict(ibuf=None), "null pointer"),
                     (dict(n=-1), "negative record count"), (dict(shape=(B, N, S, 2049, Hd, P, ND)), "T=2049"),
                     (dict(shape=(B, N, 32, T, Hd, P, ND)), "sentence slots"), (dict(shape=(B, N, 0, T, Hd, P, ND)), "sentence slots"),
                     (dict(shape=(0, N, S, T, Hd, P, ND)), "bad shape"), (dict(shape=(B, N, S, T, 513, P, ND)), "bad shape"),
                     (dict(caps=(-1, 4)), "bad capacities"), (dict(scratch=q, se=-1), "short workspace"), (dict(rec=q + 4), "aligned")):
        rc, msg = fwd(**kw)
        assert rc == 1 and what in msg, (kw, msg)
    for name, tail in (("gcpr_producer_bwd", ()), ("gcpr_producer_bwd_det", (q, need.value))):
        for kw, what in ((dict(rec=None), "null pointer records"), (dict(dE=None), "null pointer"), (dict(n=-2), "negative record count"),
                         (dict(shape=(B, N, S, 4096, Hd, P, ND)), "T=4096")):
            rc, msg = bwd(name, tail=tail, **kw)
            assert rc == 1 and what in msg, (name, kw, msg)
    for tail, what in (((None, need.value), "null pointer detbuf"), ((q, need.value - 1), "short workspace"), ((q + 4, need.value), "aligned")):
        rc, msg = bwd("gcpr_producer_bwd_det", tail=tail)
        assert rc == 1 and what in msg, (tail, msg)


@pytest.mark.parametrize("name", sorted(C.BATCHES))
def test_live_counts_match_the_dense_tensors(name):
    """data.live_counts against a numpy restatement of what gcgcn_tensorise writes into sen_matrix (a record's clipped range set to
    1) and of how the dense route counts it (token 0 of a slot of two real entities)."""
    docs, N, S, T = C.BATCHES[name]()
    sen = C.dense_numpy(docs, N, S, T)[0]
    live = sen[..., 0] != 0
    for b, d in enumerate(docs):
        live[b, d.n:] = False
        live[b, :, d.n:] = False
    want = (int(live.sum()), int(live.any(-1).sum()))
    assert D.live_counts(docs, N, S, T) == want
    if name == "hand":
        assert want[0] > 0 and want[1] < want[0]                          # some pair has more than one live slot
    if name == "none_live":
        assert want == (0, 0)


def test_live_counts_ignore_the_record_order_and_clip():
    docs, N, S, T = C.BATCHES["hand"]()
    want = D.live_counts(docs, N, S, T)
    rng = np.random.default_rng(0)
    for d in docs:
        d.slots = d.slots[rng.permutation(d.slots.shape[0])]
    assert D.live_counts(docs, N, S, T) == want
    assert D.live_counts(docs, N, 1, T)[0] <= want[0] and D.live_counts(docs, 2, S, T)[1] <= 4 * len(docs)


def test_value_errors():
    """Both sources at once, neither, records without S, a table of the wrong dtype / shape, S out of range: ValueError before
    anything touches a GPU; CPU records are refused as every CPU tensor is."""
    t = torch.zeros
    tok, node, table, flat = t(1, 4, 8), t(1, 2, 8), t(5, 3), t(10)
    sen, ph, pt = t(1, 2, 2, 1, 4, dtype=torch.uint8), t(1, 2, 2, 1, 4, dtype=torch.uint8), t(1, 2, 2, 1, 4, dtype=torch.uint8)
    rec = t(3, 10, dtype=torch.int32)
    with pytest.raises(ValueError, match="not both"):
        F_.edge_features(tok, sen, ph, pt, node, table, flat, slot_records=rec, slot_shape=1)
    with pytest.raises(ValueError, match="not both"):
        F_.edge_features(tok, None, ph, None, node, table, flat, slot_records=rec, slot_shape=1)
    with pytest.raises(ValueError, match="required without slot_records"):
        F_.edge_features(tok, None, None, None, node, table, flat)
    with pytest.raises(ValueError, match="needs slot_shape"):
        F_.edge_features(tok, None, None, None, node, table, flat, slot_records=rec)
    for bad in (t(3, 10, dtype=torch.int64), t(3, 9, dtype=torch.int32), t(30, dtype=torch.int32), [[0] * 10]):
        with pytest.raises(ValueError, match="slot_records: expected an int32 tensor"):
            F_.edge_features(tok, None, None, None, node, table, flat, slot_records=bad, slot_shape=1)
    for s in (0, 32, (1, 2, 2, 40)):
        with pytest.raises(ValueError, match="sentence slots per pair"):
            F_.edge_features(tok, None, None, None, node, table, flat, slot_records=rec, slot_shape=s)
    with pytest.raises(RuntimeError, match="MI355X only"):
        F_.edge_features(tok, None, None, None, node, table, flat, slot_records=rec, slot_shape=1)
    prod = gcgcn_amd.EdgeFeatureProducer(8, 3)
    with pytest.raises(ValueError, match="not both"):
        prod(tok, sen, ph, pt, node, table, slot_records=rec, slot_shape=1)
    with pytest.raises(ValueError, match="batched inputs"):
        prod(tok[0], None, None, None, node[0], table, slot_records=rec, slot_shape=1)
