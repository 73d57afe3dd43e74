"""Relation evaluation, the parts that need no GPU: the two forms of the restatement agree exactly, the ordinal decoder inverts
the ordinal formula, the workspace-sizing entry refuses what a 32-bit ordinal cannot hold, and the evaluator refuses CPU tensors."""
import numpy as np
import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib
import eval_restatement as ER


def _sigmoid32(x):
    return torch.sigmoid(torch.from_numpy(x)).numpy()


@pytest.mark.parametrize("theta", [-1, 0.5, 2.0])
@pytest.mark.parametrize("with_train", [False, True])
def test_vectorised_restatement_equals_literal(theta, with_train):
    logits, labels, nv, in_train = ER.tiny_case(seed=3, with_train=with_train)
    docs = ER.crop(_sigmoid32(logits), labels, nv, in_train)
    a, b = ER.literal(docs, 7, input_theta=theta), ER.vectorised(docs, 7, input_theta=theta)
    assert ER.same(a, b)
    assert len(a["ranked"]) == (5 * 4 + 3 * 2) * 6 and a["total_recall"] > 0
    if theta == 2.0:
        assert a["w"] == 0
    # truncation keeps a prefix of the same ranking
    c, d = ER.literal(docs, 7, input_theta=theta, max_n=50), ER.vectorised(docs, 7, input_theta=theta, max_n=50)
    assert ER.same(c, d) and c["ranked"] == a["ranked"][:50]


def test_restatement_ties_keep_append_order():
    logits, labels, nv, _ = ER.tiny_case(seed=5)
    docs = ER.crop(_sigmoid32(logits), labels, nv)
    res = ER.literal(docs, 7)
    recs = res["ranked"]
    score = {(ix, h, t, r): float(docs[ix][0][h, t, r]) for _, ix, h, t, r in recs}
    order = [(-score[x[1:]], x[1:]) for x in recs]                   # (index, h, t, r) ascending IS the append order
    assert order == sorted(order) and len({s for s, _ in order}) < len(order) // 2, "the case must hold many exact ties"


def test_decode_ordinals_inverts_the_formula():
    R = 7
    doc_n = torch.tensor([3, 0, 1, 2, 5, 1, 4])
    want, o = [], 0
    for index, n in enumerate(doc_n.tolist()):
        base = o
        for i in range(n):
            for j in range(n):
                if i == j:
                    continue
                jp = j - (1 if j > i else 0)
                for k in range(1, R):
                    assert o == base + (i * (n - 1) + jp) * (R - 1) + (k - 1)
                    want.append((index, i, j, k))
                    o += 1
    assert o == int(gcgcn_amd.evaluation.record_counts(doc_n, R).sum()) == (6 + 2 + 20 + 12) * 6
    got = torch.stack(gcgcn_amd.evaluation.decode_ordinals(torch.arange(o), doc_n, R), 1)
    assert got.dtype == torch.int64 and got.tolist() == [list(x) for x in want]
    perm = torch.randperm(o, generator=torch.Generator().manual_seed(0))
    assert torch.equal(torch.stack(gcgcn_amd.evaluation.decode_ordinals(perm, doc_n, R), 1), got[perm])


def test_exports():
    assert gcgcn_amd.RelationEvaluator is gcgcn_amd.evaluation.RelationEvaluator
    assert gcgcn_amd.evaluate is gcgcn_amd.evaluation.evaluate
    assert {"RelationEvaluator", "evaluate", "EvalResult"} <= set(gcgcn_amd.__all__)
    ev = gcgcn_amd.RelationEvaluator()
    assert ev.relation_num == 97 and ev.max_n == 1_000_000 and ev.n_records == 0


def test_update_refuses_cpu_tensors():
    ev = gcgcn_amd.RelationEvaluator(relation_num=7)
    x = torch.zeros(2, 4, 4, 7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.update(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.update(x[0], x[0])
    assert ev.n_records == 0
    with pytest.raises(ValueError, match="no records"):
        ev.compute()


def test_workspace_sizing_refuses_more_records_than_an_ordinal_holds():
    lib = _lib.lib()
    small = lib.gcgcn_eval_ws_bytes(50_688, 1000)
    assert small >= 2 * 8 * 50_688                                    # two ranking buffers at the least
    assert lib.gcgcn_eval_ws_bytes(2 ** 32 - 1, 10 ** 6) > 0
    assert lib.gcgcn_eval_ws_bytes(2 ** 32, 10 ** 6) == -1
    assert b"32-bit ordinal" in lib.gcgcn_last_error()
    ev = gcgcn_amd.RelationEvaluator()
    with pytest.raises(RuntimeError, match="32-bit ordinal"):
        ev._reserve(2 ** 32, torch.device("cpu"))                     # raised before anything is allocated
