"""Training accuracy counters, the parts that need no GPU: the symbol is declared, bound and exported; the two forms of the
restatement agree and the guard on its inputs holds on every case the GPU tests use; CPU tensors are refused; ``pair_bce_loss``
keeps its signature; the epoch's log line is the reference's."""
import inspect

import numpy as np
import pytest
import torch

import gcgcn_amd
from gcgcn_amd import _lib
import train_stats_restatement as TR
from train_stats_restatement import SHAPE_IDS, SHAPES


def test_symbol_is_declared_bound_and_exported():
    """gcgcn_pair_stats against the header and the library (its eight arguments, type by type): tests/test_abi_cpu.py."""
    lib = _lib.lib()
    assert _lib.ABI_VERSION == 7 and lib.gcgcn_version() == 7                              # additive
    assert lib.gcgcn_pair_stats(0, 4, 7, None, None, None, None, None) == 1               # refused before any launch
    assert b"pair_stats: bad shape" in lib.gcgcn_last_error()
    assert lib.gcgcn_pair_stats(1, 4, 7, None, None, None, None, None) == 1
    assert b"pair_stats: null pointer" in lib.gcgcn_last_error()
    for name in ("TrainStats", "TrainStatsResult", "train_epoch", "TrainEpochResult"):
        assert name in gcgcn_amd.__all__ and callable(getattr(gcgcn_amd, name))
    assert gcgcn_amd.TrainStats is gcgcn_amd.functional.TrainStats
    assert gcgcn_amd.train_epoch is gcgcn_amd.training.train_epoch


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_vectorised_restatement_equals_literal_and_guard_holds(shape):
    B, N, R, nv = shape
    logits, labels, n_valid = TR.make_case(11, B, N, R, nv)
    pairs = sum(n * n - n for n in ([N] * B if nv is None else nv))
    assert TR.guard(logits, n_valid) == pairs
    counters, accs = TR.literal(logits, labels, n_valid)
    assert counters == TR.vectorised(logits, labels, n_valid)
    assert counters[5] == pairs == counters[1] + counters[3] and counters[4] == counters[0] + counters[2]
    assert counters[6] == 0 and counters[7] == B
    assert [a.total for a in accs] == [counters[1], counters[3], counters[5]]
    one, _ = TR.literal(logits[0], labels[0])                                              # an unbatched document
    assert one == TR.vectorised(logits[0], labels[0]) and one[7] == 1


def test_planted_rows_restatement():
    logits, labels, _ = TR.make_case(5, 2, 6, 97)
    base, _ = TR.literal(logits, labels)
    want = TR.plant(logits, labels, b=1)
    assert TR.guard(logits) == 2 * 30 - 1                                                  # the NaN row is not a pair to guard
    rstar = TR.first_argmax(logits[1])
    for (h, t), r in want.items():
        if r is not None:
            assert rstar[h, t] == r, (h, t)
    counters, _ = TR.literal(logits, labels)
    assert counters == TR.vectorised(logits, labels)
    assert counters[6] == 1 and counters[5] == base[5] - 1 and counters[7] == 2
    # the NaN row alone: counter [6] and the document, nothing else
    x, y = logits[1:, 2:4, 2:4].copy(), labels[1:, 2:4, 2:4].copy()
    x[0, 0, 1], x[0, 1, 0] = logits[1, 2, 1], logits[1, 2, 1]
    assert TR.literal(x, y)[0] == (0, 0, 0, 0, 0, 0, 2, 1) == TR.vectorised(x, y)


def test_guard_refuses_what_it_should():
    x = np.full((1, 2, 2, 3), -6.0, np.float32)
    x[0, 0, 1] = [6.0, 5.99, -6.0]                                                         # runner-up 5e-6 below the maximum
    with pytest.raises(AssertionError, match="runner-up"):
        TR.guard(x)
    x[0, 0, 1] = [18.0, 19.0, -6.0]                                                        # p == 1 for both, by rounding only
    with pytest.raises(AssertionError, match="by accident"):
        TR.guard(x)
    x[0, 0, 1] = [20.0, 45.0, 6.0]
    assert TR.guard(x) == 2


def test_accuracy_get_and_result_properties():
    a = TR.Accuracy()
    assert a.get() == 0.0
    a.add(True), a.add(False), a.add(np.float32(1.0) == 1)
    assert (a.correct, a.total) == (2, 3) and a.get() == 2 / 3
    r = gcgcn_amd.TrainStatsResult(1, 2, 1, 4, 2, 6, 0, 3)
    assert r.counters == (1, 2, 1, 4, 2, 6, 0, 3)
    assert (r.na_acc, r.not_na_acc, r.total_acc) == (0.5, 0.25, 2 / 6)
    z = gcgcn_amd.TrainStatsResult(*[0] * 8)
    assert (z.na_acc, z.not_na_acc, z.total_acc) == (0.0, 0.0, 0.0) and isinstance(z.na_acc, float)


def test_cpu_tensors_are_refused():
    x = torch.zeros(2, 4, 4, 7)
    stats = gcgcn_amd.TrainStats()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stats.update(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        stats.update(x[0], x[0])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gcgcn_amd.pair_bce_loss(x, x, stats=stats)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gcgcn_amd.TrainStats("cpu")
    with pytest.raises(TypeError, match="TrainStats"):
        gcgcn_amd.pair_bce_loss(x, x, stats=object())


def test_pair_bce_loss_without_stats_is_what_it_was():
    params = inspect.signature(gcgcn_amd.pair_bce_loss).parameters
    assert list(params) == ["logits", "labels", "n_valid", "stats"]
    assert params["n_valid"].default is None and params["stats"].default is None
    assert all(p.kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for p in params.values())
    x = torch.zeros(2, 4, 4, 7)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gcgcn_amd.pair_bce_loss(x, x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        gcgcn_amd.pair_bce_loss(x[0], x[0], None)


def test_log_line_is_the_reference_format():
    stats = gcgcn_amd.TrainStatsResult(1, 2, 1, 4, 2, 6, 0, 3)
    res = gcgcn_amd.TrainEpochResult(loss_sum=1.23456, n_documents=3, n_steps=2, stats=stats)
    assert res.log_line(3, 12.345) == ("| epoch  3 | ms/b 12.35 | train loss 1.235 | NA acc: 0.50 | not NA acc: 0.25  "
                                       "| tot acc: 0.33 ")
    empty = gcgcn_amd.TrainEpochResult(0.0, 0, 0, gcgcn_amd.TrainStatsResult(*[0] * 8))
    assert empty.log_line(12, 100.0) == ("| epoch 12 | ms/b 100.00 | train loss 0.000 | NA acc: 0.00 | not NA acc: 0.00  "
                                         "| tot acc: 0.00 ")
