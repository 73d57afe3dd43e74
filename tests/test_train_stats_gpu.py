"""Training accuracy counters on the device (``gcgcn_pair_stats`` behind ``TrainStats``, ``pair_bce_loss(stats=)`` and
``train_epoch``) against the restatement of config/Config.py:377-393 in tests/train_stats_restatement.py.  The counters are
integers and must be EQUAL; the guard of the restatement runs on every case's inputs first, so the expected first argmax does
not depend on the last ulp of the device's ``expf``.  The loss with ``stats`` must be bit-equal to the loss without."""
import numpy as np
import pytest
import torch

import gcgcn_amd
from gcgcn_amd.evaluation import FORWARD_KEYS
import train_stats_restatement as TR
from train_stats_restatement import SHAPE_IDS, SHAPES

pytestmark = pytest.mark.gpu


def _dev(dev, logits, labels, n_valid):
    return (torch.from_numpy(logits).to(dev), torch.from_numpy(labels).to(dev),
            None if n_valid is None else torch.from_numpy(n_valid).to(dev))


def _same_bits(a, b):
    """torch.equal on the bit patterns: a document without pairs has the loss 0 / 0 = NaN, with and without stats."""
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.view(torch.int32), b.view(torch.int32))


def _expected(logits, labels, n_valid):
    TR.guard(logits, n_valid)                                         # a condition on the inputs, checked before the device's result
    want = TR.vectorised(logits, labels, n_valid)
    assert want == TR.literal(logits, labels, n_valid)[0]
    return want


@pytest.mark.parametrize("shape", SHAPES, ids=SHAPE_IDS)
def test_counters_equal_the_restatement(gpu_device, shape):
    B, N, R, nv = shape
    logits, labels, n_valid = TR.make_case(11, B, N, R, nv)
    want = _expected(logits, labels, n_valid)
    x, y, nvd = _dev(gpu_device, logits, labels, n_valid)
    stats = gcgcn_amd.TrainStats(gpu_device)
    loss = gcgcn_amd.pair_bce_loss(x, y, nvd, stats=stats)
    got = stats.get()
    print(f"{shape}: device {got.counters} restatement {want}")
    assert got.counters == want
    assert got.documents == B and got.total == sum(n * n - n for n in ([N] * B if nv is None else nv))
    assert _same_bits(loss, gcgcn_amd.pair_bce_loss(x, y, nvd))
    direct = gcgcn_amd.TrainStats(gpu_device)
    direct.update(x, y, nvd)
    assert direct.get() == got


def test_unbatched_document(gpu_device):
    logits, labels, _ = TR.make_case(3, 1, 6, 97)
    want = _expected(logits[0], labels[0], None)
    x, y, _ = _dev(gpu_device, logits, labels, None)
    stats = gcgcn_amd.TrainStats(gpu_device)
    loss = gcgcn_amd.pair_bce_loss(x[0], y[0], stats=stats)
    assert loss.dim() == 0 and torch.equal(loss, gcgcn_amd.pair_bce_loss(x[0], y[0]))
    assert stats.get().counters == want and want[7] == 1 and want[5] == 30
    stats.reset()
    stats.update(x[0], y[0].to(torch.float64))                        # labels of another dtype are converted, as by the loss
    assert stats.get().counters == want


def test_planted_rows(gpu_device):
    logits, labels, _ = TR.make_case(5, 2, 6, 97)
    expect = TR.plant(logits, labels, b=1)
    rstar = TR.first_argmax(logits[1])
    assert all(rstar[h, t] == r for (h, t), r in expect.items() if r is not None)
    want = _expected(logits, labels, None)
    assert want[6] == 1
    x, y, _ = _dev(gpu_device, logits, labels, None)
    stats = gcgcn_amd.TrainStats(gpu_device)
    stats.update(x, y)
    print(f"planted: device {stats.get().counters} restatement {want}")
    assert stats.get().counters == want
    # each planted row alone, as the only pair (h = 0, t = 1) of a two-entity document: a wrong r* flips its own counters
    for (h, t), r in expect.items():
        x1, y1 = torch.zeros(1, 2, 2, 97, device=gpu_device), torch.zeros(1, 2, 2, 97, device=gpu_device)
        x1[0, 0, 1], y1[0, 0, 1] = x[1, h, t], y[1, h, t]
        x1[0, 1, 0, 96], y1[0, 1, 0, 96] = 3.0, 1.0                   # the other pair: r* = 96, a not-NA hit
        stats.reset()
        stats.update(x1, y1)
        want1 = TR.vectorised(x1.cpu().numpy(), y1.cpu().numpy())
        assert stats.get().counters == want1, (h, t, r)
        if r is None:
            assert want1 == (0, 0, 1, 1, 1, 1, 1, 1)                  # the NaN row moved counter [6] only
        else:
            hit, na = int(labels[1, h, t, r] == 1), int(labels[1, h, t, 0] == 1)
            assert want1 == (na * hit, na, 1 + (1 - na) * hit, 2 - na, 1 + hit, 2, 0, 1)


def test_updates_accumulate_reset_zeroes_runs_repeat(gpu_device):
    a = TR.make_case(21, 2, 5, 97, (5, 3))
    b = TR.make_case(22, 3, 6, 65, (6, 0, 2))
    wa, wb = _expected(*a), _expected(*b)
    da, db = _dev(gpu_device, *a), _dev(gpu_device, *b)
    stats = gcgcn_amd.TrainStats(gpu_device)
    stats.update(*da)
    stats.update(*db)
    assert stats.get().counters == TR.add(wa, wb)
    stats.reset()
    assert stats.get().counters == (0,) * 8
    stats.update(*db)
    assert stats.get().counters == wb
    again = gcgcn_amd.TrainStats(gpu_device)                          # two fresh runs are equal
    again.update(*da)
    again.update(*db)
    stats.update(*da)
    assert again.get() == stats.get()
    with pytest.raises(ValueError):
        stats.update(da[0], da[1][:, :, :3])
    with pytest.raises(ValueError):
        stats.update(da[0], da[1], da[2][:1])


class _Stub(torch.nn.Module):
    """logits = document * w with one parameter: a model whose logits the test knows (w stays within 1e-4 of 1, far inside the
    guard's margin: equal inputs stay tied, saturated ones stay saturated, and a grid step moves q by >= 2.4e-4)."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(()))
        self.seen = []

    def forward(self, document, *rest, n_valid=None, t_valid=None):
        assert len(rest) == len(FORWARD_KEYS) - 1
        self.seen.append((n_valid, t_valid, self.training))
        return document * self.w


def test_counts_inside_a_captured_step(gpu_device):
    B, N, R, nv = 2, 5, 9, (5, 3)
    cases = [TR.make_case(31 + i, B, N, R, nv) for i in range(3)]
    want = TR.add(*[_expected(*c) for c in cases])
    model = _Stub().to(gpu_device)
    opt = gcgcn_amd.FusedAdam(model.parameters(), lr=1e-6, capturable=True)
    stats = gcgcn_amd.TrainStats(gpu_device)

    def step_fn(logits, labels, n_valid):
        return gcgcn_amd.pair_bce_loss(model(logits, *[None] * 9), labels, n_valid, stats=stats).sum() / B

    x0, y0, nvd = _dev(gpu_device, *cases[0])
    train = gcgcn_amd.GraphedTrainStep(step_fn, opt, {"logits": x0.clone(), "labels": y0.clone(), "n_valid": nvd})
    assert stats.get().documents == 3 * B                             # the three warm-up steps ran for real
    stats.reset()
    for c in cases:
        x, y, _ = _dev(gpu_device, *c)
        train(logits=x, labels=y)
    got = stats.get()
    assert got.counters == want and got.documents == 3 * B
    assert 0 < abs(model.w.item() - 1.0) < 1e-4


def _batch(dev, case, with_t_valid):
    x, y, nvd = _dev(dev, *case)
    bt = {k: torch.zeros(1, device=dev) for k in FORWARD_KEYS}
    bt.update(document=x, label_matrix=y, n_valid=nvd)
    if with_t_valid:
        bt["t_valid"] = torch.tensor([7, 4], dtype=torch.int32, device=dev)
    return bt


def test_train_epoch(gpu_device):
    cases = [TR.make_case(41, 2, 5, 9, (2, 5)), TR.make_case(42, 2, 5, 9, (4, 3))]
    want = TR.add(*[_expected(*c) for c in cases])
    batches = [_batch(gpu_device, cases[0], True), _batch(gpu_device, cases[1], False)]
    eager, sums = _Stub().to(gpu_device), []
    opt_e = torch.optim.SGD(eager.parameters(), lr=1e-5)
    for bt in batches:                                                # the same steps by hand, without stats
        opt_e.zero_grad(set_to_none=True)
        loss = gcgcn_amd.pair_bce_loss(eager(bt["document"], *[None] * 9), bt["label_matrix"], bt["n_valid"]).sum()
        (loss / 2).backward()
        opt_e.step()
        sums.append(loss.item())
    model = _Stub().to(gpu_device).eval()
    res = gcgcn_amd.train_epoch(model, torch.optim.SGD(model.parameters(), lr=1e-5), iter(batches))
    assert res.stats.counters == want and res.n_documents == 4 and res.n_steps == 2
    np.testing.assert_allclose(res.loss_sum, sums[0] + sums[1], rtol=1e-6)
    assert model.w.item() != 1.0 and model.w.item() == eager.w.item()
    assert not model.training and [s[2] for s in model.seen] == [True, True]
    assert model.seen[0][1] is batches[0]["t_valid"] and model.seen[1][1] is None
    assert model.seen[0][0] is batches[0]["n_valid"] and model.seen[1][0] is batches[1]["n_valid"]
    assert res.log_line(0, 1.0).startswith("| epoch  0 | ms/b  1.00 | train loss ")
    # a TrainStats of the caller's is added to; loss_scale replaces 1 / B
    mine = gcgcn_amd.TrainStats(gpu_device)
    mine.update(*_dev(gpu_device, *cases[0]))
    m2 = _Stub().to(gpu_device)
    r2 = gcgcn_amd.train_epoch(m2, torch.optim.SGD(m2.parameters(), lr=1e-3), batches[:1], stats=mine, loss_scale=0.25)
    assert r2.stats == mine.get() and r2.stats.counters == TR.add(TR.vectorised(*cases[0]), TR.vectorised(*cases[0]))
    m3 = _Stub().to(gpu_device)
    gcgcn_amd.train_epoch(m3, torch.optim.SGD(m3.parameters(), lr=1e-3), batches[:1])
    np.testing.assert_allclose(1.0 - m2.w.item(), (1.0 - m3.w.item()) / 2, rtol=1e-3)
    with pytest.raises(ValueError, match="no batches"):
        gcgcn_amd.train_epoch(m3, torch.optim.SGD(m3.parameters(), lr=1e-5), [])
    assert m3.training
