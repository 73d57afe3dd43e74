"""Restatement of the reference trainer's accuracy bookkeeping, the yardstick of tests/test_train_stats_cpu.py and
tests/test_train_stats_gpu.py.

``Config.train`` (config/Config.py:330-401) calls ``.cuda()`` and reads dataset files, so it cannot run in a test.  ``literal``
restates what its lines 377-393 do, in this project's own names with line citations: the second sigmoid over the
probabilities of :355, the host copy, the double loop over ordered pairs, ``argmax`` and the three ``Accuracy`` objects.
``vectorised`` is the same computation in numpy.  Both work on fp32 ``torch.sigmoid(torch.sigmoid(x))`` on the CPU and
return the eight counters of ``gcgcn_pair_stats`` as a tuple:

    (NA correct, NA total, not-NA correct, not-NA total, correct, total, NaN pairs, documents)

A pair whose row of logits holds a NaN is counted in ``NaN pairs`` and nowhere else (the library's rule; the reference never
meets one).

``make_case`` draws logits from the grid {-6, -5.5, ..., 6}.  Equal grid values give exact ties (the same input gives the
same fp32 output on any device); distinct ones differ in q = sigmoid(sigmoid(x)) by at least p'(6) * 0.5 * q'(1) =
0.002467 * 0.5 * 0.1966 = 2.4e-4 (both derivatives are smallest at the top of the grid).  ``plant`` adds rows with the
saturations 20, 30 and 45: exp(-20) = 2.1e-9 is far below half an ulp of 1 (6e-8), so p == 1.0f under any ``expf`` and all
three tie bit for bit, 4.9e-4 above the grid's top.  ``guard`` asserts exactly that of a case, on the CPU, before any device
result is looked at: in every pair the maximum q is shared bit for bit by its holders (which hold the same logit, or all a
logit >= 20) or exceeds the runner-up by >= 1e-4 -- three orders of magnitude above the few ulp (1e-7) by which a device's
``expf`` may differ from the host's.  So the expected first argmax does not depend on the last ulp of either ``expf``.  The
guard is a condition on the inputs, not a tolerance on the result.
"""
import numpy as np
import torch

GRID = np.arange(-6.0, 6.25, 0.5, dtype=np.float32)
SATURATED = (20.0, 30.0, 45.0)
MARGIN = 1e-4
# (B, N, R, n_valid): the shapes of both test files, in the issue's order: R over the lane chunks, N over the waves, ragged.
# The last four are the kernel's own thresholds: R = 128 | 129 (two chunks in registers | any R, here three chunks with one
# lane in the last), N = 18 (a wave's second group of four tails; the waves take 16 tails per sweep) and N = 258 (a second
# block of 256 tails per row).
SHAPES = [(2, 5, 97, None), (2, 5, 64, None), (2, 5, 65, None), (2, 5, 2, None), (2, 5, 1, None),
          (2, 1, 7, None), (2, 2, 7, None), (2, 5, 7, None), (2, 6, 7, None),
          (3, 6, 97, (0, 1, 6)), (3, 6, 97, (2, 6, 3)),
          (1, 5, 128, None), (2, 5, 129, (5, 4)), (2, 18, 7, (18, 17)), (1, 258, 3, None)]
SHAPE_IDS = [f"B{b}-N{n}-R{r}" + ("" if nv is None else "-nv" + "_".join(map(str, nv))) for b, n, r, nv in SHAPES]
COUNTERS = ("na_correct", "na_total", "not_na_correct", "not_na_total", "correct", "total", "nan_pairs", "documents")


class Accuracy(object):
    """Config.py:40-55."""

    def __init__(self):
        self.correct = 0                                              # :42-43
        self.total = 0

    def add(self, is_correct):                                        # :44-47
        self.total += 1
        if is_correct:
            self.correct += 1

    def get(self):                                                    # :48-52
        if self.total == 0:
            return 0.0
        return float(self.correct) / self.total

    def clear(self):                                                  # :53-55
        self.correct = 0
        self.total = 0


def double_sigmoid(logits):
    """fp32 [.., R] numpy: ``torch.sigmoid`` at Config.py:355 and again at :377."""
    return torch.sigmoid(torch.sigmoid(torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)))).numpy()


def _docs(logits, labels, n_valid):
    """Padded [B,N,N,R] (or one [N,N,R] document) -> the documents as the trainer sees them, one at a time."""
    logits, labels = np.asarray(logits, np.float32), np.asarray(labels, np.float32)
    if logits.ndim == 3:
        logits, labels = logits[None], labels[None]
    B, N = logits.shape[:2]
    for b in range(B):
        n = N if n_valid is None else min(max(int(n_valid[b]), 0), N)
        yield logits[b, :n, :n], labels[b, :n, :n]


def literal(logits, labels, n_valid=None):
    """The loop form.  Returns ``(counters, accuracies)``: the eight integers and the three ``Accuracy`` objects."""
    acc_na, acc_not_na, acc_total = Accuracy(), Accuracy(), Accuracy()
    nan_pairs = documents = 0
    for x, gold in _docs(logits, labels, n_valid):
        documents += 1
        output = double_sigmoid(x)                                    # :355 then :377
        for i in range(output.shape[0]):                              # :382-385, ordered pairs, diagonal skipped
            for j in range(output.shape[1]):
                if i == j:
                    continue
                if np.isnan(output[i, j]).any():
                    nan_pairs += 1
                    continue
                true_label = gold[i, j]                               # :386
                r = output[i, j].argmax()                             # :387, first maximum of the probabilities
                if true_label[0] == 1:                                # :388-391
                    acc_na.add(true_label[r] == 1)
                else:
                    acc_not_na.add(true_label[r] == 1)
                acc_total.add(true_label[r] == 1)                     # :393
    counters = (acc_na.correct, acc_na.total, acc_not_na.correct, acc_not_na.total, acc_total.correct, acc_total.total,
                nan_pairs, documents)
    return counters, (acc_na, acc_not_na, acc_total)


def vectorised(logits, labels, n_valid=None):
    c = [0] * 8
    for x, gold in _docs(logits, labels, n_valid):
        c[7] += 1
        n = x.shape[0]
        if n < 2:
            continue
        h, t = np.nonzero(~np.eye(n, dtype=bool))
        q, y = double_sigmoid(x[h, t]), gold[h, t]                    # [pairs, R]
        bad = np.isnan(q).any(-1)
        c[6] += int(bad.sum())
        q, y = q[~bad], y[~bad]
        r = q.argmax(-1)                                              # first maximum
        hit = y[np.arange(len(r)), r] == 1
        na = y[:, 0] == 1
        c[0] += int((na & hit).sum())
        c[1] += int(na.sum())
        c[2] += int((~na & hit).sum())
        c[3] += int((~na).sum())
        c[4] += int(hit.sum())
        c[5] += len(r)
    return tuple(c)


def first_argmax(logits):
    """r* of every pair of one document ``[n,n,R]`` (int64 [n,n]; the diagonal is computed too and means nothing)."""
    return double_sigmoid(logits).argmax(-1)


def add(*counter_tuples):
    return tuple(int(sum(v)) for v in zip(*counter_tuples))


def guard(logits, n_valid=None):
    """Asserts the condition of the module docstring on every pair that forms.  Returns the number of pairs checked."""
    checked = 0
    labels_unused = np.zeros_like(np.asarray(logits, np.float32))
    for x, _ in _docs(logits, labels_unused, n_valid):
        n = x.shape[0]
        if n < 2:
            continue
        h, t = np.nonzero(~np.eye(n, dtype=bool))
        rows = x[h, t]
        q = double_sigmoid(rows)
        keep = ~np.isnan(q).any(-1)
        rows, q = rows[keep], q[keep]
        top = q.max(-1, keepdims=True)
        holders = q.view(np.uint32) == top.view(np.uint32)            # bit for bit
        assert holders.any(-1).all() and (q[~holders] < np.broadcast_to(top, q.shape)[~holders]).all()
        lo, hi = np.where(holders, rows, np.inf).min(-1), np.where(holders, rows, -np.inf).max(-1)
        bad = ~((lo == hi) | (lo >= 20.0))
        assert not bad.any(), f"holders of the maximum tie by accident: logits {rows[bad][0][holders[bad][0]]}"
        runner_up = np.where(holders, -np.inf, q).max(-1)             # -inf where every relation holds the maximum
        bad = top[:, 0].astype(np.float64) - runner_up < MARGIN
        assert not bad.any(), f"runner-up within {MARGIN} of the maximum: {rows[bad][0]}"
        checked += len(rows)
    return checked


def make_case(seed, B, N, R, n_valid=None, p_label=0.3):
    """Drawn logits fp32 ``[B,N,N,R]`` from GRID, 0/1 labels fp32 (relation 0 set in about half of the pairs, so that both
    ``acc_NA`` and ``acc_not_NA`` fill), and ``n_valid`` as int32 ``[B]`` or None."""
    rs = np.random.RandomState(seed)
    logits = GRID[rs.randint(0, len(GRID), size=(B, N, N, R))]
    labels = (rs.rand(B, N, N, R) < p_label).astype(np.float32)
    labels[..., 0] = (rs.rand(B, N, N) < 0.5).astype(np.float32)
    return logits, labels, None if n_valid is None else np.asarray(n_valid, np.int32)


def plant(logits, labels, b=0):
    """Overwrites eight pairs of document ``b`` (needs N >= 4 valid entities there and R >= 71) with the rows of the issue and
    returns ``{(h, t): expected r*}`` (None for the NaN row).  Each row's labels are set so that a wrong r* changes a counter."""
    R = logits.shape[-1]
    assert R >= 71 and logits.shape[1] >= 4
    want = {}

    def row(h, t, base, spikes, ones, rstar):
        logits[b, h, t] = base
        for k, v in spikes.items():
            logits[b, h, t, k] = v
        labels[b, h, t] = 0.0
        for k in ones:
            labels[b, h, t, k] = 1.0
        want[(h, t)] = rstar

    row(0, 1, -6.0, {7: 5.0, 71: 5.0}, [7], 7)                        # maxima at k and k + 64: one lane, two chunks
    row(0, 2, -6.0, {10: 4.0, 40: 4.0}, [10], 10)                     # maxima in two lanes of one chunk
    row(0, 3, 1.5, {}, [0], 0)                                        # an all-equal row: r* = 0, NA and hit
    row(1, 0, -2.0, {3: 20.0, 70: 45.0}, [3], 3)                      # both saturate to p == 1: the lower index wins
    row(1, 2, -2.0, {0: 30.0, 64: 45.0}, [0], 0)                      # NA row hit: labels[0] == 1 and r* = 0
    row(1, 3, -6.0, {5: 3.0}, [0], 5)                                 # NA row missed: labels[0] == 1, labels[r*] == 0
    row(2, 0, -6.0, {69: 2.0, 5: 2.0}, [0, 5], 5)                     # NA row hit away from relation 0
    row(2, 1, 0.0, {11: np.nan}, [0, 11], None)                       # one NaN row: counter [6] only
    return want
