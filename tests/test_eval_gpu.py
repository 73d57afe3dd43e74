"""Device-side relation evaluation (gcgcn_amd.RelationEvaluator: scan -> radix ranking -> curve, gcgcn_amd/csrc/eval.hip) against
the restatement of the reference's ``test`` methods (tests/eval_restatement.py).  Every comparison is EXACT: the restatement is fed
the probabilities the device produced (the one legitimate device/host difference is ``expf``), read back from ``ranked()``; the NA
column, which has no records, comes from a second run on the logits rolled by one relation.  Those probabilities are compared
with ``torch.sigmoid`` separately, at the bounds test_pair_bce_loss_batched_ragged uses for the same expression."""
import functools

import numpy as np
import pytest
import sklearn.metrics
import torch

import gcgcn_amd
from gcgcn_amd import RelationEvaluator
import eval_restatement as ER

pytestmark = pytest.mark.gpu

trapz = getattr(np, "trapezoid", None) or np.trapz


def _run_probs(lg, nv):
    B, N, _, R = lg.shape
    ev = RelationEvaluator(R, max_n=1 << 30)
    ev.update(lg, torch.zeros_like(lg), n_valid=nv)
    d = ev.ranked()
    P = torch.zeros(B, N, N, R, device=lg.device)
    P[d["index"], d["h"], d["t"], d["r"]] = d["score"]
    return P


def device_probs(lg, nv):
    """[B,N,N,R] probabilities as the scan pass computes them (valid off-diagonal pairs; zero elsewhere)."""
    P = _run_probs(lg, nv)
    P[..., 0] = _run_probs(lg.roll(1, dims=-1), nv)[..., 1]
    return P


def check_sigmoid(P, lg, nv):
    B, N = lg.shape[:2]
    want = torch.sigmoid(lg)
    for b in range(B):
        n = N if nv is None else int(nv[b])
        off = ~torch.eye(n, dtype=torch.bool, device=lg.device)
        torch.testing.assert_close(P[b, :n, :n][off], want[b, :n, :n][off], rtol=1e-5, atol=1e-6)


def check(ev, res, ref, ign=False):
    for k in ER.COUNTERS:
        assert getattr(res, k) == ref[k], k
    d = ev.ranked()
    got = list(zip(*(d[k].long().tolist() for k in ("label", "index", "h", "t", "r"))))
    assert res.n_records >= len(got) == len(ref["ranked"])
    assert got == ref["ranked"]
    assert torch.equal(res.pr_x.cpu(), torch.from_numpy(ref["pr_x"])) and torch.equal(res.pr_y.cpu(), torch.from_numpy(ref["pr_y"]))
    for k in ("f1", "f1_pos", "theta", "p", "r", "w", "f1_at_w"):
        assert getattr(res, k) == ref[k], (k, getattr(res, k), ref[k])
    assert ev.predictions().tolist() == [list(x) for x in ref["predictions"]]
    if ign:
        assert d["flag"].tolist() == ref["flags"]
        assert torch.equal(res.ign_pr_y.cpu(), torch.from_numpy(ref["ign_pr_y"]))
        assert res.ign_f1 == ref["ign_f1"]
    else:
        assert res.ign_f1 is None and res.ign_auc is None and res.ign_pr_y is None
    check_auc(res, ign)


def check_auc(res, ign=False):
    """(1) the fixed-order fp64 trapezoid against numpy's in float64 over the returned arrays: at most 1e6 non-negative terms,
    n 2^-53 ~ 1e-10; (2) against sklearn on the fp32 arrays, which sums in fp32: the gap is its rounding."""
    x = res.pr_x.cpu().numpy()
    for got, y in ((res.auc, res.pr_y), (res.ign_auc, res.ign_pr_y))[:2 if ign else 1]:
        y = y.cpu().numpy()
        want = float(trapz(y.astype(np.float64), x.astype(np.float64)))
        sk = float(sklearn.metrics.auc(x=x, y=y)) if len(x) > 1 else 0.0
        if want == 0.0:                                                # a curve of zeros: exact, a relative bound says nothing
            assert got == 0.0 and sk == 0.0
            continue
        assert got == pytest.approx(want, rel=1e-9, abs=0.0)
        if len(x) > 1:
            assert got == pytest.approx(sk, rel=1e-5, abs=0.0)


# ---- inputs (seeded; each reference computed once) -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tiny(dev):
    logits, labels, nv, in_train = ER.tiny_case(seed=0)
    lg, lb = torch.from_numpy(logits).to(dev), torch.from_numpy(labels).to(dev)
    nvd, it = torch.from_numpy(nv).to(dev), torch.from_numpy(in_train).to(dev)
    P = device_probs(lg, nvd)
    check_sigmoid(P, lg, nv)
    return lg, lb, nvd, it, ER.crop(P.cpu().numpy(), labels, nv, in_train), ER.crop(P.cpu().numpy(), labels, nv)


BIG = {"ragged": (12, 9, 12, 5), "two_to_the_16": (12,) * 6}        # 4*132*96 = 50 688 records at most; 6*132*96 = 76 032 > 2^16


@functools.lru_cache(maxsize=None)
def big(dev, name):
    """R = 97, N = 12: several radix tiles (4096 records each).  Half the logits are quantised, so exact ties are common; the
    train mask has pairs with a train-fact positive at a low k and a non-train positive at a higher k (sticky flag)."""
    nv = np.array(BIG[name], np.int32)
    B, N, R = len(nv), 12, 97
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, N, N, R, generator=g) * 3 - 2
    q = torch.rand(B, N, N, R, generator=g) < 0.5
    lg = torch.where(q, torch.round(x * 2) / 2, x)
    lg[0, 0, 1, :] = 30.0                                            # a saturated pair: all 97 probabilities tie at 1.0
    lb = (torch.rand(B, N, N, R, generator=g) < 0.04).float()
    it = torch.rand(B, N, N, R, generator=g) < 0.5
    lb[0, 2, 3, 5], lb[0, 2, 3, 40], lb[0, 2, 3, 80] = 1.0, 1.0, 1.0
    it[0, 2, 3, 5], it[0, 2, 3, 40], it[0, 2, 3, 80] = True, False, False    # k = 40 / 80: not train facts, flagged all the same
    lgd, lbd, nvd, itd = lg.to(dev), lb.to(dev), torch.from_numpy(nv).to(dev), it.to(dev)
    P = device_probs(lgd, nvd)
    check_sigmoid(P, lgd, nv)
    docs = ER.crop(P.cpu().numpy(), lb.numpy(), nv, it.numpy())
    sticky = sum(int(((d[1][..., 1:] != 0) & ~d[2][..., 1:] & np.logical_or.accumulate((d[1][..., 1:] != 0) & d[2][..., 1:], -1)).sum())
                 for d in docs)
    assert sticky > 10, "the mask must make the sticky flag matter"
    return lgd, lbd, nvd, itd, docs


def run(lg, lb, nv, it=None, theta=-1.0, max_n=1_000_000):
    ev = RelationEvaluator(lg.shape[-1], max_n=max_n)
    ev.update(lg, lb, n_valid=nv, in_train=it)
    return ev, ev.compute(theta)


# ---- 1. tiny ragged batch against the literal loops ----------------------------------------------------------------------------
@pytest.mark.parametrize("theta", [-1.0, 0.5, 2.0])
def test_tiny_ragged_equals_the_literal_loops(gpu_device, theta):
    lg, lb, nv, _, _, docs = tiny(gpu_device)
    ref = ER.literal(docs, 7, input_theta=theta)
    ev, res = run(lg, lb, nv, theta=theta)
    assert res.n_records == (5 * 4 + 3 * 2) * 6 and ev.n_documents == 3
    check(ev, res, ref)
    if theta == 2.0:
        assert res.w == 0 and ev.predictions().shape == (1, 4)


# ---- 2. R = 97 across tile boundaries ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(BIG))
@pytest.mark.parametrize("theta", [-1.0, 0.3])
def test_r97_across_tiles(gpu_device, name, theta):
    lg, lb, nv, _, docs = big(gpu_device, name)
    ref = ER.vectorised([(p, y, None) for p, y, _ in docs], 97, input_theta=theta)
    ev, res = run(lg, lb, nv, theta=theta)
    assert res.n_records == sum(n * (n - 1) * 96 for n in BIG[name])
    check(ev, res, ref)


# ---- 3. truncation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("delta", [None, -1, 0, 1])
def test_truncation_is_a_prefix_of_the_ranking(gpu_device, delta):
    lg, lb, nv, _, docs = big(gpu_device, "ragged")
    n = sum(k * (k - 1) * 96 for k in BIG["ragged"])
    max_n = 1000 if delta is None else n + delta
    ref = ER.vectorised([(p, y, None) for p, y, _ in docs], 97, max_n=max_n)
    ev, res = run(lg, lb, nv, max_n=max_n)
    assert len(res.pr_x) == min(n, max_n) and res.n_records == n
    check(ev, res, ref)


# ---- 4. streaming --------------------------------------------------------------------------------------------------------------
def test_streaming_equals_one_call_and_reset_is_clean(gpu_device):
    lg, lb, nv, it, docs = big(gpu_device, "ragged")
    one, res_one = run(lg, lb, nv, it)
    ev = RelationEvaluator(97)
    ev.update(lg[:1], lb[:1], n_valid=nv[:1], in_train=it[:1])                                   # B = 1, N = 12
    ev.update(lg[1:, :9, :9].contiguous(), lb[1:, :9, :9].contiguous(), n_valid=nv[1:].clamp(max=9),
              in_train=it[1:, :9, :9].contiguous())                                              # B = 3, N = 9: document 2 loses rows
    res = ev.compute()
    nv2 = nv.clone()
    nv2[1:] = nv2[1:].clamp(max=9)
    cat, res_cat = run(lg, lb, nv2, it)                       # the concatenation, padded to the larger N
    assert ev.n_documents == 4 and res.n_records == res_cat.n_records
    a, b = ev.ranked(), cat.ranked()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert a["index"].max().item() == 3
    for k in ("pr_x", "pr_y", "ign_pr_y"):
        assert torch.equal(getattr(res, k), getattr(res_cat, k))
    for k in ("f1", "auc", "theta", "f1_pos", "w", "ign_f1", "ign_auc") + ER.COUNTERS:
        assert getattr(res, k) == getattr(res_cat, k), k
    ev.reset()
    assert ev.n_records == 0 and ev.n_documents == 0
    ev.update(lg, lb, n_valid=nv, in_train=it)
    again = ev.compute()
    for k in ("pr_x", "pr_y", "ign_pr_y"):
        assert torch.equal(getattr(again, k), getattr(res_one, k))
    for k in ("f1", "auc", "theta", "f1_pos", "w", "ign_f1", "ign_auc", "n_records") + ER.COUNTERS:
        assert getattr(again, k) == getattr(res_one, k), k
    for k, v in ev.ranked().items():
        assert torch.equal(v, one.ranked()[k]), k


# ---- 5. ignore-train-facts variant ---------------------------------------------------------------------------------------------
def test_ignore_variant_tiny_literal(gpu_device):
    lg, lb, nv, it, docs, _ = tiny(gpu_device)
    ev, res = run(lg, lb, nv, it)
    check(ev, res, ER.literal(docs, 7), ign=True)


def test_ignore_variant_r97(gpu_device):
    lg, lb, nv, it, docs = big(gpu_device, "ragged")
    ev, res = run(lg, lb, nv, it)
    check(ev, res, ER.vectorised(docs, 97), ign=True)
    d = ev.ranked()
    sel = (d["index"] == 0) & (d["h"] == 2) & (d["t"] == 3)
    assert d["flag"][sel & (d["r"] >= 5)].all() and not d["flag"][sel & (d["r"] < 5)].any()       # sticky from k = 5 on
    ev0, res0 = run(lg, lb, nv, torch.zeros_like(it))
    assert torch.equal(res0.ign_pr_y, res0.pr_y) and res0.ign_f1 == res0.f1 and not ev0.ranked()["flag"].any()
    assert torch.equal(res0.pr_y, res.pr_y)


# ---- 6. degenerate inputs ------------------------------------------------------------------------------------------------------
def test_degenerate_inputs(gpu_device):
    lg, lb, nv, _, _, docs = tiny(gpu_device)
    zero = torch.zeros_like(lb)
    ev, res = run(lg, zero, nv)                                        # no positive label anywhere: total_recall -> 1
    assert res.total_recall == 0 and res.have_label == 0 and res.top1_acc == 0
    assert not res.pr_x.any() and not res.pr_y.any() and res.f1 == 0.0 and res.auc == 0.0 and res.f1_pos == 0
    check(ev, res, ER.literal([(p, np.zeros_like(y), None) for p, y, _ in docs], 7))
    na = zero.clone()
    na[..., 0] = 1.0                                                   # all-NA labels
    ev, res = run(lg, na, nv)
    assert res.na_recall == 5 * 4 + 3 * 2 and res.total_recall == 0 and not res.pr_y.any()
    def only_na(y):
        z = np.zeros_like(y)
        z[..., 0] = 1.0
        return z
    check(ev, res, ER.literal([(p, only_na(y), None) for p, y, _ in docs], 7))
    ev = RelationEvaluator(7)                                          # one unbatched document of two entities
    ev.update(lg[0, :2, :2].contiguous(), lb[0, :2, :2].contiguous())
    res = ev.compute()
    assert res.n_records == 12 and len(res.pr_x) == 12 and ev.predictions().shape[1] == 4
    ev = RelationEvaluator(7)                                          # zero records: a clear error, no launch
    with pytest.raises(ValueError, match="no records"):
        ev.compute()
    ev.update(lg[:1], lb[:1], n_valid=torch.tensor([1]))
    assert ev.n_records == 0 and ev.n_documents == 1
    with pytest.raises(ValueError, match="no records"):
        ev.compute()


# ---- 8. one model-level case ---------------------------------------------------------------------------------------------------
class _TailAsModel(torch.nn.Module):
    """The tail_c1 fixture model behind GCGCN_glove's forward signature; the fixture's token states stand in for the encoder."""

    def __init__(self, tail, ctx, dis, ner):
        super().__init__()
        self.tail, self.ctx, self.dis, self.ner = tail, ctx, dis, ner

    def forward(self, document, document_ner, document_pos, adj_matrix, sen_matrix, pos_matrix_h, pos_matrix_t, node_pos, node_type,
                node_relative_pos, n_valid=None):
        return self.tail(context_output=self.ctx, node_feat=node_pos @ self.ctx, adj_matrix=adj_matrix, sen_matrix=sen_matrix,
                         pos_matrix_h=pos_matrix_h, pos_matrix_t=pos_matrix_t, node_type=node_type,
                         node_relative_pos=node_relative_pos, dis_embed_weight=self.dis, ner_emb_weight=self.ner)


def test_evaluate_runs_the_model_in_eval_mode(gpu_device):
    import test_tail_gpu as TT
    g, sd, tail = TT._setup(gpu_device)
    r = g["raw"]
    docs = range(g["meta"]["docs"])
    t = lambda k: torch.stack([torch.from_numpy(r[f"doc{i}.{k}"]) for i in docs]).to(gpu_device)
    ctx = t("ctx")
    model = _TailAsModel(tail, ctx, sd["dis_embed.weight"].to(gpu_device), sd["ner_emb.weight"].to(gpu_device)).train()
    B, N = t("node_type").shape
    labels = (torch.rand(B, N, N, 97, generator=torch.Generator().manual_seed(2)) < 0.05).float().to(gpu_device)
    tok = torch.zeros(B, ctx.shape[1], dtype=torch.int64, device=gpu_device)
    batch = {"document": tok, "document_ner": tok, "document_pos": tok, "adj_matrix": t("adj"), "sen_matrix": t("sen"),
             "pos_matrix_h": t("pos_h"), "pos_matrix_t": t("pos_t"), "node_pos": t("node_pos"), "node_type": t("node_type"),
             "node_relative_pos": t("rel"), "label_matrix": labels}
    res = gcgcn_amd.evaluate(model, [batch])
    assert model.training                                              # restored
    again = gcgcn_amd.evaluate(model, [batch])                         # dropout off: two runs are bitwise equal
    with torch.no_grad():
        logits = model.eval()(*[batch[k] for k in gcgcn_amd.evaluation.FORWARD_KEYS])
    ev, direct = run(logits, labels, None)
    for other in (again, direct):
        for k in ("pr_x", "pr_y"):
            assert torch.equal(getattr(res, k), getattr(other, k))
        for k in ("f1", "auc", "theta", "p", "r", "f1_pos", "w", "f1_at_w", "n_records") + ER.COUNTERS:
            assert getattr(res, k) == getattr(other, k), k
    assert res.n_records == B * N * (N - 1) * 96 and res.total_recall > 0
