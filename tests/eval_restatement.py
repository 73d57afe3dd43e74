"""Restatement of the reference's evaluation, the yardstick of tests/test_eval_cpu.py and tests/test_eval_gpu.py.

The reference's ``test`` methods (config/Config.py:432-561 and, for the ignore-train-facts curve, config/Config_bert.py:488-656)
call ``.cuda()`` and read dataset files, so they cannot run in a test.  ``literal`` restates what their lines do, in this
project's own names with line citations (line numbers of Config_bert.py, which is Config.py plus the in-train bookkeeping):
the Python loops, the tuple list,
``list.sort(key=..., reverse=True)``, the prefix loops, the numpy fp32 ``f1_arr`` and ``sklearn.metrics.auc``.  ``vectorised`` is
the same computation in numpy, with ``np.argsort(-score, kind="stable")``, for sizes the loops are too slow for.

Both take ``docs``: one ``(predicts, labels, in_train)`` triple per document, ``predicts`` the fp32 probabilities ``[n,n,R]`` of the
document's n valid entities (what ``torch.sigmoid(predict_re).cpu().numpy()`` is there), ``labels`` fp32 0/1 ``[n,n,R]``,
``in_train`` a bool ``[n,n,R]`` (``label_set`` as an array) or None.  Both return the same dict.
"""
import numpy as np
import sklearn.metrics

COUNTERS = ("top1_acc", "na_recall", "na_correct", "total_recall", "total_correct", "have_label")


def _curves(labels, scores, flags, total_recall, input_theta):
    """Config_bert.py:583-648 over the sorted, truncated list (given as columns)."""
    n = len(labels)
    pr_x, pr_y, ign_y = [], [], []
    correct = 0
    correct_in_train = 0
    w = 0
    if total_recall == 0:
        total_recall = 1                                              # :588-589
    for i in range(n):                                                # :591-597 and :630-641 in one walk
        correct += labels[i]
        if int(labels[i]) & bool(flags[i]):
            correct_in_train += 1
        pr_y.append(float(correct) / (i + 1))
        pr_x.append(float(correct) / total_recall)
        if correct_in_train == correct:
            ign_y.append(0)
        else:
            ign_y.append(float(correct - correct_in_train) / (i + 1 - correct_in_train))
        if float(scores[i]) > input_theta:
            w = i
    return pr_x, pr_y, ign_y, w


def _finish(out, labels, scores, flags, pr_x, pr_y, ign_y, w, input_theta):
    pr_x = np.asarray(pr_x, dtype="float32")                          # :599-606
    pr_y = np.asarray(pr_y, dtype="float32")
    f1_arr = (2 * pr_x * pr_y / (pr_x + pr_y + 1e-20))
    f1 = f1_arr.max()
    f1_pos = int(f1_arr.argmax())
    if input_theta == -1:                                             # :608-610
        w = f1_pos
    ign_y = np.asarray(ign_y, dtype="float32")                        # :643-648
    ign_f1_arr = (2 * pr_x * ign_y / (pr_x + ign_y + 1e-20))
    out.update(pr_x=pr_x, pr_y=pr_y, ign_pr_y=ign_y, f1=float(f1), f1_pos=f1_pos, p=float(pr_x[f1_pos]), r=float(pr_y[f1_pos]),
               theta=float(scores[f1_pos]), w=int(w), f1_at_w=float(f1_arr[w]), ign_f1=float(ign_f1_arr.max()),
               auc=float(sklearn.metrics.auc(x=pr_x, y=pr_y)) if len(pr_x) > 1 else 0.0,
               ign_auc=float(sklearn.metrics.auc(x=pr_x, y=ign_y)) if len(pr_x) > 1 else 0.0)
    return out


def literal(docs, relation_num, input_theta=-1, max_n=1000000):
    """The loop form, in this project's own names.  Citations are to Config_bert.py; Config.py:480-515 is the same without the
    in-train bookkeeping."""
    records = []                                                      # (label, score, sticky flag, document, head, tail, relation)
    cnt = dict.fromkeys(COUNTERS, 0)
    for doc, (prob, gold, train_facts) in enumerate(docs):            # :512, documents in order
        n = prob.shape[0]
        for head in range(n):                                         # :535-538, ordered pairs, diagonal skipped
            for tail in range(n):
                if head == tail:
                    continue
                best = np.argmax(prob[head, tail])                    # :539, first maximum of the probabilities
                if gold[head, tail, best]:                            # :541-542
                    cnt["top1_acc"] += 1
                if gold[head, tail, 0]:                               # :547-552, the NA relation: counted, never recorded
                    cnt["na_recall"] += 1
                    if best == 0:
                        cnt["na_correct"] += 1
                any_positive = False
                sticky = False                                        # :545, reset per pair, never cleared inside it
                for rel in range(1, relation_num):
                    if gold[head, tail, rel]:                         # :553-559
                        cnt["total_recall"] += 1
                        if best == rel:
                            cnt["total_correct"] += 1
                        any_positive = True
                        if train_facts is not None and bool(train_facts[head, tail, rel]):
                            sticky = True
                    records.append((gold[head, tail, rel], float(prob[head, tail, rel]), sticky, doc, head, tail, rel))   # :562
                if any_positive:                                      # :564-565
                    cnt["have_label"] += 1
    records.sort(key=lambda rec: rec[1], reverse=True)                # :579, Python's stable sort: ties keep append order
    records = records[:min(max_n, len(records))]                      # :580-581
    out = dict(cnt)
    out["ranked"] = [(int(rec[0]), rec[3], rec[4], rec[5], rec[6]) for rec in records]
    out["flags"] = [bool(rec[2]) for rec in records]
    labels = [rec[0] for rec in records]
    scores = [rec[1] for rec in records]
    pr_x, pr_y, ign_y, w = _curves(labels, scores, out["flags"], cnt["total_recall"], input_theta)
    _finish(out, labels, scores, out["flags"], pr_x, pr_y, ign_y, w, input_theta)
    out["predictions"] = [rec[3:] for rec in records[:out["w"] + 1]]  # :619
    return out


def vectorised(docs, relation_num, input_theta=-1, max_n=1000000):
    R = relation_num
    cnt = dict.fromkeys(COUNTERS, 0)
    cols = {k: [] for k in ("label", "score", "flag", "index", "h", "t", "r")}
    for index, (predicts, labels, label_set) in enumerate(docs):
        n = predicts.shape[0]
        if n < 2:
            continue
        h, t = np.nonzero(~np.eye(n, dtype=bool))                     # row-major: i outer, j inner, diagonal skipped
        p, y = predicts[h, t], labels[h, t] != 0                      # [pairs, R]
        r = p.argmax(-1)                                              # first maximum
        hit = y[np.arange(len(r)), r]
        cnt["top1_acc"] += int(hit.sum())
        cnt["na_recall"] += int(y[:, 0].sum())
        cnt["na_correct"] += int((y[:, 0] & (r == 0)).sum())
        cnt["total_recall"] += int(y[:, 1:].sum())
        cnt["total_correct"] += int((hit & (r >= 1)).sum())
        cnt["have_label"] += int(y[:, 1:].any(-1).sum())
        if label_set is None:
            flag = np.zeros((len(r), R - 1), bool)
        else:
            flag = np.logical_or.accumulate(y[:, 1:] & (label_set[h, t][:, 1:] != 0), axis=-1)   # sticky within the pair
        cols["label"].append(y[:, 1:].ravel()), cols["score"].append(p[:, 1:].ravel()), cols["flag"].append(flag.ravel())
        cols["index"].append(np.full(len(r) * (R - 1), index)), cols["h"].append(np.repeat(h, R - 1))
        cols["t"].append(np.repeat(t, R - 1)), cols["r"].append(np.tile(np.arange(1, R), len(r)))
    c = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in cols.items()}
    score = c["score"].astype(np.float32)
    order = np.argsort(-score, kind="stable")[:max_n]
    label, score, flag = c["label"][order].astype(np.int64), score[order], c["flag"][order].astype(bool)
    out = dict(cnt)
    out["ranked"] = list(zip(label.tolist(), *(c[k][order].astype(np.int64).tolist() for k in ("index", "h", "t", "r"))))
    out["flags"] = flag.tolist()
    m = len(order)
    correct = np.cumsum(label)
    cit = np.cumsum(label & flag)
    tr = cnt["total_recall"] if cnt["total_recall"] else 1
    pos = np.arange(1, m + 1)
    pr_y = correct.astype(np.float64) / pos
    pr_x = correct.astype(np.float64) / tr
    with np.errstate(invalid="ignore", divide="ignore"):
        ign_y = np.where(cit == correct, 0.0, (correct - cit).astype(np.float64) / (pos - cit))
    above = np.nonzero(score.astype(np.float64) > input_theta)[0]
    w = int(above[-1]) if len(above) else 0
    _finish(out, label, score, flag, pr_x, pr_y, ign_y, w, input_theta)
    out["predictions"] = [tuple(x[1:]) for x in out["ranked"][:out["w"] + 1]]
    return out


def same(a, b):
    """Exact equality of two restatement results (arrays bitwise)."""
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
        elif isinstance(a[k], list):
            assert [tuple(x) if isinstance(x, (tuple, list)) else x for x in a[k]] == \
                   [tuple(x) if isinstance(x, (tuple, list)) else x for x in b[k]], k
        else:
            assert a[k] == b[k], (k, a[k], b[k])
    return True


def tiny_case(seed=0, ragged=(5, 1, 3), N=5, R=7, with_train=True):
    """The tiny ragged batch of the issue: logits from a small set of values, several with |x| >= 20, so that exact ties and
    saturated probabilities are common.  Returns numpy ``logits``, ``labels`` (fp32 [B,N,N,R]), ``n_valid``, ``in_train``."""
    rs = np.random.RandomState(seed)
    B = len(ragged)
    values = np.array([-30.0, -20.0, -2.5, -0.5, 0.0, 0.5, 0.75, 3.0, 20.0, 25.0, 40.0], np.float32)
    logits = values[rs.randint(0, len(values), size=(B, N, N, R))]
    labels = (rs.rand(B, N, N, R) < 0.3).astype(np.float32)
    in_train = (rs.rand(B, N, N, R) < 0.4) if with_train else None
    return logits, labels, np.array(ragged, np.int32), in_train


def crop(probs, labels, n_valid, in_train=None):
    """Padded batch -> the ``docs`` list of ``literal`` / ``vectorised``."""
    docs = []
    for b, n in enumerate(n_valid):
        n = int(n)
        docs.append((probs[b, :n, :n], labels[b, :n, :n], None if in_train is None else in_train[b, :n, :n]))
    return docs
