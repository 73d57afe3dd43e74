"""Device-side relation evaluation: the reference's ``Config.test`` (config/Config.py:432-561) and the ignore-train-facts
curve of ``Config_bert.test`` (config/Config_bert.py:488-656) without the per-document host loop.

The reference copies every document's ``[N,N,R]`` probabilities to the host, appends one Python tuple per (head, tail,
relation != NA), sorts the list by score (stable, descending), cuts it to ``max_n`` and walks it for the precision/recall
curve, F1, theta and AUC.  ``RelationEvaluator`` keeps one 64-bit record per such tuple on the device, written at the
tuple's position in the reference's append order (its *ordinal*), ranks the records with the library's own stable radix sort
and computes the curve in one pass (gcgcn_amd/csrc/eval.hip).  The ranking is the strict total order (score
descending, ordinal ascending), which is what Python's stable sort yields, so every result below is the reference's.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, Iterable, Optional

import torch

from . import _lib
from ._lib import call
from .functional import _chk, _p, _stream

Tensor = torch.Tensor

MAX_RECORDS = 0xFFFFFFFF          # a record's ordinal has 32 bits (include/gcgcn.h)
_SCORE_SHIFT, _SCORE_MAX = 34, 0x3FFFFFFF
COUNTERS = ("top1_acc", "na_recall", "na_correct", "total_recall", "total_correct", "have_label")
FORWARD_KEYS = ("document", "document_ner", "document_pos", "adj_matrix", "sen_matrix", "pos_matrix_h", "pos_matrix_t", "node_pos",
                "node_type", "node_relative_pos")
DENSE_SLOT_KEYS = ("sen_matrix", "pos_matrix_h", "pos_matrix_t")


def forward_args(bt: dict):
    """A batch dict of ``data.collate`` -> (positional arguments of the models' forward, keywords of the record route).  A batch of
    ``collate(dense_slots=False)`` has ``slot_records`` instead of the three dense slot tensors: those positions are None, and the
    records travel with ``slot_shape`` (S) and the host-side capacities ``max_live_slots`` / ``max_live_pairs``."""
    if bt.get("slot_records") is None:
        return [bt[k] for k in FORWARD_KEYS], {}
    kw = dict(slot_records=bt["slot_records"], slot_shape=bt["S"])
    kw.update({k: bt[k] for k in ("max_live_slots", "max_live_pairs") if bt.get(k) is not None})
    return [None if k in DENSE_SLOT_KEYS else bt[k] for k in FORWARD_KEYS], kw


@dataclass
class EvalResult:
    """What ``Config.test`` computes.  ``p`` and ``r`` are named as the reference names them (Config.py:537-538): ``p`` is
    ``pr_x[f1_pos]`` (the recall axis) and ``r`` is ``pr_y[f1_pos]`` (the precision axis) -- the swap is the reference's and is
    kept.  ``pr_x``, ``pr_y``, ``ign_pr_y`` are fp32 device tensors over the kept records; the ``ign_*`` fields are ``None`` when
    no ``in_train`` mask was given."""
    f1: float
    auc: float
    theta: float
    p: float
    r: float
    f1_pos: int
    w: int
    f1_at_w: float
    pr_x: Tensor
    pr_y: Tensor
    ign_f1: Optional[float]
    ign_auc: Optional[float]
    ign_pr_y: Optional[Tensor]
    top1_acc: int
    na_recall: int
    na_correct: int
    total_recall: int
    total_correct: int
    have_label: int
    n_records: int


def record_counts(doc_n: Tensor, relation_num: int) -> Tensor:
    """Records per document: n (n - 1) (R - 1) for n valid entities (int64; 0 for n < 2)."""
    n = doc_n.to(torch.int64).clamp(min=0)
    return n * (n - 1).clamp(min=0) * (relation_num - 1)


def decode_ordinals(ordinals: Tensor, doc_n: Tensor, relation_num: int):
    """Ordinal -> ``(index, h_idx, t_idx, r_idx)`` (int64 tensors), the inverse of
    ``base[index] + ((h (n - 1) + t') (R - 1)) + (r - 1)`` with ``t'`` = ``t`` with the diagonal skipped and ``base`` the
    exclusive prefix of ``record_counts`` over the documents seen so far.  Vectorised; any device."""
    ordinals = ordinals.to(torch.int64)
    doc_n = doc_n.to(device=ordinals.device, dtype=torch.int64)
    cnt = record_counts(doc_n, relation_num)
    ends = torch.cumsum(cnt, 0)
    index = torch.searchsorted(ends, ordinals, right=True)          # first document whose end lies past the ordinal
    local = ordinals - (ends[index] - cnt[index])
    pair = torch.div(local, relation_num - 1, rounding_mode="floor")
    r = local - pair * (relation_num - 1) + 1
    n1 = doc_n[index] - 1
    h = torch.div(pair, n1, rounding_mode="floor")
    tp = pair - h * n1
    return index, h, tp + (tp >= h).to(torch.int64), r


class RelationEvaluator:
    """Streaming replacement of the loop in ``Config.test``: ``update`` per batch, then ``compute``.

    ``logits`` / ``labels``: ``[B,N,N,R]`` (or one unbatched ``[N,N,R]`` document) on the GPU; ``n_valid[B]`` for ragged
    batches; ``in_train`` a boolean fact mask of the same shape (``label_set`` of Config_bert.py:558 as a tensor) switches the
    ignore-train-facts curve on.  Document indices and ordinals continue across ``update`` calls.  Labels are 0/1."""

    def __init__(self, relation_num: int = 97, max_n: int = 1_000_000):
        if relation_num < 2 or max_n < 1:
            raise ValueError(f"RelationEvaluator: relation_num={relation_num}, max_n={max_n}")
        self.relation_num, self.max_n = int(relation_num), int(max_n)
        self.reset()

    def reset(self) -> None:
        self._rec: Optional[Tensor] = None       # int64[capacity]: the records, in ordinal order
        self._n = 0
        self._doc_n = []                         # host int64 tensors: valid entities per document, in order
        self._counters: Optional[Tensor] = None  # device int64[8]
        self._ign: Optional[bool] = None
        self._ranked: Optional[Tensor] = None    # view into the workspace of the last ranking
        self._ws: Optional[Tensor] = None
        self._last: Optional[EvalResult] = None

    # ---- accumulation ------------------------------------------------------------------------------------------------
    @property
    def n_records(self) -> int:
        return self._n

    @property
    def n_documents(self) -> int:
        return int(sum(t.numel() for t in self._doc_n))

    def _ws_bytes(self, n: int, keep: int) -> int:
        h = _lib.lib()
        b = h.gcgcn_eval_ws_bytes(n, keep)
        if b < 0:
            raise RuntimeError(f"gcgcn_eval_ws_bytes failed: {h.gcgcn_last_error().decode()}")
        return int(b)

    def _reserve(self, total: int, dev) -> None:
        self._ws_bytes(total, min(total, self.max_n))          # raises when the ordinal would not fit: never wraps
        cap = 0 if self._rec is None else self._rec.numel()
        if total <= cap:
            return
        new_cap = min(MAX_RECORDS, max(total, 2 * cap, 1 << 16))
        rec = torch.empty(new_cap, dtype=torch.int64, device=dev)
        if self._n:
            rec[:self._n].copy_(self._rec[:self._n])
        self._rec = rec

    def update(self, logits: Tensor, labels: Tensor, n_valid: Optional[Tensor] = None, in_train: Optional[Tensor] = None) -> None:
        single = isinstance(logits, torch.Tensor) and logits.dim() == 3
        lg = _chk(logits.unsqueeze(0) if single else logits, "logits", 4)
        if not isinstance(labels, torch.Tensor):
            raise TypeError(f"labels: expected a tensor, got {type(labels).__name__}")
        lb = _chk((labels.unsqueeze(0) if single else labels).to(torch.float32), "labels", 4)
        B, N, N2, R = lg.shape
        if lb.shape != lg.shape or N != N2:
            raise ValueError(f"RelationEvaluator.update: logits {tuple(lg.shape)} vs labels {tuple(lb.shape)}")
        if R != self.relation_num:
            raise ValueError(f"RelationEvaluator.update: {R} relations, evaluator built for {self.relation_num}")
        it = None
        if in_train is not None:
            it = in_train.unsqueeze(0) if single else in_train
            if not it.is_cuda:
                raise RuntimeError(f"in_train: gcgcn_amd runs on MI355X only; got a {it.device} tensor (no CPU fallback)")
            if it.shape != lg.shape:
                raise ValueError(f"RelationEvaluator.update: in_train {tuple(it.shape)} vs logits {tuple(lg.shape)}")
            it = (it if it.dtype == torch.bool else it != 0).contiguous().view(torch.uint8)
        if self._ign is not None and self._ign != (it is not None):
            raise ValueError("RelationEvaluator.update: in_train must be given to every update of a run or to none")
        if B == 0:
            return
        nv_dev = None
        if n_valid is None:
            doc_n = torch.full((B,), N, dtype=torch.int64)
        else:
            nv_dev = torch.as_tensor(n_valid).reshape(-1).to(device=lg.device, dtype=torch.int32).contiguous()
            if nv_dev.shape != (B,):
                raise ValueError(f"n_valid: expected shape ({B},), got {tuple(nv_dev.shape)}")
            doc_n = nv_dev.cpu().to(torch.int64).clamp(0, N)
        cnt = record_counts(doc_n, R)
        ends = torch.cumsum(cnt, 0)
        total = self._n + int(ends[-1])
        self._reserve(max(total, 1), lg.device)
        if self._counters is None:
            self._counters = torch.zeros(8, dtype=torch.int64, device=lg.device)
        if total > self._n:
            base = (ends - cnt + self._n).to(lg.device)
            call("gcgcn_eval_scan", B, N, R, _p(lg), _p(lb), _p(it), _p(nv_dev), _p(base), _p(self._rec), self._rec.numel(),
                 _p(self._counters), _stream())
        self._ign = it is not None
        self._doc_n.append(doc_n)
        self._n = total
        self._ranked = self._ws = self._last = None

    # ---- ranking and curve ------------------------------------------------------------------------------------------------
    def _keep(self) -> int:
        return min(self._n, self.max_n)

    def _check_counters(self) -> list:
        host = self._counters.cpu().tolist()
        if host[6]:
            raise ValueError(f"RelationEvaluator: {host[6]} entity pairs hold a NaN probability; the ranking is undefined")
        if host[7]:
            raise RuntimeError("RelationEvaluator: records past the buffer's capacity (n_valid changed under the launch?)")
        return host

    def _rank(self) -> Tensor:
        if self._n == 0:
            raise ValueError("RelationEvaluator: no records to rank (no update yet, or no document with two entities)")
        if self._ranked is None:
            self._check_counters()
            nbytes = self._ws_bytes(self._n, self._keep())
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self._rec.device)
            off = ctypes.c_int64(-1)
            call("gcgcn_eval_rank", _p(self._rec), self._n, _p(ws), nbytes, ctypes.addressof(off), _stream())
            self._ws = ws
            self._ranked = ws[off.value:off.value + 8 * self._n].view(torch.int64)
        return self._ranked

    def compute(self, input_theta: float = -1.0) -> EvalResult:
        """The reference's numbers after the loop (Config.py:513-561; Config_bert.py:626-648 when ``in_train`` was given)."""
        ranked = self._rank()
        m, dev = self._keep(), ranked.device
        host = self._check_counters()
        pr_x, pr_y = torch.empty(m, dtype=torch.float32, device=dev), torch.empty(m, dtype=torch.float32, device=dev)
        ign_y = torch.empty(m, dtype=torch.float32, device=dev) if self._ign else None
        res = torch.zeros(16, dtype=torch.float64, device=dev)
        call("gcgcn_eval_curve", _p(ranked), m, self._n, _p(self._counters), float(input_theta), _p(pr_x), _p(pr_y), _p(ign_y), _p(res),
             _p(self._ws), self._ws.numel(), _stream())
        v = res.cpu().tolist()
        self._last = EvalResult(f1=v[0], auc=v[7], theta=v[2], p=v[3], r=v[4], f1_pos=int(v[1]), w=int(v[5]), f1_at_w=v[6], pr_x=pr_x,
                                pr_y=pr_y, ign_f1=v[8] if self._ign else None, ign_auc=v[9] if self._ign else None, ign_pr_y=ign_y,
                                n_records=self._n, **dict(zip(COUNTERS, host[:6])))
        return self._last

    def ranked(self, limit: Optional[int] = None) -> Dict[str, Tensor]:
        """The kept records in rank order as tensors ``score`` (fp32), ``label`` / ``flag`` (bool), ``index``, ``h``, ``t``,
        ``r`` (int64) -- ``test_result[:max_n]`` of the reference, column by column."""
        keys = self._rank()[:self._keep()]
        if limit is not None:
            keys = keys[:max(0, int(limit))]
        score = (_SCORE_MAX - ((keys >> _SCORE_SHIFT) & _SCORE_MAX)).to(torch.int32).view(torch.float32)
        index, h, t, r = decode_ordinals((keys >> 2) & 0xFFFFFFFF, torch.cat(self._doc_n), self.relation_num)
        return {"score": score, "label": (keys & 2) != 0, "flag": (keys & 1) != 0, "index": index, "h": h, "t": t, "r": r}

    def predictions(self) -> Tensor:
        """int64 ``[w + 1, 4]`` rows ``(index, h_idx, t_idx, r_idx)``: the reference's output list ``test_result[:w + 1]``
        (Config.py:553) for the ``input_theta`` of the last ``compute`` (run with its default if there was none)."""
        last = self._last or self.compute()
        d = self.ranked(last.w + 1)
        return torch.stack([d["index"], d["h"], d["t"], d["r"]], dim=1)


def evaluate(model, batches: Iterable[dict], relation_num: int = 97, max_n: int = 1_000_000, input_theta: float = -1.0,
             evaluator: Optional[RelationEvaluator] = None) -> EvalResult:
    """``Config.test``'s loop: ``model.eval()``, no gradients, one forward and one ``update`` per batch, then ``compute``.
    ``batches`` yields dicts in ``data.collate``'s format (the forward's ten inputs, ``label_matrix``, ``n_valid``; an optional
    ``in_train`` mask).  The model's training flag is restored afterwards."""
    ev = evaluator or RelationEvaluator(relation_num, max_n)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for bt in batches:
                args, rec = forward_args(bt)
                logits = model(*args, n_valid=bt.get("n_valid"), **rec)
                ev.update(logits, bt["label_matrix"], n_valid=bt.get("n_valid"), in_train=bt.get("in_train"))
    finally:
        model.train(was_training)
    return ev.compute(input_theta)
