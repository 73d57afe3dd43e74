"""One epoch of the reference's ``Config.train`` (config/Config.py:330-401) without its per-document host work: the
counterpart of ``evaluation.evaluate`` for the training loop.

The reference runs one document at a time, adds its loss to ``total_loss``, steps the optimiser on ``total_loss /
batch_size`` (:366-374) and then copies the document's ``[N,N,R]`` probabilities to the host to fill ``acc_NA``,
``acc_not_NA`` and ``acc_total`` in a Python loop over its pairs (:376-393).  ``train_epoch`` runs one ``data.collate`` batch
per step, keeps the three accuracies in a ``TrainStats`` and the epoch's loss in a device scalar, and reads both back once,
after the last step.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Iterable, Optional

import torch

from .evaluation import forward_args
from .functional import TrainStats, TrainStatsResult, pair_bce_loss

LOG_FORMAT = "| epoch {:2d} | ms/b {:5.2f} | train loss {:5.3f} | NA acc: {:4.2f} | not NA acc: {:4.2f}  | tot acc: {:4.2f} "


@dataclass
class TrainEpochResult:
    """``loss_sum`` is the trainer's ``all_loss`` (Config.py:369): the per-document losses summed over the epoch, before the
    division by the batch size.  ``stats`` holds the accuracy counters as ``TrainStats.get()`` returns them."""
    loss_sum: float
    n_documents: int
    n_steps: int
    stats: TrainStatsResult

    def log_line(self, epoch: int, ms_per_batch: float) -> str:
        """The epoch's log line as the reference formats it (Config.py:401)."""
        return LOG_FORMAT.format(epoch, ms_per_batch, float(self.loss_sum), self.stats.na_acc, self.stats.not_na_acc,
                                 self.stats.total_acc)


def train_epoch(model, optimizer, batches: Iterable[dict], stats: Optional[TrainStats] = None,
                loss_scale: Optional[float] = None) -> TrainEpochResult:
    """``Config.train``'s inner loop over one epoch: ``model.train()``; per batch, gradients to None, one forward, the summed
    per-document ``pair_bce_loss`` times ``loss_scale``, ``backward()``, ``optimizer.step()``.  ``batches`` yields dicts in
    ``data.collate``'s format (the forward's ten inputs and ``label_matrix``; ``n_valid`` / ``t_valid`` go to the model when
    the batch has them).  ``loss_scale`` defaults to ``1 / B`` of each batch, the mean over the step's documents
    (Config.py:370); pass ``1 / batch_size`` to divide a short last batch by the nominal size as the reference does.

    Nothing is read back during the epoch: the accuracy counters accumulate in ``stats`` (a fresh ``TrainStats`` when None; a
    given one is added to, not reset) and the loss in a device scalar, and both are read once at the end.  Any optimiser
    works.  The model's training flag is restored afterwards."""
    params = [p for g in optimizer.param_groups for p in g["params"]]
    was_training = model.training
    model.train()
    loss_acc = None
    n_documents = n_steps = 0
    try:
        for bt in batches:
            labels = bt["label_matrix"]
            if stats is None:
                stats = TrainStats(labels.device)
            B = labels.shape[0]
            for p in params:
                p.grad = None
            extra = {k: bt[k] for k in ("n_valid", "t_valid") if bt.get(k) is not None}
            args, rec = forward_args(bt)
            logits = model(*args, **extra, **rec)
            total = pair_bce_loss(logits, labels, n_valid=bt.get("n_valid"), stats=stats).sum()
            (total * (1.0 / B if loss_scale is None else loss_scale)).backward()
            optimizer.step()
            step_loss = total.detach().to(torch.float64)
            loss_acc = step_loss if loss_acc is None else loss_acc + step_loss
            n_documents += B
            n_steps += 1
    finally:
        model.train(was_training)
    if n_steps == 0:
        raise ValueError("train_epoch: no batches")
    return TrainEpochResult(loss_sum=float(loss_acc.item()), n_documents=n_documents, n_steps=n_steps, stats=stats.get())
