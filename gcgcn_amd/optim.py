"""The trainer's optimiser as ONE launch per step: ``FusedAdam`` is ``torch.optim.Adam`` (the reference's
``optim.Adam(filter(lambda p: p.requires_grad, model.parameters()), lr=...)``, config/Config.py:300) with its update run by
``gcgcn_adam_step`` (csrc/optim.hip) over every parameter tensor at once.  It IS a ``torch.optim.Optimizer``: ``param_groups``,
``state_dict()`` / ``load_state_dict()`` (keys ``step``, ``exp_avg``, ``exp_avg_sq`` like torch's Adam, so a checkpoint moves
between the two), ``zero_grad()``.  Parameters whose ``.grad`` is None are skipped and keep their own step count, as in torch
(the dead last hop of the model, ``linears_k.*``).  fp32 GPU parameters only.  The update is torch's formula with
``1 / sqrt(1 - beta2^t)`` as a multiplier (parameters agree with torch.optim.Adam to 1e-6 relative over five steps, not bit for bit).

Beyond plain Adam, under torch 2.10's group keys, so that a checkpoint moves to and from ``torch.optim.Adam`` / ``AdamW``:
``weight_decay`` (L2: ``g + w p`` enters the moments) with ``decoupled_weight_decay=True`` for AdamW's ``p <- p (1 - lr w)``,
``amsgrad`` (state key ``max_exp_avg_sq``), ``maximize``, and ``bias_correction=False`` (this optimiser's own key; with decoupled
decay that is BertAdam's update, without its per-tensor clipping and built-in schedule).  ``foreach`` / ``fused`` /
``differentiable`` set to True raise.  All of this is opt-in at construction: an optimiser built with none of it (and with the
default ``clip_scope``) is the plain Adam it always was, and goes on refusing a group that asks for weight decay, amsgrad or
maximize later (set by hand, or loaded from a checkpoint) -- build the receiving optimiser with the checkpoint's settings;
``add_param_group`` with such a group counts as asking, like the constructor.
``step_route()`` decides in one place which kernels a step runs: parameter groups that are
all plain Adam make the calls they always made (``gcgcn_adam_step`` / ``_dev``, one 56-byte table per group); anything else goes
through ``gcopt_adamw_step`` / ``_dev``, whose one table spans the groups -- decay and no-decay groups (``bert_param_groups``) cost
one launch, not one per group.  ``clip_scope="global"`` (capturable only) takes ONE gradient norm over all groups, which is
``clip_grad_norm_(model.parameters())``; the default ``"group"`` clips each group by its own norm, as before.

``step()`` never waits for the GPU: the launch table travels through a small ring of pinned staging buffers, each with its own
event recorded right behind its host-to-device copy; a buffer's event is only waited for when the ring comes round to it again
(three steps later, long done).

``FusedAdam(..., capturable=True)`` is the form whose ``step()`` may be captured in a hipGraph (``GraphedTrainStep`` below).  The
default form decides the bias correction of step ``t`` on the host and bakes it, with the learning rate, into the launch table:
a replayed graph would apply the correction of the step at which it was captured for ever.  The capturable form decides nothing
on the host (``gcgcn_adam_step_dev``, two launches):

* ``state["step"]`` is a 0-dim fp32 device tensor, torch's capturable format; a one-workgroup tick launch advances it and
  computes ``lr / (1 - beta1^t)`` and ``1 / sqrt(1 - beta2^t)`` from it in double, as the host does in the default form.
* The learning rate lives in a device scalar per parameter group.  ``sync_lr()`` refreshes it from ``group["lr"]`` with a
  stream-ordered fill whenever the two differ; ``step()`` calls it when it is not being captured, ``GraphedTrainStep`` before
  every replay: a schedule needs no re-capture.
* The launch table of a captured ``step()`` is uploaded from a pinned buffer of its own, which the optimiser keeps and never
  rewrites (every replay reads it again); outside capture the ring serves.
* ``max_grad_norm=c`` (capturable only: the default form stays the one launch it is; asking for it there raises) clips by the
  global gradient norm inside the same call, one launch more: ``coef = min(1, c / (norm + 1e-6))``,
  ``torch.nn.utils.clip_grad_norm_``'s formula, over all gradients of a parameter GROUP (each group is one table; with one
  group, the usual case, that is the global norm).  Unlike ``clip_grad_norm_`` it does NOT modify ``.grad``: the update reads
  ``g * coef``.  ``last_grad_norm`` is a device tensor holding the norm before clipping (0-dim with one group, one entry per
  group otherwise), bit-reproducible (no float atomics); a non-finite norm propagates into the parameters as with torch's
  default ``error_if_nonfinite=False``.

Checkpoints move between the two forms and torch's Adam in every direction: ``load_state_dict`` converts the counters to what
the loading optimiser keeps (int, or 0-dim fp32 device tensor), and the loading optimiser's own ``capturable`` wins over the
checkpoint's.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from ._lib import call, lib
from .functional import _stream


def _written(params):
    """The kernels write parameters through raw pointers, which autograd's version counters do not see: count the write here,
    host side only.  GATAttention keeps its folded projection while ``flat._version`` stands still (eval mode), and autograd
    checks saved tensors against it."""
    torch.autograd.graph.increment_version(params)


# flag word of a group record (include/gcgcn_optim.h)
_L2, _DECOUPLED, _AMSGRAD, _MAXIMIZE, _NO_BIAS_CORRECTION = 1, 2, 4, 8, 16


def _group_flags(group) -> int:
    decay = group.get("weight_decay", 0) != 0
    return ((_DECOUPLED if group.get("decoupled_weight_decay", False) else _L2) if decay else 0) \
        | (_AMSGRAD if group.get("amsgrad", False) else 0) | (_MAXIMIZE if group.get("maximize", False) else 0) \
        | (0 if group.get("bias_correction", True) else _NO_BIAS_CORRECTION)


def pack_adamw_image(per_group):
    """The image that gcopt_adamw_step / gcopt_adamw_step_dev read (include/gcgcn_optim.h): 9 int64 words per tensor row, then 6 per
    group record.  `per_group`: one ``(record, rows)`` per parameter group in order -- ``record`` its six words, ``rows`` one
    ``(p, g, m, v, vmax, numel, last)`` per tensor.  A group WITHOUT rows is left out and the rows' group index counts the groups
    that are kept: the kernels read every record they are handed (the capturable form follows each record's lr pointer), so none
    may be there that no row refers to.  -> (int64 array, number of rows, number of records, total workgroups)."""
    rows, recs, blocks = [], [], 0
    for rec, grows in per_group:
        if not grows:
            continue
        for (p, g, m, v, vmax, n, last) in grows:
            rows.append((p, g, m, v, vmax, n, blocks, last, len(recs)))
            blocks += (n + 1023) // 1024
        recs.append(tuple(rec))
    image = np.concatenate([np.asarray(rows, dtype=np.int64).reshape(-1), np.asarray(recs, dtype=np.int64).reshape(-1)])
    return image, len(rows), len(recs), blocks


def step_route(param_groups, clip_scope: str = "group") -> str:
    """Which entry points a step over these parameter groups calls; the ONE place where that is decided.  ``"adam"``: every group
    is plain Adam (no weight decay, amsgrad, maximize; bias correction on) and clipping is per group -- ``gcgcn_adam_step`` /
    ``gcgcn_adam_step_dev`` with one 56-byte table per group, the calls this optimiser made before it knew anything else.
    ``"adamw"``: anything else -- ``gcopt_adamw_step`` / ``gcopt_adamw_step_dev`` with one table over the groups."""
    if clip_scope not in ("group", "global"):
        raise ValueError(f"FusedAdam: clip_scope must be 'group' or 'global', not {clip_scope!r}")
    return "adam" if clip_scope == "group" and all(_group_flags(g) == 0 for g in param_groups) else "adamw"


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0,
                 decoupled_weight_decay: bool = False, amsgrad: bool = False, maximize: bool = False, bias_correction: bool = True,
                 capturable: bool = False, max_grad_norm=None, clip_scope: str = "group"):
        if lr < 0 or eps < 0 or weight_decay < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("FusedAdam: bad hyper-parameters")
        if max_grad_norm is not None and not (capturable and max_grad_norm > 0):
            raise ValueError("FusedAdam: max_grad_norm needs capturable=True and a positive value (the default form is one launch "
                             "with nothing decided on the device)")
        if clip_scope not in ("group", "global"):
            raise ValueError(f"FusedAdam: clip_scope must be 'group' or 'global', not {clip_scope!r}")
        if clip_scope == "global" and not capturable:
            raise ValueError("FusedAdam: clip_scope='global' needs capturable=True (the norm is taken on the device)")
        # torch.optim.Adam's keys under torch's names (checkpoint interchange with Adam and AdamW), plus bias_correction
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=bool(amsgrad),
                                      maximize=bool(maximize), decoupled_weight_decay=bool(decoupled_weight_decay),
                                      bias_correction=bool(bias_correction), capturable=bool(capturable), max_grad_norm=max_grad_norm))
        self.clip_scope = clip_scope
        # Opt-in: an optimiser built as plain Adam stays the plain Adam it was, refusal included (step()).  Asking the constructor
        # for any of the new things, in its arguments or in a group of `params`, builds the extended one.
        self.extended = clip_scope == "global" or bool(decoupled_weight_decay) or any(_group_flags(g) for g in self.param_groups)
        self._ring = []          # pinned staging buffers of the launch table: [tensor, event or None]
        self._ring_next = 0
        self._dev = {}             # capturable groups, by index: device scalars and workspace (_group_dev)
        self._graph_tables = []    # pinned launch tables of captured steps: read by every replay, never rewritten
        self._graph_refs = []      # device buffers whose addresses captured steps hold
        self._spare = None         # the pinned buffer that the next captured step will own
        self._norms = None         # fp32[len(param_groups)]: each clipping group's gradient norm of its last step

    _RING = 3

    def add_param_group(self, param_group):
        """torch's, and a group that asks for decay / amsgrad / maximize / no bias correction makes the optimiser the extended one,
        as asking the constructor does (the constructor adds its groups through here, before ``extended`` exists)."""
        super().add_param_group(param_group)
        if hasattr(self, "extended"):
            self.extended = self.extended or bool(_group_flags(self.param_groups[-1]))

    def _staging(self, rows: int):
        """The next pinned buffer of the ring with room for `rows` table rows; waits (host side only) for the copy that last read
        it -- issued _RING steps ago -- and never for anything else on the stream."""
        if len(self._ring) < self._RING:
            self._ring.append([torch.empty(max(64, rows), 7, dtype=torch.int64).pin_memory(), None])
            slot = self._ring[-1]
        else:
            slot = self._ring[self._ring_next % self._RING]
        self._ring_next += 1
        if slot[1] is not None and not torch.cuda.is_current_stream_capturing():
            slot[1].synchronize()
            slot[1] = None
        if slot[0].shape[0] < rows:
            slot[0] = torch.empty(rows, 7, dtype=torch.int64).pin_memory()
        return slot

    @staticmethod
    def _check_group(group):
        for key in ("foreach", "fused", "differentiable"):
            if group.get(key):
                raise RuntimeError(f"FusedAdam: a parameter group asks for {key}=True, which is torch's own implementation choice and "
                                   "means nothing here; clear it")
        if group.get("weight_decay", 0) < 0:
            raise RuntimeError("FusedAdam: negative weight_decay")

    def route(self) -> str:
        """``step_route`` of this optimiser as it stands now."""
        return step_route(self.param_groups, self.clip_scope)

    @staticmethod
    def _check_param(p, g):
        if not (p.is_cuda and p.dtype == torch.float32 and g.dtype == torch.float32 and p.is_contiguous()):
            raise RuntimeError("FusedAdam: fp32 contiguous GPU parameters only (no CPU fallback)")
        if g.is_sparse:
            raise RuntimeError("FusedAdam: sparse gradients are not supported")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            self._check_group(group)
            if not self.extended and _group_flags(group):
                raise RuntimeError("FusedAdam: this optimiser was built as plain Adam (the reference trainer's, config/Config.py:300) and a "
                                   "parameter group now asks for weight_decay / amsgrad / maximize / bias_correction=False, set after "
                                   "construction or loaded from a checkpoint; it does not change arithmetic behind the caller's back.  "
                                   "Build it with those settings (FusedAdam(..., weight_decay=...)) and load the checkpoint into that")
        if self.route() == "adamw":
            self._step_adamw()
            return loss
        for gi, group in enumerate(self.param_groups):
            if group.get("capturable", False):
                self._step_capturable(gi, group)
                continue
            if group.get("max_grad_norm") is not None:
                raise RuntimeError("FusedAdam: max_grad_norm needs capturable=True")
            b1, b2 = group["betas"]
            rows, blocks, keep, keep_p = [], 0, [], []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                self._check_param(p, g)
                g = g.contiguous()
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["step"] = int(st["step"]) + 1
                t = st["step"]
                ss = group["lr"] / (1.0 - b1 ** t)
                ib = 1.0 / math.sqrt(1.0 - b2 ** t)
                n = p.numel()
                if n == 0:
                    continue
                rows.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), n, blocks, ss, ib))
                blocks += (n + 1023) // 1024
                keep.append(g)
                keep_p.append(p)
            if not rows:
                continue
            dev = group["params"][0].device
            tab = np.zeros((len(rows), 7), dtype=np.int64)
            for i, r in enumerate(rows):
                tab[i, :6] = r[:6]
                tab[i, 6] = np.array([r[6], r[7]], dtype=np.float32).view(np.int64)[0]
            slot = self._staging(len(rows))
            slot[0][:len(rows)].copy_(torch.from_numpy(tab))
            dtab = slot[0][:len(rows)].to(dev, non_blocking=True)
            if not torch.cuda.is_current_stream_capturing():
                slot[1] = torch.cuda.Event()
                slot[1].record()                 # right behind the copy: what a later reuse of this pinned buffer waits for
            call("gcgcn_adam_step", len(rows), dtab.data_ptr(), blocks, float(b1), float(b2), float(group["eps"]), _stream())
            # dtab and the gradients are released to the caching allocator in stream order: nothing to wait for here
            _written(keep_p)
        return loss

    # ---- the capturable form ------------------------------------------------------------------------------------------------------
    def _group_dev(self, gi, group):
        """Device-side companions of capturable group gi: {"lr": fp32 scalar, "lr_host": the value it holds, "ws": workspace}."""
        d = self._dev.get(gi)
        if d is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("FusedAdam: run one step() (or sync_lr()) before capturing: the learning rate's device scalar "
                                   "must exist, and be filled, outside the graph")
            dev = group["params"][0].device
            d = self._dev[gi] = {"lr": torch.empty((), dtype=torch.float32, device=dev), "lr_host": None, "ws": None}
        return d

    def sync_lr(self):
        """Bring the device-side learning rate of every capturable group up to ``group["lr"]``: a stream-ordered fill where the two
        differ, nothing otherwise; never a synchronisation.  Call it after changing ``group["lr"]`` and before replaying a graph
        that holds ``step()`` (``GraphedTrainStep`` does); never inside a capture, where the fill would become part of the graph."""
        for gi, group in enumerate(self.param_groups):
            if not group.get("capturable", False) or not group["params"]:
                continue
            d = self._group_dev(gi, group)
            lr = float(group["lr"])
            if d["lr_host"] != lr:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("FusedAdam.sync_lr: group['lr'] changed since the last step; call sync_lr() before the capture")
                d["lr"].fill_(lr)
                d["lr_host"] = lr

    @property
    def last_grad_norm(self):
        """Gradient norm (before clipping) of the last step of the groups with ``max_grad_norm``: a device tensor that every
        step, captured or not, rewrites in place.  0-dim with one parameter group or ``clip_scope="global"`` (one norm over all
        groups), else one entry per group.  None before the first step."""
        if self._norms is None:
            return None
        return self._norms[0] if self._norms.numel() == 1 or self.clip_scope == "global" else self._norms

    def _step_capturable(self, gi, group):
        capturing = torch.cuda.is_current_stream_capturing()
        b1, b2 = group["betas"]
        rows, blocks, keep, keep_p = [], 0, [], []
        for p in group["params"]:
            g = p.grad
            if g is None:
                continue
            self._check_param(p, g)
            g = g.contiguous()
            st = self.state[p]
            if not st:
                if capturing:
                    raise RuntimeError("FusedAdam: a parameter meets its first step() inside a capture; its state would be zeroed by "
                                       "every replay.  Warm up with one step() first")
                st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            step = st["step"]
            if not (torch.is_tensor(step) and step.is_cuda and step.dtype == torch.float32 and step.numel() == 1):
                raise RuntimeError("FusedAdam(capturable=True): state['step'] must be an fp32 device scalar (load_state_dict converts it)")
            n = p.numel()                        # an empty tensor keeps its row: it owns no workgroup, but its counter ticks
            rows.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), n, blocks, step.data_ptr()))
            blocks += (n + 1023) // 1024
            keep.append(g)
            keep_p.append(p)
        if not rows:
            return
        dev = group["params"][0].device
        d = self._group_dev(gi, group)
        self.sync_lr()
        max_norm = group.get("max_grad_norm")
        if self._norms is None or self._norms.numel() != len(self.param_groups):
            if capturing:
                raise RuntimeError("FusedAdam: warm up with one step() before capturing")
            self._norms = torch.zeros(len(self.param_groups), dtype=torch.float32, device=dev)
        need = lib().gcgcn_adam_ws_bytes(len(rows), blocks)
        if d["ws"] is None or d["ws"].numel() < need:
            d["ws"] = torch.empty(need, dtype=torch.uint8, device=dev)    # under capture: from the graph's pool, kept alive here
        tab = torch.from_numpy(np.asarray(rows, dtype=np.int64))
        if capturing:
            # Every replay copies the table from this buffer again: it is owned for good and never rewritten, so not a ring slot.
            # It was pinned by the eager step before (no host allocation while a stream is capturing).
            pinned, self._spare = self._spare, None
            if pinned is None or pinned.shape[0] < len(rows):
                raise RuntimeError("FusedAdam: run one step() with the same gradients outside the capture first (warm-up)")
            self._graph_tables.append(pinned)
            self._graph_refs += [d["ws"], d["lr"], self._norms]      # the graph holds their addresses: never freed, whatever replaces them
            pinned[:len(rows)].copy_(tab)
            dtab = pinned[:len(rows)].to(dev, non_blocking=True)
        else:
            if self._spare is None or self._spare.shape[0] < len(rows):
                self._spare = torch.empty(max(64, len(rows)), 7, dtype=torch.int64).pin_memory()    # for a capture that may follow
            slot = self._staging(len(rows))
            slot[0][:len(rows)].copy_(tab)
            dtab = slot[0][:len(rows)].to(dev, non_blocking=True)
            slot[1] = torch.cuda.Event()
            slot[1].record()
        call("gcgcn_adam_step_dev", len(rows), dtab.data_ptr(), blocks, float(b1), float(b2), float(group["eps"]), d["lr"].data_ptr(),
             float(max_norm) if max_norm is not None else 0.0, d["ws"].data_ptr(), d["ws"].numel(),
             self._norms.data_ptr() + 4 * gi, _stream())
        _written(keep_p)

    # ---- weight decay / amsgrad / maximize / global clipping: one table over the groups (route "adamw") -------------------------------
    def _step_adamw(self):
        cap = [gi for gi, g in enumerate(self.param_groups) if g.get("capturable", False)]
        host = [gi for gi, g in enumerate(self.param_groups) if not g.get("capturable", False)]
        for gi in host:
            if self.param_groups[gi].get("max_grad_norm") is not None:
                raise RuntimeError("FusedAdam: max_grad_norm needs capturable=True")
        if self.clip_scope == "global":
            if host:
                raise RuntimeError("FusedAdam: clip_scope='global' needs capturable=True in every parameter group")
            if len({self.param_groups[gi].get("max_grad_norm") for gi in cap}) > 1:
                raise RuntimeError("FusedAdam: clip_scope='global' takes ONE norm over all groups: max_grad_norm must be the same in "
                                   "every parameter group")
            self._adamw_call(cap, True, 0)
            return
        if host:
            self._adamw_call(host, False, 0)
        for gi in cap:                           # clipping per group: each group's norm is its own call's
            self._adamw_call([gi], True, gi)

    def _adamw_call(self, gis, dev_form: bool, norm_slot: int):
        """One gcopt_adamw_step (dev_form False) or gcopt_adamw_step_dev call over the parameter groups `gis`: a 72-byte row per
        tensor and a 48-byte record per group, uploaded as one image (rows, then records)."""
        capturing = torch.cuda.is_current_stream_capturing()
        per_group, keep, keep_p, devs = [], [], [], []
        for gi in gis:
            group = self.param_groups[gi]
            b1, b2 = group["betas"]
            lr, flags = float(group["lr"]), _group_flags(group)
            grows = []
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                self._check_param(p, g)
                g = g.contiguous()
                st = self.state[p]
                if not st:
                    if capturing:
                        raise RuntimeError("FusedAdam: a parameter meets its first step() inside a capture; its state would be zeroed by "
                                           "every replay.  Warm up with one step() first")
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if dev_form else 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                vmax = 0
                if flags & _AMSGRAD:
                    if "max_exp_avg_sq" not in st:
                        if capturing:
                            raise RuntimeError("FusedAdam: amsgrad's max_exp_avg_sq must exist before the capture; warm up with one step()")
                        st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    vmax = st["max_exp_avg_sq"].data_ptr()
                n = p.numel()
                if dev_form:
                    step = st["step"]
                    if not (torch.is_tensor(step) and step.is_cuda and step.dtype == torch.float32 and step.numel() == 1):
                        raise RuntimeError("FusedAdam(capturable=True): state['step'] must be an fp32 device scalar (load_state_dict converts it)")
                    last = step.data_ptr()       # an empty tensor keeps its row: it owns no workgroup, but its counter ticks
                else:
                    st["step"] = t = int(st["step"]) + 1
                    if n == 0:
                        continue
                    ss, ib = (lr / (1.0 - b1 ** t), 1.0 / math.sqrt(1.0 - b2 ** t)) if not flags & _NO_BIAS_CORRECTION else (lr, 1.0)
                    last = int(np.array([ss, ib], dtype=np.float32).view(np.int64)[0])
                grows.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), vmax, n, last))
                keep.append(g)
                keep_p.append(p)
            if not grows:
                continue                         # a group without a row gets no record either (pack_adamw_image); in the capturable
            if dev_form:                         # form its record would have no device-side lr to point at
                devs.append(self._group_dev(gi, group))
                lr_word = devs[-1]["lr"].data_ptr()
            else:
                lr_word = int(np.array([lr], dtype=np.float64).view(np.int64)[0])
            rec = [int(w) for w in np.array([b1, b2, group["eps"], group.get("weight_decay", 0)], dtype=np.float64).view(np.int64)]
            per_group.append((rec + [lr_word, flags], grows))
        image, n_rows, n_recs, blocks = pack_adamw_image(per_group)
        if n_rows == 0:
            return
        dev = keep_p[0].device
        image = torch.from_numpy(image)
        slots = (image.numel() + 6) // 7         # the staging buffers are counted in 56-byte rows
        if dev_form:
            self.sync_lr()
            max_norm = self.param_groups[gis[0]].get("max_grad_norm")
            if self._norms is None or self._norms.numel() != len(self.param_groups):
                if capturing:
                    raise RuntimeError("FusedAdam: warm up with one step() before capturing")
                self._norms = torch.zeros(len(self.param_groups), dtype=torch.float32, device=dev)
            d = devs[0]
            need = lib().gcopt_adamw_ws_bytes(n_rows, n_recs, blocks)
            if d["ws"] is None or d["ws"].numel() < need:
                d["ws"] = torch.empty(need, dtype=torch.uint8, device=dev)
        if capturing and dev_form:
            # as in _step_capturable: the image of a captured call lives in a pinned buffer of its own, which an eager step pinned
            pinned, self._spare = self._spare, None
            if pinned is None or pinned.shape[0] < slots:
                raise RuntimeError("FusedAdam: run one step() with the same gradients outside the capture first (warm-up)")
            self._graph_tables.append(pinned)
            self._graph_refs += [d["ws"], self._norms] + [x["lr"] for x in devs]
            pinned.view(-1)[:image.numel()].copy_(image)
            dimg = pinned.view(-1)[:image.numel()].to(dev, non_blocking=True)
        else:
            if dev_form and (self._spare is None or self._spare.shape[0] < slots):
                self._spare = torch.empty(max(64, slots), 7, dtype=torch.int64).pin_memory()
            slot = self._staging(slots)
            slot[0].view(-1)[:image.numel()].copy_(image)
            dimg = slot[0].view(-1)[:image.numel()].to(dev, non_blocking=True)
            if not capturing:
                slot[1] = torch.cuda.Event()
                slot[1].record()
        table, records = dimg.data_ptr(), dimg.data_ptr() + 72 * n_rows
        if dev_form:
            call("gcopt_adamw_step_dev", n_rows, table, n_recs, records, blocks, float(max_norm) if max_norm is not None else 0.0,
                 d["ws"].data_ptr(), d["ws"].numel(), self._norms.data_ptr() + 4 * norm_slot, _stream())
        else:
            call("gcopt_adamw_step", n_rows, table, n_recs, records, blocks, _stream())
        _written(keep_p)

    # ---- checkpoints ----------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        """torch's ``load_state_dict``, then: each group keeps ITS OWN ``capturable`` (a checkpoint of the other form, or of
        torch's Adam, loads into either), ``max_grad_norm`` comes from the checkpoint where it has one (capturable groups only),
        and every step counter is converted to what this optimiser keeps: a 0-dim fp32 device tensor in a capturable group, an
        int otherwise.  The state tensors are NEW ones, as with every torch optimiser: load before a step is captured, not after
        (a graph captured earlier goes on updating the old ones)."""
        mine = [(g.get("capturable", False), g.get("max_grad_norm")) for g in self.param_groups]
        own = [{k: g[k] for k in ("decoupled_weight_decay", "bias_correction") if k in g} for g in self.param_groups]
        super().load_state_dict(state_dict)
        for group, (cap, mgn), keys in zip(self.param_groups, mine, own):
            group["capturable"] = cap
            for k, v in keys.items():            # a checkpoint that does not know these keys (an older torch, this optimiser before
                group.setdefault(k, v)           # it had them) leaves the loading optimiser's setting in place
            if group.get("amsgrad", False):      # a checkpoint written without amsgrad: the running maximum starts at zero
                for p in group["params"]:
                    st = self.state.get(p)
                    if st and "exp_avg_sq" in st and "max_exp_avg_sq" not in st:
                        st["max_exp_avg_sq"] = torch.zeros_like(st["exp_avg_sq"])
            if not cap or "max_grad_norm" not in group:
                group["max_grad_norm"] = mgn     # (the default form does not clip: a clipped checkpoint loads, its setting does not)
            for p in group["params"]:
                st = self.state.get(p)
                if not st or "step" not in st:
                    continue
                step = st["step"]
                if cap:
                    st["step"] = (step.detach().to(device=p.device, dtype=torch.float32).reshape(()).clone() if torch.is_tensor(step)
                                  else torch.tensor(float(step), dtype=torch.float32, device=p.device))
                elif torch.is_tensor(step) and step.is_cuda:
                    st["step"] = int(step.item())
        for d in self._dev.values():
            d["lr_host"] = None                  # the checkpoint's lr: filled into the same device scalars at the next sync_lr()


def bert_param_groups(model, weight_decay: float, no_decay=("bias", "LayerNorm.weight", "LayerNorm.bias")):
    """The two parameter groups of the usual BERT fine-tuning recipe, for ``BertModel`` or a model that holds one
    (``GraphCNN_multihead_bert_gate_cls``): ``[{"params": decayed, "weight_decay": weight_decay}, {"params": the rest,
    "weight_decay": 0.0}]``.  A parameter goes to the second group when its name (``model.named_parameters()``) ends in one of
    ``no_decay``; parameters with ``requires_grad=False`` are left out, and each of the others is in exactly one group.  A group
    that would hold no parameter (only biases and LayerNorm train, or ``no_decay=()``) is not returned."""
    decay, rest = [], []
    for name, p in model.named_parameters():
        if p.requires_grad:
            (rest if no_decay and name.endswith(tuple(no_decay)) else decay).append(p)
    groups = [{"params": decay, "weight_decay": float(weight_decay)}, {"params": rest, "weight_decay": 0.0}]
    return [g for g in groups if g["params"]]    # a group that would be empty is left out


class GraphedTrainStep:
    """One training step -- ``step_fn(**static_inputs) -> scalar loss``, ``backward()``, ``optimizer.step()`` -- captured once in
    a hipGraph and replayed by every call::

        opt = FusedAdam(params, lr=1e-4, capturable=True, max_grad_norm=1.0)
        train = GraphedTrainStep(lambda **bt: loss_of(model(**bt)), opt, static_inputs=batch)
        for batch in loader:
            loss = train(**batch)            # copies into the static buffers, replays; no synchronisation

    ``static_inputs`` maps the keyword arguments of ``step_fn`` to their values.  The tensors among them ARE the graph's static
    buffers from then on: a call copies its keyword arguments into them (same shape and dtype, or ``ValueError``) and a key it
    leaves out keeps what the buffer holds.  Values that are not tensors (capacities, flags) are constants of the graph.
    ``step_fn`` must read nothing back to the host.  Every parameter of the optimiser has its ``.grad`` set to None at the start
    of the step; after a call, ``.grad`` is the graph's own tensor, rewritten by the next call.

    Construction does not train: parameters and optimiser state (the step counters too) are saved before the ``warmup`` steps,
    which run on a side stream, and copied back IN PLACE after the capture, so the addresses the graph holds stay valid.  The
    dropout generator is not put back: it advances by ``warmup + 1`` steps during construction.  The whole step is captured
    on ONE stream; ``step_fn`` must not fork work onto others.

    The optimiser must be a ``FusedAdam`` with ``capturable=True`` in every group (``ValueError`` otherwise): any other step
    replays the bias correction, and the learning rate, of the moment of capture.  ``__call__`` runs ``optimizer.sync_lr()``
    first, so changing ``group["lr"]`` between calls just works."""

    def __init__(self, step_fn, optimizer, static_inputs, warmup: int = 3):
        if not isinstance(optimizer, FusedAdam) or not all(g.get("capturable", False) for g in optimizer.param_groups):
            raise ValueError("GraphedTrainStep: the optimiser must be a FusedAdam(capturable=True); any other step() replays the bias "
                             "correction of the step at which it was captured")
        if warmup < 1:
            raise ValueError("GraphedTrainStep: at least one warm-up step (the optimiser's state must exist before the capture)")
        self.optimizer = optimizer
        self._inputs = dict(static_inputs)
        self._params = [p for g in optimizer.param_groups for p in g["params"]]

        def one_step():
            for p in self._params:
                p.grad = None
            loss = step_fn(**self._inputs)
            loss.backward()
            optimizer.step()
            return loss

        with torch.no_grad():
            saved_p = [p.detach().clone() for p in self._params]
            saved_s = [{k: v.clone() for k, v in optimizer.state[p].items() if torch.is_tensor(v)} if p in optimizer.state else None
                       for p in self._params]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                one_step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss = one_step()
        torch.cuda.synchronize()
        with torch.no_grad():
            for p, sp, ss in zip(self._params, saved_p, saved_s):
                p.copy_(sp)
                for k, v in optimizer.state.get(p, {}).items():
                    if torch.is_tensor(v):
                        v.copy_(ss[k]) if ss is not None and k in ss else v.zero_()
        optimizer.sync_lr()

    def __call__(self, **inputs):
        for k, v in inputs.items():
            buf = self._inputs.get(k)
            if not torch.is_tensor(buf):
                raise ValueError(f"GraphedTrainStep: '{k}' is not one of the static input tensors")
            if not torch.is_tensor(v) or v.shape != buf.shape or v.dtype != buf.dtype:
                raise ValueError(f"GraphedTrainStep: '{k}' must be a {buf.dtype} tensor of shape {tuple(buf.shape)}")
            if v is not buf:
                with torch.no_grad():
                    buf.copy_(v, non_blocking=True)
        self.optimizer.sync_lr()
        self.graph.replay()
        _written(self._params)
        return self.loss
