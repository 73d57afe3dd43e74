"""The trainer's optimiser as ONE launch per step: ``FusedAdam`` is ``torch.optim.Adam`` (the reference's
``optim.Adam(filter(lambda p: p.requires_grad, model.parameters()), lr=...)``, config/Config.py:300) with its update run by
``gcgcn_adam_step`` (csrc/optim.hip) over every parameter tensor at once.  It IS a ``torch.optim.Optimizer``: ``param_groups``,
``state_dict()`` / ``load_state_dict()`` (keys ``step``, ``exp_avg``, ``exp_avg_sq`` like torch's Adam, so a checkpoint moves
between the two), ``zero_grad()``.  Parameters whose ``.grad`` is None are skipped and keep their own step count, as in torch
(the dead last hop of the model, ``linears_k.*``).  fp32 GPU parameters only; no weight decay / amsgrad / maximize (the reference
uses none of them): ``param_groups`` carry those keys with torch's defaults so that a checkpoint moves in either direction, and a
group that asks for one of them (e.g. loaded from a torch Adam checkpoint trained with weight decay) raises instead of silently
training with different arithmetic.  The update is torch's formula with ``1 / sqrt(1 - beta2^t)`` as a multiplier (parameters agree
with torch.optim.Adam to 1e-6 relative over five steps, not bit for bit).

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


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, capturable: bool = False,
                 max_grad_norm=None):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1 and 0 <= betas[1] < 1):
            raise ValueError("FusedAdam: bad hyper-parameters")
        if max_grad_norm is not None and not (capturable and max_grad_norm > 0):
            raise ValueError("FusedAdam: max_grad_norm needs capturable=True and a positive value (the default form is one launch "
                             "with nothing decided on the device)")
        # weight_decay / amsgrad / maximize: torch.optim.Adam's keys at their defaults (checkpoint interchange); anything else raises
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False, maximize=False,
                                      capturable=bool(capturable), max_grad_norm=max_grad_norm))
        self._ring = []            # pinned staging buffers of the launch table: [tensor, event or None]
        self._ring_next = 0
        self._dev = {}             # capturable groups, by index: device scalars and workspace (_group_dev)
        self._graph_tables = []    # pinned launch tables of captured steps: read by every replay, never rewritten
        self._graph_refs = []      # device buffers whose addresses captured steps hold
        self._spare = None         # the pinned buffer that the next captured step will own
        self._norms = None         # fp32[len(param_groups)]: each clipping group's gradient norm of its last step

    _RING = 3

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
        if group.get("weight_decay", 0) != 0 or group.get("amsgrad", False) or group.get("maximize", False):
            raise RuntimeError("FusedAdam: weight_decay / amsgrad / maximize are not implemented (the reference trainer uses "
                               "plain Adam, config/Config.py:300); this parameter group asks for one of them")

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
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
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
        step, captured or not, rewrites in place.  0-dim with one parameter group, else one entry per group.  None before the
        first step."""
        if self._norms is None:
            return None
        return self._norms[0] if self._norms.numel() == 1 else self._norms

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

    # ---- checkpoints ----------------------------------------------------------------------------------------------------------------
    def load_state_dict(self, state_dict):
        """torch's ``load_state_dict``, then: each group keeps ITS OWN ``capturable`` (a checkpoint of the other form, or of
        torch's Adam, loads into either), ``max_grad_norm`` comes from the checkpoint where it has one (capturable groups only),
        and every step counter is converted to what this optimiser keeps: a 0-dim fp32 device tensor in a capturable group, an
        int otherwise.  The state tensors are NEW ones, as with every torch optimiser: load before a step is captured, not after
        (a graph captured earlier goes on updating the old ones)."""
        mine = [(g.get("capturable", False), g.get("max_grad_norm")) for g in self.param_groups]
        super().load_state_dict(state_dict)
        for group, (cap, mgn) in zip(self.param_groups, mine):
            group["capturable"] = cap
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
