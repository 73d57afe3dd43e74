"""torch.autograd bindings of the HIP blocks (C ABI in include/gcgcn.h).

PyTorch is used for device memory (caching allocator), the current HIP stream and autograd
bookkeeping only; all arithmetic happens in libgcgcn_hip.so.  Inputs must be fp32 tensors on a
GPU -- anything else raises (no CPU path).
"""
from __future__ import annotations

import ctypes
import os
import threading
import weakref
from dataclasses import dataclass
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import SALT_GLUE, call

Tensor = torch.Tensor


def _p(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()          # ctypes turns the int into the void* the ABI declares


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """hipStream_t of torch's current stream.  The raw getter costs ~0.3 us; ``torch.cuda.current_stream()`` builds a
    Stream object (~15 us), which at ten C calls per step was a fifth of the host time of a step."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _bytes_or_raise(name: str, *dims) -> int:
    """What a ``*_ws_bytes`` symbol answers for these dimensions; a refusal (negative) raises with the library's message."""
    need = getattr(_lib.lib(), name)(*dims)
    if need < 0:
        raise RuntimeError(f"{name} failed: {_lib.lib().gcgcn_last_error().decode()}")
    return need


def _f32_buf(nbytes: int, dev) -> Tensor:
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)


def _chk(t: Tensor, name: str, ndim: Optional[int] = None) -> Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise RuntimeError(f"{name}: gcgcn_amd runs on MI355X only; got a {t.device} tensor (no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    if ndim is not None and t.dim() != ndim:
        raise ValueError(f"{name}: expected {ndim} dims, got shape {tuple(t.shape)}")
    return t.contiguous()


def _nv(n_valid: Optional[Tensor], B: int, N: int, dev) -> Optional[Tensor]:
    if n_valid is None:
        return None
    nv = n_valid.to(device=dev, dtype=torch.int32).contiguous()
    if nv.shape != (B,):
        raise ValueError(f"n_valid: expected shape ({B},), got {tuple(nv.shape)}")
    return nv


# ---- ragged batches: the entity rows that exist ------------------------------------------------------------------------
# With n_valid the node-phase products of a block (X WnX, Ebar We, the output projection, every data and weight gradient) run
# on the LIVE 16-row blocks of the [B N]-row tensors only (block r of document b is live iff 16 r < n_valid[b]); the tensors
# stay padded in memory, so nothing else changes.  The list is built on the device from n_valid (one tiny launch, no host
# read, captured with the step) once per hop loop and handed to every block call.  N must be a multiple of 16; the blocks fall
# back to the dense products by themselves where the column-strip chain kernels do not serve the shape.
row_block_launches = os.environ.get("GCGCN_ROW_BLOCKS", "1") != "0"      # GCGCN_ROW_BLOCKS=0: A/B knob (every padded row computed)


def row_blocks(n_valid: Optional[Tensor], B: int, N: int) -> Optional[Tensor]:
    """int32[gcgcn_row_blocks_ints(B, N)] for gcgcn_gcn_fwd / _bwd / gcgcn_mha_fwd / _bwd (``rowblk``), or None (dense products)."""
    # (N = 16 is one block per document: nothing to skip but whole empty documents, and the list's lookups cost cfg 1 10 %)
    if n_valid is None or not row_block_launches or N % 16 != 0 or N < 32 or not n_valid.is_cuda:
        return None
    nv = n_valid.to(dtype=torch.int32).contiguous()
    out = torch.empty(int(_lib.lib().gcgcn_row_blocks_ints(B, N)), dtype=torch.int32, device=nv.device)
    call("gcgcn_row_blocks", B, N, _p(nv), _p(out), _stream())
    return out


# ---- dropout RNG state -----------------------------------------------------------------------------
# One generator per DEVICE, like torch's own default CUDA generator behind nn.Dropout (which the reference uses): a
# device-resident {seed, counter} pair advanced by the kernels themselves.  This is the one piece of process-wide state of the
# product path; creation / re-seeding is guarded by a lock, the counter advances on the device in stream order.
_rng_state = {}
_rng_lock = threading.Lock()


def manual_seed(seed: int, device=None):
    """Seed the dropout generator of this library (per device): state = {seed, counter = 0}."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    st = torch.tensor([seed, 0], dtype=torch.int64, device=dev)
    with _rng_lock:
        _rng_state[dev.index or 0] = st


_tls = threading.local()   # .scope: [snaps tensor [count, 2], next index, pending] while a rng_scope is active on this
                           # thread; .handoff: the edge means parked on this thread (no process-global mutable state)


def _get_scope():
    return getattr(_tls, "scope", None)


def _state(dev: torch.device) -> Tensor:
    idx = dev.index or 0
    st = _rng_state.get(idx)
    if st is None:
        st = torch.tensor([torch.initial_seed() & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64, device=dev)
        with _rng_lock:
            st = _rng_state.setdefault(idx, st)     # two threads racing here agree on one state
    return st


def _new_snaps(dev: torch.device, count: int) -> Tensor:
    snaps = torch.empty(count, 2, dtype=torch.int64, device=dev)
    call("gcgcn_rng_next", _p(_state(dev)), _p(snaps), count, _stream())
    return snaps


class rng_scope:
    """Draw the {seed, counter} snapshots of up to `count` dropout-using forwards at once (GraphHops uses it for a whole
    hop loop); outside a scope every forward launches its own tiny kernel.  The draw itself is LAZY: the scope only
    allocates the snapshot buffer; GATAttention's forward -- the first kernel of a hop loop -- fills it inside its own
    first launch (gcgcn_gat_fwd's rng_state argument), and any other consumer that comes first launches gcgcn_rng_next."""

    def __init__(self, dev: torch.device, count: int, enabled: bool = True):
        self.dev, self.count, self.enabled = dev, count, enabled

    def __enter__(self):
        self.prev = _get_scope()
        if self.enabled:
            _tls.scope = [torch.empty(self.count, 2, dtype=torch.int64, device=self.dev), 0, True]
        return self

    def __exit__(self, *exc):
        _tls.scope = self.prev
        return False


def _take_pending_rng(dev: torch.device):
    """(state, snaps, count) of the active scope if its snapshots have not been drawn yet -- the caller promises to draw
    them in its next launch, before anything reads a snapshot -- else None."""
    sc = _get_scope()
    if sc is not None and sc[2] and sc[0].device == dev:
        sc[2] = False
        return _state(dev), sc[0], sc[0].shape[0]
    return None


def rng_snapshot(dev: torch.device, lazy: bool = False) -> Tensor:
    """Device-side {seed, counter} for one dropout-using forward; the counter advances on the GPU, so a
    captured hipGraph draws a fresh mask at every replay.  lazy=True: the caller will take the pending draw itself
    (_take_pending_rng) in the launch that reads this snapshot."""
    sc = _get_scope()
    if sc is not None and sc[1] < sc[0].shape[0] and sc[0].device == dev:
        if sc[2] and not lazy:                          # somebody other than GATAttention comes first: draw now
            sc[2] = False
            call("gcgcn_rng_next", _p(_state(dev)), _p(sc[0]), sc[0].shape[0], _stream())
        snap = sc[0][sc[1]]
        sc[1] += 1
        return snap
    return _new_snaps(dev, 1)[0]


def dropout_keep_mask(snap: Tensor, salt: int, p: float, numel: int) -> Tensor:
    """Boolean keep-mask of a dropout site (test aid: lets the CPU oracle replay the same mask)."""
    keep = torch.empty(numel, dtype=torch.uint8, device=snap.device)
    call("gcgcn_dropout_keep", _p(keep), numel, _p(snap), salt, float(p), _stream())
    return keep.bool()


# ---- GATAttention + single pass over E -------------------------------------------------------------
def _gat_fwd_buffers(x: Tensor, snap, pending, uvc, uvc_valid):
    """What gcgcn_gat_fwd / gcgcn_gat_fwd_compact fill: (uvc, uvc_valid, s, P, A, ebar) and the pending-rng triple."""
    B, N, D = x.shape
    dev = x.device
    rng = pending if pending is not None else (None, None, 0)
    if uvc is None:
        uvc, uvc_valid = torch.empty(2 * D + 1, device=dev), False
    s = torch.empty(B, N, device=dev)
    P = torch.empty(B, N, N, device=dev)
    A = torch.empty(B, N, N, device=dev) if snap is not None else None
    ebar = torch.empty(B, N, D, device=dev)
    return uvc, uvc_valid, s, P, A, ebar, rng


def _gat_bwd_buffers(x: Tensor, dA, dEbar, dXin, scratch_elems: str):
    """The incoming gradients made contiguous (dA: zeros if absent) and the workspaces of gcgcn_gat_bwd / gcgcn_gat_bwd_compact:
    (dA, dEbar, dXin, dlogit, ds, dvpart, duvc, scratch); scratch_elems names the size entry point that goes with the call."""
    B, N, D = x.shape
    dev = x.device
    dA = torch.zeros(B, N, N, device=dev) if dA is None else dA.contiguous()
    dEbar = None if dEbar is None else dEbar.contiguous()
    dXin = None if dXin is None else dXin.contiguous()
    dlogit = torch.empty(B, N, N, device=dev)
    ds = torch.empty(B, N, device=dev)
    dvpart = torch.empty(B * N, D, device=dev)
    duvc = torch.empty(2 * D + 1, device=dev)
    scratch = torch.empty(max(getattr(_lib.lib(), scratch_elems)(B, N, D), 1), device=dev)
    return dA, dEbar, dXin, dlogit, ds, dvpart, duvc, scratch


class GatFn(torch.autograd.Function):
    """(X[B,N,D], E[B,N,N,D], flat) -> (A[B,N,N], Ebar[B,N,D], X).  GCGCN_glove.py:154-168 (+ :40-41).
    The third output is X itself: a hop that hands THIS alias to its convolution lets the convolution's dX arrive
    here, where the attention's own dX kernel adds it -- instead of autograd summing the two with one more launch."""

    @staticmethod
    def forward(ctx, x, e, flat, n_valid, p, snap, pending, Dh, mask, uvc, uvc_valid):
        B, N, D = x.shape
        uvc, uvc_valid, s, P, A, ebar, (st, sn, cnt) = _gat_fwd_buffers(x, snap, pending, uvc, uvc_valid)
        call("gcgcn_gat_fwd", B, N, D, Dh, _p(x), _p(e), _p(n_valid), _p(flat), _p(snap), float(p), _p(uvc), _p(s),
             _p(P), _p(A), _p(ebar), _p(st), _p(sn), cnt, _p(mask), 1 if uvc_valid else 0, _stream())
        ctx.save_for_backward(x, e, flat, uvc, P)
        ctx.n_valid, ctx.p, ctx.snap, ctx.Dh, ctx.mask = n_valid, float(p), snap, Dh, mask
        return (P if A is None else A), ebar, x.view_as(x)

    @staticmethod
    def backward(ctx, dA, dEbar, dXin):
        x, e, flat, uvc, P = ctx.saved_tensors
        B, N, D = x.shape
        dev = x.device
        dA, dEbar, dXin, dlogit, ds, dvpart, duvc, scratch = _gat_bwd_buffers(x, dA, dEbar, dXin, "gcgcn_gat_bwd_scratch")
        if ctx.mask is not None:
            # opt-in mask: masked_fill passes no gradient to a masked energy.  In a partially masked row those entries have
            # P == 0 and the kernels' P (g - P.g) is zero by itself; a row whose real columns are ALL masked comes out
            # uniform (P = 1/n), so its dA row is cleared here -- the kernels then give that row a zero logit gradient
            gone = ctx.mask.bool()
            if ctx.n_valid is not None:
                gone = gone | (torch.arange(N, device=dev)[None, None, :] >= ctx.n_valid[:, None, None])
            dA = dA.masked_fill(gone.all(-1, keepdim=True), 0.0)
        dX = torch.empty_like(x)
        dE = torch.empty_like(e) if ctx.needs_input_grad[1] else None
        dflat = torch.empty_like(flat)
        bp = _current_pass()                     # weight gradients parked earlier in this backward pass ride in the edge pass
        call("gcgcn_gat_bwd", B, N, D, ctx.Dh, _p(x), _p(e), _p(ctx.n_valid), _p(flat), _p(ctx.snap), ctx.p, _p(uvc), _p(P),
             _p(dA), _p(dEbar), _p(dXin), _p(dX), _p(dE), _p(dflat), _p(dlogit), _p(ds), _p(dvpart), _p(duvc),
             _p(scratch), None if bp is None else bp.queue, _stream())
        return dX, dE, dflat, None, None, None, None, None, None, None, None


class EdgeMeanFn(torch.autograd.Function):
    """E[B,N,N,D] -> Ebar[B,N,D] = mean_j E  (GraphConv edge term, GCGCN_glove.py:40-41 commuted)."""

    @staticmethod
    def forward(ctx, e, n_valid):
        B, N, _, D = e.shape
        ebar = torch.empty(B, N, D, device=e.device)
        call("gcgcn_edge_mean_fwd", B, N, D, _p(e), _p(n_valid), _p(ebar), _stream())
        ctx.n_valid, ctx.shape = n_valid, (B, N, D)
        return ebar

    @staticmethod
    def backward(ctx, dEbar):
        B, N, D = ctx.shape
        dEbar = dEbar.contiguous()
        dE = torch.empty(B, N, N, D, device=dEbar.device)
        call("gcgcn_edge_mean_bwd", B, N, D, _p(dEbar), _p(ctx.n_valid), _p(dE), _stream())
        return dE, None


class MhaFn(torch.autograd.Function):
    """(X[B,N,D], flat) -> (A[B,H,N,N], X).  MultiHeadAttention.forward, GCGCN_glove.py:133-142.  The second output
    is the alias of X described at GatFn."""

    @staticmethod
    def forward(ctx, x, flat, n_valid, H, p, snap, rowblk=None):
        B, N, D = x.shape
        dev = x.device
        Q = torch.empty(B, N, D, device=dev)
        P = torch.empty(B, H, N, N, device=dev)
        A = torch.empty(B, H, N, N, device=dev) if snap is not None else None
        scratch = torch.empty(max(_lib.lib().gcgcn_mha_scratch(B, N, D), 1), device=dev)
        call("gcgcn_mha_fwd", B, N, D, H, _p(x), _p(n_valid), _p(flat), _p(snap), float(p), _p(Q), _p(P), _p(A),
             _p(scratch), _p(rowblk), _stream())
        ctx.save_for_backward(x, flat, Q, P)
        ctx.H, ctx.p, ctx.snap, ctx.rowblk = H, float(p), snap, rowblk
        return (P if A is None else A), x.view_as(x)

    @staticmethod
    def backward(ctx, dA, dXin):
        x, flat, Q, P = ctx.saved_tensors
        B, N, D = x.shape
        H, dev = ctx.H, x.device
        dA = torch.zeros(B, H, N, N, device=dev) if dA is None else dA.contiguous()
        dXin = None if dXin is None else dXin.contiguous()
        dX = torch.empty_like(x)
        dflat = torch.empty_like(flat)
        dS = torch.empty(B, H, N, N, device=dev)
        dQ = torch.empty(B, N, D, device=dev)
        scratch = torch.empty(max(_lib.lib().gcgcn_mha_scratch(B, N, D), 1), device=dev)
        # dWq is not parked: measured neutral at cfg 2 -- the carrying edge pass is already the longer side with the two
        # convolutions' products (0.652 vs 0.648 ms) -- so it stays with its own group launch
        call("gcgcn_mha_bwd", B, N, D, H, _p(x), _p(flat), _p(ctx.snap), ctx.p, _p(Q), _p(P), _p(dA), _p(dXin), _p(dX),
             _p(dflat), _p(dS), _p(dQ), _p(scratch), None, 0, _p(ctx.rowblk), _stream())
        return dX, dflat, None, None, None, None, None


# ---- deferred weight gradients ---------------------------------------------------------------------------------
# A block's weight-gradient products (7 GFLOP for MAGGC at cfg 2) are needed by nobody before the end of backward, and the
# last big kernel of backward -- GATAttention's pass over E -- is HBM-bound with idle matrix pipes.  gcgcn_gcn_bwd parks
# them in the queue of the running backward pass (include/gcgcn.h); gcgcn_gat_bwd carries them as extra workgroups of its
# edge pass; the pass's end-of-backward callback launches whatever is still parked and hands the gradients over.
#
# Soundness.  A parked gradient is NOT returned to autograd (the function returns None for it): autograd would add or
# clone the tensor -- e.g. when one module is called twice inside one backward pass, the reference trainer's own pattern,
# config/Config.py:340-372 -- before the parked products have written it.  Instead the callback, which runs after every
# node of the pass, installs each finished buffer as ``.grad`` (or adds it to a ``.grad`` that exists by then: gradient
# accumulation, other consumers of the parameter).  Parking is refused -- the products then run inside the block's own
# backward and the gradient takes autograd's normal route -- unless this is a ``.backward()`` pass that will reach the
# parameter's AccumulateGrad node (not ``autograd.grad``, not ``inputs=[...]`` without it) and the parameter has no hooks.
# Node-level hooks on AccumulateGrad (torch DistributedDataParallel) cannot be seen from Python; a forward that runs inside
# DDP's own forward is recognised instead (_under_ddp) and its blocks do not park.  (gcgcn_amd.dist.FlatGradBucket needs
# nothing: it reduces after backward, or uses tensor hooks, which are seen.)
#
# State.  One _BackwardPass per autograd graph task, registered under the task's id and owned by the engine through the
# queued callback: a pass that raises half-way is destroyed with its graph task -- parked operands, queue and all --
# and leaves nothing behind; passes of other models, devices or threads never share a queue.
defer_weight_grads = os.environ.get("GCGCN_DEFER", "1") != "0"      # GCGCN_DEFER=0: A/B knob
defer_fused_mha_weight_grads = os.environ.get("GCGCN_DEFER_MHA", "1") != "0"   # the fused MAGGC hop's dWq + dbq second stage (A/B knob)
_warned_ddp = [False]


def _under_ddp() -> bool:
    """True while torch's DistributedDataParallel is running the forward this block is part of.  DDP reduces gradients from
    C++ hooks on the parameters' AccumulateGrad nodes, which fire when autograd delivers a gradient -- a parked gradient is
    installed after backward and would never be reduced.  Blocks whose forward ran under DDP therefore do not park."""
    ddp = getattr(torch.nn.parallel, "DistributedDataParallel", None)
    if ddp is not None and not hasattr(ddp, "_active_ddp_module"):
        # a torch build without the (private) marker this test relies on: fail CLOSED -- with several ranks a DDP wrapper may be
        # active and cannot be recognised, so nothing is parked (FlatGradBucket users: pass through, it reduces after backward)
        import torch.distributed as dist
        on = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    else:
        on = ddp is not None and getattr(ddp, "_active_ddp_module", None) is not None
    if on and defer_weight_grads and not _warned_ddp[0]:
        _warned_ddp[0] = True
        import warnings
        warnings.warn("gcgcn_amd: running under torch DistributedDataParallel -- deferred weight gradients are switched off "
                      "for these blocks (their AccumulateGrad hooks need the gradient during backward); "
                      "gcgcn_amd.dist.FlatGradBucket reduces the flat gradients without that cost")
    return on
_passes = {}            # graph task id -> weakref to its _BackwardPass
_passes_lock = threading.Lock()


class _BackwardPass:
    def __init__(self, task_id: int):
        self.task_id = task_id
        self.queue = _lib.lib().gcgcn_defer_create()
        if not self.queue:
            raise MemoryError("gcgcn_defer_create failed")
        self.keep = []          # operands of parked products
        self.installs = []      # (leaf parameter, its finished flat gradient)

    def park(self, leaf, dflat, operands):
        self.keep.append(operands)
        self.installs.append((leaf, dflat))

    def __call__(self):         # end of the backward pass (autograd final callback; runs on the caller's stream)
        with _passes_lock:
            _passes.pop(self.task_id, None)
        try:
            if _lib.lib().gcgcn_defer_count(self.queue) > 0:
                call("gcgcn_defer_flush", self.queue, _stream())
            with torch.no_grad():
                for leaf, dflat in self.installs:
                    if leaf.grad is None:
                        leaf.grad = dflat
                    else:
                        leaf.grad.add_(dflat)
        finally:
            self.keep.clear()
            self.installs.clear()

    def __del__(self):          # also the only thing that happens to the pass of a backward that raised
        q, self.queue = self.queue, None
        if q:
            try:
                _lib.lib().gcgcn_defer_destroy(q)
            except Exception:   # interpreter shutdown
                pass


def _current_pass() -> Optional[_BackwardPass]:
    """The pass object of the graph task this thread is executing, if a block has parked something in it."""
    tid = torch._C._current_graph_task_id()
    if tid < 0:
        return None
    ref = _passes.get(tid)
    return None if ref is None else ref()


def _pass_for_parking(ctx, idx: int, leaf=None) -> Optional[_BackwardPass]:
    """The running backward pass if input ``idx`` of this function (a flat parameter: ``leaf``, default ``ctx.flat_leaf``) may be
    parked, else None."""
    if not (defer_weight_grads and ctx.needs_input_grad[idx]):
        return None
    leaf = ctx.flat_leaf if leaf is None else leaf
    if leaf is None or leaf._post_accumulate_grad_hooks or leaf._backward_hooks:
        return None
    tid = torch._C._current_graph_task_id()
    if tid < 0:
        return None
    try:
        acc = ctx.next_functions[idx][0]         # the parameter's AccumulateGrad node
        if acc is None or getattr(acc, "variable", None) is not leaf or torch._C._will_engine_execute_node(acc) is not True:
            return None
    except RuntimeError:                          # autograd.grad(): the gradient is captured, not accumulated
        return None
    with _passes_lock:
        ref = _passes.get(tid)
        bp = None if ref is None else ref()
        if bp is None:
            # (a dead entry under this id belongs to an earlier process-lifetime task that failed: ids are not reused
            # while a task lives)
            bp = _BackwardPass(tid)
            _passes[tid] = weakref.ref(bp)
            torch.autograd.Variable._execution_engine.queue_callback(bp)     # the engine owns the pass from here on
            for k in [k for k, r in _passes.items() if r() is None]:
                del _passes[k]
    return bp


def _ride(inp, n_valid, out, B, N, D):
    """ctypes gcgcn_edge_ride for (inp -> out); the caller keeps the struct alive across the call."""
    r = _lib.EdgeRide(B, N, D, inp.data_ptr(), None if n_valid is None else n_valid.data_ptr(), out.data_ptr())
    return r, ctypes.cast(ctypes.pointer(r), ctypes.c_void_p)


# The sum over heads of the output projection (gcgcn_gcn_fwd's wsum) rides in the forward call and is kept for backward;
# False: backward sums it itself in a small launch (what a caller of the C ABI that passes NULL gets).  A/B and test switch.
head_sum_in_forward = True


def _gcn_forward(ctx, x, ebar, adj, flat, n_valid, L, H, p, snap, e_next, out_p, out_snap, rowblk, hook=None, saved=()):
    """The forward of GcnFn and MaggcFn: buffers, ride, the gcgcn_gcn_fwd call (``hook``: MaggcFn's gcgcn_mha_hook -- the call then
    writes ``adj`` itself) and what _gcn_backward needs on ctx (``saved``: the caller's tensors, behind the block's)."""
    B, N, D = x.shape
    dev = x.device
    HD = H * D
    out = torch.empty(B, N, D, device=dev)
    Pn, Y, HO = (torch.empty(B, N, HD, device=dev) for _ in range(3))
    if hook is None:        # (GcnFn has always asked for rinv before G, MaggcFn after it: kept, so that the caching allocator of
        rinv = torch.empty(B, H, N, device=dev)      # a captured step sees the request sequence it saw before)
        G = torch.empty(B, N, HD, device=dev)
    else:
        G = torch.empty(B, N, HD, device=dev)
        rinv = torch.empty(B, H, N, device=dev)
    # sum over heads of the output projection's column blocks: a by-product of the first launch, used by backward
    wsum = torch.empty(D, D, device=dev) if (H > 1 and head_sum_in_forward and any(ctx.needs_input_grad[:4])) else None
    scratch = torch.empty(max(_lib.lib().gcgcn_gcn_scratch(B, N, D, H), 1), device=dev)
    ebar_next, ride, ride_p = None, None, None
    if e_next is not None:
        ebar_next = torch.empty(e_next.shape[0], e_next.shape[1], e_next.shape[3], device=dev)
        ride, ride_p = _ride(e_next, n_valid, ebar_next, *ebar_next.shape)
    call("gcgcn_gcn_fwd", B, N, D, L, H, _p(x), _p(ebar), None if hook is not None else _p(adj), _p(n_valid), _p(flat), _p(snap),
         float(p), _p(out_snap), float(out_p), _p(out), _p(Pn), _p(Y), _p(HO), _p(rinv), _p(G), _p(wsum), _p(scratch), ride_p,
         None if hook is None else ctypes.cast(ctypes.pointer(hook), ctypes.c_void_p), _p(rowblk), _stream())
    del ride
    ctx.save_for_backward(x, ebar, adj, flat, Pn, Y, HO, rinv, *saved)
    ctx.wsum, ctx.rowblk, ctx.n_valid, ctx.L, ctx.H = wsum, rowblk, n_valid, L, H
    ctx.p, ctx.snap, ctx.out_p, ctx.out_snap = float(p), snap, float(out_p), out_snap
    # to see in backward whether .grad will be installed or added to (never parked under DDP: see _under_ddp)
    ctx.flat_leaf = flat if (flat.is_leaf and not _under_ddp()) else None
    ctx.next_shape = None if e_next is None else tuple(e_next.shape)
    return out, ebar_next


def _gcn_backward(ctx, dout, debar_next, e_next_input, mha_hook=None):
    """The backward of GcnFn and MaggcFn: workspaces, ride, parking -> (dX, dEbar, dA, dflat or None if parked, dE_next, dQ).
    ``e_next_input``: E_next's place among the function's inputs; ``mha_hook``: MaggcFn's, dQ -> gcgcn_mha_hook (dQ[B,N,D] is
    allocated here, behind the block's own workspaces, where it always was; None without a hook)."""
    x, ebar, adj, flat, Pn, Y, HO, rinv = ctx.saved_tensors[:8]
    B, N, D = x.shape
    L, H, dev = ctx.L, ctx.H, x.device
    HD = H * D
    dout = dout.contiguous()
    dX, dEbar = torch.empty_like(x), torch.empty_like(ebar)
    dA = torch.empty_like(adj)
    dflat = torch.empty_like(flat)
    W1, W2, W3 = (torch.empty(B, N, HD, device=dev) for _ in range(3))
    drow = torch.empty(B, H, N, device=dev)
    dXres = torch.empty(B, N, D, device=dev)
    dout_m = torch.empty(B, N, D, device=dev) if (ctx.n_valid is not None or ctx.out_snap is not None) else None
    scratch = torch.empty(max(_lib.lib().gcgcn_gcn_scratch(B, N, D, H), 1), device=dev)
    dQ = None if mha_hook is None else torch.empty(B, N, D, device=dev)
    hook = None if mha_hook is None else mha_hook(dQ)
    dE_next, ride, ride_p = None, None, None
    if ctx.next_shape is not None and ctx.needs_input_grad[e_next_input] and debar_next is not None:
        debar_next = debar_next.contiguous()
        dE_next = torch.empty(ctx.next_shape, device=dev)
        ride, ride_p = _ride(debar_next, ctx.n_valid, dE_next, *debar_next.shape)
    bp = _pass_for_parking(ctx, 3)
    call("gcgcn_gcn_bwd", B, N, D, L, H, _p(x), _p(ebar), _p(adj), _p(ctx.n_valid), _p(flat), _p(ctx.snap),
         ctx.p, _p(ctx.out_snap), ctx.out_p, _p(Pn), _p(Y), _p(HO), _p(rinv), _p(ctx.wsum), _p(dout), _p(dX), _p(dEbar), _p(dA),
         _p(dflat), _p(W1), _p(W2), _p(W3), _p(drow), _p(dXres), _p(dout_m), _p(scratch), ride_p,
         None if hook is None else ctypes.cast(ctypes.pointer(hook), ctypes.c_void_p),
         None if bp is None else bp.queue, _p(ctx.rowblk), _stream())
    del ride, hook
    if bp is not None:
        bp.park(ctx.flat_leaf, dflat, (x, ebar, Y, HO, dout, dout_m, W2, W3, ctx.rowblk))
        dflat = None                                # installed as .grad by the pass's end-of-backward callback
    return dX, dEbar, dA, dflat, dE_next, dQ


class GcnFn(torch.autograd.Function):
    """(X[B,N,D], Ebar[B,N,D], A[B,H,N,N], flat[, E_next[B,N,N,D]]) -> out[B,N,D][, mean_j E_next].
    GraphConvolution.forward (H = 1) / MultiGraphConvolution.forward, GCGCN_glove.py:63-80 / 97-120.  The optional
    E_next is the NEXT hop's edge tensor: its mean (all that hop needs of it, glove:40-41) rides inside this block's
    latency-bound chain launch, and so does its backward."""

    @staticmethod
    def forward(ctx, x, ebar, adj, flat, n_valid, L, H, p, snap, e_next, out_p, out_snap, rowblk=None):
        return _gcn_forward(ctx, x, ebar, adj, flat, n_valid, L, H, p, snap, e_next, out_p, out_snap, rowblk)

    @staticmethod
    def backward(ctx, dout, debar_next):
        dX, dEbar, dA, dflat, dE_next, _ = _gcn_backward(ctx, dout, debar_next, 9)
        return dX, dEbar, dA, dflat, None, None, None, None, None, dE_next, None, None, None


class MaggcFn(torch.autograd.Function):
    """One MAGGC hop as ONE autograd node: MultiHeadAttention.forward (glove:133-142) + MultiGraphConvolution.forward
    (glove:97-120) on its adjacencies, (X[B,N,D], Ebar[B,N,D], flat_mha, flat_gcn[, E_next]) -> out[B,N,D][, mean_j E_next].
    The attention's launches ride inside the convolution's (gcgcn_mha_hook, include/gcgcn.h): the query projection is one more
    problem of the convolution's first group launch, the attention core's backward runs as passenger workgroups of its last
    one -- two launches fewer per step than MhaFn + GcnFn, the same arithmetic (same kernels' bodies, same dropout draws)."""

    @staticmethod
    def forward(ctx, x, ebar, flat_mha, flat, n_valid, L, H, p_mha, snap_mha, p, snap, e_next, out_p, out_snap, rowblk=None):
        B, N, D = x.shape
        dev = x.device
        Q = torch.empty(B, N, D, device=dev)
        P = torch.empty(B, H, N, N, device=dev)
        A = torch.empty(B, H, N, N, device=dev) if snap_mha is not None else None
        hook = _lib.MhaHook(flat_mha.data_ptr(), Q.data_ptr(), P.data_ptr(), _p(A), None, _p(snap_mha), float(p_mha))
        ctx.p_mha, ctx.snap_mha = float(p_mha), snap_mha
        ctx.flat_mha_leaf = flat_mha if (flat_mha.is_leaf and not _under_ddp()) else None
        return _gcn_forward(ctx, x, ebar, P if A is None else A, flat, n_valid, L, H, p, snap, e_next, out_p, out_snap, rowblk,
                            hook=hook, saved=(flat_mha, Q, P))

    @staticmethod
    def backward(ctx, dout, debar_next):
        x, flat_mha, Q, P = ctx.saved_tensors[0], *ctx.saved_tensors[8:]
        B, N, D = x.shape
        H, dev = ctx.H, x.device
        dXc, dEbar, dA, dflat, dE_next, dQ = _gcn_backward(         # dXc: the convolution's share of dX
            ctx, dout, debar_next, 11, lambda dQ: _lib.MhaHook(None, Q.data_ptr(), P.data_ptr(), None, dQ.data_ptr(), _p(ctx.snap_mha), ctx.p_mha))
        # the rest of the attention's backward: dX = dQ Wq + dXc, dWq = dQ^T X, dbq (the core already ran, as passengers).
        # dWq and the second stage of dbq's column sums are needed by nobody before the end of backward: parked like the
        # convolution's weight gradients (round 5: the launch then has nothing to reduce -- one launch less, a shorter group)
        dX = torch.empty_like(x)
        dflat_mha = torch.empty_like(flat_mha)
        dS = torch.empty(1, device=dev)
        scratch2 = torch.empty(max(_lib.lib().gcgcn_mha_scratch(B, N, D), 1), device=dev)
        bq = _pass_for_parking(ctx, 2, ctx.flat_mha_leaf) if (defer_fused_mha_weight_grads and ctx.flat_mha_leaf is not None) else None
        call("gcgcn_mha_bwd", B, N, D, H, _p(x), _p(flat_mha), _p(ctx.snap_mha), ctx.p_mha, _p(Q), _p(P), _p(dA), _p(dXc), _p(dX),
             _p(dflat_mha), _p(dS), _p(dQ), _p(scratch2), None if bq is None else bq.queue, 1, _p(ctx.rowblk), _stream())
        if bq is not None:
            bq.park(ctx.flat_mha_leaf, dflat_mha, (x, dQ, scratch2, ctx.rowblk))
            dflat_mha = None
        return dX, dEbar, dflat_mha, dflat, None, None, None, None, None, None, None, dE_next, None, None, None


class GraphConvFn(torch.autograd.Function):
    """(X[B,N,Din], Ebar[B,N,De], A[B,N,N], We, Wn, bias|None) -> out[B,N,Dout].  GraphConv.forward, glove:36-50."""

    @staticmethod
    def forward(ctx, x, ebar, adj, we, wn, bias):
        B, N, Din = x.shape
        De, Dout = we.shape
        dev = x.device
        out = torch.empty(B, N, Dout, device=dev)
        T = torch.empty(B, N, Dout, device=dev)
        rinv = torch.empty(B, N, device=dev)
        scratch = torch.empty(max(_lib.lib().gcgcn_gcn_scratch(B, N, max(Din, Dout), 1), 1), device=dev)
        call("gcgcn_graphconv_fwd", B, N, Din, De, Dout, _p(x), _p(ebar), _p(adj), _p(we), _p(wn), _p(bias), _p(out),
             _p(T), _p(rinv), _p(scratch), _stream())
        ctx.save_for_backward(x, ebar, adj, we, wn, out, T, rinv)
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        x, ebar, adj, we, wn, out, T, rinv = ctx.saved_tensors
        B, N, Din = x.shape
        De, Dout = we.shape
        dev = x.device
        dout = dout.contiguous()
        dX, dEbar, dA = torch.empty_like(x), torch.empty_like(ebar), torch.empty_like(adj)
        dWe, dWn = torch.empty_like(we), torch.empty_like(wn)
        dbias = torch.empty(Dout, device=dev) if ctx.has_bias else None
        dS, dT = torch.empty(B, N, Dout, device=dev), torch.empty(B, N, Dout, device=dev)
        drow = torch.empty(B, N, device=dev)
        scratch = torch.empty(max(_lib.lib().gcgcn_gcn_scratch(B, N, max(Din, Dout), 1), 1), device=dev)
        call("gcgcn_graphconv_bwd", B, N, Din, De, Dout, _p(x), _p(ebar), _p(adj), _p(we), _p(wn), _p(out), _p(T),
             _p(rinv), _p(dout), _p(dX), _p(dEbar), _p(dA), _p(dWe), _p(dWn), _p(dbias), _p(dS), _p(dT), _p(drow),
             _p(scratch), _stream())
        return dX, dEbar, dA, dWe, dWn, dbias


class DropoutFn(torch.autograd.Function):
    """Elementwise dropout of the hop glue (GCGCN_glove.py:341); backward replays the same mask."""

    @staticmethod
    def forward(ctx, x, p, snap, salt):
        y = torch.empty_like(x)
        call("gcgcn_dropout", _p(x), _p(y), x.numel(), _p(snap), salt, float(p), _stream())
        ctx.p, ctx.snap, ctx.salt = float(p), snap, salt
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        call("gcgcn_dropout", _p(dy), _p(dx), dy.numel(), _p(ctx.snap), ctx.salt, ctx.p, _stream())
        return dx, None, None, None


class PairBceFn(torch.autograd.Function):
    """(logits[B,N,N,R], labels[B,N,N,R]) -> loss[B].  The trainer's per-document loss, config/Config.py:355-366."""

    @staticmethod
    def forward(ctx, logits, labels, n_valid):
        B, N, _, R = logits.shape
        loss = torch.empty(B, device=logits.device)
        part = torch.empty(B * N, device=logits.device)
        call("gcgcn_pair_bce_fwd", B, N, R, _p(logits), _p(labels), _p(n_valid), _p(loss), _p(part), _stream())
        ctx.save_for_backward(logits, labels)
        ctx.n_valid = n_valid
        return loss

    @staticmethod
    def backward(ctx, dloss):
        logits, labels = ctx.saved_tensors
        B, N, _, R = logits.shape
        dlogits = torch.empty_like(logits)
        call("gcgcn_pair_bce_bwd", B, N, R, _p(logits), _p(labels), _p(ctx.n_valid), _p(dloss.contiguous()), _p(dlogits),
             _stream())
        return dlogits, None, None


class ProducerFn(torch.autograd.Function):
    """(ctx[B,T,Hd], node[B,N,Hd], dis_table[ND,P], flat; sen, pos_h, pos_t) -> E[B,N,N,Hd].  The edge-feature producer of
    one hop: WordAttention x2 + linear_word_att + SentenceAttention x2 + linear_sentence_att, GCGCN_glove.py:171-214 as
    called at :300-330.  ``compact``: E is never written; the outputs are the compact rows Ec[rows, Hd] (one per entity pair with
    a live sentence slot) and the pair -> row index, for the consumers in csrc/compact.hip (CompactEdges)."""

    @staticmethod
    def forward(ctx_, tok, node, dis_table, flat, sen, pos_h, pos_t, n_valid, cap_rows, cap_pairs, compact, deterministic):
        B, T, Hd = tok.shape
        N, S = sen.shape[1], sen.shape[3]
        ND, P = dis_table.shape
        dev = tok.device
        if compact:
            cap_pairs = max(int(cap_pairs), 1)
        sizes = (ctypes.c_int64 * 7)()
        call("gcgcn_producer_sizes", B, N, S, T, Hd, P, ND, cap_rows, cap_pairs, ctypes.cast(sizes, ctypes.c_void_p))
        ibuf = torch.empty(sizes[0], dtype=torch.int32, device=dev)
        fbuf = torch.empty(sizes[1], device=dev)
        E = None if compact else torch.empty(B, N, N, Hd, device=dev)
        pb = pos_h.element_size()
        call("gcgcn_producer_fwd", B, N, S, T, Hd, P, ND, _p(tok), _p(sen), _p(pos_h), _p(pos_t), pb, _p(node), _p(dis_table),
             _p(n_valid), _p(flat), cap_rows, cap_pairs, _p(ibuf), _p(fbuf), None, 0, _p(E), _stream())
        ctx_.save_for_backward(tok, node, dis_table, flat, sen, pos_h, pos_t, ibuf, fbuf)
        ctx_.n_valid, ctx_.caps, ctx_.nbwd, ctx_.compact = n_valid, (cap_rows, cap_pairs), int(sizes[2]), bool(compact)
        ctx_.ndet = None                                    # deterministic backward: floats of its extra workspace
        if deterministic:
            ndet = ctypes.c_int64()
            call("gcgcn_producer_det_elems", B, N, Hd, cap_pairs, ctypes.cast(ctypes.pointer(ndet), ctypes.c_void_p))
            ctx_.ndet = int(ndet.value)
        counts = ibuf[int(sizes[3]):int(sizes[3]) + 4]      # {live rows, live pairs, over capacity, 0}, on the device
        if not compact:
            ctx_.mark_non_differentiable(counts)
            return E, counts
        rows = int(sizes[6])
        Ec = fbuf[int(sizes[5]):int(sizes[5]) + rows * Hd].view(rows, Hd)
        prow = ibuf[int(sizes[4]):int(sizes[4]) + B * N * N].view(B, N, N)
        ctx_.mark_non_differentiable(counts, prow)
        return Ec, counts, prow

    @staticmethod
    def backward(ctx_, dE, _dcounts=None, _dprow=None):
        tok, node, dis_table, flat, sen, pos_h, pos_t, ibuf, fbuf = ctx_.saved_tensors
        B, T, Hd = tok.shape
        N, S = sen.shape[1], sen.shape[3]
        ND, P = dis_table.shape
        dev = tok.device
        dE = dE.contiguous()                       # compact: the gradient of Ec (rows beyond the live pairs are zero)
        bbuf = torch.empty(ctx_.nbwd, device=dev)
        dtok, dnode = torch.empty_like(tok), torch.empty_like(node)
        dtab, dflat = torch.empty_like(dis_table), torch.zeros_like(flat)       # (zeros: the layout's alignment gaps)
        args = (B, N, S, T, Hd, P, ND, _p(tok), _p(sen), _p(pos_h), _p(pos_t), pos_h.element_size(), _p(node),
                _p(dis_table), _p(ctx_.n_valid), _p(flat), ctx_.caps[0], ctx_.caps[1], _p(ibuf), _p(fbuf), _p(bbuf),
                None if ctx_.compact else _p(dE), _p(dE) if ctx_.compact else None, _p(dtok), _p(dnode), _p(dtab), _p(dflat))
        if ctx_.ndet is None:
            call("gcgcn_producer_bwd", *args, _stream())
        else:                                      # owner-computes, no float atomics: bit-reproducible (csrc/producer.hip)
            detbuf = torch.empty(ctx_.ndet, device=dev)
            call("gcgcn_producer_bwd_det", *args, _p(detbuf), ctx_.ndet, _stream())
        return dtok, dnode, dtab, dflat, None, None, None, None, None, None, None, None


class ProducerRecFn(torch.autograd.Function):
    """ProducerFn on the packed slot records: (ctx[B,T,Hd], node[B,N,Hd], dis_table[ND,P], flat; records int32[n,10]) -> the same
    outputs, bit for bit what ProducerFn gives on the tensors gcgcn_tensorise writes from those records (csrc/producer_rec.hip,
    include/gcgcn_producer_rec.h).  The three [B,N,N,S,T] byte tensors are never built."""

    @staticmethod
    def forward(ctx_, tok, node, dis_table, flat, records, n_valid, S, dis_plus, cap_rows, cap_pairs, compact, deterministic):
        B, T, Hd = tok.shape
        N = node.shape[1]
        ND, P = dis_table.shape
        dev = tok.device
        if compact:
            cap_pairs = max(int(cap_pairs), 1)
        sizes = (ctypes.c_int64 * 7)()
        call("gcgcn_producer_sizes", B, N, S, T, Hd, P, ND, cap_rows, cap_pairs, ctypes.cast(sizes, ctypes.c_void_p))
        ibuf = torch.empty(sizes[0], dtype=torch.int32, device=dev)
        fbuf = torch.empty(sizes[1], device=dev)
        E = None if compact else torch.empty(B, N, N, Hd, device=dev)
        n = int(records.shape[0])
        call("gcpr_producer_fwd", B, N, S, T, Hd, P, ND, _p(tok), n, _p(records) if n else None, dis_plus, _p(node), _p(dis_table),
             _p(n_valid), _p(flat), cap_rows, cap_pairs, _p(ibuf), _p(fbuf), None, 0, _p(E), _stream())
        ctx_.save_for_backward(tok, node, dis_table, flat, records, ibuf, fbuf)
        ctx_.n_valid, ctx_.caps, ctx_.nbwd, ctx_.compact = n_valid, (cap_rows, cap_pairs), int(sizes[2]), bool(compact)
        ctx_.S, ctx_.dis_plus = S, dis_plus
        ctx_.ndet = None
        if deterministic:
            ndet = ctypes.c_int64()
            call("gcgcn_producer_det_elems", B, N, Hd, cap_pairs, ctypes.cast(ctypes.pointer(ndet), ctypes.c_void_p))
            ctx_.ndet = int(ndet.value)
        counts = ibuf[int(sizes[3]):int(sizes[3]) + 4]      # {live rows, live pairs, over capacity, 0}, on the device
        if not compact:
            ctx_.mark_non_differentiable(counts)
            return E, counts
        rows = int(sizes[6])
        Ec = fbuf[int(sizes[5]):int(sizes[5]) + rows * Hd].view(rows, Hd)
        prow = ibuf[int(sizes[4]):int(sizes[4]) + B * N * N].view(B, N, N)
        ctx_.mark_non_differentiable(counts, prow)
        return Ec, counts, prow

    @staticmethod
    def backward(ctx_, dE, _dcounts=None, _dprow=None):
        tok, node, dis_table, flat, records, ibuf, fbuf = ctx_.saved_tensors
        B, T, Hd = tok.shape
        N = node.shape[1]
        ND, P = dis_table.shape
        dev = tok.device
        dE = dE.contiguous()
        bbuf = torch.empty(ctx_.nbwd, device=dev)
        dtok, dnode = torch.empty_like(tok), torch.empty_like(node)
        dtab, dflat = torch.empty_like(dis_table), torch.zeros_like(flat)       # (zeros: the layout's alignment gaps)
        n = int(records.shape[0])
        args = (B, N, ctx_.S, T, Hd, P, ND, _p(tok), n, _p(records) if n else None, ctx_.dis_plus, _p(node), _p(dis_table),
                _p(ctx_.n_valid), _p(flat), ctx_.caps[0], ctx_.caps[1], _p(ibuf), _p(fbuf), _p(bbuf),
                None if ctx_.compact else _p(dE), _p(dE) if ctx_.compact else None, _p(dtok), _p(dnode), _p(dtab), _p(dflat))
        if ctx_.ndet is None:
            call("gcpr_producer_bwd", *args, _stream())
        else:
            detbuf = torch.empty(ctx_.ndet, device=dev)
            call("gcpr_producer_bwd_det", *args, _p(detbuf), ctx_.ndet, _stream())
        return dtok, dnode, dtab, dflat, None, None, None, None, None, None, None, None


class CompactEdges:
    """A hop's edge tensor without the tensor: ``Ec[rows, Hd]`` (one row per entity pair with a live sentence slot), ``prow[B,N,N]``
    (row of a pair, -1 = none) and ``bias[Hd]`` -- every other real pair of ``context_sent_att`` equals the bias of
    ``linear_sentence_att`` (EdgeFeatureProducer).  GATAttention / GraphConvolution / MultiGraphConvolution (and GraphHops,
    GraphModelTail) accept it wherever they accept the dense ``edge_feat``; ``dense()`` expands it (tests, other consumers)."""

    def __init__(self, Ec: Tensor, prow: Tensor, bias: Tensor, n_valid: Optional[Tensor], batched: bool = True):
        self.Ec, self.prow, self.bias, self.n_valid, self.batched = Ec, prow, bias, n_valid, batched

    @property
    def _version(self):                       # (the edge-mean hand-off keys on it, like on a tensor's version counter)
        return self.Ec._version

    @property
    def shape(self):
        B, N, _ = self.prow.shape
        return (B, N, N, self.Ec.shape[1]) if self.batched else (N, N, self.Ec.shape[1])

    def dense(self) -> Tensor:
        B, N, _ = self.prow.shape
        live = (self.prow >= 0).unsqueeze(-1)
        e = torch.where(live, self.Ec[self.prow.clamp_min(0).long()], self.bias.expand(B, N, N, -1))
        if self.n_valid is not None:
            ok = torch.arange(N, device=e.device)[None, :] < self.n_valid[:, None]
            e = e * (ok[:, :, None] & ok[:, None, :]).unsqueeze(-1).to(e.dtype)
        return e if self.batched else e[0]


class GatCompactFn(torch.autograd.Function):
    """GatFn on compact rows: (X[B,N,D], Ec[rows,D], bias[D], flat) -> (A[B,N,N], Ebar[B,N,D], X)."""

    @staticmethod
    def forward(ctx, x, Ec, bias, flat, prow, n_valid, p, snap, pending, Dh, uvc, uvc_valid):
        B, N, D = x.shape
        uvc, uvc_valid, s, P, A, ebar, (st, sn, cnt) = _gat_fwd_buffers(x, snap, pending, uvc, uvc_valid)
        call("gcgcn_gat_fwd_compact", B, N, D, Dh, _p(x), _p(Ec), _p(prow), _p(bias), _p(n_valid), _p(flat), _p(snap), float(p),
             _p(uvc), _p(s), _p(P), _p(A), _p(ebar), _p(st), _p(sn), cnt, 1 if uvc_valid else 0, _stream())
        ctx.save_for_backward(x, Ec, bias, flat, uvc, P, prow)
        ctx.n_valid, ctx.p, ctx.snap, ctx.Dh = n_valid, float(p), snap, Dh
        return (P if A is None else A), ebar, x.view_as(x)

    @staticmethod
    def backward(ctx, dA, dEbar, dXin):
        x, Ec, bias, flat, uvc, P, prow = ctx.saved_tensors
        B, N, D = x.shape
        dA, dEbar, dXin, dlogit, ds, dvpart, duvc, scratch = _gat_bwd_buffers(x, dA, dEbar, dXin, "gcgcn_gat_bwd_compact_scratch")
        dX = torch.empty_like(x)
        dEc = torch.zeros_like(Ec)                       # rows beyond the live pairs stay zero (the producer's GEMMs read them)
        dbias = torch.empty_like(bias)
        dflat = torch.empty_like(flat)
        call("gcgcn_gat_bwd_compact", B, N, D, ctx.Dh, _p(x), _p(Ec), _p(prow), _p(bias), _p(ctx.n_valid), _p(flat), _p(ctx.snap), ctx.p,
             _p(uvc), _p(P), _p(dA), _p(dEbar), _p(dXin), _p(dX), _p(dEc), _p(dbias), _p(dflat), _p(dlogit), _p(ds), _p(dvpart), _p(duvc),
             _p(scratch), _stream())
        return dX, dEc, dbias, dflat, None, None, None, None, None, None, None, None


class EdgeMeanCompactFn(torch.autograd.Function):
    """EdgeMeanFn on compact rows: (Ec[rows,D], bias[D]; prow[B,N,N]) -> Ebar[B,N,D]."""

    @staticmethod
    def forward(ctx, Ec, bias, prow, n_valid):
        B, N, _ = prow.shape
        D = Ec.shape[1]
        ebar = torch.empty(B, N, D, device=Ec.device)
        call("gcgcn_edge_mean_fwd_compact", B, N, D, _p(Ec), _p(prow), _p(bias), _p(n_valid), _p(ebar), _stream())
        ctx.save_for_backward(prow)
        ctx.n_valid, ctx.rows = n_valid, Ec.shape[0]
        return ebar

    @staticmethod
    def backward(ctx, dEbar):
        prow, = ctx.saved_tensors
        B, N, _ = prow.shape
        dEbar = dEbar.contiguous()
        D = dEbar.shape[-1]
        dEc = torch.zeros(ctx.rows, D, device=dEbar.device)
        dbias = torch.empty(D, device=dEbar.device)
        rowbuf = torch.empty(2 * B * N, device=dEbar.device)
        call("gcgcn_edge_mean_bwd_compact", B, N, D, _p(prow), _p(ctx.n_valid), _p(dEbar), _p(dEc), _p(dbias), _p(rowbuf), _stream())
        return dEc, dbias, None, None


def _head_call(matmul: int, name: str, *args):
    """One head entry point with the argument matmul.  0: the call alone, as always.  1: announced to the library on this thread
    right before the call, which takes the announcement (include/gcgcn.h, gcgcn_head_fwd) -- per thread and per call: a head on
    another thread, or the next call on this one, is not affected."""
    if matmul:
        call("gcgcn_set_option", b"head_matmul", matmul)
    call(name, *args)


class HeadFn(torch.autograd.Function):
    """(flat, ner_emb[7,Pt], dis_table[ND,Pr], feats_0 .. feats_{nf-1} [B,N,Hd]; node_type, node_relative_pos) ->
    logits[B,N,N,R].  The classifier head, GCGCN_glove.py:306-307, 344-358."""

    @staticmethod
    def forward(ctx, flat, ner_emb, dis_table, node_type, rel, n_valid, R, dis_plus, *feats):
        return HeadFn._forward(ctx, 0, flat, ner_emb, dis_table, node_type, rel, n_valid, R, dis_plus, *feats)

    @staticmethod
    def _forward(ctx, matmul, flat, ner_emb, dis_table, node_type, rel, n_valid, R, dis_plus, *feats):
        """matmul: the argument of the forward and of the backward call (_head_call)."""
        B, N, Hd = feats[0].shape
        nf, Pt, (ND, Pr) = len(feats), ner_emb.shape[1], dis_table.shape
        dev = flat.device
        sizes = (ctypes.c_int64 * 3)()
        call("gcgcn_head_sizes", B, N, R, ND, ctypes.cast(sizes, ctypes.c_void_p))
        fbuf = torch.empty(sizes[0], device=dev)
        # ragged batch: the pair passes run on the pairs that exist (compacted rows; the index lives in ibuf, on the device)
        ibuf = torch.empty(sizes[2], dtype=torch.int32, device=dev) if n_valid is not None else None
        logits = torch.empty(B, N, N, R, device=dev)
        fp = (ctypes.c_void_p * nf)(*[f.data_ptr() for f in feats])
        args = (B, N, Hd, nf, Pt, Pr, R, ND, dis_plus, ctypes.cast(fp, ctypes.c_void_p), _p(node_type), _p(rel), _p(ner_emb), _p(dis_table),
                _p(n_valid), _p(flat), _p(fbuf), _p(ibuf), _p(logits), _stream())
        _head_call(matmul, "gcgcn_head_fwd", *args)
        ctx.save_for_backward(flat, ner_emb, dis_table, node_type, rel, fbuf, *feats)
        ctx.n_valid, ctx.R, ctx.dis_plus, ctx.nbwd, ctx.ibuf, ctx.matmul = n_valid, R, dis_plus, int(sizes[1]), ibuf, matmul
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        flat, ner_emb, dis_table, node_type, rel, fbuf, *feats = ctx.saved_tensors
        B, N, Hd = feats[0].shape
        nf, Pt, (ND, Pr) = len(feats), ner_emb.shape[1], dis_table.shape
        dev = flat.device
        dlogits = dlogits.contiguous()
        bbuf = torch.empty(ctx.nbwd, device=dev)
        dfeats = [torch.empty_like(f) for f in feats]
        dner, dtab, dflat = torch.empty_like(ner_emb), torch.empty_like(dis_table), torch.zeros_like(flat)   # (gaps stay zero)
        fp = (ctypes.c_void_p * nf)(*[f.data_ptr() for f in feats])
        dp = (ctypes.c_void_p * nf)(*[f.data_ptr() for f in dfeats])
        args = (B, N, Hd, nf, Pt, Pr, ctx.R, ND, ctx.dis_plus, ctypes.cast(fp, ctypes.c_void_p), _p(node_type), _p(rel), _p(ner_emb),
                _p(dis_table), _p(ctx.n_valid), _p(flat), _p(fbuf), _p(ctx.ibuf), _p(bbuf), _p(dlogits), ctypes.cast(dp, ctypes.c_void_p),
                _p(dner), _p(dtab), _p(dflat), _stream())
        _head_call(ctx.matmul, "gcgcn_head_bwd", *args)
        return (dflat, dner, dtab, None, None, None, None, None, *dfeats)


class HeadBf16Fn(HeadFn):
    """HeadFn with the four bilinear passes on bf16 operands (csrc/head_bf16.hip; Bf16HeadBilinearFn below is their definition)."""

    @staticmethod
    def forward(ctx, flat, ner_emb, dis_table, node_type, rel, n_valid, R, dis_plus, *feats):
        return HeadFn._forward(ctx, 1, flat, ner_emb, dis_table, node_type, rel, n_valid, R, dis_plus, *feats)


HEAD_MATMUL = {"fp32": HeadFn, "bf16": HeadBf16Fn}   # classifier_head's matmul -> the autograd node


def _round_bf16(t: Tensor) -> Tensor:
    """Round once to bf16 (nearest even) through float32, back in the dtype of ``t``."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


class Bf16HeadBilinearFn(torch.autograd.Function):
    """The DEFINITION of ``classifier_head(..., matmul="bf16")``'s bilinear passes, in plain PyTorch on any device and dtype (its
    float64 run is the reference of the tests): ``(eh[P,128], et[P,128], W_b[R,128,128], W_c[R,256], bias[R]) -> out[P,R]``, where
    ``eh`` / ``et`` are the fp32 results of the unchanged gather + tanh and ``bias = bili_layer_01.bias +
    classification_layer_01.bias``.  ``bf16(.)`` rounds once to nearest even; every sum is exact in the dtype it runs in (fp32 on the
    device)::

        out[p,r]    = sum_ab bf16(eh[p,a] et[p,b]) bf16(W_b[r,a,b]) + sum_k bf16(cat(eh, et)[p,k]) bf16(W_c[r,k]) + bias[r]
        d eh[p,a]   = sum_rb bf16(dout[p,r] et[p,b]) bf16(W_b[r,a,b]) + sum_r bf16(dout[p,r]) bf16(W_c[r,a])
        d et[p,b]   = sum_ra bf16(dout[p,r] eh[p,a]) bf16(W_b[r,a,b]) + sum_r bf16(dout[p,r]) bf16(W_c[r,128 + b])
        dW_b[r,a,b] = sum_p bf16(dout[p,r]) bf16(eh[p,a] et[p,b])
        dW_c        = bf16(dout)^T bf16(cat(eh, et)),        d bias = column sums of the UNROUNDED dout

    The generated operands are formed as FLOAT32 products (whatever the dtype of the run) and rounded once; the bias never passes
    through a rounding.  ``rnd`` replaces the rounding (the identity turns the function into the exact head)."""

    @staticmethod
    def forward(ctx, eh, et, Wb, Wc, bias, rnd=None):
        rnd = rnd or _round_bf16
        ctx.rnd = rnd
        ctx.save_for_backward(eh, et, Wb, Wc)
        Pn, R = eh.shape[0], Wb.shape[0]
        outer = rnd(Bf16HeadBilinearFn._prod(eh, et, rnd)).reshape(Pn, -1)                    # [P, (a, b)]
        return outer @ rnd(Wb).reshape(R, -1).t() + rnd(torch.cat([eh, et], 1)) @ rnd(Wc).t() + bias

    @staticmethod
    def _prod(x, y, rnd):
        """x[p,i] y[p,j] as the kernel forms it: a float32 product (exact dtype when the rounding is switched off)."""
        if rnd is _round_bf16:
            return (x.to(torch.float32).unsqueeze(2) * y.to(torch.float32).unsqueeze(1)).to(x.dtype)
        return x.unsqueeze(2) * y.unsqueeze(1)

    @staticmethod
    def backward(ctx, dout):
        eh, et, Wb, Wc = ctx.saved_tensors
        rnd, H = ctx.rnd, eh.shape[1]
        Wbr, Wcr, dr = rnd(Wb), rnd(Wc), rnd(dout)
        de = rnd(Bf16HeadBilinearFn._prod(dout, et, rnd))                                      # [P, r, b]
        deh = torch.einsum("prb,rab->pa", de, Wbr) + dr @ Wcr[:, :H]
        dt = rnd(Bf16HeadBilinearFn._prod(dout, eh, rnd))                                      # [P, r, a]
        det = torch.einsum("pra,rab->pb", dt, Wbr) + dr @ Wcr[:, H:]
        outer = rnd(Bf16HeadBilinearFn._prod(eh, et, rnd))                                     # [P, a, b]
        dWb = torch.einsum("pr,pab->rab", dr, outer)
        dWc = dr.t() @ rnd(torch.cat([eh, et], 1))
        return deh, det, dWb, dWc, dout.sum(0), None


# Range-check the integer ids handed to the head / the producer before the kernels index with them.  The reference's
# embedding lookups raise IndexError on an id outside the table; the kernels clamp instead (an out-of-range id must never
# become an out-of-bounds read), which would turn corrupt inputs into plausible logits.  The check is one fused reduction and
# ONE host read per call; it is skipped inside a hipGraph capture, and a training loop that has validated its data once can
# switch it off (``gcgcn_amd.functional.check_ids = False``).
check_ids = True
NER_ROWS = 7        # nn.Embedding(7, entity_type_size, padding_idx=0), GCGCN_glove.py:241 -- the head's kernels index 7 rows
HEAD_MAX_DIS_ROWS = 32   # csrc/head.hip HT_IDS: rows of dis_embed the head's backward pass can sum


def _check_id_range(checks):
    """checks: [(name, tensor, lo, hi)] -- raise IndexError naming the first tensor with an id outside [lo, hi]."""
    if not check_ids or torch.cuda.is_current_stream_capturing():
        return
    bad = torch.stack([((t < lo) | (t > hi)).any() for _, t, lo, hi in checks])
    if bool(bad.any().item()):
        flags = bad.tolist()
        name, t, lo, hi = next(c for c, f in zip(checks, flags) if f)
        raise IndexError(f"{name}: ids must lie in [{lo}, {hi}], got min {int(t.min())} / max {int(t.max())}")


def classifier_head(feats, node_type, node_relative_pos, ner_emb, dis_table, flat, relation_num, n_valid=None, dis_plus=10, matmul="fp32"):
    """logits[B,N,N,R] from the model's node_feats list (each [B,N,Hd]), node_type int64[B,N], node_relative_pos
    int64[B,N,N], the two embedding tables and the head's flat parameters.

    ``matmul="bf16"`` (opt-in): the forward pass, ``d eh``, ``d et`` and the weight gradients of the bilinear and the Linear layer take
    bf16 operands with fp32 accumulation (csrc/head_bf16.hip; :class:`Bf16HeadBilinearFn` is the definition); everything else, and
    every tensor in memory, stays fp32.  ``"fp32"`` (default) issues the calls it always issued."""
    if matmul not in HEAD_MATMUL:
        raise ValueError(f"classifier_head: matmul must be 'fp32' or 'bf16', got {matmul!r}")
    feats = [_chk(f, f"node_feats[{i}]", 3) for i, f in enumerate(feats)]
    B, N, Hd = feats[0].shape
    if any(tuple(f.shape) != (B, N, Hd) for f in feats):
        raise ValueError("node_feats: every entry must have the same [B,N,H] shape")
    for nm, t, shp in (("node_type", node_type, (B, N)), ("node_relative_pos", node_relative_pos, (B, N, N))):
        if not t.is_cuda or t.dtype != torch.int64 or tuple(t.shape) != shp:
            raise ValueError(f"{nm}: expected a GPU int64 tensor of shape {shp}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if ner_emb.dim() != 2 or ner_emb.shape[0] != NER_ROWS:
        raise ValueError(f"ner_emb.weight: the head indexes {NER_ROWS} rows (nn.Embedding(7, .), glove:241), got {tuple(ner_emb.shape)}")
    if dis_table.dim() != 2 or dis_table.shape[0] < 2 * int(dis_plus) + 1:
        raise ValueError(f"dis_embed.weight: needs at least 2 * dis_plus + 1 = {2 * int(dis_plus) + 1} rows, got {tuple(dis_table.shape)}")
    if dis_table.shape[0] > HEAD_MAX_DIS_ROWS:
        raise ValueError(f"dis_embed.weight: the head handles at most {HEAD_MAX_DIS_ROWS} rows of the distance table (its backward "
                         f"pass keeps one sum per id in LDS), got {tuple(dis_table.shape)}")
    _check_id_range([("node_type", node_type, 0, NER_ROWS - 1),
                     ("node_relative_pos", node_relative_pos, -int(dis_plus), int(dis_plus))])
    return HEAD_MATMUL[matmul].apply(_chk(flat, "flat"), _chk(ner_emb, "ner_emb.weight", 2), _chk(dis_table, "dis_embed.weight", 2),
                                     node_type.contiguous(), node_relative_pos.contiguous(), _nv(n_valid, B, N, flat.device),
                                     int(relation_num), int(dis_plus), *feats)


def producer_live_counts(sen: Tensor, n_valid=None):
    """(live sentence slots, entity pairs with a live slot) of a batch -- one small kernel and a device-to-host read.
    A slot is live iff token 0 belongs to it: the reference's own padding test (``~sen_matrix[..., 0:1]``, glove:305)."""
    B, N, _, S, T = sen.shape
    counts = torch.empty(2, dtype=torch.int32, device=sen.device)
    call("gcgcn_producer_count", B, N, S, T, _p(sen), _p(n_valid), _p(counts), _stream())
    r, q = counts.tolist()
    return r, q


# The position matrices are [B,N,N,S,T] (77 MB per DocRED document as int64): a range check reads them once more, which the
# producer's own kernels do not (they touch live slots only).  Off by default; the head's ids (a few KB) are always checked.
check_position_ids = False


class ProducerCapacityError(RuntimeError):
    """max_live_slots / max_live_pairs were smaller than what the batch holds."""


def edge_features(tok, sen, pos_h, pos_t, node, dis_table, flat, n_valid=None, max_live_slots=None, max_live_pairs=None,
                  check_capacity=False, return_counts=False, compact=False, deterministic=False, slot_records=None, dis_plus=10,
                  slot_shape=None):
    """E[B,N,N,Hd] of one hop from token states tok[B,T,Hd], sentence masks sen[B,N,N,S,T] (bool / uint8), distance ids
    pos_h / pos_t [B,N,N,S,T] (int64 as the reference passes them, or int32 / uint8), entity features node[B,N,Hd] and
    the distance-embedding table dis_table[ND,P].  Without ``max_live_*`` the live slots are counted first (one host
    synchronisation per call, as cheap as the reference's own ``.cuda()`` copies); with them nothing synchronises and the
    call can be captured in a hipGraph.  Capacities that turn out too small are never silent: the kernels compute nothing
    and write NaN into every real pair of E (so a captured graph fails loudly downstream); ``check_capacity=True`` reads the
    device-side flag back (one synchronisation) and raises :class:`ProducerCapacityError`; ``return_counts=True`` also returns
    the device tensor ``int32[4] = {live slots, live pairs, over capacity, 0}`` for a check of the caller's own timing.
    ``compact=True``: returns ``(Ec[rows,Hd], prow[B,N,N])`` instead of E -- E is never written (see CompactEdges).
    ``deterministic=True``: the backward sums the per-entity node-term gradient and the sentence attention's vector / bias gradient
    by their owners instead of with fp32 atomics (two more launches, one more workspace): every gradient is bit-reproducible.
    ``slot_records``: the packed records themselves -- int32 ``[n, 10]`` on the GPU, rows ``doc, u, v, j, s0, s1, h0, h1, t0, t1`` as
    ``data.collate`` uploads them -- in place of ``sen`` / ``pos_h`` / ``pos_t``, which must then be None; ``slot_shape`` carries S
    (an int, or anything whose last entry is S) and ``dis_plus`` the offset of the distance ids.  The result equals, bit for bit, what
    the dense tensors ``gcgcn_tensorise`` writes from those records give; no ``[B,N,N,S,T]`` tensor exists.  ``(doc, u, v, j)`` must be
    unique.  Pass ``max_live_slots`` / ``max_live_pairs`` from ``data.live_counts`` (``collate(dense_slots=False)`` returns both) or a
    batch-independent bound of your data.  Without them the capacities fall back to the table's own bounds, ``min(n, B N N S)`` rows
    and ``min(n, B N N)`` pairs: still no host read, but every per-row buffer (about ``7 Hd`` floats per row forward and as much
    again backward) is sized for ALL records, live or not -- several times the live rows on DocRED-like batches, and at B = 32, N = 42,
    S = 5, Hd = 128 with a full table hundreds of MB, more than the dense tensors this route avoids."""
    if slot_records is not None and (sen is not None or pos_h is not None or pos_t is not None):
        raise ValueError("edge_features: give either slot_records or sen_matrix / pos_matrix_h / pos_matrix_t, not both")
    if slot_records is None and (sen is None or pos_h is None or pos_t is None):
        raise ValueError("edge_features: sen_matrix / pos_matrix_h / pos_matrix_t are required without slot_records")
    if slot_records is not None:
        _check_slot_records(slot_records, slot_shape)
    tok, node, dis_table = _chk(tok, "context_output", 3), _chk(node, "node_feat", 3), _chk(dis_table, "dis_embed.weight", 2)
    B, T, Hd = tok.shape
    if slot_records is not None:
        return _edge_features_rec(tok, slot_records, node, dis_table, flat, n_valid, max_live_slots, max_live_pairs, check_capacity,
                                  return_counts, compact, deterministic, dis_plus, slot_shape)
    if sen.dim() != 5 or sen.shape[0] != B or sen.shape[4] != T or sen.shape[1] != sen.shape[2]:
        raise ValueError(f"sen_matrix: expected [B={B}, N, N, S, T={T}], got {tuple(sen.shape)}")
    N, S = sen.shape[1], sen.shape[3]
    if node.shape != (B, N, Hd):
        raise ValueError(f"node_feat: expected {(B, N, Hd)}, got {tuple(node.shape)}")
    if not sen.is_cuda:
        raise RuntimeError("sen_matrix: gcgcn_amd runs on MI355X only (no CPU fallback)")
    if sen.dtype == torch.bool:
        sen = sen.view(torch.uint8)
    elif sen.dtype != torch.uint8:
        sen = (sen != 0).to(torch.uint8)
    sen = sen.contiguous()
    for nm, p in (("pos_matrix_h", pos_h), ("pos_matrix_t", pos_t)):
        if tuple(p.shape) != tuple(sen.shape) or p.dtype not in (torch.int64, torch.int32, torch.uint8) or not p.is_cuda:
            raise ValueError(f"{nm}: expected a GPU int64 / int32 / uint8 tensor of shape {tuple(sen.shape)}")
    if pos_t.dtype != pos_h.dtype:
        raise ValueError("pos_matrix_h and pos_matrix_t must have the same dtype")
    if check_position_ids:
        _check_id_range([("pos_matrix_h", pos_h, 0, dis_table.shape[0] - 1), ("pos_matrix_t", pos_t, 0, dis_table.shape[0] - 1)])
    nv = _nv(n_valid, B, N, tok.device)
    given = max_live_slots is not None and max_live_pairs is not None
    if not given:
        r, q = producer_live_counts(sen, nv)
        max_live_slots = r if max_live_slots is None else max_live_slots
        max_live_pairs = q if max_live_pairs is None else max_live_pairs
    out = ProducerFn.apply(tok, node, dis_table, _chk(flat, "flat"), sen, pos_h.contiguous(), pos_t.contiguous(), nv,
                           int(max_live_slots), int(max_live_pairs), bool(compact), bool(deterministic))
    if compact:
        E, counts = (out[0], out[2]), out[1]          # (Ec, prow): the caller adds the bias and wraps them in CompactEdges
    else:
        E, counts = out
    if check_capacity and not torch.cuda.is_current_stream_capturing():
        if int(counts[2].item()) != 0:
            raise ProducerCapacityError(f"edge_features: max_live_slots={max_live_slots} / max_live_pairs={max_live_pairs} are "
                                        "smaller than the batch's live sentence slots / entity pairs (producer_live_counts "
                                        "reports both); nothing was computed")
    return (E, counts) if return_counts else E


def _check_slot_records(records, slot_shape) -> int:
    """The argument checks of the record route that need no GPU -> S."""
    if slot_shape is None:
        raise ValueError("edge_features: slot_records needs slot_shape (S, the sentence slots per pair; collate returns it)")
    S = int(slot_shape if isinstance(slot_shape, int) else tuple(slot_shape)[-1])
    if not 1 <= S <= 31:
        raise ValueError(f"edge_features: slot_shape gives S={S} sentence slots per pair (1..31 supported)")
    if not isinstance(records, Tensor) or records.dtype != torch.int32 or records.dim() != 2 or records.shape[1] != 10:
        raise ValueError("slot_records: expected an int32 tensor of shape [n, 10] (doc, u, v, j, s0, s1, h0, h1, t0, t1), got "
                         f"{getattr(records, 'dtype', type(records))} {tuple(getattr(records, 'shape', ()))}")
    return S


def _edge_features_rec(tok, records, node, dis_table, flat, n_valid, max_live_slots, max_live_pairs, check_capacity, return_counts,
                       compact, deterministic, dis_plus, slot_shape):
    """edge_features on the record table (ProducerRecFn)."""
    B, T, Hd = tok.shape
    S = _check_slot_records(records, slot_shape)
    if not records.is_cuda:
        raise RuntimeError("slot_records: gcgcn_amd runs on MI355X only (no CPU fallback)")
    if node.dim() != 3 or node.shape[0] != B or node.shape[2] != Hd:
        raise ValueError(f"node_feat: expected [B={B}, N, Hd={Hd}], got {tuple(node.shape)}")
    N = node.shape[1]
    nv = _nv(n_valid, B, N, tok.device)
    n = int(records.shape[0])
    if max_live_slots is None:
        max_live_slots = min(n, B * N * N * S)            # no record, no row: bounds that need no read
    if max_live_pairs is None:
        max_live_pairs = min(n, B * N * N)
    out = ProducerRecFn.apply(tok, node, dis_table, _chk(flat, "flat"), records.contiguous(), nv, S, int(dis_plus), int(max_live_slots),
                              int(max_live_pairs), bool(compact), bool(deterministic))
    if compact:
        E, counts = (out[0], out[2]), out[1]
    else:
        E, counts = out
    if check_capacity and not torch.cuda.is_current_stream_capturing():
        if int(counts[2].item()) != 0:
            raise ProducerCapacityError(f"edge_features: max_live_slots={max_live_slots} / max_live_pairs={max_live_pairs} are "
                                        "smaller than the batch's live sentence slots / entity pairs (data.live_counts "
                                        "reports both); nothing was computed")
    return (E, counts) if return_counts else E


# ---- functional entry points -------------------------------------------------------------------------
def _snap_for(training: bool, p: float, dev) -> Optional[Tensor]:
    return rng_snapshot(dev) if (training and p > 0.0) else None


def gat_attention(x, e, flat, n_valid=None, p=0.1, training=False, hidden_dim=None, mask=None, uvc=None, uvc_valid=False):
    """``mask`` (bool/uint8 ``[B,N,N]``, True = fill with -100000): the paper-faithful opt-in; None = the reference.
    ``uvc``: caller-owned buffer ``[2D+1]`` for the folded projection; ``uvc_valid``: it already holds the fold of THESE
    parameter values (kept from an earlier call) and the fold kernel is skipped."""
    x, e = _chk(x, "node_feat", 3), _chk(e, "edge_feat", 4)
    B, N, D = x.shape
    if e.shape != (B, N, N, D):
        raise ValueError(f"edge_feat: expected {(B, N, N, D)}, got {tuple(e.shape)}")
    nv = _nv(n_valid, B, N, x.device)
    snap = rng_snapshot(x.device, lazy=True) if (training and p > 0.0) else None
    if mask is not None:
        if not mask.is_cuda or tuple(mask.shape) != (B, N, N):
            raise ValueError(f"mask: expected a GPU tensor of shape {(B, N, N)}, got {tuple(mask.shape)} on {mask.device}")
        mask = (mask != 0).to(torch.uint8).contiguous()
    return GatFn.apply(x, e, _chk(flat, "flat"), nv, p, snap, _take_pending_rng(x.device),
                       D if hidden_dim is None else int(hidden_dim), mask, uvc, bool(uvc_valid))   # (A, Ebar, alias of x)


def gat_attention_compact(x, ce: CompactEdges, flat, n_valid=None, p=0.1, training=False, hidden_dim=None, uvc=None, uvc_valid=False):
    x = _chk(x, "node_feat", 3)
    B, N, D = x.shape
    if tuple(ce.prow.shape) != (B, N, N) or ce.Ec.shape[1] != D:
        raise ValueError(f"compact edge_feat: pairs {tuple(ce.prow.shape)} / width {ce.Ec.shape[1]} do not match node_feat {tuple(x.shape)}")
    nv = _nv(n_valid, B, N, x.device)
    snap = rng_snapshot(x.device, lazy=True) if (training and p > 0.0) else None
    return GatCompactFn.apply(x, _chk(ce.Ec, "Ec", 2), _chk(ce.bias, "bias", 1), _chk(flat, "flat"), ce.prow, nv, p, snap,
                              _take_pending_rng(x.device), D if hidden_dim is None else int(hidden_dim), uvc, bool(uvc_valid))


def edge_mean_compact(ce: CompactEdges, n_valid=None):
    B, N, _ = ce.prow.shape
    return EdgeMeanCompactFn.apply(_chk(ce.Ec, "Ec", 2), _chk(ce.bias, "bias", 1), ce.prow, _nv(n_valid, B, N, ce.Ec.device))


def edge_mean(e, n_valid=None):
    if isinstance(e, CompactEdges):
        return edge_mean_compact(e, n_valid)
    e = _chk(e, "edge_feat", 4)
    B, N = e.shape[0], e.shape[1]
    return EdgeMeanFn.apply(e, _nv(n_valid, B, N, e.device))


def multi_head_adjacency(x, flat, H, n_valid=None, p=0.1, training=False, rowblk=None):
    x = _chk(x, "node_feat", 3)
    B, N, D = x.shape
    return MhaFn.apply(x, _chk(flat, "flat"), _nv(n_valid, B, N, x.device), H, p, _snap_for(training, p, x.device), rowblk)


def gcn_stack(x, ebar, adj, flat, L, H, n_valid=None, p=0.2, training=False, e_next=None, out_dropout=0.0, rowblk=None):
    """Returns ``out`` -- or ``(out, mean_j e_next)`` when the next hop's edge tensor ``e_next[B,N,N,D']`` is given.
    ``out_dropout`` > 0 (training only): the hop's ``x <- dropout(out)`` (glove:341) applied inside the block."""
    x, ebar, adj = _chk(x, "node_feat", 3), _chk(ebar, "edge_mean", 3), _chk(adj, "adjacency", 4)
    B, N, D = x.shape
    if ebar.shape != (B, N, D) or adj.shape != (B, H, N, N):
        raise ValueError(f"gcn_stack: shapes x{tuple(x.shape)} ebar{tuple(ebar.shape)} adj{tuple(adj.shape)} H={H}")
    nv = _nv(n_valid, B, N, x.device)
    if e_next is not None:
        e_next = _chk(e_next, "next edge_feat", 4)
        if e_next.shape[:3] != (B, N, N):
            raise ValueError(f"gcn_stack: next edge tensor {tuple(e_next.shape)} does not match B={B} N={N}")
    snap = _snap_for(training, p, x.device)                       # draw order: block, then the hop's output dropout
    out_snap = _snap_for(training, out_dropout, x.device)
    if rowblk is None:                                            # a block called on its own: its own list
        rowblk = row_blocks(nv, B, N)
    out, ebar_next = GcnFn.apply(x, ebar, adj, _chk(flat, "flat"), nv, L, H, p, snap, e_next,
                                 out_dropout if out_snap is not None else 0.0, out_snap, rowblk)
    return out if e_next is None else (out, ebar_next)


def maggc_fusable(x: Tensor, H: int) -> bool:
    """Can MultiHeadAttention + MultiGraphConvolution of one hop run as one fused call pair on this input?  (graph of at most 64
    entities, narrow heads; gcgcn_maggc_fusable)"""
    return x.is_cuda and x.dim() == 3 and bool(_lib.lib().gcgcn_maggc_fusable(x.shape[1], x.shape[2], int(H)))


def maggc_hop(x, ebar, flat_mha, flat, L, H, n_valid=None, p_mha=0.1, p=0.2, training=False, e_next=None, out_dropout=0.0, rowblk=None):
    """MultiHeadAttention (its own draw first, like the separate modules) + MultiGraphConvolution of one hop, fused (MaggcFn)."""
    x, ebar = _chk(x, "node_feat", 3), _chk(ebar, "edge_mean", 3)
    B, N, D = x.shape
    if ebar.shape != (B, N, D):
        raise ValueError(f"maggc_hop: shapes x{tuple(x.shape)} ebar{tuple(ebar.shape)}")
    nv = _nv(n_valid, B, N, x.device)
    if e_next is not None:
        e_next = _chk(e_next, "next edge_feat", 4)
    snap_mha = _snap_for(training, p_mha, x.device)                 # draw order of the separate modules: attention, block, glue
    snap = _snap_for(training, p, x.device)
    out_snap = _snap_for(training, out_dropout, x.device)
    if rowblk is None:
        rowblk = row_blocks(nv, B, N)
    out, ebar_next = MaggcFn.apply(x, ebar, _chk(flat_mha, "flat"), _chk(flat, "flat"), nv, L, H, p_mha, snap_mha, p, snap, e_next,
                                   out_dropout if out_snap is not None else 0.0, out_snap, rowblk)
    return out if e_next is None else (out, ebar_next)


def graph_conv(x, ebar, adj, we, wn, bias=None):
    x, ebar, adj = _chk(x, "inputs", 3), _chk(ebar, "edge_mean", 3), _chk(adj, "adjacency_matrix", 3)
    return GraphConvFn.apply(x, ebar, adj, _chk(we, "weights_edge", 2), _chk(wn, "weights_node", 2),
                             None if bias is None else _chk(bias, "bias", 1))


def dropout(x, p=0.2, training=False, salt=SALT_GLUE):
    x = _chk(x, "x")
    if not training or p <= 0.0:
        return x
    return DropoutFn.apply(x, p, rng_snapshot(x.device), salt)


# ---- hand-off of the edge mean from GATAttention to the GraphConvolution that follows ---------------
# The reference calls gat(X, E, mask) and then graphcnn[0](X, E, A) with the SAME E (glove:332-333).
# GATAttention's single pass over E also yields mean_j E; it is parked here so the convolution does
# not stream E from HBM a second time.  Per thread, keyed by the edge tensor's identity (a few entries: interleaved
# models keep theirs), consumed on use, dropped when the tensor dies or changes (version counter).
_HANDOFF_SLOTS = 4


def _handoffs() -> dict:
    h = getattr(_tls, "handoff", None)
    if h is None:
        h = _tls.handoff = {}
    return h


def park_edge_mean(e: Tensor, n_valid, ebar: Tensor):
    h = _handoffs()
    for k in [k for k, v in h.items() if v[0]() is None]:
        del h[k]
    h.pop(id(e), None)
    while len(h) >= _HANDOFF_SLOTS:
        del h[next(iter(h))]                       # oldest first
    h[id(e)] = (weakref.ref(e), e._version, n_valid, ebar)


def take_edge_mean(e: Tensor, n_valid) -> Optional[Tensor]:
    ent = _handoffs().pop(id(e), None)
    if ent is None:
        return None
    ref, ver, nvp, ebar = ent
    if ref() is e and e._version == ver and nvp is n_valid:
        return ebar
    return None


def _pair_inputs(logits, labels, n_valid, who: str):
    """(logits[B,N,N,R], labels[B,N,N,R], n_valid int32[B] or None, unbatched?) of a pair-wise call, checked."""
    single = isinstance(logits, torch.Tensor) and logits.dim() == 3
    lg = _chk(logits.unsqueeze(0) if single else logits, "logits", 4)
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f"labels: expected a tensor, got {type(labels).__name__}")
    lb = _chk((labels.unsqueeze(0) if single else labels).to(torch.float32), "labels", 4)
    if lb.shape != lg.shape or lg.shape[1] != lg.shape[2]:
        raise ValueError(f"{who}: logits {tuple(lg.shape)} vs labels {tuple(lb.shape)}")
    return lg, lb, _nv(n_valid, lg.shape[0], lg.shape[1], lg.device), single


@dataclass(frozen=True)
class TrainStatsResult:
    """The eight counters of ``gcgcn_pair_stats`` after one read-back.  ``na_*``, ``not_na_*`` and ``correct`` / ``total`` are
    the ``correct`` / ``total`` fields of the trainer's ``acc_NA``, ``acc_not_NA`` and ``acc_total`` (config/Config.py:388-393);
    ``nan_pairs`` counts the entity pairs whose row of logits holds a NaN (they are in no other counter)."""
    na_correct: int
    na_total: int
    not_na_correct: int
    not_na_total: int
    correct: int
    total: int
    nan_pairs: int
    documents: int

    @property
    def counters(self) -> tuple:
        return (self.na_correct, self.na_total, self.not_na_correct, self.not_na_total, self.correct, self.total, self.nan_pairs,
                self.documents)

    # Accuracy.get() (Config.py:48-52): 0.0 on an empty total
    @property
    def na_acc(self) -> float:
        return float(self.na_correct) / self.na_total if self.na_total else 0.0

    @property
    def not_na_acc(self) -> float:
        return float(self.not_na_correct) / self.not_na_total if self.not_na_total else 0.0

    @property
    def total_acc(self) -> float:
        return float(self.correct) / self.total if self.total else 0.0


class TrainStats:
    """The trainer's per-epoch accuracy bookkeeping (``acc_NA``, ``acc_not_NA``, ``acc_total``: config/Config.py:376-393) kept in
    a device ``int64[8]`` buffer instead of a host copy of every document's probabilities and a Python loop over its pairs::

        stats = TrainStats(device)
        for batch in loader:
            loss = pair_bce_loss(logits, labels, n_valid, stats=stats).sum() / B     # or stats.update(logits, labels, n_valid)
            ...
        r = stats.get()                 # the one host read: r.na_acc, r.not_na_acc, r.total_acc, the eight integers
        stats.reset()                   # next epoch (Config.py:332-334)

    ``update`` is one launch on the current stream; it does not synchronise and can be captured in a graph (the buffer is the
    graph's from then on).  ``GraphedTrainStep`` runs its warm-up steps and the capture for real, so a ``step_fn`` that updates
    a ``TrainStats`` has counted those steps by the time the constructor returns: call ``reset()`` after constructing it.

    Per ordered pair the predicted relation is the first maximum of ``sigmoid(sigmoid(logit))`` in fp32, as in the reference
    (the trainer applies the sigmoid twice; saturated logits tie and the lowest index wins)."""

    def __init__(self, device=None):
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError(f"TrainStats: gcgcn_amd runs on MI355X only; got device {dev} (no CPU fallback)")
        # allocated here, never inside a captured step; without a GPU the object exists but every use raises
        self._counters = torch.zeros(8, dtype=torch.int64, device=dev) if torch.cuda.is_available() else None

    def _buf(self) -> Tensor:
        if self._counters is None:
            raise RuntimeError("TrainStats: gcgcn_amd runs on MI355X only; no GPU is available (no CPU fallback)")
        return self._counters

    def reset(self) -> None:
        """Zero the counters, in stream order."""
        self._buf().zero_()

    def _launch(self, lg: Tensor, lb: Tensor, nv: Optional[Tensor]) -> None:
        buf = self._buf()
        if lg.device != buf.device:
            raise ValueError(f"TrainStats: counters on {buf.device}, logits on {lg.device}")
        B, N, _, R = lg.shape
        if B:
            call("gcgcn_pair_stats", B, N, R, _p(lg), _p(lb), _p(nv), _p(buf), _stream())

    def update(self, logits, labels, n_valid=None) -> None:
        """Add the pairs of ``logits`` / ``labels`` (``[B,N,N,R]`` or one ``[N,N,R]`` document; ``n_valid[B]`` for ragged batches)."""
        lg, lb, nv, _ = _pair_inputs(logits, labels, n_valid, "TrainStats.update")
        self._launch(lg.detach(), lb.detach(), nv)

    def get(self) -> TrainStatsResult:
        """One read-back (synchronises with the work queued before it)."""
        return TrainStatsResult(*self._buf().cpu().tolist())


def pair_bce_loss(logits, labels, n_valid=None, stats=None):
    """Per-document loss of the reference trainer (config/Config.py:355-366): sigmoid, BCE averaged over the relation
    axis, summed over ordered entity pairs h != t and divided by n^2 - n.  ``logits``/``labels``: ``[N,N,R]`` (returns
    a scalar, like the trainer's ``temp_loss``) or ``[B,N,N,R]`` (returns ``[B]``; ``n_valid[B]`` for ragged batches).
    The reference accumulates ``total_loss`` over documents and divides by ``batch_size`` (:366-369): that is
    ``pair_bce_loss(...).sum() / batch_size``.  ``stats``: a ``TrainStats`` that counts the same pairs (one more launch on the
    same stream, just before the loss kernel); the loss returned is the same either way."""
    if stats is not None and not isinstance(stats, TrainStats):
        raise TypeError(f"pair_bce_loss: stats must be a TrainStats, got {type(stats).__name__}")
    lg, lb, nv, single = _pair_inputs(logits, labels, n_valid, "pair_bce_loss")
    if stats is not None:
        stats._launch(lg.detach(), lb.detach(), nv)
    out = PairBceFn.apply(lg, lb, nv)
    return out[0] if single else out


# ---- the token encoder's LSTM layer (csrc/lstm.hip) ----------------------------------------------------------------------------
class LstmFn(torch.autograd.Function):
    """(x[B,T,I], w_ih[nd*4H,I], w_hh[nd*4H,H], bias[nd*4H], h0[nd,B,H], c0[nd,B,H]) -> out[B,T,nd*H]: one ``nn.LSTM`` layer over
    all T steps with the directions' parameters stacked and ``bias = b_ih + b_hh`` (``lstm_layer`` stacks and splits them).
    ``lens``: ``None`` or the rows' lengths, int32 ``[B]`` on the device (saved for the backward).  ``recurrent``: 0 = fp32, 1 = bf16
    operands for the recurrent products (``lstm_layer``); kept for the backward, announced before each of the two calls."""

    @staticmethod
    def _call(recurrent: int, name: str, *args):
        """One LSTM entry point with the argument recurrent.  0: the call alone, as always.  1: announced to the library on this
        thread right before the call, which takes the announcement (include/gcgcn.h, the LSTM block)."""
        if recurrent:
            call("gcgcn_set_option", b"lstm_recurrent", recurrent)
        call(name, *args)

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, bias, h0, c0, lens=None, recurrent=0):
        B, T, I = x.shape
        nd, H = h0.shape[0], h0.shape[2]
        need_grad = any(ctx.needs_input_grad)
        out = torch.empty(B, T, nd * H, device=x.device)
        gates = torch.empty(B * T, nd * 4 * H, device=x.device)
        csave = torch.empty(B, T, nd * H, device=x.device) if need_grad else None
        LstmFn._call(recurrent, "gcgcn_lstm_fwd_len", B, T, I, H, nd, _p(x), _p(w_ih), _p(w_hh), _p(bias), _p(h0), _p(c0), _p(out),
                     _p(gates), _p(csave), _p(lens), _stream())     # null lengths: every step of every row
        written = (out, gates) if csave is None else (out, gates, csave)
        torch.autograd.graph.increment_version(written)     # raw-pointer writes, as in optim._written
        ctx.has_lens, ctx.recurrent = lens is not None, recurrent
        if need_grad:
            ctx.save_for_backward(x, w_ih, w_hh, h0, c0, out, gates, csave, *(() if lens is None else (lens,)))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        x, w_ih, w_hh, h0, c0, out, gates, csave = ctx.saved_tensors[:8]
        lens = ctx.saved_tensors[8] if ctx.has_lens else None
        B, T, I = x.shape
        nd, H = h0.shape[0], h0.shape[2]
        dout = dout.contiguous()
        if dout.data_ptr() == out.data_ptr():
            raise RuntimeError("lstm_layer: the output's gradient aliases the output itself")
        dgates = torch.empty_like(gates)
        dx, dw_ih, dw_hh = torch.empty_like(x), torch.empty_like(w_ih), torch.empty_like(w_hh)
        db = torch.empty(nd * 4 * H, device=x.device)
        dh0, dc0 = torch.empty_like(h0), torch.empty_like(c0)
        ws = _f32_buf(_bytes_or_raise("gcgcn_lstm_ws_bytes", B, T, I, H, nd), x.device)
        LstmFn._call(ctx.recurrent, "gcgcn_lstm_bwd_len", B, T, I, H, nd, _p(x), _p(w_ih), _p(w_hh), _p(h0), _p(c0), _p(out), _p(gates),
                     _p(csave), _p(dout), _p(dgates), _p(dx), _p(dw_ih), _p(dw_hh), _p(db), _p(dh0), _p(dc0), _p(ws), ws.numel() * 4,
                     _p(lens), _stream())
        torch.autograd.graph.increment_version((dx, dw_ih, dw_hh, db, dh0, dc0))
        return dx, dw_ih, dw_hh, db, dh0, dc0, None, None


def _lstm_lengths(lengths, B: int, T: int, dev) -> Tensor:
    """The rows' lengths as the kernels take them: int32 ``[B]`` on the device, converted there.  Values outside [1, T] raise --
    ONE host read, skipped inside a hipGraph capture and with ``check_ids = False`` (the kernels clamp into [0, T] regardless)."""
    if not isinstance(lengths, Tensor) or lengths.dtype not in (torch.int32, torch.int64) or tuple(lengths.shape) != (B,) \
            or lengths.device != dev:
        got = f"{lengths.dtype} {tuple(lengths.shape)} on {lengths.device}" if isinstance(lengths, Tensor) else type(lengths).__name__
        raise ValueError(f"lstm_layer: lengths must be an int32 or int64 tensor of shape ({B},) on {dev}, got {got}")
    if check_ids and not torch.cuda.is_current_stream_capturing():
        lo_hi = torch.stack([lengths.min(), lengths.max()]).tolist()
        if lo_hi[0] < 1 or lo_hi[1] > T:
            raise IndexError(f"lstm_layer: lengths must lie in [1, {T}], got min {lo_hi[0]} / max {lo_hi[1]}")
    return lengths.to(torch.int32).contiguous()


LSTM_RECURRENT = {"fp32": 0, "bf16": 1}     # lstm_layer's recurrent -> the library's lstm_recurrent (include/gcgcn.h)


def _bf16_round(t: Tensor) -> Tensor:
    """r(.): one rounding to bf16, nearest even, kept in ``t``'s own dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


class Bf16RecurrentFn(torch.autograd.Function):
    """The recurrent product of ``recurrent="bf16"``, as plain PyTorch on any device in float32 / float64 -- the contract of the HIP
    kernels ("bf16 recurrence").  ``(a[B,K], w[N,K]) -> r(a) r(w)^T`` with r = one rounding to bf16, sums in ``a``'s
    dtype.  Backward: ``da = r(dy) r(w)`` -- the cotangent is rounded like any other operand -- and ``dw = dy^T a`` on the UNROUNDED
    values: the weight gradient treats the rounding as the identity.  ``rounding=False`` switches every r off (then this is
    ``a @ w.T`` and its ordinary gradients)."""

    @staticmethod
    def forward(ctx, a, w, rounding=True):
        ctx.save_for_backward(a, w)
        ctx.rounding = rounding
        r = _bf16_round if rounding else (lambda t: t)
        return r(a) @ r(w).t()

    @staticmethod
    def backward(ctx, dy):
        a, w = ctx.saved_tensors
        r = _bf16_round if ctx.rounding else (lambda t: t)
        return r(dy) @ r(w), dy.t() @ a, None


def lstm_layer_bf16_definition(x, w_ih, w_hh, b_ih, b_hh, h0, c0, w_ih_r=None, w_hh_r=None, b_ih_r=None, b_hh_r=None, lengths=None,
                               rounding=True):
    """What ``lstm_layer(..., recurrent="bf16")`` computes, written as a Python time loop (any device, float32 / float64; slow):

        gates_t = (x_t W_ih^T + b_ih + b_hh) + Bf16RecurrentFn(h_{t-1}, W_hh)

    the input projection, the sum and the cell update in the tensors' dtype, unrounded; ``h0`` is rounded like any other ``h`` when
    it becomes an operand.  Gradients are autograd's through ``Bf16RecurrentFn``.  ``lengths`` (int tensor ``[B]``) as in
    ``lstm_layer``: an inactive step is the identity on ``h`` and ``c``, the output is 0 there, and everything of an inactive step
    goes through a select (``torch.where``), so NaN in the cotangent at a padded position reaches nothing."""
    B, T, _ = x.shape
    H = w_hh.shape[1]
    outs = []
    for d, (wi, wh, bi, bh) in enumerate(((w_ih, w_hh, b_ih, b_hh),) if w_ih_r is None else ((w_ih, w_hh, b_ih, b_hh), (w_ih_r, w_hh_r, b_ih_r, b_hh_r))):
        xp = x @ wi.t() + (bi + bh)
        h, c = h0[d].expand(B, H), c0[d].expand(B, H)
        steps = [None] * T
        for t in (range(T - 1, -1, -1) if d else range(T)):
            gi, gf, gg, go = (xp[:, t] + Bf16RecurrentFn.apply(h, wh, rounding)).chunk(4, 1)
            gi, gf, gg, go = torch.sigmoid(gi), torch.sigmoid(gf), torch.tanh(gg), torch.sigmoid(go)
            cn = gf * c + gi * gg
            hn = go * torch.tanh(cn)
            if lengths is None:
                c, h, steps[t] = cn, hn, hn
            else:
                act = (lengths > t)[:, None]
                c, h, steps[t] = torch.where(act, cn, c), torch.where(act, hn, h), torch.where(act, hn, torch.zeros_like(hn))
        outs.append(torch.stack(steps, 1))
    return torch.cat(outs, 2)


def lstm_layer(x, w_ih, w_hh, b_ih, b_hh, h0, c0, w_ih_r=None, w_hh_r=None, b_ih_r=None, b_hh_r=None, lengths=None, recurrent="fp32"):
    """One ``nn.LSTM(input_size, H, 1, batch_first=True)`` layer in HIP: ``x[B,T,I]``, ``h0``/``c0`` ``[nd,B,H]`` (a ``[nd,1,H]``
    state is broadcast over the batch) -> the output ``[B,T,nd*H]``.  Gate order i, f, g, o and all T padded steps, as torch runs
    it.  The four ``*_r`` parameters of the reverse direction make it bidirectional (all four or none).  ``H = 128`` is served;
    another width raises.  Gradients reach ``x``, every weight and bias, ``h0`` and ``c0``.

    ``lengths``: ``None``, or an int32 / int64 tensor ``[B]`` on ``x``'s device, every value in ``[1, T]`` (checked with one host
    read outside a capture).  The layer then computes what ``pack_padded_sequence`` -> ``nn.LSTM`` ->
    ``pad_packed_sequence(total_length=T)`` computes: row ``b`` runs its own ``lengths[b]`` steps (the reverse direction from
    ``t = lengths[b] - 1``), the output is exactly 0 at ``t >= lengths[b]``, and so is the gradient to ``x`` there, whatever the
    output's gradient holds at those positions.  ``x`` itself must be finite there.

    ``recurrent``: ``"fp32"`` (the default: the kernels and the bits of a call without the keyword) or ``"bf16"``: the two
    recurrent products -- ``h W_hh^T`` forward, ``dgates W_hh`` backward -- take bf16 operands with fp32 accumulation
    (``lstm_layer_bf16_definition`` / ``Bf16RecurrentFn`` is the definition).  The input projection, the cell update, the output,
    the three gradient products and every parameter and gradient stay fp32."""
    if recurrent not in LSTM_RECURRENT:
        raise ValueError(f"lstm_layer: recurrent={recurrent!r} (\"fp32\" or \"bf16\")")
    rev = (w_ih_r, w_hh_r, b_ih_r, b_hh_r)
    if any(t is None for t in rev) and not all(t is None for t in rev):
        raise ValueError("lstm_layer: the reverse direction needs all of w_ih_r, w_hh_r, b_ih_r, b_hh_r")
    nd = 1 if w_ih_r is None else 2
    x = _chk(x, "x", 3)
    for name, t in (("w_ih", w_ih), ("w_hh", w_hh), ("b_ih", b_ih), ("b_hh", b_hh), ("h0", h0), ("c0", c0)) + \
            ((("w_ih_r", w_ih_r), ("w_hh_r", w_hh_r), ("b_ih_r", b_ih_r), ("b_hh_r", b_hh_r)) if nd == 2 else ()):
        _chk(t, name)
    B, T, I = x.shape
    H = w_hh.shape[1]
    if tuple(w_ih.shape) != (4 * H, I) or tuple(w_hh.shape) != (4 * H, H) or tuple(b_ih.shape) != (4 * H,) or tuple(b_hh.shape) != (4 * H,):
        raise ValueError(f"lstm_layer: parameter shapes {tuple(w_ih.shape)}, {tuple(w_hh.shape)}, {tuple(b_ih.shape)}, {tuple(b_hh.shape)} "
                         f"do not describe an LSTM of input {I}, width {H}")
    if nd == 2 and (w_ih_r.shape != w_ih.shape or w_hh_r.shape != w_hh.shape or b_ih_r.shape != b_ih.shape or b_hh_r.shape != b_hh.shape):
        raise ValueError("lstm_layer: the reverse direction's parameters differ in shape from the forward direction's")
    if h0.dim() != 3 or c0.shape != h0.shape or h0.shape[0] != nd or h0.shape[2] != H or h0.shape[1] not in (1, B):
        raise ValueError(f"lstm_layer: h0 {tuple(h0.shape)} / c0 {tuple(c0.shape)}, expected [{nd}, {B} or 1, {H}]")
    # the directions' parameters stacked, the two biases added: a few small copies (autograd splits the gradients again)
    if nd == 2:
        W_ih, W_hh = torch.cat([w_ih, w_ih_r], 0), torch.cat([w_hh, w_hh_r], 0)
        bias = torch.cat([b_ih + b_hh, b_ih_r + b_hh_r], 0)
    else:
        W_ih, W_hh, bias = w_ih.contiguous(), w_hh.contiguous(), b_ih + b_hh
    lens = None if lengths is None else _lstm_lengths(lengths, B, T, x.device)
    if recurrent != "fp32":
        return LstmFn.apply(x, W_ih, W_hh, bias, h0.expand(nd, B, H).contiguous(), c0.expand(nd, B, H).contiguous(), lens,
                            LSTM_RECURRENT[recurrent])
    if lens is None:
        return LstmFn.apply(x, W_ih, W_hh, bias, h0.expand(nd, B, H).contiguous(), c0.expand(nd, B, H).contiguous())
    return LstmFn.apply(x, W_ih, W_hh, bias, h0.expand(nd, B, H).contiguous(), c0.expand(nd, B, H).contiguous(), lens)


# ---- the token front end either side of the BiLSTM (csrc/frontend.hip) -----------------------------------------------------------
class TokenEmbedFn(torch.autograd.Function):
    """(word_w[V,Dw], coref_w[P,Dc], ner_w[R,Dn], document, document_pos, document_ner int64 [B,T], scale[B,I] or None) ->
    x[B,T,I]: the three gathers side by side, times the locked-dropout factor."""

    @staticmethod
    def forward(ctx, word_w, coref_w, ner_w, document, document_pos, document_ner, scale, coref_pad, ner_pad):
        B, T = document.shape
        dims = (B, T, word_w.shape[0], coref_w.shape[0], ner_w.shape[0], word_w.shape[1], coref_w.shape[1], ner_w.shape[1])
        x = torch.empty(B, T, dims[5] + dims[6] + dims[7], device=word_w.device)
        call("gcgcn_embed_fwd", *dims, _p(document), _p(document_pos), _p(document_ner), _p(word_w), _p(coref_w), _p(ner_w), _p(scale), _p(x),
             _stream())
        torch.autograd.graph.increment_version((x,))
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(document, document_pos, document_ner, scale)
            ctx.dims, ctx.pads = dims, (coref_pad, ner_pad)
        return x

    @staticmethod
    @once_differentiable
    def backward(ctx, dx):
        document, document_pos, document_ner, scale = ctx.saved_tensors
        B, T, V, P, R, Dw, Dc, Dn = ctx.dims
        dx = dx.contiguous()
        dev = dx.device
        dword, dcoref, dner = torch.empty(V, Dw, device=dev), torch.empty(P, Dc, device=dev), torch.empty(R, Dn, device=dev)
        ws = _f32_buf(_bytes_or_raise("gcgcn_frontend_ws_bytes", *ctx.dims, 0), dev)                      # K = 0: the embeddings alone
        call("gcgcn_embed_bwd", *ctx.dims, _p(document), _p(document_pos), _p(document_ner), _p(dx), _p(scale), ctx.pads[0], ctx.pads[1],
             _p(dword), _p(dcoref), _p(dner), _p(ws), ws.numel() * 4, _stream())
        torch.autograd.graph.increment_version((dword, dcoref, dner))
        return dword, dcoref, dner, None, None, None, None, None, None


def token_embed(document, document_pos, document_ner, word_w, coref_w, ner_w, scale=None, coref_padding_idx=0, ner_padding_idx=0):
    """``x[B,T,Dw+Dc+Dn] = word_w[document] | coref_w[document_pos] | ner_w[document_ner]`` (glove:282-289) in HIP, every element
    times ``scale[b, i]`` when ``scale`` (``[B,I]`` or ``[B,1,I]``: the ``LockedDropout`` factor) is given.  Ids are int64
    ``[B,T]``.  The gradients of the three tables come back dense and bit-reproducible; the row at a padding index (``None``:
    the table has none; ``word_w`` never has one) stays exactly zero.  ``scale`` gets no gradient."""
    tabs = [_chk(w, nm, 2) for nm, w in (("word_w", word_w), ("coref_w", coref_w), ("ner_w", ner_w))]
    ids = []
    for nm, t in (("document", document), ("document_pos", document_pos), ("document_ner", document_ner)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int64 or t.dim() != 2 or t.shape != document.shape:
            raise ValueError(f"{nm}: expected a GPU int64 tensor of shape [B,T]")
        ids.append(t.contiguous())
    B, T = ids[0].shape
    I = sum(w.shape[1] for w in tabs)
    if scale is not None:
        scale = _chk(scale, "scale")
        if tuple(scale.shape) not in ((B, I), (B, 1, I)):
            raise ValueError(f"scale: expected [{B},{I}] or [{B},1,{I}], got {tuple(scale.shape)}")
        scale = scale.detach().reshape(B, I)
    _check_id_range([(nm, t, 0, w.shape[0] - 1) for nm, t, w in zip(("document", "document_pos", "document_ner"), ids, tabs)])
    pads = [-1 if p is None else int(p) for p in (coref_padding_idx, ner_padding_idx)]
    return TokenEmbedFn.apply(*tabs, *ids, scale, *pads)


class TokenContextFn(torch.autograd.Function):
    """(h[B,T,K], weight[128,K], bias[128], node_pos[B,N,T]) -> (ctx[B,T,128], node_feat[B,N,128])."""

    @staticmethod
    def forward(ctx, h, weight, bias, node_pos):
        B, T, K = h.shape
        N, Hd = node_pos.shape[1], weight.shape[0]
        pre, out = torch.empty(B, T, Hd, device=h.device), torch.empty(B, T, Hd, device=h.device)
        node_feat = torch.empty(B, N, Hd, device=h.device)
        call("gcgcn_context_fwd", B, T, N, K, Hd, _p(h), _p(weight), _p(bias), _p(node_pos), _p(pre), _p(out), _p(node_feat), _stream())
        torch.autograd.graph.increment_version((out, node_feat))
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(h, weight, node_pos, out)
        return out, node_feat

    @staticmethod
    @once_differentiable
    def backward(ctx, dctx, dnode):
        h, weight, node_pos, out = ctx.saved_tensors
        B, T, K = h.shape
        N, Hd = node_pos.shape[1], weight.shape[0]
        dctx, dnode = dctx.contiguous(), dnode.contiguous()
        dpre, dh, dw = torch.empty_like(out), torch.empty_like(h), torch.empty_like(weight)
        db = torch.empty(Hd, device=h.device)
        ws = _f32_buf(_bytes_or_raise("gcgcn_frontend_ws_bytes", B, T, 0, 0, 0, 0, 0, 0, K), h.device)    # no tables: the context alone
        call("gcgcn_context_bwd", B, T, N, K, Hd, _p(h), _p(weight), _p(node_pos), _p(out), _p(dctx), _p(dnode), _p(dpre), _p(dh), _p(dw),
             _p(db), _p(ws), ws.numel() * 4, _stream())
        torch.autograd.graph.increment_version((dh, dw, db))
        return dh, dw, db, None


def token_context(h, weight, bias, node_pos):
    """``ctx[B,T,128] = tanh(h weight^T + bias)`` (``linear_re`` + tanh, glove:290-292) and the entity pooling
    ``node_feat[B,N,128] = bmm(node_pos, ctx)`` (glove:293-298) in HIP.  ``h[B,T,K]``, ``weight[128,K]``, ``bias[128]``,
    ``node_pos[B,N,T]`` (mention spans: the pooling visits its non-zeros only).  Gradients reach ``h``, ``weight`` and ``bias``;
    ``node_pos`` gets none.  A width other than 128 raises."""
    h, weight, bias, node_pos = _chk(h, "h", 3), _chk(weight, "weight", 2), _chk(bias, "bias", 1), _chk(node_pos.detach(), "node_pos", 3)
    B, T, K = h.shape
    if weight.shape[1] != K or bias.shape[0] != weight.shape[0]:
        raise ValueError(f"token_context: weight {tuple(weight.shape)} / bias {tuple(bias.shape)} do not project h {tuple(h.shape)}")
    if node_pos.shape[0] != B or node_pos.shape[2] != T:
        raise ValueError(f"token_context: node_pos {tuple(node_pos.shape)}, expected [{B}, N, {T}]")
    return TokenContextFn.apply(h, weight, bias, node_pos)


# ---- the BERT graph model's glue either side of the tail (csrc/bert_frontend.hip, include/gcgcn_bert_frontend.h) -----------------
class BertTokenContextFn(torch.autograd.Function):
    """(states[B,T,Dw], coref_w[P,Dc], ner_w[R,Dn], weight[128,Dw+Dc+Dn], bias[128], document_pos, document_ner int64 [B,T],
    node_pos[B,N,T]) -> (ctx[B,T,128], node_feat[B,N,128]) (gcbf_context_fwd / gcbf_context_bwd)."""

    @staticmethod
    def forward(ctx, states, coref_w, ner_w, weight, bias, document_pos, document_ner, node_pos, coref_pad, ner_pad):
        B, T, Dw = states.shape
        dims = (B, T, node_pos.shape[1], Dw, coref_w.shape[1], ner_w.shape[1], coref_w.shape[0], ner_w.shape[0])
        dev, Hd = states.device, weight.shape[0]
        fold = torch.empty(dims[6] + dims[7], Hd, device=dev)
        pre, out = torch.empty(B, T, Hd, device=dev), torch.empty(B, T, Hd, device=dev)
        node_feat = torch.empty(B, dims[2], Hd, device=dev)
        call("gcbf_context_fwd", *dims, _p(states), _p(document_pos), _p(document_ner), _p(coref_w), _p(ner_w), _p(weight), _p(bias),
             _p(node_pos), _p(fold), _p(pre), _p(out), _p(node_feat), _stream())
        torch.autograd.graph.increment_version((out, node_feat))
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(states, coref_w, ner_w, weight, document_pos, document_ner, node_pos, out)
            ctx.dims, ctx.pads = dims, (coref_pad, ner_pad)
        return out, node_feat

    @staticmethod
    @once_differentiable
    def backward(ctx, dctx, dnode):
        states, coref_w, ner_w, weight, document_pos, document_ner, node_pos, out = ctx.saved_tensors
        dctx, dnode = dctx.contiguous(), dnode.contiguous()
        dev = states.device
        dstates, dcoref, dner, dw = torch.empty_like(states), torch.empty_like(coref_w), torch.empty_like(ner_w), torch.empty_like(weight)
        db = torch.empty(weight.shape[0], device=dev)
        ws = _f32_buf(_bytes_or_raise("gcbf_context_ws_bytes", *ctx.dims), dev)
        call("gcbf_context_bwd", *ctx.dims, _p(states), _p(document_pos), _p(document_ner), _p(coref_w), _p(ner_w), _p(weight), _p(node_pos),
             _p(out), _p(dctx), _p(dnode), ctx.pads[0], ctx.pads[1], _p(dstates), _p(dw), _p(db), _p(dcoref), _p(dner), _p(ws),
             ws.numel() * 4, _stream())
        torch.autograd.graph.increment_version((dstates, dcoref, dner, dw, db))
        return dstates, dcoref, dner, dw, db, None, None, None, None, None


def bert_token_context(states, document_pos, document_ner, coref_w, ner_w, weight, bias, node_pos, coref_padding_idx=0, ner_padding_idx=0):
    """The context pair of ``GraphCNN_multihead_bert_gate_cls`` (bert:278-283 and the pooling) without its concatenated tensor::

        ctx[B,T,128] = tanh(F.linear(cat([states, coref_w[document_pos], ner_w[document_ner]], -1), weight, bias))
        node_feat[B,N,128] = bmm(node_pos, ctx)

    computed with ``weight = W1 | W2 | W3`` split by columns as ``states W1^T + bias + F2[document_pos] + F3[document_ner]``,
    ``F2 = coref_w W2^T``, ``F3 = ner_w W3^T``: the large product runs at ``K = Dw`` with ``W1`` read in place, and no
    ``[B,T,Dw+Dc+Dn]`` tensor exists in either direction.  ``states[B,T,Dw]``, ids int64 ``[B,T]``, ``coref_w[P,Dc]``,
    ``ner_w[R,Dn]``, ``weight[128,Dw+Dc+Dn]``, ``bias[128]``, ``node_pos[B,N,T]``.

    The five gradients (``states``, ``coref_w``, ``ner_w``, ``weight``, ``bias``) come back dense, fully written and bit-reproducible;
    the row at a padding index (``None``: the table has none) of ``coref_w`` / ``ner_w`` is exactly zero, while ``weight``'s gradient
    counts the padding tokens as torch's does.  Nothing is read on the host (the id range check apart, skipped under capture):
    capturable.  ``node_pos`` gets no gradient.  A width other than 128 raises."""
    states, weight, bias = _chk(states, "states", 3), _chk(weight, "weight", 2), _chk(bias, "bias", 1)
    coref_w, ner_w, node_pos = _chk(coref_w, "coref_w", 2), _chk(ner_w, "ner_w", 2), _chk(node_pos.detach(), "node_pos", 3)
    B, T, Dw = states.shape
    ids = []
    for nm, t in (("document_pos", document_pos), ("document_ner", document_ner)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int64 or tuple(t.shape) != (B, T):
            raise ValueError(f"{nm}: expected a GPU int64 tensor of shape [{B},{T}]")
        ids.append(t.contiguous())
    K = Dw + coref_w.shape[1] + ner_w.shape[1]
    if weight.shape[0] != 128 or weight.shape[1] != K or bias.shape[0] != weight.shape[0]:
        raise ValueError(f"bert_token_context: weight {tuple(weight.shape)} / bias {tuple(bias.shape)} do not project "
                         f"{Dw} + {coref_w.shape[1]} + {ner_w.shape[1]} features onto 128")
    if node_pos.shape[0] != B or node_pos.shape[2] != T:
        raise ValueError(f"bert_token_context: node_pos {tuple(node_pos.shape)}, expected [{B}, N, {T}]")
    _check_id_range([("document_pos", ids[0], 0, coref_w.shape[0] - 1), ("document_ner", ids[1], 0, ner_w.shape[0] - 1)])
    pads = [-1 if p is None else int(p) for p in (coref_padding_idx, ner_padding_idx)]
    return BertTokenContextFn.apply(states, coref_w, ner_w, weight, bias, *ids, node_pos, *pads)


class PairLogitBiasFn(torch.autograd.Function):
    """(logits[B,N,N,R], cls[B,R], n_valid int32 [B] or None) -> out[B,N,N,R] (gcbf_logit_bias_fwd / gcbf_logit_bias_bwd)."""

    @staticmethod
    def forward(ctx, logits, cls, n_valid):
        B, N, _, R = logits.shape
        out = torch.empty_like(logits)
        call("gcbf_logit_bias_fwd", B, N, R, _p(logits), _p(cls), _p(n_valid), _p(out), _stream())
        torch.autograd.graph.increment_version((out,))
        ctx.n_valid = n_valid
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        dcls = None
        if ctx.needs_input_grad[1]:
            dout = dout.contiguous()
            B, N, _, R = dout.shape
            dcls = torch.empty(B, R, device=dout.device)
            ws = _f32_buf(_bytes_or_raise("gcbf_logit_bias_ws_bytes", B, N, R), dout.device)
            call("gcbf_logit_bias_bwd", B, N, R, _p(dout), _p(ctx.n_valid), _p(dcls), _p(ws), ws.numel() * 4, _stream())
            torch.autograd.graph.increment_version((dcls,))
        return dout, dcls, None                                  # the gradient of logits is the incoming one: no copy, no launch


def pair_logit_bias(logits, cls_logits, n_valid=None):
    """``out[b,i,j,:] = logits[b,i,j,:] + cls_logits[b,:]`` where ``i, j < n_valid[b]`` (everywhere without ``n_valid``), ``logits``
    unchanged elsewhere: ``linear_cls`` of the [CLS] state added to every pair's logits (bert:345-346), in one launch instead of a
    mask, a multiply and an add over ``[B,N,N,R]``.  Backward: the gradient of ``logits`` is the incoming gradient itself, and
    ``dcls[b,:]`` is its sum over the live pairs in a fixed two-stage order (bit-reproducible, no atomics).  Capturable."""
    logits, cls_logits = _chk(logits, "logits", 4), _chk(cls_logits, "cls_logits", 2)
    B, N, N2, R = logits.shape
    if N2 != N or tuple(cls_logits.shape) != (B, R):
        raise ValueError(f"pair_logit_bias: logits {tuple(logits.shape)} / cls_logits {tuple(cls_logits.shape)}, expected [B,N,N,R] and [B,R]")
    if B < 1 or N < 1 or R < 1:
        raise ValueError(f"pair_logit_bias: empty logits {tuple(logits.shape)}")
    return PairLogitBiasFn.apply(logits, cls_logits, _nv(n_valid, B, N, logits.device))


# ---- the BERT encoder layer (csrc/bert.hip) --------------------------------------------------------------------------------------
class ResLayerNormFn(torch.autograd.Function):
    """y = LayerNorm(dropout(x + bias) + res) over the last axis (eps = 1e-12, biased variance); bias, res, dropout optional."""

    @staticmethod
    def forward(ctx, x, bias, res, weight, lnb, p, snap, salt, t_valid=None):
        D = x.shape[-1]
        rows = x.numel() // D
        y = torch.empty_like(x)
        mean, rstd = torch.empty(rows, device=x.device), torch.empty(rows, device=x.device)
        # the _len symbols take the lengths in the middle of the plain ones' list, and refuse a null t_valid
        name, lens = ("gcgcn_res_ln_fwd", ()) if t_valid is None else ("gcgcn_res_ln_fwd_len", (_p(t_valid), x.shape[-2]))
        call(name, rows, D, _p(x), _p(bias), _p(res), _p(weight), _p(lnb), *lens, _p(y), _p(mean), _p(rstd), _p(snap), salt, float(p), _stream())
        torch.autograd.graph.increment_version((y, mean, rstd))
        ctx.p, ctx.snap, ctx.salt, ctx.has, ctx.t_valid = float(p), snap, salt, (bias is not None, res is not None), t_valid
        ctx.save_for_backward(x, weight, mean, rstd, *(t for t in (bias, res) if t is not None))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight, mean, rstd = ctx.saved_tensors[:4]
        rest = list(ctx.saved_tensors[4:])
        bias = rest.pop(0) if ctx.has[0] else None
        res = rest.pop(0) if ctx.has[1] else None
        D = x.shape[-1]
        rows = x.numel() // D
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        dres = torch.empty_like(x) if res is not None else None
        dw, db = torch.empty_like(weight), torch.empty_like(weight)
        ws = _f32_buf(_bytes_or_raise("gcgcn_res_ln_ws_bytes", D), x.device)
        name, lens = ("gcgcn_res_ln_bwd", ()) if ctx.t_valid is None else ("gcgcn_res_ln_bwd_len", (_p(ctx.t_valid), x.shape[-2]))
        call(name, rows, D, _p(dy), _p(x), _p(bias), _p(res), _p(weight), _p(mean), _p(rstd), *lens, _p(dx), _p(dres), _p(dw), _p(db),
             _p(ws), ws.numel() * 4, _p(ctx.snap), ctx.salt, ctx.p, _stream())
        torch.autograd.graph.increment_version((dx, dw, db) + (() if dres is None else (dres,)))
        dbias = dx.reshape(rows, D).sum(0) if bias is not None and ctx.needs_input_grad[1] else None
        return dx, dbias, dres, dw, db, None, None, None, None


def res_layer_norm(x, weight, bias, lin_bias=None, res=None, p=0.0, training=False, snap=None, salt=_lib.SALT_BERT_EMB, t_valid=None):
    """``LayerNorm(dropout(x + lin_bias) + res)`` over the last axis in HIP, with the contract's LayerNorm: biased variance,
    ``weight * (v - mean) / sqrt(var + 1e-12) + bias``.  ``lin_bias`` ``[D]``, ``res`` (``x``'s shape) and the dropout are each
    optional.  ``D`` a multiple of 64, at most 1024.  ``snap``: the rng snapshot of the dropout site (default: a fresh one).

    ``t_valid``: token counts ``[B]`` for ``x[B,T,D]`` (row ``(b, t)`` is live iff ``t < t_valid[b]``).  Padding rows of the output and
    of the gradients of ``x`` and ``res`` are exactly zero, neither ``x``, ``res`` nor the arriving gradient is read there, and
    the parameter gradients sum over the live rows.  ``None``: every row, the call as it was."""
    x = _chk(x, "x")
    if t_valid is not None:
        if x.dim() != 3:
            raise ValueError(f"res_layer_norm: t_valid needs x[B,T,D], got shape {tuple(x.shape)}")
        t_valid = _nv(t_valid, x.shape[0], x.shape[1], x.device)
    weight, bias = _chk(weight, "weight", 1), _chk(bias, "bias", 1)
    D = x.shape[-1]
    if weight.shape != (D,) or bias.shape != (D,):
        raise ValueError(f"res_layer_norm: weight {tuple(weight.shape)} / bias {tuple(bias.shape)} for rows of {D}")
    if lin_bias is not None and _chk(lin_bias, "lin_bias", 1).shape != (D,):
        raise ValueError(f"res_layer_norm: lin_bias {tuple(lin_bias.shape)} for rows of {D}")
    if res is not None:
        res = _chk(res, "res")
        if res.shape != x.shape:
            raise ValueError(f"res_layer_norm: res {tuple(res.shape)} against x {tuple(x.shape)}")
    p = float(p) if training else 0.0
    if p > 0 and snap is None:
        snap = rng_snapshot(x.device)
    return ResLayerNormFn.apply(x, None if lin_bias is None else lin_bias.contiguous(), res, weight, bias, p, snap if p > 0 else None, salt,
                                t_valid)


class BertEmbeddingsFn(torch.autograd.Function):
    """(word_w[V,D], pos_w[Pmax,D], type_w[Ty,D], ln_w[D], ln_b[D], input_ids, token_type_ids int64 [B,T]) -> y[B,T,D]
    (include/gcgcn_bert_embed.h: gcbe_fwd / gcbe_bwd)."""

    @staticmethod
    def forward(ctx, word_w, pos_w, type_w, ln_w, ln_b, input_ids, token_type_ids, p, snap, t_valid):
        B, T = input_ids.shape
        dims = (B, T, word_w.shape[1], word_w.shape[0], pos_w.shape[0], type_w.shape[0])
        dev = word_w.device
        y = torch.empty(B, T, dims[2], device=dev)
        mean, rstd = torch.empty(B * T, device=dev), torch.empty(B * T, device=dev)
        call("gcbe_fwd", *dims, _p(input_ids), _p(token_type_ids), _p(word_w), _p(pos_w), _p(type_w), _p(ln_w), _p(ln_b), _p(t_valid), _p(y),
             _p(mean), _p(rstd), _p(snap), float(p), _stream())
        torch.autograd.graph.increment_version((y, mean, rstd))
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(word_w, pos_w, type_w, ln_w, input_ids, token_type_ids, mean, rstd)
            ctx.dims, ctx.p, ctx.snap, ctx.t_valid = dims, float(p), snap, t_valid
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        word_w, pos_w, type_w, ln_w, input_ids, token_type_ids, mean, rstd = ctx.saved_tensors
        dy = dy.contiguous()
        dev = dy.device
        dword, dpos, dtype = torch.empty_like(word_w), torch.empty_like(pos_w), torch.empty_like(type_w)
        dw, db = torch.empty_like(ln_w), torch.empty_like(ln_w)
        ws = _f32_buf(_bytes_or_raise("gcbe_ws_bytes", *ctx.dims), dev)
        call("gcbe_bwd", *ctx.dims, _p(input_ids), _p(token_type_ids), _p(word_w), _p(pos_w), _p(type_w), _p(ln_w), _p(ctx.t_valid), _p(mean),
             _p(rstd), _p(dy), _p(dword), _p(dpos), _p(dtype), _p(dw), _p(db), _p(ws), ws.numel() * 4, _p(ctx.snap), ctx.p, _stream())
        torch.autograd.graph.increment_version((dword, dpos, dtype, dw, db))
        return dword, dpos, dtype, dw, db, None, None, None, None, None


def bert_embeddings(input_ids, token_type_ids, word_w, pos_w, type_w, ln_w, ln_b, p=0.0, training=False, snap=None, t_valid=None):
    """The stage in front of the BERT encoder layers as ONE launch (csrc/bert_embed.hip)::

        emb[b,t] = (word_w[input_ids[b,t]] + pos_w[t]) + type_w[token_type_ids[b,t]]      y = dropout(LayerNorm(emb))

    with the contract's LayerNorm (biased variance, eps = 1e-12 inside the root; ``res_layer_norm``'s row arithmetic, bit for bit)
    and, in training with ``p > 0``, the mask ``DropoutFn`` draws from ``snap`` (default: a fresh snapshot) with ``SALT_BERT_EMB``.
    Ids are int64 ``[B,T]`` (``token_type_ids`` None: zeros); ``word_w[V,D]``, ``pos_w[Pmax,D]`` with ``T <= Pmax``, ``type_w[Ty,D]``,
    ``ln_w`` / ``ln_b`` ``[D]``; ``D`` a multiple of 64, at most 1024.  ``emb`` is never stored.

    ``t_valid``: token counts ``[B]`` (row ``(b, t)`` is live iff ``t < t_valid[b]``).  Padding rows of ``y`` are exactly zero, the
    ids there are not read, a gradient arriving there is not read (NaN included) and nothing of them reaches any gradient.

    The five gradients (three tables, LayerNorm weight and bias) come back dense, every row written, each element summed by one
    owner in a fixed order: two backward passes are bitwise equal.  Nothing is read on the host (the id range check apart, which is
    skipped under capture, as ``token_embed``'s is): capturable, and a captured stage follows new ids and lengths."""
    tabs = [_chk(w, nm, 2) for nm, w in (("word_w", word_w), ("pos_w", pos_w), ("type_w", type_w))]
    ln_w, ln_b = _chk(ln_w, "ln_w", 1), _chk(ln_b, "ln_b", 1)
    if not isinstance(input_ids, torch.Tensor) or not input_ids.is_cuda or input_ids.dtype != torch.int64 or input_ids.dim() != 2:
        raise ValueError("input_ids: expected a GPU int64 tensor of shape [B,T]")
    if token_type_ids is None:
        token_type_ids = torch.zeros_like(input_ids)
    if (not isinstance(token_type_ids, torch.Tensor) or not token_type_ids.is_cuda or token_type_ids.dtype != torch.int64
            or token_type_ids.shape != input_ids.shape):
        raise ValueError("token_type_ids: expected a GPU int64 tensor of input_ids' shape")
    input_ids, token_type_ids = input_ids.contiguous(), token_type_ids.contiguous()
    B, T = input_ids.shape
    D = tabs[0].shape[1]
    if D % 64 != 0 or D < 64 or D > 1024:
        raise ValueError(f"bert_embeddings: D = {D} (a multiple of 64, at most 1024)")
    if any(w.shape[1] != D for w in tabs) or ln_w.shape != (D,) or ln_b.shape != (D,):
        raise ValueError(f"bert_embeddings: tables {[tuple(w.shape) for w in tabs]} / LayerNorm {tuple(ln_w.shape)}, {tuple(ln_b.shape)} "
                         f"do not share the width {D}")
    if T > tabs[1].shape[0]:
        raise ValueError(f"bert_embeddings: {T} tokens exceed the position table's {tabs[1].shape[0]} rows")
    if B < 1 or T < 1:
        raise ValueError(f"bert_embeddings: empty batch {tuple(input_ids.shape)}")
    _check_id_range([("input_ids", input_ids, 0, tabs[0].shape[0] - 1), ("token_type_ids", token_type_ids, 0, tabs[2].shape[0] - 1)])
    t_valid = _nv(t_valid, B, T, input_ids.device)
    p = float(p) if training else 0.0
    if not 0.0 <= p < 1.0:
        raise ValueError(f"bert_embeddings: p = {p} out of [0, 1)")
    if p > 0 and snap is None:
        snap = rng_snapshot(input_ids.device)
    return BertEmbeddingsFn.apply(*tabs, ln_w, ln_b, input_ids, token_type_ids, p, snap if p > 0 else None, t_valid)


BERT_LAYER_TENSORS = ("query.weight", "query.bias", "key.weight", "key.bias", "value.weight", "value.bias", "attention.output.dense.weight",
                      "attention.output.dense.bias", "attention.output.LayerNorm.weight", "attention.output.LayerNorm.bias",
                      "intermediate.dense.weight", "intermediate.dense.bias", "output.dense.weight", "output.dense.bias",
                      "output.LayerNorm.weight", "output.LayerNorm.bias")


def _ptr_array(tensors):
    return (ctypes.c_void_p * len(tensors))(*(t.data_ptr() for t in tensors))


class BertLayerFn(torch.autograd.Function):
    """(x[B,T,D], key_bias[B,T] | None, t_valid[B] | None, rowblk | None, matmul, attn, the 12 tensors of gcgcn_bert_layer_fwd's
    parameter list) -> y[B,T,D].  Every route is one call of the _mx entry points (include/gcgcn.h): null t_valid / rowblk = no lengths /
    dense products, matmul = 0 / 1 = fp32 / bf16 operands of the Linears, attn = 0 / 1 = the same for the attention core."""

    @staticmethod
    def forward(ctx, x, key_bias, H, p_attn, p_hidden, snap, t_valid, rowblk, matmul, attn, *params):
        B, T, D = x.shape
        Dff = params[6].shape[0]
        dims = (B, T, D, H, Dff)
        saved = _f32_buf(_bytes_or_raise("gcgcn_bert_layer_ws_bytes", *dims, 0), x.device)
        y = torch.empty_like(x)
        ctx.matmul, ctx.attn = matmul, attn
        call("gcgcn_bert_layer_fwd_mx", *dims, _p(x), _p(key_bias), _p(t_valid), _p(rowblk), _ptr_array(params), _p(y), _p(saved),
             saved.numel() * 4, _p(snap), float(p_attn), float(p_hidden), _stream(), matmul, attn)
        torch.autograd.graph.increment_version((y, saved))
        ctx.dims, ctx.ps, ctx.snap, ctx.has_kb = dims, (float(p_attn), float(p_hidden)), snap, key_bias is not None
        ctx.t_valid, ctx.rowblk = t_valid, rowblk
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(x, saved, *params, *(() if key_bias is None else (key_bias,)))
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, saved = ctx.saved_tensors[:2]
        params = ctx.saved_tensors[2:14]
        key_bias = ctx.saved_tensors[14] if ctx.has_kb else None
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        grads = tuple(torch.empty_like(t) for t in params)
        ws = _f32_buf(_bytes_or_raise("gcgcn_bert_layer_ws_bytes", *ctx.dims, 1), x.device)
        call("gcgcn_bert_layer_bwd_mx", *ctx.dims, _p(x), _p(key_bias), _p(ctx.t_valid), _p(ctx.rowblk), _ptr_array(params), _p(saved),
             saved.numel() * 4, _p(dy), _p(dx), _ptr_array(grads), _p(ws), ws.numel() * 4, _p(ctx.snap), ctx.ps[0], ctx.ps[1], _stream(),
             ctx.matmul, ctx.attn)
        torch.autograd.graph.increment_version((dx,) + grads)
        return (dx, None, None, None, None, None, None, None, None, None) + grads


BERT_MATMULS = ("fp32", "bf16")     # the value of gcgcn_bert_layer_*_mm's selector is the index


def bert_matmul_index(matmul, who: str) -> int:
    if matmul not in BERT_MATMULS:
        raise ValueError(f"{who}: matmul must be 'fp32' or 'bf16', got {matmul!r}")
    return BERT_MATMULS.index(matmul)


BERT_ATTENTIONS = ("fp32", "bf16")  # the value of the _mx entry points' attn selector is the index


def bert_attention_index(attention, who: str) -> int:
    if not isinstance(attention, str) or attention not in BERT_ATTENTIONS:
        raise ValueError(f"{who}: attention must be 'fp32' or 'bf16', got {attention!r}")
    return BERT_ATTENTIONS.index(attention)


class BertAttentionFn(torch.autograd.Function):
    """(qkv[B,T,3D], key_bias[B,T] | None, t_valid[B] | None) -> ctx[B,T,D] through gcgcn_bert_attn_fwd_mx / _bwd_mx."""

    @staticmethod
    def forward(ctx, qkv, key_bias, H, p, snap, t_valid, attn):
        B, T, D3 = qkv.shape
        out = torch.empty(B, T, D3 // 3, device=qkv.device)
        lse = torch.empty(B, H, T, device=qkv.device)
        call("gcgcn_bert_attn_fwd_mx", B, T, H, 64, _p(qkv), _p(key_bias), _p(t_valid), _p(out), _p(lse), _p(snap), _lib.SALT_BERT_ATTN,
             float(p), _stream(), attn)
        torch.autograd.graph.increment_version((out, lse))
        ctx.H, ctx.p, ctx.snap, ctx.t_valid, ctx.attn, ctx.has_kb = H, float(p), snap, t_valid, attn, key_bias is not None
        ctx.save_for_backward(qkv, out, lse, *(() if key_bias is None else (key_bias,)))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dctx):
        qkv, out, lse = ctx.saved_tensors[:3]
        key_bias = ctx.saved_tensors[3] if ctx.has_kb else None
        B, T, _ = qkv.shape
        dctx = dctx.contiguous()
        dqkv, delta = torch.empty_like(qkv), torch.empty_like(lse)
        call("gcgcn_bert_attn_bwd_mx", B, T, ctx.H, 64, _p(qkv), _p(key_bias), _p(ctx.t_valid), _p(out), _p(lse), _p(dctx), _p(dqkv),
             _p(delta), _p(ctx.snap), _lib.SALT_BERT_ATTN, ctx.p, _stream(), ctx.attn)
        torch.autograd.graph.increment_version((dqkv, delta))
        return dqkv, None, None, None, None, None, None


def bert_attention(qkv, key_bias, H, p=0.0, training=False, snap=None, t_valid=None, attention="fp32"):
    """The BERT attention core in HIP on packed ``qkv[B,T,3D]``, ``D = 64 H``: row ``(b, t)`` holds ``q | k | v``, head ``h`` in
    columns ``[64 h, 64 h + 64)`` of each.  Returns ``ctx[B,T,D] = dropout(softmax(q k^T / 8 + key_bias[b, key])) v``; the gradient
    reaches ``qkv``.  ``key_bias``: ``[B,T]`` additive penalty per key or None.  ``T <= 512``.  In training mode with ``p > 0`` the
    probabilities are dropped with the mask of ``dropout_keep_mask(snap, SALT_BERT_ATTN, p, B * H * T * T)`` (``snap``: default a
    fresh snapshot), regenerated in the backward.  ``t_valid``: token counts ``[B]``: rows at or past ``t_valid[b]`` are no keys, their
    ``ctx`` and gradient are exactly zero and the gradient arriving there is not read.  ``attention``: ``"fp32"`` (csrc/bert.hip) or
    ``"bf16"`` (csrc/bert_attn_bf16.hip: the four products on bf16 operands, ``gcgcn_amd.bert.Bf16AttentionFn`` is the definition;
    the mask drawn is the same).  Nothing of size ``[T,T]`` reaches memory; two runs from one seed are bitwise equal."""
    attn = bert_attention_index(attention, "bert_attention")
    qkv = _chk(qkv, "qkv", 3)
    B, T, D3 = qkv.shape
    if H < 1 or D3 != 3 * 64 * H:
        raise ValueError(f"bert_attention: qkv {tuple(qkv.shape)} is not [B, T, 3 * 64 * {H}] (the kernels serve a head width of 64)")
    if key_bias is not None:
        key_bias = _chk(key_bias, "key_bias", 2)
        if key_bias.shape != (B, T):
            raise ValueError(f"bert_attention: key_bias {tuple(key_bias.shape)}, expected ({B}, {T})")
    p = float(p) if training else 0.0
    if p > 0 and snap is None:
        snap = rng_snapshot(qkv.device)
    if t_valid is not None:
        t_valid = _nv(t_valid, B, T, qkv.device)
    return BertAttentionFn.apply(qkv, key_bias, H, p, snap if p > 0 else None, t_valid, attn)


def bert_layer(x, key_bias, wq, bq, wk, bk, wv, bv, wo, bo, ln1_w, ln1_b, wi, bi, wo2, bo2, ln2_w, ln2_b, p_attn=0.1, p_hidden=0.1,
               training=False, snap=None, t_valid=None, rowblk=None, matmul="fp32", attention="fp32"):
    """One BERT encoder layer (``pytorch_pretrained_bert`` 0.6 ``BertLayer``) in HIP: ``x[B,T,D]`` -> ``[B,T,D]``.  ``key_bias``:
    ``[B,T]`` additive score penalty per key (``(1 - mask) * -10000``) or None.  The 16 parameter tensors in ``BERT_LAYER_TENSORS``'
    order, Linear weights ``[out, in]``; the number of heads is ``D / 64`` (the attention kernels serve a head width of 64) and
    ``T <= 512``.  In training mode three dropout sites draw from one rng snapshot (``snap``, default a fresh one, inside an
    ``rng_scope`` the scope's next): the attention probabilities (``p_attn``, salt ``SALT_BERT_ATTN``, index = offset in
    ``[B,H,T,T]``) and the two Linear outputs in front of the LayerNorms (``p_hidden``, ``SALT_BERT_AO`` / ``SALT_BERT_OUT``,
    index = offset in ``[B,T,D]``).  Gradients reach ``x`` and all 16 tensors; two runs from one seed are bitwise equal.

    ``t_valid``: the documents' token counts ``[B]`` (int, on the device, ``0 <= t_valid[b] <= T``).  Live rows ``t < t_valid[b]`` get what
    the layer computes for document ``b`` alone at ``T = t_valid[b]`` with no mask (``key_bias`` may still punch holes inside the
    prefix); the output and the gradient of ``x`` are exactly zero on padding rows, the gradient arriving there is ignored (NaN
    included) and ``x`` must be zero there.  The dropout indices do not move.  ``rowblk``: ``row_blocks(t_valid, B, T)``, built once
    per model forward and shared by the layers -- the Linears then run on the live 16-row blocks where the GEMM launcher serves the
    list and dense elsewhere (always when ``T % 16 != 0``), with the same results contract; ``None`` with ``t_valid``: dense.
    ``t_valid=None``: the call as it was.

    ``matmul``: ``"fp32"`` (default: exactly the calls made without the argument) or ``"bf16"``: the twelve Linear products of the
    forward and the backward take bf16 operands -- every operand element rounded once, round to nearest even, what
    ``t.to(torch.bfloat16)`` does -- on the bf16 matrix cores, with fp32 accumulation; activations, weights and gradients stay fp32
    in memory, the bias gradients are fp32 sums of the unrounded gradients and everything between the products is unchanged.  With
    ``rowblk`` these products, too, run on the live 16-row blocks where their launcher serves the list (weight gradients skip the
    64-deep steps without a live block), bit for bit what the dense products give; the contract of the padding rows holds.
    ``BertModel(impl="torch", matmul="bf16")`` is the definition.

    ``attention``: ``"fp32"`` (default: the attention kernels as they were) or ``"bf16"``: the core's four matrix products take bf16
    operands on the bf16 matrix cores (csrc/bert_attn_bf16.hip) -- ``q``, ``k``, ``v`` and the arriving gradient rounded once, ``P``
    and ``dS`` when they become operands, fp32 accumulation, softmax, ``lse`` and ``delta`` in fp32; masks, token lengths and the
    dropout mask are the fp32 core's.  Independent of ``matmul``.  ``gcgcn_amd.bert.Bf16AttentionFn`` is the definition."""
    mm = bert_matmul_index(matmul, "bert_layer")
    attn = bert_attention_index(attention, "bert_layer")
    x = _chk(x, "x", 3)
    names = ("wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo", "ln1_w", "ln1_b", "wi", "bi", "wo2", "bo2", "ln2_w", "ln2_b")
    ts = [_chk(t, n) for n, t in zip(names, (wq, bq, wk, bk, wv, bv, wo, bo, ln1_w, ln1_b, wi, bi, wo2, bo2, ln2_w, ln2_b))]
    B, T, D = x.shape
    if D % 64:
        raise ValueError(f"bert_layer: D = {D} is no multiple of the head width 64")
    Dff = ts[10].shape[0]
    want = [(D, D), (D,)] * 3 + [(D, D), (D,), (D,), (D,), (Dff, D), (Dff,), (D, Dff), (D,), (D,), (D,)]
    for n, t, s in zip(names, ts, want):
        if tuple(t.shape) != s:
            raise ValueError(f"bert_layer: {n} has shape {tuple(t.shape)}, expected {s}")
    if key_bias is not None:
        key_bias = _chk(key_bias, "key_bias", 2)
        if key_bias.shape != (B, T):
            raise ValueError(f"bert_layer: key_bias {tuple(key_bias.shape)}, expected ({B}, {T})")
    p_attn, p_hidden = (float(p_attn), float(p_hidden)) if training else (0.0, 0.0)
    if (p_attn > 0 or p_hidden > 0) and snap is None:
        snap = rng_snapshot(x.device)
    # query | key | value stacked: one product instead of three (autograd splits the gradients again), as lstm_layer stacks directions
    wqkv, bqkv = torch.cat([ts[0], ts[2], ts[4]], 0), torch.cat([ts[1], ts[3], ts[5]], 0)
    if t_valid is not None:
        t_valid = _nv(t_valid, B, T, x.device)
        if rowblk is not None and (T % 16 or rowblk.dtype != torch.int32 or rowblk.device != x.device or
                                   rowblk.numel() < int(_lib.lib().gcgcn_row_blocks_ints(B, T))):
            raise ValueError(f"bert_layer: rowblk is not row_blocks(t_valid, {B}, {T})")
    elif rowblk is not None:
        raise ValueError("bert_layer: rowblk without t_valid")
    return BertLayerFn.apply(x, key_bias, D // 64, p_attn, p_hidden, snap if (p_attn > 0 or p_hidden > 0) else None, t_valid, rowblk, mm,
                             attn, wqkv, bqkv, *ts[6:])


def gemm_bf16(a, b, form="nt", bias=None, add=None):
    """``op(a) op(b) + bias[col] + add`` with bf16 operands and fp32 accumulation (csrc/gemm_bf16.hip through ``gcgcn_gemm_bf16``): fp32
    in, fp32 out, every operand element rounded once to bf16.  ``form`` names how the operands are STORED: ``"nn"``: ``a[M,K] @
    b[K,N]``; ``"nt"``: ``a[M,K] @ b[N,K].T``; ``"tn"``: ``a[K,M].T @ b[K,N]``.  ``a``, ``b`` and ``add`` may be row-strided views
    (unit stride in the last axis).  ``bias`` ``[N]``, ``add`` ``[M,N]``.  No autograd: a binding for tests and tools."""
    if form not in ("nn", "nt", "tn"):
        raise ValueError(f"gemm_bf16: form must be 'nn', 'nt' or 'tn', got {form!r}")
    for n, t in (("a", a), ("b", b), ("bias", bias), ("add", add)):
        if t is None:
            continue
        if not t.is_cuda or t.dtype != torch.float32:
            raise RuntimeError(f"gemm_bf16: {n} must be a float32 tensor on the GPU (there is no CPU fallback)")
        if t.dim() != (1 if n == "bias" else 2) or t.stride(-1) != 1:
            raise ValueError(f"gemm_bf16: {n} has shape {tuple(t.shape)} and strides {t.stride()}")
    a_kc, b_kc = form != "tn", form == "nt"
    M, K = a.shape if a_kc else a.shape[::-1]
    N, Kb = b.shape if b_kc else b.shape[::-1]
    if K != Kb or min(M, N, K) < 1:
        raise ValueError(f"gemm_bf16: a {tuple(a.shape)} and b {tuple(b.shape)} do not form a '{form}' product")
    if bias is not None and bias.shape != (N,):
        raise ValueError(f"gemm_bf16: bias {tuple(bias.shape)}, expected ({N},)")
    if add is not None and add.shape != (M, N):
        raise ValueError(f"gemm_bf16: add {tuple(add.shape)}, expected ({M}, {N})")
    c = torch.empty(M, N, device=a.device)
    ws = _f32_buf(_bytes_or_raise("gcgcn_gemm_bf16_ws_bytes", M, N, K), a.device)
    call("gcgcn_gemm_bf16", int(a_kc), int(b_kc), _p(a), a.stride(0), _p(b), b.stride(0), _p(c), N, M, N, K, _p(bias), _p(add),
         0 if add is None else add.stride(0), _p(ws) if ws.numel() else None, ws.numel() * 4, _stream())
    return c
