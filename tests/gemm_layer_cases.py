"""Cases, float64 restatement and bound of the GEMM layer's suites (csrc/gemm.hip, csrc/gemm_body.hpp through gcgcn_debug_gemm_run).
test_gemm_layer_cpu.py checks the restatement and the case tables without a GPU, test_gemm_layer_gpu.py runs the launchers on them.
Importable without a GPU.

A case is a launch form (FORM_*, the numbering of gcgcn_debug_gemm_run), a list of problems and, for a group launch, a ride.  Every
operand of a problem is (buffer name, element offset) into a flat float32 buffer plus the strides of csrc/gemm.hpp, so a shifted
view, an interleaved view, a zero stride or an operand one float off a 16-byte boundary are all just numbers.

Inputs.  make_tensors(case) is seeded; the float32 masters live on the CPU, kernel and restatement read the same values.  Inputs
are standard normal (rowscale in +-[0.5, 1.5]), every buffer is drawn on its own, leading dimensions carry padding (lda = width + 4,
ldb = width + 8, ldc = N + 4 unless the case says otherwise) and batch strides carry more, so no two operands are equal, no leading
dimension is square and no stride that matters runs along constant data.  Output buffers (C, C2, workspace, column-sum partials)
are allocated with a margin in front, slack rows behind and filled with SENTINEL; a problem that accumulates gets a random prior in
exactly the window it may write.

Restatement.  reference() follows the epilogue lines of csrc/gemm.hpp in their order, in float64, and returns per output buffer the
expected values, the bound and the mask of elements the launch must write; everything outside the mask must keep SENTINEL bit for
bit.  Row blocks: mode 1 leaves the rows of dead blocks alone (rb_zero = 0) or expects exact zeros there (rb_zero = 1), mode 2 sums
over the live blocks only; device-side forms use the exact count (interior shapes: the count rounded up to 64, as gemm.hpp says).

Bound.  fp32 MFMA products are exact and accumulate in fp32 in some order; for any order |fl(sum a_k b_k) - sum a_k b_k| <=
gamma_K sum |a_k b_k|, gamma_K = K u / (1 - K u), u = 2^-24.  Per element: gamma_{K+8} (|alpha| (|A| |B|) + |add| + |bias| + |rowadd|
+ |C_prior|), carried through rowscale (times |rowscale|), relu (1-Lipschitz) and the dropout scale (times 1 / (1 - p)); the + 8 covers
the epilogue's own roundings.  |C_prior| enters after rowscale in the epilogue's order; the issue's formula puts it inside: the
smaller of the two readings is used.  Padding rows, zero-stored rows and dropped elements have bound 0 (exact).  Column sums: gamma_R
sum |x| over the summed rows.  There is no rtol / atol."""
import ctypes
from types import SimpleNamespace

import numpy as np
import torch

FORM_GEMM, FORM_GROUP, FORM_PARK, FORM_PAIR_WX, FORM_PAIR_WW, FORM_PAIR_XX = 0, 1, 2, 5, 6, 7
NI, NF, NP = 40, 2, 14                               # gcgcn_debug_gemm_run: int64 / float / pointers per problem
PTR_ORDER = ("A", "B", "C", "add", "bias", "rowadd", "rowscale", "C2", "add2", "n_valid", "rb", "rb_n", "ws", "rng_snap")
INT_ORDER = ("M", "N", "K", "a_kc", "b_kc", "lda", "ldb", "ldc", "batch1", "batch2", "rb_mode", "ws_elems", "unused12",
             "sA1", "sA2", "sB1", "sB2", "sC1", "sC2", "ldadd", "sAdd1", "sAdd2", "sRa1", "sRa2", "sRs1", "sRs2",
             "ldc2", "sC21", "sC22", "ldadd2", "sAdd21", "sAdd22", "relu", "accumulate", "nv_rows", "nv_zdoc", "rb_zero",
             "drop_base", "salt", "unused39")
COL_RIDE_SLICES, MAXP, DEFER_CAP, BK = 64, 9, 32, 32   # csrc/gemm.hpp, csrc/gemm_body.hpp
SENTINEL = 12345.678710937500                        # exactly representable in float32
U = 2.0 ** -24
FORMS = {"nn": (1, 0), "nt": (1, 1), "tn": (0, 0)}
ALL_FEATS = ("alpha", "add", "bias", "rowadd", "rowscale", "C2", "add2")


def gamma(k):
    return k * U / (1.0 - k * U)


# ---- building cases ---------------------------------------------------------------------------------------------------------------
class Builder:
    """Collects the buffers of one case: name -> (numel, kind); kind 'in' random normal, 'scale' rowscale, 'out' SENTINEL, 'int'."""

    def __init__(self, name, form, seed, **kw):
        self.case = SimpleNamespace(name=name, form=form, seed=seed, probs=[], buffers={}, ints={}, ride=None, tile=0, splits=1,
                                    cnt=None, cap=0, expect=[], nan_rows=[], **kw)

    def buf(self, name, numel, kind):
        assert name not in self.case.buffers, name
        self.case.buffers[name] = (int(numel), kind)
        return name

    def problem(self, form, M, N, K, feats=(), relu=0, accumulate=0, batch=(1, 1), ldc_pad=4, misalign=(), shared_B=False,
                n_valid=None, nv_rows=1, nv_zdoc=0, p=0.0, rb=None, rb_mode=0, rb_zero=0, ws_elems=0, ws=None,
                alloc_M=None, alloc_K=None, expect=None, tag=None):
        """One problem with buffers of its own.  feats: names out of ALL_FEATS.  misalign: operand names placed one float off a 16-byte
        boundary.  alloc_M / alloc_K: rows the buffers hold (device-side forms: the capacity).  expect: plan fields to assert."""
        c, i = self.case, len(self.case.probs)
        a_kc, b_kc = FORMS[form]
        b1, b2 = batch
        Ma, Ka = alloc_M or M, alloc_K or K
        q = SimpleNamespace(form=form, M=M, N=N, K=K, a_kc=a_kc, b_kc=b_kc, batch1=b1, batch2=b2, relu=relu, accumulate=accumulate,
                            nv_rows=nv_rows, nv_zdoc=nv_zdoc, rb_mode=rb_mode, rb_zero=rb_zero, ws_elems=ws_elems, p=p,
                            alpha=-1.25 if "alpha" in feats else 1.0, salt=0x47454D31 + i, drop_base=0, ptr={}, tag=tag or f"p{i}",
                            alloc_M=Ma, alloc_K=Ka, dyn=0)
        for f in INT_ORDER:
            if not hasattr(q, f):
                setattr(q, f, 0)
        off = lambda name: 4 + (1 if name in misalign else 0)    # 4 floats of margin: a write in front of the window shows

        def operand(name, rows, width, ld, batched=True, kind="in"):
            s2 = rows * ld + 8
            s1 = b2 * s2 + 16
            self.buf(f"{name}_{i}", off(name) + (b1 * s1 if batched else rows * ld) + 2 * ld + 8, kind)
            q.ptr[name] = (f"{name}_{i}", off(name))
            return (s1, s2) if batched else (0, 0)
        ra, wa = (Ma, Ka) if a_kc else (Ka, Ma)
        q.lda = wa + 4
        q.sA1, q.sA2 = operand("A", ra, wa, q.lda)
        rb_, wb = (N, Ka) if b_kc else (Ka, N)
        q.ldb = wb + 8
        q.sB1, q.sB2 = operand("B", rb_, wb, q.ldb)
        if shared_B:
            q.sB1 = 0
        q.ldc = N + ldc_pad
        q.sC1, q.sC2 = operand("C", Ma, N, q.ldc, kind="out")
        if "add" in feats:
            q.ldadd = N + 12
            q.sAdd1, q.sAdd2 = operand("add", Ma, N, q.ldadd)
        if "bias" in feats:
            operand("bias", 1, N, N, batched=False)
        if "rowadd" in feats:
            q.sRa1, q.sRa2 = operand("rowadd", 1, Ma, Ma)
        if "rowscale" in feats:
            q.sRs1, q.sRs2 = operand("rowscale", 1, Ma, Ma, kind="scale")
        if "C2" in feats:
            q.ldc2 = N + 16
            q.sC21, q.sC22 = operand("C2", Ma, N, q.ldc2, kind="out")
            q.drop_base = 1000 + 3 * i                                  # C2 as a shifted view of the dropout site
            if "add2" in feats:
                q.ldadd2 = N + 20
                q.sAdd21, q.sAdd22 = operand("add2", Ma, N, q.ldadd2)
        if n_valid is not None:
            c.ints[f"nv{i}"] = list(n_valid)
            q.ptr["n_valid"] = (f"nv{i}", 0)
        if rb is not None:
            q.ptr["rb"], q.ptr["rb_n"] = (rb, 4), (rb, 0)
        if ws is not None:
            q.ptr["ws"] = ws
        elif ws_elems:
            self.buf(f"ws_{i}", ws_elems + 8 + 4096, "out")
            q.ptr["ws"] = (f"ws_{i}", 4)
        if p > 0:
            q.ptr["rng_snap"] = ("snap", 0)
        c.probs.append(q)
        c.expect.append(expect or {})
        return q


def make_tensors(case):
    """name -> CPU tensor.  Seeded by the case; 'snap' is the dropout site's {seed, counter}."""
    g = torch.Generator().manual_seed(case.seed)
    T = {}
    for name, (numel, kind) in case.buffers.items():
        if kind == "out":
            T[name] = torch.full((numel,), SENTINEL, dtype=torch.float32)
        elif kind == "scale":
            mag = torch.rand(numel, generator=g) + 0.5
            T[name] = torch.where(torch.rand(numel, generator=g) < 0.5, -mag, mag)
        else:
            T[name] = torch.randn(numel, generator=g)
    for name, vals in case.ints.items():
        T[name] = torch.tensor(vals, dtype=torch.int32)
    T["snap"] = torch.tensor([0x5EED0000 + case.seed, 17], dtype=torch.int64)
    for q in case.probs:
        if q.accumulate:                                       # a random prior in exactly the window the problem may write
            idx = _idx(q.ptr["C"][1], q.sC1, q.sC2, q.ldc, 1, q.batch1, q.batch2, q.alloc_M if q.dyn == 1 else q.M, q.N).reshape(-1)
            T[q.ptr["C"][0]][idx] = torch.randn(idx.numel(), generator=g)
    for name, off, count in case.nan_rows:                     # rows no correct launch reads
        T[name][off:off + count] = float("nan")
    return T


def live_blocks(n_valid, rows_per_doc):
    """gcgcn_row_blocks' list for documents of rows_per_doc rows: {live, 0, 0, 0 | live blocks ascending, dead blocks ascending}."""
    per = rows_per_doc // 16
    live = [b * per + r for b, n in enumerate(n_valid) for r in range(per) if 16 * r < n]
    dead = [b * per + r for b, n in enumerate(n_valid) for r in range(per) if 16 * r >= n]
    return [len(live), 0, 0, 0] + live + dead


# ---- the float64 restatement ----------------------------------------------------------------------------------------------------
def _idx(off, s1, s2, ld, colstep, b1, b2, rows, cols):
    """element index [b1, b2, rows, cols] of a [rows][ld] operand (colstep 1), batch strided"""
    z1 = torch.arange(b1).view(-1, 1, 1, 1)
    z2 = torch.arange(b2).view(1, -1, 1, 1)
    r = torch.arange(rows).view(1, 1, -1, 1)
    c = torch.arange(cols).view(1, 1, 1, -1)
    return off + z1 * s1 + z2 * s2 + r * ld + c * colstep


def _take(T, q, name, idx):
    return T[q.ptr[name][0]].double()[idx]


def problem_reference(q, T, keep=None, count=None, interior=None):
    """The nine epilogue lines of csrc/gemm.hpp for one problem -> {buffer: (indices, values, bound)} of what it must write.
    count / interior: a device-side form's row count and whether its plan takes the unguarded body (count rounded up to 64)."""
    M, N, K, b1, b2 = q.M, q.N, q.K, q.batch1, q.batch2
    if q.dyn:
        eff = (count + 63) // 64 * 64 if interior else count
        M, K = (eff, K) if q.dyn == 1 else (M, eff)
    if M == 0 or N == 0:
        return {}
    Kq = max(K, 1)
    oa, ob = q.ptr["A"][1], q.ptr["B"][1]
    A = _take(T, q, "A", _idx(oa, q.sA1, q.sA2, q.lda, 1, b1, b2, M, Kq) if q.a_kc else _idx(oa, q.sA1, q.sA2, 1, q.lda, b1, b2, M, Kq))
    B = _take(T, q, "B", _idx(ob, q.sB1, q.sB2, 1, q.ldb, b1, b2, Kq, N) if q.b_kc else _idx(ob, q.sB1, q.sB2, q.ldb, 1, b1, b2, Kq, N))
    if K == 0:                                                  # a device-side count of zero: the empty sum
        A, B = torch.zeros_like(A), torch.zeros_like(B)
    klen = K
    live = None
    if q.rb_mode:
        lst = T[q.ptr["rb"][0]].tolist()
        live = torch.zeros(len(lst) - 4, dtype=torch.bool)
        live[lst[4:4 + lst[0]]] = True
    if q.rb_mode == 2:                                          # K = document rows: the live 16-row blocks only
        kl = live[torch.arange(K) // 16]
        A = torch.where(kl.view(1, 1, 1, -1), A, torch.zeros_like(A))
        B = torch.where(kl.view(1, 1, -1, 1), B, torch.zeros_like(B))
        klen = int(kl.sum())
    v = q.alpha * (A @ B)                                       # v = alpha * acc
    mag = abs(q.alpha) * (A.abs() @ B.abs())
    rows = lambda s1, s2: _idx(0, s1, s2, 1, 0, b1, b2, M, 1)
    if "add" in q.ptr:                                          # v += add[row * ldadd + col]
        t = _take(T, q, "add", _idx(q.ptr["add"][1], q.sAdd1, q.sAdd2, q.ldadd, 1, b1, b2, M, N))
        v, mag = v + t, mag + t.abs()
    if "bias" in q.ptr:                                         # v += bias[col]
        t = _take(T, q, "bias", q.ptr["bias"][1] + torch.arange(N)).view(1, 1, 1, N)
        v, mag = v + t, mag + t.abs()
    if "rowadd" in q.ptr:                                       # v += rowadd[row]
        t = _take(T, q, "rowadd", q.ptr["rowadd"][1] + rows(q.sRa1, q.sRa2))
        v, mag = v + t, mag + t.abs()
    mag_in = mag
    if "rowscale" in q.ptr:                                     # v *= rowscale[row]
        t = _take(T, q, "rowscale", q.ptr["rowscale"][1] + rows(q.sRs1, q.sRs2))
        v, mag = v * t, mag * t.abs()
        scale = t.abs()
    else:
        scale = torch.ones(1, dtype=torch.float64)
    if q.relu:                                                  # v = max(v, 0)
        v = v.clamp_min(0.0)
    cidx = _idx(q.ptr["C"][1], q.sC1, q.sC2, q.ldc, 1, b1, b2, M, N)
    if q.accumulate:                                            # v += C[row, col]
        t = _take(T, q, "C", cidx)
        v = v + t
        mag = torch.minimum(mag + t.abs(), (mag_in + t.abs()) * scale)
    bound = gamma(klen + 8) * mag
    written = torch.ones(b1, b2, M, 1, dtype=torch.bool)
    if "n_valid" in q.ptr:                                      # v = 0 if the row is a padding row
        nv = T[q.ptr["n_valid"][0]].long()
        r = torch.arange(M).view(1, 1, -1, 1)
        doc = torch.arange(b1).view(-1, 1, 1, 1) * q.nv_zdoc + r // q.nv_rows
        pad = (r % q.nv_rows) >= nv[doc]
    else:
        pad = torch.zeros(1, 1, M, 1, dtype=torch.bool)
    if q.rb_mode == 1:                                          # M = document rows: dead blocks are zero-stored or left alone
        dead = ~live[torch.arange(M) // 16].view(1, 1, -1, 1)
        if q.rb_zero:
            pad = pad | dead
        else:
            written = written & ~dead
    pad = pad.expand(b1, b2, M, 1)
    v = torch.where(pad, torch.zeros_like(v), v)
    bound = torch.where(pad, torch.zeros_like(bound), bound)
    w = written.expand(b1, b2, M, N)
    out = {q.ptr["C"][0]: (cidx[w], v[w], bound[w])}            # C[row, col] = v
    if "C2" in q.ptr:                                           # C2[row, col] = dropout(v) + add2[row * ldadd2 + col]
        o2 = _idx(0, q.sC21, q.sC22, q.ldc2, 1, b1, b2, M, N)
        v2, bound2 = v, bound
        if q.p > 0:
            k = keep[o2 + q.drop_base].bool()
            v2 = torch.where(k, v / (1.0 - q.p), torch.zeros_like(v))
            bound2 = torch.where(k, bound / (1.0 - q.p), torch.zeros_like(bound))
        if "add2" in q.ptr:
            v2 = v2 + _take(T, q, "add2", _idx(q.ptr["add2"][1], q.sAdd21, q.sAdd22, q.ldadd2, 1, b1, b2, M, N))
        v2 = torch.where(pad, torch.zeros_like(v2), v2)         # padding rows of C2 are zero (add2 is not added there)
        out[q.ptr["C2"][0]] = ((o2 + q.ptr["C2"][1])[w], v2[w], bound2[w])
    return out


def keep_extent(q):
    """dropout indices the problem may draw: [0, n)"""
    return q.drop_base + (q.batch1 - 1) * q.sC21 + (q.batch2 - 1) * q.sC22 + (q.M - 1) * q.ldc2 + q.N


def ride_reference(ride, T):
    """A riding column sum (col_sum / .stage2 / head_sum) -> {buffer: (indices, values, bound)}; col_sum also gives its partials."""
    out = {}
    X = T[ride.X[0]].double() if ride.X else None
    if ride.kind == 3:
        H, D = ride.R, ride.ld
        k, h, c = torch.arange(D).view(-1, 1, 1), torch.arange(H).view(1, -1, 1), torch.arange(D).view(1, 1, -1)
        w = X[ride.X[1] + (k * H + h) * D + c]
        out[ride.out[0]] = (ride.out[1] + torch.arange(D * D), w.sum(1).reshape(-1), gamma(H) * w.abs().sum(1).reshape(-1))
        return out
    C = ride.C
    if ride.kind == 2:
        part = T[ride.part[0]].double()[ride.part[1] + torch.arange(ride.slices).view(-1, 1) * C + torch.arange(C)]
        out[ride.out[0]] = (ride.out[1] + torch.arange(C), part.sum(0), gamma(ride.slices) * part.abs().sum(0))
        return out
    x = X[ride.X[1] + torch.arange(ride.R).view(-1, 1) * ride.ld + torch.arange(C)]
    rps = -(-ride.R // COL_RIDE_SLICES)
    part = torch.zeros(COL_RIDE_SLICES, C, dtype=torch.float64)
    pb = torch.zeros_like(part)
    for s in range(COL_RIDE_SLICES):
        part[s], pb[s] = x[s * rps:(s + 1) * rps].sum(0), gamma(rps) * x[s * rps:(s + 1) * rps].abs().sum(0)
    out[ride.part[0]] = (ride.part[1] + torch.arange(COL_RIDE_SLICES * C), part.reshape(-1), pb.reshape(-1))
    # (with col_later set the caller finishes stage 2: the test does, through a .stage2(COL_RIDE_SLICES) launch of its own)
    out[ride.out[0]] = (ride.out[1] + torch.arange(C), x.sum(0), gamma(ride.R + COL_RIDE_SLICES) * x.abs().sum(0))
    return out


def reference(case, T, keeps=None, interior=None):
    """-> {buffer: (expected float64, bound float64, written bool)} over the whole of every buffer a launch of the case writes.
    keeps: problem index -> the uint8 keep mask of its dropout site (gcgcn_dropout_keep); interior: per problem, a device-side form's
    plan takes the unguarded body."""
    res = {}

    def put(name, idx, val, bnd):
        if name not in res:
            n = T[name].numel()
            res[name] = (T[name].double().clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.bool))
        e, b, w = res[name]
        idx = idx.reshape(-1)
        assert not w[idx].any(), f"{case.name}: two problems write the same element of {name}"
        e[idx], b[idx], w[idx] = val.reshape(-1), bnd.reshape(-1), True
    for i, q in enumerate(case.probs):
        for name, (idx, val, bnd) in problem_reference(q, T, (keeps or {}).get(i), case.cnt, (interior or {}).get(i)).items():
            put(name, idx, val, bnd)
    if case.ride is not None:
        for name, (idx, val, bnd) in ride_reference(case.ride, T).items():
            put(name, idx, val, bnd)
    return res


# ---- the route a case means to take (gcgcn_debug_gemm_plan) -----------------------------------------------------------------------
PLAN_FIELDS = ("ok", "interior", "splits", "ksplit", "widen", "rb_mode", "vecA", "vecB", "tiles", "reduce", "zero_fill", "grid")


def plan_row(q):
    mis = (q.ptr["A"][1] % 4 != 0) | 2 * (q.ptr["B"][1] % 4 != 0) | 4 * ("ws" in q.ptr and q.ptr["ws"][1] % 4 != 0)
    ws = q.ws_elems if "ws" in q.ptr else 0
    return [max(q.M, 1) if q.dyn == 1 else q.M, q.N, max(q.K, 1), q.a_kc, q.b_kc, q.lda, q.ldb, q.ldc, q.batch1, q.batch2, q.rb_mode, ws, mis]


def work_of(q):
    return -(-q.M // 64) * -(-q.N // 64) * q.batch1 * q.batch2 * -(-q.K // BK)


def plans(case, lib_call):
    """per problem: the plan's fields by name (a pair adds 'fused'), from the form the case launches through"""
    def ask(form, a, b, splits, work, cap):
        out = np.full(26, -7, np.int32)
        pa, pb = (ctypes.c_int64 * 13)(*a), (ctypes.c_int64 * 13)(*b) if b is not None else None
        lib_call("gcgcn_debug_gemm_plan", form, pa, pb, splits, work, cap, out.ctypes.data_as(ctypes.c_void_p))
        return [int(x) for x in out]
    if case.form >= FORM_PAIR_WX:
        o = ask(case.form, plan_row(case.probs[0]), plan_row(case.probs[1]), 1, 0, case.cap)
        return [dict(zip(PLAN_FIELDS, o[12 * i:12 * i + 12]), fused=o[24]) for i in range(2)]
    work = sum(work_of(q) for q in case.probs)
    res = []
    for q in case.probs:
        if q.M == 0 or q.N == 0:
            res.append({})
            continue
        res.append(dict(zip(PLAN_FIELDS, ask(case.form, plan_row(q), None, case.splits, work, 0))))
    return res


def assert_routes(case, lib_call):
    got = plans(case, lib_call)
    for i, (want, have) in enumerate(zip(case.expect, got)):
        for k, v in want.items():
            assert have.get(k) == v, f"{case.name}: problem {i} plans {k} = {have.get(k)}, the case means {v} ({have})"
    return got


# ---- the flat rows of gcgcn_debug_gemm_run ----------------------------------------------------------------------------------------
def pack(case, address):
    """address(buffer name) -> base address of its copy (0 for a CPU-only check of the layout).  Returns the ctypes arguments."""
    n = len(case.probs)
    ints = np.zeros((max(n, 1), NI), np.int64)
    scal = np.zeros((max(n, 1), NF), np.float32)
    ptrs = np.zeros((max(n, 1), NP), np.uint64)
    for i, q in enumerate(case.probs):
        ints[i] = [getattr(q, f) for f in INT_ORDER]
        scal[i] = [q.alpha, q.p]
        for j, name in enumerate(PTR_ORDER):
            if name in q.ptr:
                buf, off = q.ptr[name]
                ptrs[i, j] = address(buf) + 4 * off
    ride = np.zeros(6, np.int64)
    rptr = np.zeros(3, np.uint64)
    r = case.ride
    if r is not None:
        ride[:] = [r.kind, r.R, r.ld, r.C, r.slices, r.col_later]
        for j, o in enumerate((r.X, r.out, r.part)):
            if o:
                rptr[j] = address(o[0]) + 4 * o[1]
    return ints, scal, ptrs, ride, rptr


def make_ride(b, kind, R, C=0, ld=None, slices=0, col_later=0, later_expected=False):
    """kind 1 col_sum(X [R][ld], C), 2 its .stage2(slices) on partials the test writes, 3 head_sum(W, H = R, D = ld)"""
    r = SimpleNamespace(kind=kind, R=R, C=C, ld=ld if ld is not None else C + 5, slices=slices, col_later=col_later, X=None, out=None,
                        part=None, later_expected=later_expected)
    if kind == 3:
        r.C = r.ld * r.ld
        r.X = (b.buf("rideX", 4 + R * r.ld * r.ld + 8, "in"), 4)
    elif kind == 1:
        r.X = (b.buf("rideX", 4 + R * r.ld + 8, "in"), 4)
    r.out = (b.buf("rideOut", 4 + r.C + 64, "out"), 4)
    if kind == 1:
        r.part = (b.buf("ridePart", 4 + COL_RIDE_SLICES * C + 64, "out"), 4)
    elif kind == 2:
        r.part = (b.buf("ridePart", 4 + slices * C + 64, "in"), 4)
    b.case.ride = r
    return r


# ---- the case tables ----------------------------------------------------------------------------------------------------------------
BODIES = {"i64": (64, 64, 32), "i128": (128, 64, 96), "guard": (70, 36, 37)}
INTERIOR = {"ok": 1, "interior": 1, "splits": 1, "reduce": 0}
GUARDED = {"ok": 1, "interior": 0, "splits": 1, "reduce": 0}
FEATURE_SETS = {"plain": (), "alpha": ("alpha",), "add": ("add",), "bias": ("bias",), "rowadd": ("rowadd",), "rowscale": ("rowscale",),
                "C2": ("C2",), "C2add2": ("C2", "add2"), "all": ALL_FEATS}


def epilogue_case(form, body, feat, relu=0, accumulate=0, p=0.0, misalign=(), nv=None, seed=1):
    M, N, K = BODIES[body]
    name = f"epi-{form}-{body}-{feat}-r{relu}a{accumulate}" + (f"-p{p}" if p else "") + ("-off" + "".join(misalign) if misalign else "") + \
        (f"-nv{nv}" if nv is not None else "")
    b = Builder(name, FORM_GEMM, seed)
    guarded = body == "guard" or "A" in misalign or "B" in misalign
    kw = {}
    if nv is not None:
        docs = -(-M // 16)
        kw = dict(n_valid=[nv, 16 - nv if nv else 5, 1, 16, 0][:docs] + [3] * max(0, docs - 5), nv_rows=16)
    b.problem(form, M, N, K, FEATURE_SETS[feat], relu, accumulate, p=p, misalign=misalign, expect=GUARDED if guarded else INTERIOR, **kw)
    return b.case


def epilogue_cases():
    cases = []
    for form in FORMS:
        for body in BODIES:
            for feat in FEATURE_SETS:
                cases.append(epilogue_case(form, body, feat, seed=len(cases) + 1))
            cases.append(epilogue_case(form, body, "all", 1, 1, p=0.25, seed=len(cases) + 1))
            cases.append(epilogue_case(form, body, "all", 1, 0, seed=len(cases) + 1))
            cases.append(epilogue_case(form, body, "all", 0, 1, p=0.25, seed=len(cases) + 1))
        cases.append(epilogue_case(form, "i64", "all", 1, 1, p=0.25, misalign=("A",), seed=len(cases) + 1))       # vecA = 0: guarded body
        cases.append(epilogue_case(form, "i128", "all", 1, 1, p=0.25, misalign=("add", "add2", "C2"), seed=len(cases) + 1))  # epi scalar path
    for nv in (0, 1, 16):
        for body in ("i128", "guard"):
            cases.append(epilogue_case("nn", body, "all", 1, 1, p=0.25, nv=nv, seed=len(cases) + 1))
    return cases


def batch_cases():
    cases = []
    for form in FORMS:
        for body in ("i64", "guard"):
            M, N, K = BODIES[body]
            b = Builder(f"batch-{form}-{body}", FORM_GEMM, 100 + len(cases))
            q = b.problem(form, M, N, K, ALL_FEATS, 1, 1, batch=(2, 3), ldc_pad=8, shared_B=True, p=0.25,
                          expect=INTERIOR if body == "i64" else GUARDED)
            q.sAdd22 = 0                                        # as plan_fwd_agg passes add2
            cases.append(b.case)
    cases += [stack_case(k) for k in ("dense", "agg", "dP", "dA", "dY")]
    return cases


def stack_case(kind, N=16, gh=32, L=2, H=2, B=2):
    """The five plan_* descriptions of csrc/gcn_plan.hpp with exactly their strides and flags, on [B N, H, L, gh] tensors; l = 1 (dA:
    l = 0, its rowadd pass)."""
    D, HD = L * gh, H * L * gh
    b = Builder(f"stack-{kind}", FORM_GEMM, 200 + len(kind))
    rows = B * N * HD + 64
    sb, sh, l = N * HD, L * gh, 1
    off = l * gh
    sa = (H * N * N, N * N)
    q = SimpleNamespace(**{f: 0 for f in INT_ORDER if f != "salt"}, ptr={}, alpha=1.0, p=0.0, salt=0x47434E31, tag=kind, dyn=0, form="", alloc_M=N, alloc_K=0)
    q.batch1, q.batch2, q.nv_rows = B, H, 1

    def t(name, numel, kind_="in"):
        return b.buf(name, numel + 16, kind_)
    if kind == "dense":      # Pn_l += [Y_0 .. Y_{l-1}] Wd_l
        q.form, q.M, q.N, q.K, q.a_kc, q.b_kc = "nn", N, gh, l * gh, 1, 0
        q.ptr = {"A": (t("Y", rows), 4), "B": (t("Wd", H * 80 * gh), 4), "C": (t("Pn", rows, "out"), 4 + off)}
        q.lda, q.ldb, q.ldc = HD, gh, HD
        q.sA1, q.sA2, q.sB1, q.sB2, q.sC1, q.sC2 = sb, sh, 0, 80 * gh, sb, sh
        q.accumulate = 1
    elif kind == "agg":      # Y_l = relu((G_l + A_h Pn_l) * rinv); HO_l = dropout(Y_l) + X_l: C and C2 are views of [M, H, L, gh] tensors
        q.form, q.M, q.N, q.K, q.a_kc, q.b_kc = "nn", N, gh, N, 1, 0
        q.ptr = {"A": (t("Adj", B * H * N * N), 4), "B": (t("Pn", rows), 4 + off), "C": (t("Y", rows, "out"), 4 + off),
                 "add": (t("G", rows), 4 + off), "rowscale": (t("rinv", B * H * N, "scale"), 4), "C2": (t("HO", rows, "out"), 4 + off),
                 "add2": (t("X", B * N * D), 4 + off), "rng_snap": ("snap", 0)}
        q.lda, q.ldb, q.ldc = N, HD, HD
        q.sA1, q.sA2, q.sB1, q.sB2, q.sC1, q.sC2 = sa[0], sa[1], sb, sh, sb, sh
        q.ldadd, q.sAdd1, q.sAdd2 = HD, sb, sh
        q.sRs1, q.sRs2 = H * N, N
        q.relu, q.ldc2, q.sC21, q.sC22 = 1, HD, sb, sh
        q.ldadd2, q.sAdd21, q.sAdd22 = D, N * D, 0
        q.p, q.drop_base = 0.25, off
    elif kind == "dP":       # dPn_l = A_h^T dM_l
        q.form, q.M, q.N, q.K, q.a_kc, q.b_kc = "tn", N, gh, N, 0, 0
        q.ptr = {"A": (t("Adj", B * H * N * N), 4), "B": (t("dM", rows), 4 + off), "C": (t("dP", rows, "out"), 4 + off)}
        q.lda, q.ldb, q.ldc = N, HD, HD
        q.sA1, q.sA2, q.sB1, q.sB2, q.sC1, q.sC2 = sa[0], sa[1], sb, sh, sb, sh
    elif kind == "dA":       # dA_h (+)= dM_l Pn_l^T, drow added on the last pass (l = 0): L = 2, so it accumulates
        off = 0
        q.form, q.M, q.N, q.K, q.a_kc, q.b_kc = "nt", N, N, gh, 1, 1
        q.ptr = {"A": (t("dM", rows), 4 + off), "B": (t("Pn", rows), 4 + off), "C": (t("dA", B * H * N * N, "out"), 4),
                 "rowadd": (t("drow", B * H * N), 4)}
        q.lda, q.ldb, q.ldc = HD, HD, N
        q.sA1, q.sA2, q.sB1, q.sB2, q.sC1, q.sC2 = sb, sh, sb, sh, sa[0], sa[1]
        q.accumulate, q.sRa1, q.sRa2 = 1, H * N, N
    else:                    # dY_{0..l-1} += dPn_l Wd_l^T
        q.form, q.M, q.N, q.K, q.a_kc, q.b_kc = "nt", N, l * gh, gh, 1, 1
        q.ptr = {"A": (t("dP", rows), 4 + off), "B": (t("Wd", H * 80 * gh), 4), "C": (t("dYa", rows, "out"), 4)}
        q.lda, q.ldb, q.ldc = HD, gh, HD
        q.sA1, q.sA2, q.sB1, q.sB2, q.sC1, q.sC2 = sb, sh, 0, 80 * gh, sb, sh
        q.accumulate = 1
    b.case.probs.append(q)
    b.case.expect.append(GUARDED)                               # N = 16 rows: no whole tile
    return b.case


def splitk_cases():
    cases = []
    for form in FORMS:
        # splits = 0 leaves the choice to pick_splits, which keeps slices of 8 k-steps: K = 256 stays whole, K = 512 is cut in two
        for splits, K, want in ((2, 256, 2), (4, 256, 4), (0, 512, 2)):
            b = Builder(f"splitk-{form}-s{splits}", FORM_GEMM, 300 + len(cases))
            b.problem(form, 128, 64, K, ALL_FEATS, 1, 1, p=0.25, ws_elems=4 * 128 * 64,
                      expect={"interior": 1, "splits": want, "ksplit": K // want, "reduce": 1})
            b.case.splits = splits
            cases.append(b.case)
    b = Builder("splitk-ws-too-small", FORM_GEMM, 390)
    b.problem("nn", 128, 64, 256, ALL_FEATS, 1, 1, p=0.25, ws_elems=4 * 128 * 64 - 1, expect={"interior": 1, "splits": 1, "reduce": 0})
    b.case.splits = 4
    cases.append(b.case)
    b = Builder("splitk-N-not-4", FORM_GEMM, 391)
    b.problem("nn", 128, 62, 256, ALL_FEATS, 1, 1, p=0.25, ldc_pad=6, ws_elems=4 * 128 * 64, expect={"interior": 0, "splits": 1, "reduce": 0})
    b.case.splits = 4
    cases.append(b.case)
    return cases


NV_LISTS = ([0, 17, 64], [64, 64, 64], [1, 16, 33], [0, 0, 0])


def rb1_cases():
    """Mode 1 as a member of a group launch: three documents of 64 rows."""
    cases = []
    for nv in NV_LISTS:
        for rb_zero in (1, 0):
            for with_nv in (1, 0):
                b = Builder(f"rb1-{'_'.join(map(str, nv))}-z{rb_zero}-nv{with_nv}", FORM_GROUP, 400 + len(cases))
                b.case.ints["rb"] = live_blocks(nv, 64)
                b.problem("nn", 192, 64, 64, ALL_FEATS, 1, 0, p=0.25, rb="rb", rb_mode=1, rb_zero=rb_zero,
                          n_valid=nv if with_nv else None, nv_rows=64, expect={"interior": 1, "rb_mode": 1, "splits": 1})
                b.problem("nt", 64, 64, 32, ("bias",), expect=INTERIOR)
                cases.append(b.case)
    for nv in NV_LISTS[:3]:
        # A member's split comes from pick_splits on the launch's work: 8 slices of 8 k-steps at K = 2048 (at K = 1536 a slice of 6
        # k-steps is too short for split_width to cut: the device-side cut needs halves of 4 k-steps).  The workspace allows widen 1, 2, 4.
        for slabs, widen in ((8, 1), (16, 2), (32, 4)):
            for rb_zero in (1, 0):
                b = Builder(f"rb1-longK-{'_'.join(map(str, nv))}-w{widen}-z{rb_zero}", FORM_GROUP, 450 + len(cases))
                b.case.ints["rb"] = live_blocks(nv, 64)
                b.problem("nn", 192, 64, 2048, ALL_FEATS, 1, 0, p=0.25, rb="rb", rb_mode=1, rb_zero=rb_zero, n_valid=nv, nv_rows=64,
                          ws_elems=slabs * 192 * 64, expect={"interior": 1, "rb_mode": 1, "splits": 8, "widen": widen, "reduce": 1})
                cases.append(b.case)
    return cases


def rb2_cases():
    """Mode 2: TN, K = 192 document rows; every element of the dead blocks of both operands is NaN, padding rows inside a live block
    are zero (as the library guarantees)."""
    cases = []
    for nv in NV_LISTS:
        for form_case in (FORM_GEMM, FORM_GROUP):
            b = Builder(f"rb2-{'_'.join(map(str, nv))}-f{form_case}", form_case, 500 + len(cases))
            b.case.ints["rb"] = live_blocks(nv, 64)
            q = b.problem("tn", 64, 128, 192, ("alpha",), 0, 1, rb="rb", rb_mode=2, expect={"interior": 1, "rb_mode": 2, "splits": 1})
            b.case.row_fill = [(q, nv)]
            cases.append(b.case)
    return cases


def apply_row_fill(case, T):
    """mode 2 operands: NaN in dead blocks, zeros on the padding rows of live blocks"""
    for q, nv in getattr(case, "row_fill", []):
        for name, ld, width in (("A", q.lda, q.M), ("B", q.ldb, q.N)):
            buf, off = q.ptr[name]
            for d, n in enumerate(nv):
                for r in range(64):
                    row = d * 64 + r
                    if r >= n:
                        live_block = 16 * (r // 16) < n
                        T[buf][off + row * ld: off + row * ld + width] = 0.0 if live_block else float("nan")


def group_cases():
    cases = []
    ks = (32, 64, 256, 512)
    for n in (2, 9, 11):
        b = Builder(f"group-{n}", FORM_GROUP, 600 + n)
        for i in range(n):
            form = ("nn", "nt", "tn")[i % 3]
            b.problem(form, 64 * (1 + i % 2), 64, ks[i % 4], (("bias",), ("add", "rowscale"), ALL_FEATS)[i % 3], i % 2, (i // 2) % 2,
                      p=0.25 if i % 3 == 2 else 0.0, expect={"interior": 1})
        cases.append(b.case)
    b = Builder("group-guarded-and-empty", FORM_GROUP, 620)
    b.problem("nn", 64, 64, 64, ALL_FEATS, 1, 1, p=0.25, expect={"interior": 1})
    b.problem("nt", 70, 36, 37, ALL_FEATS, 1, 1, p=0.25, expect={"interior": 0})
    b.problem("tn", 0, 64, 64)
    b.problem("tn", 128, 64, 256, ("alpha",), expect={"interior": 1})
    cases.append(b.case)
    # split members sharing one workspace: K = 4096 k-steps ... two members of 64 x 64 x 2048 split 8 ways by the launch's work
    for room, name in ((2, "all"), (1, "first"), (0, "none")):
        b = Builder(f"group-ws-{name}", FORM_GROUP, 630 + room)
        slab = 8 * 64 * 64
        elems = room * slab
        b.buf("ws", elems + 8 + 4096, "out")
        for i in range(2):
            b.problem("tn" if i else "nn", 64, 64, 1536, ALL_FEATS, 1, 1, p=0.25, ws_elems=elems, ws=("ws", 4) if elems else None,
                      expect={"interior": 1, "splits": 8 if elems else 1})
        b.case.ws_split_members = room
        cases.append(b.case)
    return cases


def ride_cases():
    cases = []
    for R in (1, 63, 64, 200):
        for C in (4, 64, 260):
            for split in (0, 1):
                for later in (0, 1):
                    if later and (R, C) not in ((63, 64), (200, 260), (1, 4)):
                        continue
                    b = Builder(f"ride-colsum-R{R}-C{C}-split{split}-later{later}", FORM_GROUP, 700 + len(cases))
                    b.problem("nn", 64, 64, 64, ("bias",), expect={"interior": 1, "splits": 1})
                    if split:
                        b.problem("tn", 64, 64, 1536, (), ws_elems=8 * 64 * 64, expect={"interior": 1, "splits": 8, "reduce": 1})
                    make_ride(b, 1, R, C, col_later=later, later_expected=bool(later and not split))
                    cases.append(b.case)
    for slices, C in ((2, 64), (17, 260), (64, 4)):
        for n in (1, 0):
            b = Builder(f"ride-stage2-s{slices}-C{C}-n{n}", FORM_GROUP, 760 + len(cases))
            if n:
                b.problem("nn", 64, 64, 64, ("bias",), expect={"interior": 1})
            make_ride(b, 2, 0, C, slices=slices)
            cases.append(b.case)
    for n in (1, 0):
        b = Builder(f"ride-headsum-n{n}", FORM_GROUP, 780 + n)
        if n:
            b.problem("nn", 64, 64, 64, ("bias",), expect={"interior": 1})
        make_ride(b, 3, 3, ld=8)
        cases.append(b.case)
    return cases


def park_cases():
    cases = []
    for n in (3, 12, 34):
        b = Builder(f"park-{n}", FORM_PARK, 800 + n)
        accepted = []
        for i in range(n):
            if i == 1:
                b.problem("nt", 70, 36, 37, ("bias",), expect={"interior": 0})
                accepted.append(0)
                continue
            form = ("nn", "nt", "tn")[i % 3]
            b.problem(form, 64, 64 * (1 + i % 2), (64, 256, 32)[i % 3], (("bias",), ALL_FEATS, ("alpha",))[i % 3], i % 2, (i // 2) % 2,
                      p=0.25 if i % 3 == 1 else 0.0, ws_elems=4 * 64 * 128, expect={"interior": 1, "splits": 1})
            accepted.append(1 if sum(accepted) < DEFER_CAP else 0)
        b.case.accepted = accepted
        cases.append(b.case)
    return cases


def pair_cases():
    cases = []
    for form_case, tag in ((FORM_PAIR_WX, "wx"), (FORM_PAIR_WW, "ww"), (FORM_PAIR_XX, "xx")):
        for (Nw, Kw), shape in (((64, 64), "interior"), ((40, 24), "guarded")):
            for cap in (64, 200, 512):
                for count in sorted({0, 1, 63, 64, 65, cap}):
                    if count > cap or (cap == 512 and count in (63, 64)):
                        continue
                    b = Builder(f"pair-{tag}-{shape}-cap{cap}-n{count}", form_case, 900 + len(cases))
                    R = (cap + 63) // 64 * 64
                    b.case.cnt, b.case.cap = count, cap
                    hi = (count + 63) // 64 * 64 if shape == "interior" else count
                    fused = shape == "interior" and (tag == "xx" or cap == 512)
                    for i, dyn in enumerate({"wx": (2, 1), "ww": (2, 2), "xx": (1, 1)}[tag]):
                        if dyn == 2:     # a weight gradient dW [Kw x Nw] = dY[:count]^T X[:count]; a capacity of 512 rows is cut in two
                            if i == 1:   # the first problem's workspace holds both problems' partials
                                q = b.problem("tn", Kw, Nw, 0, ("alpha",), 0, 1, alloc_K=R, ws_elems=0,
                                              expect={"zero_fill": 0 if fused else 1, "fused": int(fused)})
                            else:
                                q = b.problem("tn", Kw, Nw, 0, ("alpha",), 0, 0, alloc_K=R, ws_elems=2 * 2 * Kw * Nw,
                                              expect={"zero_fill": int(cap < 512), "fused": int(fused)})
                            q.dyn = 2
                            # rows [count, roundup64) of A are zero (gemm.hpp); rows past that are never read: NaN
                            b.case.zero_rows = getattr(b.case, "zero_rows", []) + [(q, "A", count, hi)]
                            for name, ld in (("A", q.lda), ("B", q.ldb)):
                                b.case.nan_rows.append((q.ptr[name][0], q.ptr[name][1] + hi * ld, (R - hi) * ld))
                        else:            # a data gradient dX[:count] = dY[:count] W
                            q = b.problem("nn", 0, Nw, Kw, ("bias",), 0, i, alloc_M=R, expect={"fused": int(fused)})
                            q.dyn = 1
                            b.case.zero_rows = getattr(b.case, "zero_rows", []) + [(q, "A", count, hi)]
                            b.case.nan_rows.append((q.ptr["A"][0], q.ptr["A"][1] + hi * q.lda, (R - hi) * q.lda))
                    b.case.interior = shape == "interior"
                    cases.append(b.case)
    return cases


def apply_zero_rows(case, T):
    for q, name, lo, hi in getattr(case, "zero_rows", []):
        buf, off = q.ptr[name]
        T[buf][off + lo * q.lda: off + hi * q.lda] = 0.0


def tensors_of(case):
    T = make_tensors(case)
    apply_row_fill(case, T)
    apply_zero_rows(case, T)
    return T


GROUPS = {"epilogue": epilogue_cases, "batches": batch_cases, "splitk": splitk_cases, "rb1": rb1_cases, "rb2": rb2_cases,
          "group": group_cases, "ride": ride_cases, "park": park_cases, "pairs": pair_cases}


def all_cases():
    return [(g, c) for g, make in GROUPS.items() for c in make()]
