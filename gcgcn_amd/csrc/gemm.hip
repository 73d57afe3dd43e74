// Batched exact-fp32 GEMM for gfx950: v_mfma_f32_32x32x2_f32 tiles, k-major LDS images,
// register-prefetch double buffering, split-K with a deterministic reduce, fused epilogue (gemm.hpp).
//
// Block = 256 threads = 4 waves in a 2x2 arrangement; a wave owns (32*TM) x (32*TN) outputs,
// i.e. TM*TN accumulator tiles of 32x32 (16 VGPRs each).  BK = 32.
//
// LDS images are k-major: As[k][m], Bs[k][n].  The MFMA operand of lane l is
//   a = A[i = l & 31][k = l >> 5],  b = B[k = l >> 5][j = l & 31]
// so each half-wave reads 32 consecutive floats of one k-row: conflict-free ds_read_b32.
// A k-contiguous source (A as [M][K], B as [N][K]) is read 128 B per row (8 lanes x 16 B) and
// transposed on the LDS write; its row stride is BMN + 1 so that the 4-byte stores of the
// 4 rows x 8 k-quads handled by a 32-lane group fall on 32 different banks.
//
// The problems on this path are small (M = B*N ~ 2048, N, K in {64..2048}); an f32 MFMA tile
// takes 64 cycles, so a 64x64x32 step is only ~0.4 us of matrix work against ~1 us of load
// latency.  Throughput therefore comes from residency, not from big tiles: 64x64 blocks at
// 3-5 blocks per CU, and split-K (partials to a workspace + one reduce/epilogue kernel,
// bitwise reproducible) when M*N alone gives fewer than ~3 blocks per CU.
//
// Codegen note (ROCm 7.2): per-lane guarded float4 loads get if-converted into predicated
// scalar loads with a vmcnt(0) at the loop head.  The interior path (ALIGNED) is therefore a
// separate instantiation with unconditional 16-byte loads; ragged shapes take the guarded one.
#include <stdlib.h>

#include "attn_plan.hpp"
#include "edge_body.hpp"
#include "gemm_body.hpp"
#include "mha_body.hpp"
#include "rowops.hpp"

namespace gc {

template <int TM, int TN, bool AKC, bool BKC, bool ALIGNED, bool RB = false>
__global__ __launch_bounds__(256, (TM * TN == 4 ? 2 : 1)) void gemm_kernel(const GemmArgs g) {
  __shared__ __attribute__((aligned(16))) float lds[lds_floats<TM, TN, AKC, BKC>()];
  const int gx = gridDim.x, gy = gridDim.y;
  const int nwg = gx * gy * gridDim.z;
  const int q = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
  if (RB && g.rb && g.rb_mode == 1) {   // ragged batch: the live tile rows in XCD-balanced order, then the dead ones (gemm_body.hpp)
    int bx, by, zs, wide;
    if (!tile_of_rows(g, q, gx, gy, bx, by, zs, wide)) return;
    gemm_body<TM, TN, AKC, BKC, ALIGNED, GC_GEMM_EG, 0, EPI_ALL, PlainOperands, RB>(g, lds, bx, by, zs, threadIdx.x, true, PlainOperands(), nullptr, 0, wide);
    return;
  }
  const int b = xcd_remap(q, nwg);
  gemm_body<TM, TN, AKC, BKC, ALIGNED, GC_GEMM_EG, 0, EPI_ALL, PlainOperands, RB>(g, lds, b % gx, (b / gx) % gy, b / (gx * gy));
}

// Stage 1 of a riding column sum: workgroup cb sums one slice of rows for 64 columns (4 waves stride the rows,
// lanes own columns, 8 independent loads in flight per lane).
__device__ __forceinline__ void col_ride_stage1(const ColRide& cr, int cb, float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ncb = (cr.C + 63) >> 6;
  const int sp = cb / ncb, c = (cb - sp * ncb) * 64 + lane;
  const long rps = (cr.R + COL_RIDE_SLICES - 1) / COL_RIDE_SLICES;
  const long r0 = sp * rps, r1 = min(cr.R, r0 + rps);
  float acc = 0.f;
  if (c < cr.C) {
    long r = r0 + wave;
    for (; r + 28 < r1; r += 32) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = cr.X[(r + 4 * u) * cr.ld + c];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; r < r1; r += 4) acc += cr.X[r * cr.ld + c];
  }
  red[wave * 64 + lane] = acc;
  __syncthreads();
  if (wave == 0 && c < cr.C) cr.part[(long)sp * cr.C + c] = (red[lane] + red[64 + lane]) + (red[128 + lane] + red[192 + lane]);
}

// Several independent problems in ONE launch (64x64 tiles, interior shapes only): block -> problem by
// prefix sums of tile counts, layout chosen per problem by a block-uniform branch.
// Problems are laid out longest-K first and every problem starts at a workgroup id that is a multiple of 8, so
// that the XCD-contiguous remap can be applied PER PROBLEM: each XCD receives an equal, contiguous share of every
// problem's tile list.  (One remap over the whole launch would hand XCD 0 the longest problem and XCD 7 the
// shortest.)  The <= 7 padding workgroups per problem exit at once.
// workgroup `idx` past the GEMM tiles (dispatched last, round-robin over the XCDs): the riding column sum
__device__ __forceinline__ void group_tail(const GemmGroup& gg, const int idx, float* __restrict__ lds) {
  const ColRide& cr = gg.col;
  if (cr.ready_slices < 0) {  // sum over heads (sum_h Wlin[:, h, :] for the fused chain backward), eight loads in flight
    const int e = idx * 256 + threadIdx.x;
    if (e < cr.C) {
      const int ld = (int)cr.ld, H = (int)cr.R, k = e / ld, c = e - k * ld;
      float s = 0.f;
      for (int h0 = 0; h0 < H; h0 += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = cr.X[((long)k * H + min(h0 + u, H - 1)) * ld + c];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += (h0 + u < H) ? v[u] : 0.f;
      }
      cr.out[e] = s;
    }
    return;
  }
  if (cr.ready_slices > 0) {  // partial sums from an earlier launch: out[c] = their sum, slices in order
    col_ride_stage2_block(cr, idx);
    return;
  }
  col_ride_stage1(cr, idx, lds);
}

template <bool RB>
__global__ __launch_bounds__(256, 4) void gemm_group_kernel(const GemmGroup gg) {
  __shared__ __attribute__((aligned(16))) float lds[lds_floats<1, 1, true, true>()];
  const int tiles = gg.tile_begin[gg.nprob];
  if ((int)blockIdx.x >= tiles) {
    group_tail(gg, blockIdx.x - tiles, lds);
    return;
  }
  gemm_group_block<RB>(gg, blockIdx.x, lds);
}

// The same launch with MultiHeadAttention's backward core aboard: mp.count (document, head) pairs spread EVENLY through the
// tile list (behind the tiles they would start when the list has nearly drained and stretch the launch by their own latency).
template <bool RB>
__global__ __launch_bounds__(256, 4) void gemm_group_pass_kernel(const GemmGroup gg, const MhaPass mp) {
  __shared__ __attribute__((aligned(16))) float lds[lds_floats<1, 1, true, true>()];
  const int tiles = gg.tile_begin[gg.nprob], inter = tiles + mp.count;
  const int x = blockIdx.x;
  if (x >= inter) {
    group_tail(gg, x - inter, lds);
    return;
  }
  const int before = (int)((long)x * mp.count / inter);   // pairs among the workgroups [0, x)
  if ((int)((long)(x + 1) * mp.count / inter) > before) {
    mha_core_bwd_body(lds, before, mp.Q, mp.P, mp.dA, mp.dQ, mp.N, mp.D, mp.H, mp.dh, mp.kchunk, mp.alpha, mp.drop);
    return;
  }
  gemm_group_block<RB>(gg, x - before, lds);
}

// Split-K reduce: one thread sums the partials of 4 consecutive outputs (16-byte loads, split order => bitwise
// reproducible) and runs the epilogue.  N % 4 == 0 is guaranteed for split problems (they are interior shapes).
__device__ __forceinline__ void reduce4(const GemmArgs& g, int z, long idx4) {
  const long mn = (long)g.M * g.N;
  const long idx = idx4 * 4;
  if (idx >= mn) return;
  const long nb = (long)g.batch1 * g.batch2;
  int row = (int)(idx / g.N);
  const int col = (int)(idx - (long)row * g.N);
  const int z1 = z / g.batch2, z2 = z - z1 * g.batch2;
  int nsplit = g.splits;
  if (g.rb && g.rb_mode == 1) {  // ragged batch: virtual row -> its place in the padded tensors; rows past the live blocks
    const int bi = row >> 4;     // are zero-stored (outputs that leave the block) or left alone
    const int prow = g.rb[bi] * 16 + (row & 15);
    const int tm = (g.M + 63) >> 6;
    nsplit *= split_width(g, min((*g.rb_n + 3) >> 2, tm), tm);   // the tile workgroups cut K this much finer (gemm_body.hpp)
    if (bi >= *g.rb_n) {
      if (g.rb_zero) {
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        float* c = g.C + z1 * g.sC1 + z2 * g.sC2 + (long)prow * g.ldc + col;
        c[0] = 0.f, c[1] = 0.f, c[2] = 0.f, c[3] = 0.f;
        if (g.C2) {
          float* c2 = g.C2 + z1 * g.sC21 + z2 * g.sC22 + (long)prow * g.ldc2 + col;
          c2[0] = zero.x, c2[1] = zero.y, c2[2] = zero.z, c2[3] = zero.w;
        }
      }
      return;
    }
    row = prow;
  }
  const float4* w = reinterpret_cast<const float4*>(g.ws + (long)z * mn + idx);
  const long stride4 = nb * mn / 4;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  // split order, eight slabs requested together (one at a time the loop is `splits` dependent round trips: a 64-way split of the
  // classifier head's dynamic-K weight gradients took 20 us on 16 workgroups)
  if (nsplit <= 4) {   // (the block path's factors: the plain loop -- batches with clamped re-reads cost cfg 2 0.4 %)
    for (int s = 0; s < nsplit; ++s) {
      const float4 v = w[(long)s * stride4];
      acc.x += v.x, acc.y += v.y, acc.z += v.z, acc.w += v.w;
    }
  } else {
    for (int s0 = 0; s0 < nsplit; s0 += 8) {
      float4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = w[(long)min(s0 + u, nsplit - 1) * stride4];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (s0 + u < nsplit) acc.x += v[u].x, acc.y += v[u].y, acc.z += v[u].z, acc.w += v[u].w;
    }
  }
  if (!(g.add || g.bias || g.rowadd || g.rowscale || g.relu || g.accumulate || g.n_valid || g.C2) && g.alpha == 1.f) {
    float* c = g.C + z1 * g.sC1 + z2 * g.sC2 + (long)row * g.ldc + col;
    if ((((uintptr_t)c) & 15) == 0) {
      *reinterpret_cast<float4*>(c) = acc;
    } else {
      c[0] = acc.x, c[1] = acc.y, c[2] = acc.z, c[3] = acc.w;
    }
    return;
  }
  const Epi e = make_epi(g, z1, z2);
  epi_store4(g, e, row, col, acc);
}

__global__ __launch_bounds__(256) void splitk_reduce_group_kernel(const GemmGroup gg) {
  int b = blockIdx.x, i = 0;
  if (b >= gg.red_begin[gg.nprob]) {  // stage 2 of the riding column sum, slices in order
    const ColRide& cr = gg.col;
    const int c = (b - gg.red_begin[gg.nprob]) * 256 + threadIdx.x;
    if (c < cr.C) {
      float s = 0.f;
      for (int q = 0; q < COL_RIDE_SLICES; ++q) s += cr.part[(long)q * cr.C + c];
      cr.out[c] = s;
    }
    return;
  }
  while (i + 1 < gg.nprob && b >= gg.red_begin[i + 1]) ++i;
  b -= gg.red_begin[i];
  const GemmArgs& g = gg.p[i];
  if (g.splits <= 1) return;
  const int per = (int)(((long)g.M * g.N / 4 + 255) / 256);
  const int z = b / per;
  reduce4(g, z, (long)(b - z * per) * 256 + threadIdx.x);
}

// Sum the split-K partials in split order (bitwise reproducible) and run the epilogue.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const GemmArgs g) {
  reduce4(g, blockIdx.y, (long)blockIdx.x * 256 + threadIdx.x);
}

int splitk_reduce(const GemmArgs& g, hipStream_t st, const char* what) {
  ProfScope ps("gemm_splitk_reduce", st);
  dim3 rgrid(cdiv((long)g.M * g.N / 4, 256), g.batch1 * g.batch2);
  hipLaunchKernelGGL(splitk_reduce_kernel, rgrid, dim3(256), 0, st, g);
  return check_launch(what);
}

static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
// 64 x 64 output tiles (batches included, splits not), tile-k-steps and flops of a problem
static long tiles_of(const GemmArgs& g) { return (long)cdiv(g.M, 64) * cdiv(g.N, 64) * g.batch1 * g.batch2; }
static long work_of(const GemmArgs& g) { return tiles_of(g) * cdiv(g.K, BK); }
static double flops_of(const GemmArgs& g) { return 2.0 * g.M * g.N * g.K * g.batch1 * g.batch2; }

// Split factor of a problem inside a launch whose 64x64 tiles carry `work` tile-k-steps in total: no
// workgroup should run much longer than the average load of one of the 256 x 4 resident slots
// (a K = 2048 tile next to K = 256 tiles would otherwise drain alone), and a launch that cannot fill
// the slots at all is cut until its blocks are ~8 k-steps long.
static int pick_splits(int K, long work) {
  constexpr int thr_pct = 250;  // percent of the average slot load
  const long iters = cdiv(K, BK);
  long thr = work / 1024 * thr_pct / 100;
  if (thr < 8) thr = 8;
  int splits = 1;
  while (iters / splits > thr && splits < 16 && K % (splits * 2 * BK) == 0) splits *= 2;
  return splits;
}
// Split factor of a weight gradient whose K is a device-side count of at most `cap`: enough K slices to fill the chip with its few
// output tiles; each slice >= 8 k-steps
static int dyn_splits(long tiles, long cap) {
  long want = (1024 + tiles - 1) / tiles, most = cap / (8 * BK);
  if (most < 1) most = 1;
  const long splits = want < most ? want : most;
  return (int)(splits > 64 ? 64 : splits);
}
// the workspace takes `slabs` partial [M x N] images for the reduce's 16-byte loads
static bool ws_holds(const GemmArgs& g, long slabs) { return g.ws && slabs * g.M * g.N <= g.ws_elems && g.N % 4 == 0 && aligned16(g.ws); }

// ---- what the launcher decides for one problem: here and nowhere else (gcgcn_debug_gemm_plan shows the result) ----------------
enum GemmForm {    // who asks
  GEMM_SINGLE,     // gemm(): the caller's split request, the problem's own work
  GEMM_MEMBER,     // a problem of a gemm_group launch: split by the whole launch's work
  GEMM_PARK,       // gemm_defer: unsplit
  GEMM_DYN_M,      // gemm_dyn and the pairs: M, or K, is a device-side count of at most `cap`
  GEMM_DYN_K
};
struct GemmPlan {
  bool ok;         // false: the problem is refused (set_error has the reason)
  bool interior;   // the unguarded tile body: 16-byte loads, whole tiles, whole k-steps
  int splits, ksplit, widen;   // as written to GemmArgs
  int rb_mode;     // the row-block list is kept (1 / 2), or the problem runs dense (0)
  long tiles;      // tiles_of
  bool reduce;     // a split-K reduce launch follows
  bool zero_fill;  // device-side K, unsplit: gemm_dyn_zero_kernel defines C for a count of zero
  int grid;        // device-side forms: the persistent workgroups that walk the tile list
};
// Checks the problem, fills the launcher-owned fields of g (vecA, vecB, splits, ksplit, widen; a device-side form's capped dimension)
// and drops the row-block list where the problem runs dense.  `splits` counts for GEMM_SINGLE, `group_work` for GEMM_MEMBER, `cap` for
// the device-side forms.
static GemmPlan gemm_plan(GemmArgs& g, GemmForm form, int splits, long group_work, long cap) {
  GemmPlan p = {};
  const bool dyn = form == GEMM_DYN_M || form == GEMM_DYN_K;
  const long nb = (long)g.batch1 * g.batch2;
  if (dyn && nb != 1) { set_error("gemm_dyn: batched problems are not supported"); return p; }
  if (dyn && cap == 0) cap = 1;
  // the count's bound, rounded up to whole tiles, stands in for the dimension: what may run unguarded reads that far (gemm.hpp)
  if (dyn) (form == GEMM_DYN_M ? g.M : g.K) = (int)((cap + 63) & ~63L);
  if (!(g.A && g.B && g.C)) { set_error("gemm: null operand"); return p; }
  if (!(g.M >= 0 && g.N >= 0 && g.K >= 1 && g.batch1 >= 1 && g.batch2 >= 1)) { set_error("gemm: bad shape"); return p; }
  {  // the epilogue addresses one (batch entry's) [M x ld] slice with 32-bit offsets
    long ldmax = g.ldc;
    if (g.add && g.ldadd > ldmax) ldmax = g.ldadd;
    if (g.C2 && g.ldc2 > ldmax) ldmax = g.ldc2;
    if (g.add2 && g.ldadd2 > ldmax) ldmax = g.ldadd2;
    if ((long)g.M * ldmax >= (1L << 32)) { set_error("gemm: M * ld = %ld exceeds 32-bit epilogue offsets", (long)g.M * ldmax); return p; }
  }
  const bool widen_on = option("split_widen", 1) != 0;
  g.vecA = aligned16(g.A) && g.lda % 4 == 0 && g.sA1 % 4 == 0 && g.sA2 % 4 == 0;
  g.vecB = aligned16(g.B) && g.ldb % 4 == 0 && g.sB1 % 4 == 0 && g.sB2 % 4 == 0;
  p.tiles = tiles_of(g);
  if (form != GEMM_SINGLE) splits = form == GEMM_MEMBER ? 0 : 1;   // parked tiles run their whole K in one workgroup; a device-side K is cut below
  if (splits == 0) {
    splits = pick_splits(g.K, form == GEMM_MEMBER ? group_work : work_of(g));
    // The host never reads n_valid: a long-K problem on the row blocks of a ragged batch that "fills the chip" by its dense tile
    // count (cfg 3's K = 3072 data gradients: 768 tiles, three per compute unit, unsplit) runs with fewer than half of them live,
    // one to a compute unit, at a lone workgroup's pace (336 live tiles of 96 k-tiles: 109 us).  Split it once here; what the launch
    // really finds is dealt with on the device (split_width cuts finer with the workgroups of the dead rows).  Counting every
    // row-block problem at half its dense work instead split the short ones too: cfg 2 ragged 78.0k -> 71.9k docs/s.
    // (Applied before the row-block rule below has had its say: a problem that then runs dense -- a batched one, a small one -- stays
    // split.  Looks like an accident and is left for a measured change.)
    if (splits == 1 && g.rb && g.rb_mode == 1 && cdiv(g.K, BK) >= 48 && p.tiles <= 1024 && g.K % (2 * BK) == 0 && widen_on) splits = 2;
  }
  if (splits > 1 && !(ws_holds(g, splits * nb) && g.K % (splits * BK) == 0)) splits = 1;
  g.splits = splits;
  g.ksplit = (splits > 1) ? g.K / splits : g.K;
  // One predicate for every form: ksplit is K for an unsplit problem and a divisor of K whose multiple of BK divides K for a split
  // one, and a device-side form's capped dimension is a multiple of 64 by now.
  p.interior = g.vecA && g.vecB && g.M % 64 == 0 && g.N % 64 == 0 && g.ksplit % BK == 0;
  if (g.rb) {  // row blocks of a ragged batch: only what the gathering tile body serves, anything else runs dense (equally correct)
    const bool served = p.interior && g.rb_n && ((g.rb_mode == 1 && g.a_kc && nb == 1) ||
                                                  (g.rb_mode == 2 && !g.a_kc && !g.b_kc && g.K % 64 == 0 && g.K / 16 <= ROWBLK_LIST_MAX));
    // M-side: a launch that does not fill the chip anyway gains nothing from skipping tiles and pays the list's lookups in
    // its latency-bound prologue (128-tile output projection: 21 vs 16 us measured) -- dense below one tile per compute unit
    // and slot (a problem inside a group launch shares the launch and keeps the list)
    const bool small = g.rb_mode == 1 && form != GEMM_MEMBER && (long)cdiv(g.M, 64) * cdiv(g.N, 64) * splits <= 256;
    if (!served || small) g.rb = nullptr, g.rb_n = nullptr, g.rb_mode = 0, g.rb_zero = 0;
  }
  // a split row-block problem may cut K finer on the device (split_width): as far as the workspace holds the slabs
  g.widen = 1;
  if (g.rb && g.rb_mode == 1 && g.splits > 1 && widen_on)
    while (g.widen < 4 && (long)g.splits * 2 * g.widen * nb * g.M * g.N <= g.ws_elems) g.widen *= 2;
  if (form == GEMM_DYN_K) {  // the device cuts K by the count it finds (gemm_dyn_walk): any factor the workspace holds, ksplit stays K here
    g.splits = dyn_splits(p.tiles, cap);
    if (g.splits > 1 && !ws_holds(g, g.splits)) g.splits = 1;
    p.zero_fill = g.splits == 1;
  }
  if (dyn) {  // at most one workgroup per resident slot
    const long walk = form == GEMM_DYN_M ? (long)cdiv(cap, 64) * cdiv(g.N, 64) : p.tiles * g.splits;
    p.grid = (int)(walk < 1024 ? (walk > 0 ? walk : 1) : 1024);
  }
  p.ok = true;
  p.splits = g.splits, p.ksplit = g.ksplit, p.widen = g.widen;
  p.rb_mode = g.rb ? g.rb_mode : 0;
  p.reduce = g.splits > 1;
  return p;
}
// The members of a group launch share one workspace, each split one taking the next slice: fewer device-side slabs where the widened
// ones do not fit, unsplit where none do.  Returns whether the member stays split.
static bool gemm_plan_slice(GemmArgs& g, long& ws_used) {
  if (g.splits <= 1) return false;
  const long slab = (long)g.splits * g.batch1 * g.batch2 * g.M * g.N;
  while (g.widen > 1 && ws_used + slab * g.widen > g.ws_elems) g.widen /= 2;
  if (ws_used + slab * g.widen > g.ws_elems) {  // no room left: this problem goes unsplit
    g.splits = 1, g.ksplit = g.K, g.widen = 1;
    return false;
  }
  g.ws = g.ws + ws_used;
  ws_used += slab * g.widen;
  return true;
}

// gemm_kernel by [dense][guarded][A stored K x M][b_kc], in the order the code object has always held them.  The row-block paths
// exist for what gemm_plan keeps the list for: interior problems with A stored [M][K] (mode 1) or both operands stored [K][.] (mode 2).
using GemmKernel = void (*)(const GemmArgs);
static const GemmKernel gemm_kernels[2][2][2][2] = {
    {{{gemm_kernel<1, 1, true, false, true, true>, gemm_kernel<1, 1, true, true, true, true>}, {gemm_kernel<1, 1, false, false, true, true>, nullptr}},
     {{nullptr, nullptr}, {nullptr, nullptr}}},
    {{{gemm_kernel<1, 1, true, false, true>, gemm_kernel<1, 1, true, true, true>}, {gemm_kernel<1, 1, false, false, true>, gemm_kernel<1, 1, false, true, true>}},
     {{gemm_kernel<1, 1, true, false, false>, gemm_kernel<1, 1, true, true, false>}, {gemm_kernel<1, 1, false, false, false>, gemm_kernel<1, 1, false, true, false>}}}};

static int launch(const GemmArgs& g, const GemmPlan& p, hipStream_t stream) {
  const GemmKernel kernel = gemm_kernels[p.rb_mode == 0][!p.interior][!g.a_kc][g.b_kc != 0];
  GC_REQUIRE(kernel && (p.rb_mode == 0 || (p.rb_mode == 1) == (g.a_kc != 0)), "gemm: no kernel for a_kc %d b_kc %d row-block mode %d %s", g.a_kc,
             g.b_kc, p.rb_mode, p.interior ? "interior" : "guarded");
  dim3 grid(cdiv(g.N, 64), cdiv(g.M, 64), g.batch1 * g.batch2 * g.splits), block(256);
  GC_LAUNCH_TIMED(g.tag, flops_of(g), kernel, grid, block, 0, stream, g);
  if (int e = check_launch("gemm")) return e;
  return p.reduce ? splitk_reduce(g, stream) : 0;
}

int gemm(const GemmArgs& g_in, hipStream_t stream, int tile, int splits) {
  GemmArgs g = g_in;
  if (g.M == 0 || g.N == 0) return 0;
  GC_REQUIRE(tile == 0 || tile == 1, "gemm: tile %d (64 x 64 tiles are the only body; 128 x 128 bodies lost every A/B on this path)", tile);
  const GemmPlan p = gemm_plan(g, GEMM_SINGLE, splits, 0, 0);
  if (!p.ok) return 1;
  const long nb = (long)g.batch1 * g.batch2;
  GC_REQUIRE(nb * g.splits <= 65535, "gemm: batch %ld x splits %d exceeds grid.z", nb, g.splits);
  GC_REQUIRE(cdiv(g.M, 64) <= 65535, "gemm: M %d exceeds grid.y", g.M);
  if (option("group_dump", 0))   // diagnosis (with the group launches' dump)
    fprintf(stderr, "gemm: %-12s M %5d N %5d K %5d batch %3ld splits %2d a_kc %d b_kc %d rb_mode %d %s\n", g.tag, g.M, g.N, g.K, nb, g.splits,
            g.a_kc, g.b_kc, p.rb_mode, p.interior ? "interior" : "guarded");
  return launch(g, p, stream);
}

// Independent problems in one launch (plus at most one reduce launch).  Problems that are not interior
// 64x64 shapes fall back to their own launches.
// The head-feature chunk with which a (document, head) pair's scratch (score tile + one chunk of Q_h) fits a tile workgroup's
// LDS: the stand-alone kernel's chunk, or 0.  (A shorter chunk would fit wide heads too -- 32 features at a time for cfg 3's 192
// -- but such passengers use two of their four waves and run six dependent passes: the group launch grew by 45 us to save a
// 23 us launch.  Measured, not kept.)
int gemm_group_mha_chunk(int dh) {
  const size_t room = sizeof(float) * lds_floats<1, 1, true, true>();
  const int c = mha_chunk(dh);
  return mha_lds_bytes_of(c) <= room ? c : 0;
}

// What rides in the trailing workgroups of a group launch: which constructor of gemm.hpp built the ColRide (the kernels read
// ready_slices themselves)
enum RideKind {
  RIDE_NONE,
  RIDE_COLSUM,   // col_sum: stage 1 of a column sum here, stage 2 in the reduce launch (or with the caller: col_later)
  RIDE_STAGE2,   // .stage2: the partials of an earlier launch are summed here
  RIDE_HEADS     // head_sum: the sum over heads -- no partials, no second stage
};
static RideKind ride_kind(const ColRide* col) {
  if (!col || col->C <= 0) return RIDE_NONE;
  if (col->ready_slices != 0) return col->ready_slices < 0 ? RIDE_HEADS : RIDE_STAGE2;
  return col->X && col->R > 0 ? RIDE_COLSUM : RIDE_NONE;
}
// the instantiation with the row-block paths if any problem of the launch walks row blocks
template <class Kernel>
static Kernel by_row_blocks(const GemmGroup& gg, Kernel with, Kernel without) {
  for (int i = 0; i < gg.nprob; ++i)
    if (gg.p[i].rb) return with;
  return without;
}

int col_sum_stage2_launch(const ColRide& c, hipStream_t stream) {
  return colsum(c.part, nullptr, c.out, c.ready_slices, c.C, c.C, 1, 0, 0, 0, 0, nullptr, stream);
}

int gemm_group(const GemmArgs* probs, int n, hipStream_t stream, const ColRide* col, bool* col_later, const MhaPass* mha) {
  if (col_later) *col_later = false;
  GemmGroup gg;
  gg.nprob = 0;
  long work = 0;  // tile-k-steps of the whole launch
  for (int i = 0; i < n; ++i) work += work_of(probs[i]);
  int tiles = 0, reds = 0;
  double flops = 0;
  bool any_split = false;
  long ws_used = 0;
  // longest blocks first: workgroups are dispatched in tile order, and a K = 2048 tile started last would
  // run alone long after the K = 256 tiles of the same launch have drained
  int order[64];
  GC_REQUIRE(n <= 64, "gemm_group: too many problems");
  for (int i = 0; i < n; ++i) order[i] = i;
  for (int i = 1; i < n; ++i)
    for (int j = i; j > 0 && probs[order[j]].K > probs[order[j - 1]].K; --j) {
      const int t = order[j];
      order[j] = order[j - 1], order[j - 1] = t;
    }
  // pass 1: fix every problem's split factor and count its workgroups
  GemmArgs prep[64];
  bool groupable[64];
  int ng = 0;
  for (int oi = 0; oi < n; ++oi) {
    GemmArgs& g = prep[oi];
    g = probs[order[oi]];
    groupable[oi] = false;
    if (g.M == 0 || g.N == 0) continue;
    const GemmPlan p = gemm_plan(g, GEMM_MEMBER, 0, work, 0);
    if (!p.ok) return 1;
    groupable[oi] = p.interior && ng < GemmGroup::MAXP;
    if (groupable[oi]) ++ng;
  }
  // (Until round 5 a launch that overflowed the 1024 resident slots by <= 128 workgroups had its smallest problem peeled into a
  // launch of its own -- "a whole extra round for a few workgroups".  With the tile order and the kernels of this round the
  // separate launch costs more than the tail: cfg 2's Q projection, 128 tiles, was an 11 us launch in front of a 2048-tile
  // group; inside it the step is 0.5066 against 0.5124 ms, ragged 0.4085 against 0.4142, cfg 3 / cfg 5 -0.2 / -0.4 %, cfg 1 a
  // tie.  The rule is gone.)
  // pass 2: ungroupable problems first (own launches), then the group
  for (int oi = 0; oi < n; ++oi) {
    if (groupable[oi] || probs[order[oi]].M == 0 || probs[order[oi]].N == 0) continue;
    if (int e = gemm(probs[order[oi]], stream)) return e;
  }
  for (int oi = 0; oi < n; ++oi) {
    if (!groupable[oi]) continue;
    GemmArgs g = prep[oi];
    if (gemm_plan_slice(g, ws_used)) any_split = true;
    const int own = (int)(tiles_of(g) * g.splits);
    tiles = (tiles + 7) & ~7;
    gg.tile_begin[gg.nprob] = tiles;
    gg.tile_count[gg.nprob] = own;
    gg.tile_first[gg.nprob] = 0, gg.tile_take[gg.nprob] = own;
    gg.red_begin[gg.nprob] = reds;
    tiles += own;
    if (g.splits > 1) reds += g.batch1 * g.batch2 * cdiv((long)g.M * g.N / 4, 256);
    flops += flops_of(g);
    gg.p[gg.nprob++] = g;
  }
  if (option("group_dump", 0)) {   // diagnosis: what each group launch is made of
    fprintf(stderr, "gemm_group: %d problems, %d tile workgroups, mha pairs %d\n", gg.nprob, tiles, mha ? mha->count : 0);
    for (int i = 0; i < gg.nprob; ++i) {
      const GemmArgs& g = gg.p[i];
      fprintf(stderr, "  %-12s M %5d N %5d K %5d batch %3d splits %2d (widen %d) a_kc %d b_kc %d rb_mode %d tiles %5d\n", g.tag, g.M, g.N, g.K,
              g.batch1 * g.batch2, g.splits, g.widen, g.a_kc, g.b_kc, g.rb ? g.rb_mode : 0, gg.tile_count[i]);
    }
  }
  const RideKind ride = ride_kind(col);
  if (ride == RIDE_COLSUM || ride == RIDE_STAGE2) GC_REQUIRE(col->out && col->part, "gemm_group: column ride without out / part");
  if (ride == RIDE_HEADS) GC_REQUIRE(col->X && col->out && col->R > 0 && col->ld > 0 && col->C == col->ld * col->ld, "gemm_group: bad head sum");
  static_assert(sizeof(GemmGroup) + sizeof(MhaPass) + 32 <= 4096, "gemm_group_pass_kernel: kernel arguments exceed 4 KB");
  if (gg.nprob == 0 && mha && mha->count > 0)   // nothing to ride on: the pairs get their launch
    if (int e = mha_core_bwd(*mha, stream)) return e;
  if (gg.nprob == 0) {  // nothing to ride on
    if (ride == RIDE_HEADS) return mask_rows(nullptr, nullptr, 0, (int)col->ld, 1, nullptr, make_drop(nullptr, 0, 0.f), stream, col->X, col->out, (int)col->R);
    if (ride == RIDE_STAGE2) return col_sum_stage2_launch(*col, stream);
    return ride == RIDE_COLSUM ? colsum(col->X, nullptr, col->out, col->R, col->C, col->ld, 1, 0, 0, 0, 0, col->part, stream) : 0;
  }
  gg.tile_begin[gg.nprob] = tiles;
  gg.red_begin[gg.nprob] = reds;
  int col1 = 0, col2 = 0;   // trailing workgroups of the launch and of its reduce
  if (ride != RIDE_NONE) gg.col = *col;
  if (ride == RIDE_COLSUM) col1 = cdiv(col->C, 64) * COL_RIDE_SLICES, col2 = cdiv(col->C, 256);
  else if (ride != RIDE_NONE) col1 = cdiv(col->C, 256);
  if (mha && mha->count > 0)
    GC_LAUNCH_TIMED("gemm_group", flops, by_row_blocks(gg, gemm_group_pass_kernel<true>, gemm_group_pass_kernel<false>),
                    dim3(tiles + mha->count + col1), dim3(256), 0, stream, gg, *mha);
  else
    GC_LAUNCH_TIMED("gemm_group", flops, by_row_blocks(gg, gemm_group_kernel<true>, gemm_group_kernel<false>), dim3(tiles + col1), dim3(256), 0,
                    stream, gg);
  if (int e = check_launch("gemm_group")) return e;
  if (ride == RIDE_COLSUM && !any_split && col_later) {  // nothing to reduce: the caller folds stage 2 into a kernel of its own
    *col_later = true;
    return 0;
  }
  if (any_split || ride == RIDE_COLSUM) {
    ProfScope ps("gemm_splitk_reduce", stream);
    hipLaunchKernelGGL(splitk_reduce_group_kernel, dim3(reds + col2), dim3(256), 0, stream, gg);
    return check_launch("gemm_group_reduce");
  }
  return 0;
}

// ---- one dimension known only on the device (gemm.hpp) --------------------------------------------------------
// vb / vgrid: this workgroup's index and the number of workgroups walking the problem's tile list (the whole grid, or one
// problem's share of a pair launch)
template <bool AKC, bool BKC, bool ALIGNED>
__device__ __forceinline__ void gemm_dyn_walk(GemmArgs& g, float* __restrict__ lds, const int* __restrict__ cnt, const int dyn,
                                              const int splits, const int vb, const int vgrid) {
  const int c = *cnt;
  const int cr = ALIGNED ? (c + 63) & ~63 : c;
  if (dyn == 1) {
    g.M = cr, g.splits = 1, g.ksplit = g.K;
    const int tn = (g.N + 63) >> 6, tiles = ((cr + 63) >> 6) * tn;
    for (int tile = vb; tile < tiles; tile += vgrid) {
      gemm_body<1, 1, AKC, BKC, ALIGNED>(g, lds, tile % tn, tile / tn, 0);
      __syncthreads();  // the next tile restages LDS
    }
    return;
  }
  g.K = cr, g.splits = splits;
  g.ksplit = ((((cr + splits - 1) / splits) + BK - 1) / BK) * BK;
  if (g.ksplit < BK) g.ksplit = BK;
  const int tn = (g.N + 63) >> 6, tm = (g.M + 63) >> 6, tiles = tm * tn * splits;
  for (int tile = vb; tile < tiles; tile += vgrid) {
    const int sp = tile % splits, r = tile / splits;
    const int bx = r % tn, by = r / tn;
    if (sp * g.ksplit >= cr) {  // this K slice is empty
      if (splits > 1) {         // its partial tile is zero
        float* __restrict__ W = g.ws + (long)sp * g.M * g.N;
        for (int e = threadIdx.x; e < 64 * 64; e += 256) {
          const int row = by * 64 + (e >> 6), col = bx * 64 + (e & 63);
          if (row < g.M && col < g.N) W[(long)row * g.N + col] = 0.f;
        }
      }                      // (cr == 0 with one slice: gemm_dyn_zero_kernel defines C)
      continue;
    }
    gemm_body<1, 1, AKC, BKC, ALIGNED>(g, lds, bx, by, sp);
    __syncthreads();
  }
}

template <bool AKC, bool BKC, bool ALIGNED>
__global__ __launch_bounds__(256, 4) void gemm_dyn_kernel(GemmArgs g, const int* __restrict__ cnt, int dyn, int splits) {
  __shared__ __attribute__((aligned(16))) float lds[lds_floats<1, 1, AKC, BKC>()];
  gemm_dyn_walk<AKC, BKC, ALIGNED>(g, lds, cnt, dyn, splits, (int)blockIdx.x, (int)gridDim.x);
}

// The two gradients of one Linear layer on a device-side row count in ONE launch: the weight gradient (K = *cnt: operands
// [K][.], split over `splits` slices) on the first gridW workgroups, the data gradient (M = *cnt: dY [M][K] times W [K][N]) on
// the rest.  Interior shapes only (gemm_dyn_pair below checks).
// KIND 0: weight gradient + data gradient of one layer; 1: two weight gradients over the same rows (the classifier head's dW_c
// halves); 2: two data-gradient-shaped products over the same rows (M = *cnt both: the head's dout W_c halves).
template <int KIND>
__global__ __launch_bounds__(256, 4) void gemm_dyn_pair_kernel(GemmArgs gw, GemmArgs gx, const int* __restrict__ cnt, int splits,
                                                               int gridW) {
  __shared__ __attribute__((aligned(16))) float lds[lds_floats<1, 1, true, false>()];
  const int vb2 = (int)blockIdx.x - gridW, vg2 = (int)gridDim.x - gridW;
  if ((int)blockIdx.x < gridW) {
    if (KIND == 2) gemm_dyn_walk<true, false, true>(gw, lds, cnt, 1, 1, (int)blockIdx.x, gridW);
    else gemm_dyn_walk<false, false, true>(gw, lds, cnt, 2, splits, (int)blockIdx.x, gridW);
  } else if (KIND == 1) gemm_dyn_walk<false, false, true>(gx, lds, cnt, 2, splits, vb2, vg2);
  else gemm_dyn_walk<true, false, true>(gx, lds, cnt, 1, 1, vb2, vg2);
}
// the two weight gradients' reduces in one launch (blockIdx.y picks the problem)
__global__ __launch_bounds__(256) void splitk_reduce_pair_kernel(const GemmArgs ga, const GemmArgs gb) {
  reduce4(blockIdx.y ? gb : ga, 0, (long)blockIdx.x * 256 + threadIdx.x);
}

// *cnt == 0 with dyn == 2: every slice is empty; C must still be defined (zeros).
__global__ __launch_bounds__(256) void gemm_dyn_zero_kernel(GemmArgs g, const int* __restrict__ cnt) {
  if (*cnt != 0) return;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long)g.M * g.N) return;
  const int row = (int)(e / g.N), col = (int)(e - (long)row * g.N);
  if (!g.accumulate) g.C[(long)row * g.ldc + col] = 0.f;
}

using DynKernel = void (*)(GemmArgs, const int*, int, int);   // gemm_dyn_kernel by [guarded][A stored K x M][b_kc] (same order)
static const DynKernel dyn_kernels[2][2][2] = {
    {{gemm_dyn_kernel<true, false, true>, gemm_dyn_kernel<true, true, true>}, {gemm_dyn_kernel<false, false, true>, gemm_dyn_kernel<false, true, true>}},
    {{gemm_dyn_kernel<true, false, false>, gemm_dyn_kernel<true, true, false>}, {gemm_dyn_kernel<false, false, false>, gemm_dyn_kernel<false, true, false>}}};

int gemm_dyn(const GemmArgs& g_in, const int* cnt, int dyn, long cap, hipStream_t st) {
  GemmArgs g = g_in;
  GC_REQUIRE(cnt && (dyn == 1 || dyn == 2) && cap >= 0, "gemm_dyn: bad arguments");
  const GemmPlan p = gemm_plan(g, dyn == 1 ? GEMM_DYN_M : GEMM_DYN_K, 1, 0, cap);
  if (!p.ok) return 1;
  if (p.zero_fill) hipLaunchKernelGGL(gemm_dyn_zero_kernel, dim3(cdiv((long)g.M * g.N, 256)), dim3(256), 0, st, g, cnt);
  // (flops are data-dependent: not counted by the host-side timer)
  GC_LAUNCH_TIMED("gemm_dyn", 0.0, dyn_kernels[!p.interior][!g.a_kc][g.b_kc != 0], dim3(p.grid), dim3(256), 0, st, g, cnt, dyn, p.splits);
  if (int e = check_launch("gemm_dyn")) return e;
  // sums `splits` partial slabs (empty slices wrote zeros) and runs the epilogue
  return p.reduce ? splitk_reduce(g, st, "gemm_dyn_reduce") : 0;
}

// Two products on the same device-side row count in ONE launch of gemm_dyn_pair_kernel<kind>: dyn[i] says which dimension of
// problem i is the count (gemm_dyn's numbering: 1 = M, 2 = K).  The kernel instantiates one walk per dimension: A [M][K] times
// B [K][N] for a count in M, both operands [K][.] for a count in K, interior shapes only.  A count in K runs split, its partials
// reduced by splitk_reduce, or for two such problems (same shape, one split factor, one gridW) by splitk_reduce_pair_kernel.
struct DynPairForm {
  const char* name;
  int kind;
  int dyn[2];
};
struct DynPairPlan {
  bool fused;   // false: two gemm_dyn calls (guarded tiles, another storage form, an unsplittable weight gradient)
  GemmPlan p[2];
  int gridW;    // the first problem's workgroups; the second problem's follow
};
static DynPairPlan dyn_pair_plan(const DynPairForm& f, GemmArgs (&g)[2], long cap) {
  DynPairPlan pp = {};
  const bool both_k = f.dyn[0] == 2 && f.dyn[1] == 2;
  bool ok = !both_k || (g[0].M == g[1].M && g[0].N == g[1].N);
  for (int i = 0; i < 2; ++i) ok = ok && !g[i].b_kc && (g[i].a_kc != 0) == (f.dyn[i] == 1);
  for (int i = 0; i < 2 && ok; ++i) {
    if (i == 1 && both_k) {  // the first problem's workspace holds both problems' partials, one behind the other
      const long slab = (long)pp.p[0].splits * g[0].M * g[0].N;
      g[1].split_ws(g[0].ws + slab, g[0].ws_elems - slab);
    }
    pp.p[i] = gemm_plan(g[i], f.dyn[i] == 1 ? GEMM_DYN_M : GEMM_DYN_K, 1, 0, cap);
    ok = pp.p[i].ok && pp.p[i].interior && (f.dyn[i] == 1 || pp.p[i].reduce);
  }
  pp.fused = ok;
  pp.gridW = pp.p[0].grid;
  return pp;
}
using DynPairKernel = void (*)(GemmArgs, GemmArgs, const int*, int, int);
static const DynPairKernel dyn_pair_kernels[3] = {gemm_dyn_pair_kernel<0>, gemm_dyn_pair_kernel<1>, gemm_dyn_pair_kernel<2>};

static int dyn_pair(const DynPairForm& f, const GemmArgs& a_in, const GemmArgs& b_in, const int* cnt, long cap, hipStream_t st) {
  GC_REQUIRE(cnt && cap >= 0, "%s: bad arguments", f.name);
  GemmArgs g[2] = {a_in, b_in};
  const DynPairPlan pp = dyn_pair_plan(f, g, cap);
  if (!pp.fused) {
    if (int e = gemm_dyn(a_in, cnt, f.dyn[0], cap, st)) return e;
    return gemm_dyn(b_in, cnt, f.dyn[1], cap, st);
  }
  GC_LAUNCH_TIMED("gemm_dyn", 0.0, dyn_pair_kernels[f.kind], dim3(pp.gridW + pp.p[1].grid), dim3(256), 0, st, g[0], g[1], cnt, pp.p[0].splits, pp.gridW);
  if (int e = check_launch(f.name)) return e;
  if (!pp.p[1].reduce) return pp.p[0].reduce ? splitk_reduce(g[0], st, "gemm_dyn_reduce") : 0;
  ProfScope ps("gemm_splitk_reduce", st);
  dim3 rgrid(cdiv((long)g[0].M * g[0].N / 4, 256), 2);
  hipLaunchKernelGGL(splitk_reduce_pair_kernel, rgrid, dim3(256), 0, st, g[0], g[1]);
  return check_launch("gemm_dyn_reduce");
}

// dW = dY^T X (dyn = 2) and dX (+)= dY W (dyn = 1) of one Linear layer whose row count lives on the device: one launch + the
// weight gradient's reduce instead of two launches + the reduce.
static const DynPairForm pair_wx = {"gemm_dyn_pair", 0, {2, 1}};
int gemm_dyn_pair(const GemmArgs& gw, const GemmArgs& gx, const int* cnt, long cap, hipStream_t st) { return dyn_pair(pair_wx, gw, gx, cnt, cap, st); }
// Two weight gradients over the same device-side row count and of the same shape (dyn = 2 both): one launch + one reduce launch.
static const DynPairForm pair_ww = {"gemm_dyn_pair_ww", 1, {2, 2}};
int gemm_dyn_pair_ww(const GemmArgs& ga, const GemmArgs& gb, const int* cnt, long cap, hipStream_t st) { return dyn_pair(pair_ww, ga, gb, cnt, cap, st); }
// Two products whose M is the same device-side row count (dyn = 1 both, A [M][K] row-major, B [K][N]): one launch.
static const DynPairForm pair_xx = {"gemm_dyn_pair_xx", 2, {1, 1}};
int gemm_dyn_pair_xx(const GemmArgs& ga, const GemmArgs& gb, const int* cnt, long cap, hipStream_t st) { return dyn_pair(pair_xx, ga, gb, cnt, cap, st); }

// ---- deferred problems ------------------------------------------------------------------------------------------
// One DeferQueue per backward pass (owned by the host side, gcgcn_defer_create / _destroy): no process-wide state, so
// two passes -- other models, other devices, other threads -- never see each other's problems, and a pass that fails
// half-way simply drops its queue.
bool gemm_defer(DeferQueue* q, const GemmArgs& g_in) {
  if (!q) return false;
  GemmArgs g = g_in;
  if (q->n >= DeferQueue::CAP || g.M == 0 || g.N == 0) return false;
  const GemmPlan p = gemm_plan(g, GEMM_PARK, 1, 0, 0);
  if (!(p.ok && p.interior)) return false;
  g.ws = nullptr, g.ws_elems = 0;  // unsplit: the whole K inside one workgroup
  q->done[q->n] = 0;
  q->p[q->n++] = g;
  return true;
}

bool gemm_defer_col2(DeferQueue* q, const ColRide& c) {
  if (!q || q->ncol2 >= DeferQueue::COLCAP || c.ready_slices <= 0 || !c.part || !c.out || c.C <= 0) return false;
  q->col2[q->ncol2++] = c;
  return true;
}
bool gemm_take_deferred_col2(DeferQueue* q, ColRide& out) {
  if (!q || q->ncol2 == 0) return false;
  out = q->col2[--q->ncol2];
  return true;
}

// longest K first (they run the longest: start them first); small_first: among equal K the problems with the fewest tiles
// lead -- a carrier with a tile budget then completes whole small problems instead of a slice of a big one, which keeps the
// NUMBER of parked problems within what the last carrier's argument block holds (GemmGroup::MAXP)
static void sort_parked(DeferQueue* q, bool small_first = false) {
  auto before = [&](const GemmArgs& a, int da, const GemmArgs& b, int db) {
    if (a.K != b.K) return a.K > b.K;
    return small_first && tiles_of(a) - da < tiles_of(b) - db;
  };
  for (int i = 1; i < q->n; ++i)
    for (int j = i; j > 0 && before(q->p[j], q->done[j], q->p[j - 1], q->done[j - 1]); --j) {
      const GemmArgs t = q->p[j];
      const int d = q->done[j];
      q->p[j] = q->p[j - 1], q->p[j - 1] = t;
      q->done[j] = q->done[j - 1], q->done[j - 1] = d;
    }
}

// Move parked work into gg: up to G::MAXP problems, at most max_tiles tiles in all; a problem is split when the budget
// ends inside it (its remaining tiles stay parked).  Returns the number of workgroups (one per tile, ranges 8-aligned).
template <class G>
static int take_parked(DeferQueue* q, G& gg, double* flops, long max_tiles, bool small_first = false) {
  gg.nprob = 0;
  gg.tile_begin[0] = 0;
  if (!q || q->n == 0 || max_tiles <= 0) return 0;
  sort_parked(q, small_first);
  int wgs = 0, np = 0, keep = 0;
  for (int i = 0; i < q->n; ++i) {
    const GemmArgs& g = q->p[i];
    const int total = (int)tiles_of(g), avail = total - q->done[i];
    const long take = (np < G::MAXP && max_tiles > 0) ? (avail < max_tiles ? avail : max_tiles) : 0;
    if (take > 0) {
      wgs = (wgs + 7) & ~7;
      gg.tile_begin[np] = wgs, gg.tile_count[np] = total, gg.tile_first[np] = q->done[i], gg.tile_take[np] = (int)take;
      gg.red_begin[np] = 0;
      gg.p[np++] = g;
      wgs += (int)take;
      max_tiles -= take;
      if (flops) *flops += flops_of(g) * (double)take / total;
    }
    if (q->done[i] + take < total) {  // (part of) the problem stays parked
      q->p[keep] = g, q->done[keep] = q->done[i] + (int)take;
      ++keep;
    }
  }
  q->n = keep;
  for (int i = keep; i < DeferQueue::CAP; ++i) q->done[i] = 0;
  gg.nprob = np;
  gg.tile_begin[np] = wgs, gg.red_begin[np] = 0;
  return wgs;
}

int gemm_take_deferred(DeferQueue* q, GemmGroup& gg, double* flops) { return take_parked(q, gg, flops, 1L << 40); }
int gemm_take_deferred_pairs(DeferQueue* q, GemmGroup4& gg, double* flops, long max_wgs, bool small_first) {
  return take_parked(q, gg, flops, max_wgs, small_first);
}

// tiles of parked problems, unsplit, as a launch of their own (what a carrying kernel would have run as passengers)
template <bool RB>
__global__ __launch_bounds__(256, 4) void gemm_parked_kernel(const GemmGroup gg) {
  __shared__ __attribute__((aligned(16))) float lds[lds_floats<1, 1, true, true>()];
  gemm_group_block<RB>(gg, blockIdx.x, lds);
}

int gemm_flush_deferred(DeferQueue* q, hipStream_t stream) {
  while (q && q->n > 0) {
    bool partial = false;
    for (int i = 0; i < q->n; ++i) partial = partial || q->done[i] > 0;
    if (partial) {  // the rest of a partly carried problem: same unsplit tiles, same tile list
      GemmGroup gg;
      double fl = 0;
      const int wgs = gemm_take_deferred(q, gg, &fl);
      if (wgs > 0) {
        GC_LAUNCH_TIMED("gemm_group", fl, by_row_blocks(gg, gemm_parked_kernel<true>, gemm_parked_kernel<false>), dim3(wgs), dim3(256), 0, stream, gg);
        if (int e = check_launch("gemm_parked")) return e;
      }
      continue;
    }
    GemmArgs probs[GemmGroup::MAXP];
    const int n = q->n < GemmGroup::MAXP ? q->n : GemmGroup::MAXP;
    for (int i = 0; i < n; ++i) probs[i] = q->p[q->n - n + i];
    q->n -= n;
    if (int e = gemm_group(probs, n, stream)) return e;
  }
  ColRide c2;
  while (gemm_take_deferred_col2(q, c2))   // second stages of column sums that met no carrier
    if (int e = col_sum_stage2_launch(c2, stream)) return e;
  return 0;
}

}  // namespace gc

#include "../../include/gcgcn.h"

extern "C" {

// The launcher's decision for one problem (form 0..4: the GemmForm values) or for a pair on a device-side count (5 gemm_dyn_pair,
// 6 _ww, 7 _xx), by the very functions the launchers call, on made-up operand addresses.  A problem is 13 integers: M, N, K, a_kc,
// b_kc, lda, ldb, ldc, batch1, batch2, row-block mode, workspace elements (0: no workspace) and a misalign mask (bit 0 A, bit 1 B,
// bit 2 the workspace off a 16-byte boundary).  out[0..11] and, for a pair, out[12..23]: ok, interior, splits, ksplit, widen, kept
// row-block mode, vecA, vecB, tiles, reduce, zero fill, grid (a pair that is not fused: of the two gemm_dyn calls that run instead);
// out[24], out[25]: fused, gridW.  Fields that do not apply are -1.  Exposed for tests (no GPU needed).
int gcgcn_debug_gemm_plan(int form, const int64_t* prob_a, const int64_t* prob_b, int splits, int64_t group_work, int64_t cap, int32_t* out) {
  using namespace gc;
  GC_REQUIRE(form >= 0 && form <= 7 && prob_a && (form < 5 || prob_b) && cap >= 0 && out, "debug_gemm_plan: bad arguments");
  GC_REQUIRE(prob_a[0] > 0 && prob_a[1] > 0 && (form < 5 || (prob_b[0] > 0 && prob_b[1] > 0)), "debug_gemm_plan: empty problem");
  for (int i = 0; i < 26; ++i) out[i] = -1;
  int slot = 0;
  auto at = [&](bool off) { return (float*)(uintptr_t)(0x10000000ul * ++slot + (off ? 4 : 0)); };
  static const int live_blocks = 0;   // only its address is used: a row-block list is present
  auto problem = [&](const int64_t* d) {
    GemmArgs g = gemm_stored((int)d[3], (int)d[4], at(d[12] & 1), d[5], at(d[12] & 2), d[6], at(false), d[7], (int)d[0], (int)d[1], (int)d[2]);
    g.batch_z1((int)d[8], d[0] * d[2], d[1] * d[2], d[0] * d[1]).batch_z2((int)d[9], d[8] * d[0] * d[2], d[8] * d[1] * d[2], d[8] * d[0] * d[1]);
    float* ws = at(d[12] & 4);
    if (d[11] > 0) g.split_ws(ws, d[11]);
    if (d[10]) g.rb = g.rb_n = &live_blocks, g.rb_mode = (int)d[10];
    return g;
  };
  auto show = [&](const GemmArgs& g, const GemmPlan& p, int32_t* o) {
    o[0] = p.ok;
    if (!p.ok) return;
    o[1] = p.interior, o[2] = p.splits, o[3] = p.ksplit, o[4] = p.widen, o[5] = p.rb_mode, o[6] = g.vecA, o[7] = g.vecB, o[8] = (int32_t)p.tiles;
    o[9] = p.reduce, o[10] = p.zero_fill, o[11] = p.grid;
  };
  if (form < 5) {
    GemmArgs g = problem(prob_a);
    show(g, gemm_plan(g, (GemmForm)form, splits, group_work, cap), out);
    return 0;
  }
  const DynPairForm& f = form == 5 ? pair_wx : form == 6 ? pair_ww : pair_xx;
  const GemmArgs in[2] = {problem(prob_a), problem(prob_b)};
  GemmArgs g[2] = {in[0], in[1]};
  DynPairPlan pp = dyn_pair_plan(f, g, cap);
  for (int i = 0; i < 2; ++i) {
    if (!pp.fused) g[i] = in[i], pp.p[i] = gemm_plan(g[i], f.dyn[i] == 1 ? GEMM_DYN_M : GEMM_DYN_K, 1, 0, cap);
    show(g[i], pp.p[i], out + 12 * i);
  }
  out[24] = pp.fused, out[25] = pp.fused ? pp.gridW : -1;
  return 0;
}

// The run-side twin: n problems described by flat rows (layout: include/gcgcn.h), built with the constructors of gemm.hpp and handed to
// the launchers the library itself calls.  form: 0 gemm() per problem, 1 gemm_group, 2 gemm_defer each into a queue local to this call
// (a refused problem runs through gemm() at once, as the callers do) then gemm_flush_deferred, 5 / 6 / 7 the pairs on *cnt.  Allocates
// nothing, reads no device memory.  Exposed for tests.
int gcgcn_debug_gemm_run(int form, int n, const int64_t* probs, const float* scal, const void* const* ptrs, const int64_t* ride,
                         const void* const* ride_ptrs, int tile, int splits, const int32_t* cnt, int64_t cap, int32_t* out, void* stream) {
  using namespace gc;
  constexpr int NI = 40, NF = 2, NP = 14, MAXN = 40;   // (MAXN: past DeferQueue::CAP)
  GC_REQUIRE((form == 0 || form == 1 || form == 2 || (form >= 5 && form <= 7)) && n >= 0 && n <= MAXN && out, "debug_gemm_run: bad arguments");
  GC_REQUIRE(n == 0 || (probs && scal && ptrs), "debug_gemm_run: problems without their rows");
  GC_REQUIRE(form < 5 || (n == 2 && cnt && cap >= 0), "debug_gemm_run: a pair is two problems on a device-side count");
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < 2 + 2 * n; ++i) out[i] = -1;
  GemmArgs g[MAXN];
  for (int i = 0; i < n; ++i) {
    const int64_t* d = probs + (long)NI * i;
    const float* f = scal + NF * i;
    const void* const* p = ptrs + NP * i;
    GemmArgs& a = g[i];
    a = gemm_stored((int)d[3], (int)d[4], (const float*)p[0], d[5], (const float*)p[1], d[6], (float*)p[2], d[7], (int)d[0], (int)d[1], (int)d[2]);
    a.batch_z1((int)d[8], d[13], d[15], d[17]).batch_z2((int)d[9], d[14], d[16], d[18]);
    if (p[12]) a.split_ws((float*)p[12], d[11]);
    a.alpha = f[0];
    a.add = (const float*)p[3], a.ldadd = d[19], a.sAdd1 = d[20], a.sAdd2 = d[21];
    a.bias = (const float*)p[4];
    a.rowadd = (const float*)p[5], a.sRa1 = d[22], a.sRa2 = d[23];
    a.rowscale = (const float*)p[6], a.sRs1 = d[24], a.sRs2 = d[25];
    a.C2 = (float*)p[7], a.ldc2 = d[26], a.sC21 = d[27], a.sC22 = d[28];
    a.add2 = (const float*)p[8], a.ldadd2 = d[29], a.sAdd21 = d[30], a.sAdd22 = d[31];
    a.relu = (int)d[32], a.accumulate = (int)d[33];
    a.n_valid = (const int*)p[9], a.nv_rows = (int)d[34], a.nv_zdoc = (int)d[35];
    GC_REQUIRE(!a.n_valid || a.nv_rows >= 1, "debug_gemm_run: n_valid with nv_rows %d", a.nv_rows);
    if (d[10]) {
      GC_REQUIRE(p[10] && p[11], "debug_gemm_run: row-block mode %d without a list", (int)d[10]);
      a.rb = (const int*)p[10], a.rb_n = (const int*)p[11], a.rb_mode = (int)d[10], a.rb_zero = (int)d[36];
    }
    a.drop = make_drop(p[13], (uint64_t)d[38], f[1]);
    a.drop_base = d[37];
  }
  if (form == 0) {
    int rc = 0;
    for (int i = 0; i < n; ++i) {
      out[3 + 2 * i] = gemm(g[i], st, tile, splits);
      if (!rc) rc = out[3 + 2 * i];
    }
    return out[0] = rc;
  }
  if (form == 1) {
    ColRide c;
    const ColRide* col = nullptr;
    if (ride && ride[0]) {
      GC_REQUIRE(ride[0] >= 1 && ride[0] <= 3 && ride_ptrs, "debug_gemm_run: ride kind %ld", (long)ride[0]);
      const float* X = (const float*)ride_ptrs[0];
      float* o = (float*)ride_ptrs[1];
      float* part = (float*)ride_ptrs[2];
      if (ride[0] == 3) c = head_sum(X, (int)ride[1], (int)ride[2], o);
      else c = col_sum(X, ride[1], ride[2], (int)ride[3], o, part);
      if (ride[0] == 2) c = c.stage2((int)ride[4]);
      col = &c;
    }
    bool later = false;
    out[0] = gemm_group(g, n, st, col, ride && ride[5] ? &later : nullptr);
    out[1] = later;
    return out[0];
  }
  if (form == 2) {
    DeferQueue q;
    int rc = 0;
    for (int i = 0; i < n; ++i) {
      out[2 + 2 * i] = gemm_defer(&q, g[i]);
      if (!out[2 + 2 * i]) {
        out[3 + 2 * i] = gemm(g[i], st);
        if (!rc) rc = out[3 + 2 * i];
      }
    }
    out[0] = gemm_flush_deferred(&q, st);
    return rc ? rc : out[0];
  }
  out[0] = form == 5 ? gemm_dyn_pair(g[0], g[1], cnt, cap, st) : form == 6 ? gemm_dyn_pair_ww(g[0], g[1], cnt, cap, st)
                                                                            : gemm_dyn_pair_xx(g[0], g[1], cnt, cap, st);
  return out[0];
}

}  // extern "C"
