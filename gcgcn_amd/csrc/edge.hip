// Edge-feature streaming kernels: the HBM-bound half of the CAGGC/MAGGC path.
//
// E is the per-pair edge tensor [B, N, N, D] (fp32, row-major): 4*N*N*D bytes per document,
// far larger than everything else on the path.  Each byte of E is read exactly once in the
// forward pass and once in the backward pass; dE is written exactly once.
//
//   edge_fwd  : one workgroup per entity row (b, i) streams E[b, i, :, :] (N*D contiguous
//               floats, 16 B per lane, a 1-KiB row segment per wave instruction) and produces
//                 Ebar[b, i, :]  = mean_j E[b, i, j, :]          (GraphConv edge term, glove:40-41
//                                                                 after commuting mean and W_e)
//                 logit[b, i, j] = v . E[b, i, j, :]             (GATAttention edge term, glove:161-162
//                                                                 folded: v = W_r^T wt_r)
//   edge_bwd  : re-reads E for dv = sum dlogit * E and writes
//                 dE[b, i, j, :] = dlogit[b, i, j] * v + dEbar[b, i, :] / n
//   edge_bcast: dE[b, i, j, :] = dEbar[b, i, :] / n   (MAGGC hop: E only feeds the mean)
//
// Ragged batches: n_valid[b] <= N entities are real; padding rows/columns are neither read nor
// averaged, and their outputs are zero.
#include <string.h>

#include "edge_body.hpp"
#include "compact.hpp"
#include "gat_body.hpp"
#include "gemm_body.hpp"
#include "rowops.hpp"

namespace gc {

template <int VEC, bool ATT>
__global__ __launch_bounds__(64 * EW) void edge_fwd_kernel(const float* __restrict__ E, const float* __restrict__ v,
                                                           const int* __restrict__ n_valid, float* __restrict__ Ebar,
                                                           const float* __restrict__ coladd, float* __restrict__ P,
                                                           float* __restrict__ Aout, Drop drop, int N, int D,
                                                           const unsigned char* __restrict__ mask) {
  extern __shared__ __attribute__((aligned(16))) float cs[];  // [EW][D] per-wave column sums, then [N] logits
  edge_fwd_row<VEC, ATT, EW>(E, v, n_valid, Ebar, coladd, P, Aout, drop, N, D, blockIdx.x, cs, mask);
}

// ---------------------------------------------------------------------------------------------
// backward of the CAGGC hop: dE = dlogit (x) v + dEbar / n ;  dv partial per workgroup.
// dynamic LDS: N + EW * D floats.
// ---------------------------------------------------------------------------------------------
template <int VEC>
__device__ __forceinline__ void edge_bwd_row(const float* __restrict__ E, const float* __restrict__ v,
                                             const int* __restrict__ n_valid, const float* __restrict__ dlogit,
                                             const float* __restrict__ dEbar, float* __restrict__ dE,
                                             float* __restrict__ dvpart, int N, int D, int nt, const int bi,
                                             float* __restrict__ sm, const GatTail& gt) {
  float* dl = sm;                    // [N]
  float* cs = sm + ((N + 3) & ~3);   // [EW][D]
  const int b = bi / N, i = bi - b * N;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nv = n_valid ? min(max(n_valid[b], 0), N) : N;
  float* dEr = dE ? dE + (long)bi * N * D : nullptr;
  float* dvp = dvpart + (long)bi * D;
  if (i >= nv) {
    for (int c = t; c < D; c += 64 * EW) dvp[c] = 0.f;
    if (dEr) {
      const long tot = (long)N * D;
      for (long o = t; o < tot; o += 64 * EW) dEr[o] = 0.f;
    }
    return;
  }
  if (gt.P) {  // N <= 64: the row's softmax gradient straight from P and dA (dropout replayed), no dlogit tensor in between
    if (wave == 0) {
      const long o = (long)bi * N + min(lane, N - 1);
      float p = gt.P[o], g = gt.dA[o];
      if (lane >= N) p = 0.f, g = 0.f;
      if (gt.drop.snap) g = (rng_u32(drop_key(gt.drop), (uint64_t)((long)bi * N + lane)) >= gt.drop.thresh) ? g * gt.drop.scale : 0.f;
      const float dot = wave_sum(g * p);
      if (lane < N) dl[lane] = p * (g - dot);
    }
  } else {
    for (int j = t; j < N; j += 64 * EW) dl[j] = dlogit[(long)bi * N + j];
  }
  __syncthreads();
  const float* __restrict__ Er = E + (long)bi * N * D;
  const float inv = 1.f / (float)nv;
  const int nchunk = (D + 64 * VEC - 1) / (64 * VEC);
  for (int q = 0; q < nchunk; ++q) {
    const int c = (q * 64 + lane) * VEC;
    const bool act = c < D;
    float vr[VEC], g[VEC], acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) vr[e] = 0.f, g[e] = 0.f, acc[e] = 0.f;
    if (act) {
      vload<VEC>(vr, v + c);
      if (dEbar) {
        vload<VEC>(g, dEbar + (long)bi * D + c);
#pragma unroll
        for (int e = 0; e < VEC; ++e) g[e] *= inv;
      }
    }
    int j = wave;
    for (; j + (EUNR - 1) * EW < nv; j += EUNR * EW) {
      float x[EUNR][VEC];
#pragma unroll
      for (int u = 0; u < EUNR; ++u) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) x[u][e] = 0.f;
        if (act) vload_nt<VEC>(x[u], Er + (long)(j + u * EW) * D + c);
      }
#pragma unroll
      for (int u = 0; u < EUNR; ++u) {
        const float d = dl[j + u * EW];
        float o[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          acc[e] = fmaf(d, x[u][e], acc[e]);
          o[e] = fmaf(d, vr[e], g[e]);
        }
        if (dEr && act) {
          if (nt) vstore_nt<VEC>(dEr + (long)(j + u * EW) * D + c, o);
          else vstore<VEC>(dEr + (long)(j + u * EW) * D + c, o);
        }
      }
    }
    for (; j < nv; j += EW) {
      float x[VEC], o[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) x[e] = 0.f;
      if (act) vload<VEC>(x, Er + (long)j * D + c);
      const float d = dl[j];
#pragma unroll
      for (int e = 0; e < VEC; ++e) {
        acc[e] = fmaf(d, x[e], acc[e]);
        o[e] = fmaf(d, vr[e], g[e]);
      }
      if (dEr && act) {
        if (nt) vstore_nt<VEC>(dEr + (long)j * D + c, o);
        else vstore<VEC>(dEr + (long)j * D + c, o);
      }
    }
    if (dEr && act) {  // padding columns of a real row
      float z[VEC];
#pragma unroll
      for (int e = 0; e < VEC; ++e) z[e] = 0.f;
      for (int jj = nv + wave; jj < N; jj += EW) vstore<VEC>(dEr + (long)jj * D + c, z);
    }
    if (act) vstore<VEC>(cs + wave * D + c, acc);
  }
  __syncthreads();
  for (int c = t; c < D; c += 64 * EW) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < EW; ++w) s += cs[w * D + c];
    dvp[c] = s;
  }
}

template <int VEC>
__global__ __launch_bounds__(64 * EW) void edge_bwd_kernel(const float* __restrict__ E, const float* __restrict__ v,
                                                           const int* __restrict__ n_valid,
                                                           const float* __restrict__ dlogit,
                                                           const float* __restrict__ dEbar, float* __restrict__ dE,
                                                           float* __restrict__ dvpart, int N, int D, int nt,
                                                           const GatTail gt) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  // the GATAttention backward of the node scores (gat_body.hpp) rides in front: B * slices short workgroups
  const int ngat = gt.P ? gt.B * gt.slices : 0;
  if ((int)blockIdx.x < ngat) {
    const int b = blockIdx.x / gt.slices;
    gat_dlogit_doc(gt.P, gt.dA, gt.uvc, gt.dXin, nullptr, gt.ds, gt.dX, N, D, gt.drop, b, blockIdx.x - b * gt.slices, gt.slices, sm);
    return;
  }
  edge_bwd_row<VEC>(E, v, n_valid, dlogit, dEbar, dE, dvpart, N, D, nt, blockIdx.x - ngat, sm, gt);
}

// The same pass carrying deferred GEMM problems (gemm.hpp): the first gg.tile_begin[gg.nprob] workgroups each run one
// 64x64 tile of a parked weight-gradient product over its whole K -- matrix-pipe work under an HBM-bound stream --
// the rest are the entity rows.  The tiles go out in cohorts spread through the launch (Spread, common.hpp): every compute
// unit then hosts rows AND a tile for most of the launch, where tiles-first order fills the chip with tiles alone for
// ntile / 1024 rounds before the first row starts (cfg 5: 1.5 rounds, no overlap at all).
template <int VEC, bool RB>   // RB: a carried product runs on the row blocks of a ragged batch (GemmArgs::rb)
__global__ __launch_bounds__(64 * EW) void edge_bwd_carry_kernel(const float* __restrict__ E, const float* __restrict__ v,
                                                                 const int* __restrict__ n_valid,
                                                                 const float* __restrict__ dlogit,
                                                                 const float* __restrict__ dEbar, float* __restrict__ dE,
                                                                 float* __restrict__ dvpart, int N, int D, int nt,
                                                                 const Spread sp, const GatTail gt, const GemmGroup gg,
                                                                 const int col_base) {
  // one LDS image for both kinds of workgroup (the rows need N + EW * D floats of it): a fourth workgroup fits per CU
  __shared__ __attribute__((aligned(16))) float tile_lds[lds_floats<1, 1, true, true>()];
  int r;
  if (col_base > 0 && (int)blockIdx.x >= col_base) {   // behind everything else: the second stage of a parked column sum (gg.col)
    col_ride_stage2_block(gg.col, (int)blockIdx.x - col_base);
    return;
  }
  if (spread_pick((int)blockIdx.x, sp, r)) {
    gemm_group_block<RB>(gg, r, tile_lds);
    return;
  }
  const int ngat = gt.P ? gt.B * gt.slices : 0;
  if (r < ngat) {
    const int b = r / gt.slices;
    gat_dlogit_doc(gt.P, gt.dA, gt.uvc, gt.dXin, nullptr, gt.ds, gt.dX, N, D, gt.drop, b, r - b * gt.slices, gt.slices, tile_lds);
    return;
  }
  edge_bwd_row<VEC>(E, v, n_valid, dlogit, dEbar, dE, dvpart, N, D, nt, r - ngat, tile_lds, gt);
}

template <int VEC>
__global__ __launch_bounds__(64 * EW) void edge_bcast_kernel(const float* __restrict__ dEbar,
                                                             const int* __restrict__ n_valid, float* __restrict__ dE,
                                                             int N, int D, int nt) {
  edge_bcast_row<VEC, EW>(dEbar, n_valid, dE, N, D, nt, blockIdx.x);
}

// ---------------------------------------------------------------------------------------------
// the plan (edge_plan.hpp): every launch decision of the passes in this file and in compact.hip, as pure host functions
// ---------------------------------------------------------------------------------------------
static inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
unsigned edge_misalign(const void* E, const void* v, const void* dE, const void* dEbar, const void* Ebar) {
  return (al16(E) ? 0 : EDGE_MIS_E) | (al16(v) ? 0 : EDGE_MIS_V) | (al16(dE) ? 0 : EDGE_MIS_DE) | (al16(dEbar) ? 0 : EDGE_MIS_DEBAR) |
         (al16(Ebar) ? 0 : EDGE_MIS_EBAR);
}
constexpr size_t EDGE_LDS_MAX = 160 * 1024;   // dense passes: the compute unit's LDS
constexpr size_t CMP_LDS_MAX = 64 * 1024;     // compact forward
constexpr size_t TILE_LDS = sizeof(float) * lds_floats<1, 1, true, true>();   // the carrying kernel's static image
static_assert(sizeof(float) * GAT_DOC_LDS <= TILE_LDS, "GAT passenger needs more LDS than a tile");

static EdgePlan plan_rows(const EdgeQuery& q, unsigned operands) {   // one workgroup per entity row; operands: the ones that must be 16-byte aligned
  EdgePlan p;
  p.compact = q.compact, p.att = q.att;
  p.vec = (!q.compact && q.D % 4 == 0 && !(q.mis & operands)) ? 4 : 1;
  p.grid = (long)q.B * q.N;
  return p;
}

EdgePlan edge_plan_fwd(const EdgeQuery& q) {
  EdgePlan p = plan_rows(q, EDGE_MIS_E | EDGE_MIS_EBAR | (q.att ? EDGE_MIS_V : 0));
  p.lds = ((size_t)(q.compact ? CW4 : EW) * q.D + (q.att ? (size_t)q.N : 0)) * sizeof(float);
  p.lds_limit = q.compact ? CMP_LDS_MAX : EDGE_LDS_MAX;
  return p;
}

EdgePlan edge_plan_bwd(const EdgeQuery& q) {
  EdgePlan p = plan_rows(q, EDGE_MIS_E | EDGE_MIS_V | (q.has_dE ? EDGE_MIS_DE : 0) | (q.has_dEbar ? EDGE_MIS_DEBAR : 0));
  if (q.att) {
    // N <= 64: dlogit, ds and dX = ds u + dX_in come from gat_dlogit_doc (gat_body.hpp) -- as B * slices passenger workgroups of the
    // dense edge pass, whose entity rows take their dlogit row from P and dA themselves (dlogit is never stored), as a launch of
    // its own in front of the compact one; larger graphs take the three generic launches
    p.route = q.N > GT ? EdgePlan::THREE : (q.compact ? EdgePlan::ONE : EdgePlan::RIDE);
    if (p.route != EdgePlan::THREE) p.slices = gat_dlogit_slices(q.D);
    if (p.route == EdgePlan::RIDE) p.ngat = q.B * p.slices;
    // [column-sum partials of colsum3 | compact: sd, cw of cmp_bwd]
    const long a = colsum_scratch_elems((long)q.B * q.N, q.D, 1), b = 3L * 64 * (2 * q.D + 1);
    p.scratch = a > b ? a : b;
    if (q.compact) p.rowbuf_off = p.scratch, p.scratch += 2L * q.B * q.N;
  }
  if (q.compact) {
    p.lds = ((size_t)CW4 * q.D + 2 * CW4) * sizeof(float);
    return p;
  }
  const size_t lds_row = ((size_t)((q.N + 3) & ~3) + (size_t)EW * q.D) * sizeof(float);
  p.lds = (p.ngat && lds_row < sizeof(float) * GAT_DOC_LDS) ? sizeof(float) * GAT_DOC_LDS : lds_row;   // a passenger needs more than a short row
  p.lds_limit = EDGE_LDS_MAX;
  p.carry_ok = p.vec == 4 && lds_row <= TILE_LDS;
  p.grid += p.ngat;
  return p;
}

EdgePlan edge_plan_bcast(const EdgeQuery& q) {
  if (!q.compact) return plan_rows(q, EDGE_MIS_DE | EDGE_MIS_DEBAR);
  EdgeQuery m = q;
  m.att = false;
  return edge_plan_bwd(m);
}

void edge_plan_carry(EdgePlan& p, int ntile, bool any_rb, int col_C) {
  if (ntile <= 0) return;
  const long rows = p.grid;   // entity rows + GAT passengers
  p.ntile = ntile, p.RB = any_rb;
  // one parked second stage of a column sum (a bias gradient's 64 partial rows -> its C columns) in trailing workgroups
  p.ncolwg = col_C > 0 ? cdiv(col_C, 256) : 0;
  p.col_base = col_C > 0 ? (int)(rows + ntile) : 0;
  p.grid = rows + ntile + p.ncolwg;
  // the tile cohorts (cohort tiles each) are spread over spread_pct % of the launch (0: all tiles first, the order until
  // round 3); launches of fewer than spread_min tiles keep them in front
  constexpr int spread_pct = 90, cohort = 256, spread_min = 1024;
  p.spread = make_spread(ntile, rows, cohort, ntile >= spread_min ? spread_pct : 0);
  p.lds = 0;   // rows, passengers and tiles share the kernel's static image
}

// ---------------------------------------------------------------------------------------------
// host launchers: validate, plan, launch what the plan says
// ---------------------------------------------------------------------------------------------
// E is read once per pass and never again before something else has flushed the caches (a training step feeds new
// documents): all E loads are non-temporal.  Ordinary loads for the attention pass over E1 were the round-1 setting, tuned
// on a bench that replayed ONE batch (part of E1 still sat in the Infinity Cache from the previous backward); with rotating
// batches they cost 8 us in edge_fwd_att (33.6 -> 25.7 us) and 3 us in the backward edge pass.  The dE stores stay ordinary
// (nt = 0): non-temporal ones gained nothing with rotating batches and were slower with a replayed one (edge_bwd 56 -> 69 us).
constexpr int NT_STORE = 0;

int edge_fwd(const float* E, const float* v, const int* n_valid, float* Ebar, const float* coladd, float* P, float* A,
             Drop drop, int B, int N, int D, hipStream_t st, const unsigned char* mask) {
  GC_REQUIRE(E && Ebar, "edge_fwd: null pointer");
  GC_REQUIRE(B > 0 && N > 0 && D > 0, "edge_fwd: bad shape B=%d N=%d D=%d", B, N, D);
  const bool att = P != nullptr;
  GC_REQUIRE(!att || (v && coladd), "edge_fwd: attention requested without v / node scores");
  const EdgePlan p = edge_plan_fwd({B, N, D, false, att, false, false, edge_misalign(E, v, nullptr, nullptr, Ebar)});
  GC_REQUIRE(p.lds_ok(), "edge_fwd: N=%d D=%d needs %zu B of LDS", N, D, p.lds);
  dim3 grid((unsigned)p.grid), block(64 * EW);
  const char* tag = att ? "edge_fwd_att" : "edge_fwd_mean";
  const double bytes = 4.0 * B * N * N * D;
#define GC_EDGE_FWD(V, AT) \
  GC_LAUNCH_TIMED(tag, bytes, (edge_fwd_kernel<V, AT>), grid, block, p.lds, st, E, v, n_valid, Ebar, coladd, P, A, drop, N, D, mask)
  if (p.vec == 4) {
    if (att) GC_EDGE_FWD(4, true);
    else GC_EDGE_FWD(4, false);
  } else {
    if (att) GC_EDGE_FWD(1, true);
    else GC_EDGE_FWD(1, false);
  }
#undef GC_EDGE_FWD
  return check_launch("edge_fwd");
}

int edge_bwd(const float* E, const float* v, const int* n_valid, const float* dlogit, const float* dEbar, float* dE,
             float* dvpart, const EdgePlan& plan, int B, int N, int D, hipStream_t st, DeferQueue* carry, const GatTail* tail) {
  GatTail gt;
  memset(&gt, 0, sizeof gt);
  if (tail && plan.route == EdgePlan::RIDE) gt = *tail;   // the passenger rides where the plan says so
  GC_REQUIRE(E && v && (dlogit || gt.P) && dvpart, "edge_bwd: null pointer");
  GC_REQUIRE(!gt.P || (N <= GT && gt.B == B && gt.slices == plan.slices && gt.dA && gt.uvc && gt.ds && gt.dX), "edge_bwd: bad GAT passenger");
  GC_REQUIRE(!plan.compact && plan.ngat == (gt.P ? B * gt.slices : 0) &&
                 (plan.vec == 4) == (D % 4 == 0 && !edge_misalign(E, v, dE, dEbar, nullptr)),
             "edge_bwd: the plan was made for other operands");
  static_assert(sizeof(GatTail) + sizeof(GemmGroup) + 96 <= 4096, "edge_bwd_carry_kernel: kernel arguments exceed 4 KB");
  GC_REQUIRE(plan.lds_ok(), "edge_bwd: N=%d D=%d needs %zu B of LDS", N, D, plan.lds);
  EdgePlan p = plan;
  dim3 block(64 * EW);
  const double bytes = (dE ? 8.0 : 4.0) * B * N * N * D;
  GemmGroup gg;
  double gflops = 0;
  // eligibility first, then the take (it pops the queue), then the grid around what was taken
  const int ntile = (p.carry_ok && carry && carry->n > 0) ? gemm_take_deferred(carry, gg, &gflops) : 0;
  if (ntile > 0) {  // parked weight-gradient products ride along, and one parked second stage of a column sum
    const bool col = gemm_take_deferred_col2(carry, gg.col);
    bool any_rb = false;
    for (int i = 0; i < gg.nprob; ++i) any_rb = any_rb || gg.p[i].rb != nullptr;
    edge_plan_carry(p, ntile, any_rb, col ? gg.col.C : 0);
    dim3 grid((unsigned)p.grid);
#define GC_EDGE_CARRY(RBV)                                                                                                  \
  GC_LAUNCH_TIMED("edge_bwd", bytes, (edge_bwd_carry_kernel<4, RBV>), grid, block, 0, st, E, v, n_valid, dlogit, dEbar, dE, \
                  dvpart, N, D, NT_STORE, p.spread, gt, gg, p.col_base)
    if (p.RB) GC_EDGE_CARRY(true);
    else GC_EDGE_CARRY(false);
#undef GC_EDGE_CARRY
    return check_launch("edge_bwd_carry");
  }
  dim3 grid((unsigned)p.grid);
#define GC_EDGE_BWD(V)                                                                                                             \
  GC_LAUNCH_TIMED("edge_bwd", bytes, (edge_bwd_kernel<V>), grid, block, p.lds, st, E, v, n_valid, dlogit, dEbar, dE, dvpart, N, D, \
                  NT_STORE, gt)
  if (p.vec == 4) GC_EDGE_BWD(4);
  else GC_EDGE_BWD(1);
#undef GC_EDGE_BWD
  return check_launch("edge_bwd");
}

int edge_bcast(const float* dEbar, const int* n_valid, float* dE, int B, int N, int D, hipStream_t st) {
  GC_REQUIRE(dEbar && dE, "edge_bcast: null pointer");
  const EdgePlan p = edge_plan_bcast({B, N, D, false, false, true, true, edge_misalign(nullptr, nullptr, dE, dEbar, nullptr)});
  dim3 grid((unsigned)p.grid), block(64 * EW);
  ProfScope ps("edge_bcast", st, 4.0 * B * N * N * D);
  if (p.vec == 4) hipLaunchKernelGGL((edge_bcast_kernel<4>), grid, block, 0, st, dEbar, n_valid, dE, N, D, NT_STORE);
  else hipLaunchKernelGGL((edge_bcast_kernel<1>), grid, block, 0, st, dEbar, n_valid, dE, N, D, NT_STORE);
  return check_launch("edge_bcast");
}

}  // namespace gc
