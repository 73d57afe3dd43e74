// Consumers of the edge-feature producer's COMPACT rows: the graph blocks of a hop without a dense E tensor.
//
// The reference builds context_sent_att[N, N, hidden] per hop (glove:314-327) and hands it to GATAttention /
// GraphConvolution (hop 0, glove:332-333) or to MultiGraphConvolution (hop >= 1, glove:337).  The producer kernels
// (producer.hip) only ever compute the pairs with a live sentence slot -- Ec[prow, :] for the Q live pairs of the batch, with
// prow = pair_prow[b, i, j] (-1 for a pair without a live slot) -- and every other real pair of E equals the bias vector of
// linear_sentence_att (its sentence sums are exactly zero).  So instead of expanding Ec into E[B, N, N, hidden], streaming E
// through the hop's kernels, writing dE[B, N, N, hidden] and gathering it back:
//
//   mean-only hop (every MAGGC hop):  Ebar[b, i] = (sum_{j live} Ec[prow(b,i,j)] + (n - live_i) bias) / n
//                                     dEc[prow]  = dEbar[b, i] / n,     dbias = sum_{b,i} (n - live_i) / n  dEbar[b, i]
//   attention hop (hop 0):            e_ij = Ec[prow] or bias in the edge pass of GATAttention (logit = v . e_ij, mean_j e_ij),
//                                     dEc[prow] = dlogit_ij v + dEbar_i / n,   dbias = v sum_dead dlogit + sum (n - live_i)/n dEbar_i,
//                                     dv = sum_ij dlogit_ij e_ij  (dead pairs included: e = bias)
//
// E and dE never exist.  One workgroup of 4 waves per entity row (b, i), like the dense edge kernels; every sum has a fixed
// order (bitwise reproducible).  Reference arithmetic: GATAttention.forward glove:154-168 (folded: energy = u.x_j + v.e_ij + c),
// GraphConv's edge term glove:40-41 (mean commuted with the projection).
#include "edge_body.hpp"
#include "compact.hpp"

namespace gc {

// dynamic LDS: CW4 * D (+ N when ATT) floats
template <bool ATT>
__global__ __launch_bounds__(64 * CW4) void cmp_edge_fwd_kernel(const CmpE ce, const float* __restrict__ v, const int* __restrict__ n_valid,
                                                                float* __restrict__ Ebar, const float* __restrict__ coladd,
                                                                float* __restrict__ P, float* __restrict__ Aout, const Drop drop, int N, int D) {
  extern __shared__ __attribute__((aligned(16))) float cs[];
  float* lg = cs + (long)CW4 * D;
  const int bi = blockIdx.x, b = bi / N, i = bi - b * N;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nv = n_valid ? min(max(n_valid[b], 0), N) : N;
  float* eb = Ebar + (long)bi * D;
  if (i >= nv) {  // padding entity: outputs are zero
    for (int c = t; c < D; c += 64 * CW4) eb[c] = 0.f;
    if (ATT)
      for (int j = t; j < N; j += 64 * CW4) {
        P[(long)bi * N + j] = 0.f;
        if (Aout) Aout[(long)bi * N + j] = 0.f;
      }
    return;
  }
  const int* __restrict__ pr = ce.prow + (long)bi * N;
  float acc[CMAXK], vr[CMAXK];
#pragma unroll
  for (int k = 0; k < CMAXK; ++k) {
    acc[k] = 0.f;
    vr[k] = (ATT && lane + 64 * k < D) ? v[lane + 64 * k] : 0.f;
  }
  for (int j = wave; j < nv; j += CW4) {
    const int p = pr[j];
    const float* __restrict__ row = p >= 0 ? ce.Ec + (long)p * D : ce.bias;
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < CMAXK; ++k) {
      const int c = lane + 64 * k;
      if (c < D) {
        const float x = row[c];
        acc[k] += x;
        dot = fmaf(x, vr[k], dot);
      }
    }
    if (ATT) {
      dot = wave_sum(dot);
      if (lane == 0) lg[j] = dot;
    }
  }
#pragma unroll
  for (int k = 0; k < CMAXK; ++k)
    if (lane + 64 * k < D) cs[wave * D + lane + 64 * k] = acc[k];
  __syncthreads();
  const float inv = 1.f / (float)nv;
  for (int c = t; c < D; c += 64 * CW4) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < CW4; ++w) s += cs[w * D + c];
    eb[c] = s * inv;
  }
  if (ATT && wave == 0) edge_softmax_tail(lg, coladd + (long)b * N, nullptr, P, Aout, drop, N, nv, (long)bi * N, lane);
}

// dEc[prow] = dlogit_ij v + dEbar_i / n for the live pairs of row (b, i); dvpart[bi] = sum_j dlogit_ij e_ij;
// sd[bi] = sum over dead pairs of dlogit_ij; cw[bi] = (dead pairs of the row) / n.  dlogit / dEbar / dvpart may be NULL
// (mean-only hop: no attention term).  dynamic LDS: CW4 * (D + 2) floats.
__global__ __launch_bounds__(64 * CW4) void cmp_edge_bwd_kernel(const CmpE ce, const float* __restrict__ v, const int* __restrict__ n_valid,
                                                                const float* __restrict__ dlogit, const float* __restrict__ dEbar,
                                                                float* __restrict__ dEc, float* __restrict__ dvpart,
                                                                float* __restrict__ sd, float* __restrict__ cw, int N, int D) {
  extern __shared__ __attribute__((aligned(16))) float cs[];
  float* ws = cs + (long)CW4 * D;   // [CW4][2]: per-wave dead-pair sums
  const int bi = blockIdx.x, b = bi / N, i = bi - b * N;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nv = n_valid ? min(max(n_valid[b], 0), N) : N;
  if (i >= nv) {
    if (dvpart)
      for (int c = t; c < D; c += 64 * CW4) dvpart[(long)bi * D + c] = 0.f;
    if (t == 0) sd[bi] = 0.f, cw[bi] = 0.f;
    return;
  }
  const int* __restrict__ pr = ce.prow + (long)bi * N;
  const float inv = 1.f / (float)nv;
  float acc[CMAXK], vr[CMAXK], g[CMAXK], br[CMAXK];
#pragma unroll
  for (int k = 0; k < CMAXK; ++k) {
    const int c = lane + 64 * k;
    acc[k] = 0.f;
    vr[k] = (dlogit && c < D) ? v[c] : 0.f;
    g[k] = (dEbar && c < D) ? dEbar[(long)bi * D + c] * inv : 0.f;
    br[k] = (dlogit && c < D) ? ce.bias[c] : 0.f;
  }
  float sdead = 0.f;
  int ndead = 0;
  for (int j = wave; j < nv; j += CW4) {
    const int p = pr[j];
    const float d = dlogit ? dlogit[(long)bi * N + j] : 0.f;
    if (p >= 0) {
#pragma unroll
      for (int k = 0; k < CMAXK; ++k) {
        const int c = lane + 64 * k;
        if (c < D) {
          if (dlogit) acc[k] = fmaf(d, ce.Ec[(long)p * D + c], acc[k]);
          dEc[(long)p * D + c] = fmaf(d, vr[k], g[k]);
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < CMAXK; ++k) acc[k] = fmaf(d, br[k], acc[k]);
      sdead += d;
      ++ndead;
    }
  }
  if (dvpart) {
#pragma unroll
    for (int k = 0; k < CMAXK; ++k)
      if (lane + 64 * k < D) cs[wave * D + lane + 64 * k] = acc[k];
  }
  if (lane == 0) ws[2 * wave] = sdead, ws[2 * wave + 1] = (float)ndead;
  __syncthreads();
  if (dvpart)
    for (int c = t; c < D; c += 64 * CW4) {
      float s = 0.f;
#pragma unroll
      for (int w = 0; w < CW4; ++w) s += cs[w * D + c];
      dvpart[(long)bi * D + c] = s;
    }
  if (t == 0) {
    float s = 0.f, n = 0.f;
#pragma unroll
    for (int w = 0; w < CW4; ++w) s += ws[2 * w], n += ws[2 * w + 1];
    sd[bi] = s;
    cw[bi] = n * inv;
  }
}

// dbias[c] = v[c] sum_rows sd + sum_rows cw[row] dEbar[row, c]   (v / dEbar may be NULL): one workgroup per 64 columns, rows
// strided over 4 waves, fixed order
__global__ __launch_bounds__(256) void cmp_bias_grad_kernel(const float* __restrict__ sd, const float* __restrict__ cw,
                                                            const float* __restrict__ dEbar, const float* __restrict__ v,
                                                            float* __restrict__ dbias, long rows, int D) {
  __shared__ float red[4][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
  float a = 0.f, s = 0.f;
  for (long r = wave; r < rows; r += 4) {
    if (dEbar && c < D) a = fmaf(cw[r], dEbar[r * D + c], a);
    s += sd[r];
  }
  red[wave][lane] = a;
  if (lane == 0) red[wave][64] = s;
  __syncthreads();
  if (wave == 0 && c < D) {
    const float at = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
    const float st = (red[0][64] + red[1][64]) + (red[2][64] + red[3][64]);
    dbias[c] = at + (v ? v[c] * st : 0.f);
  }
}

int cmp_check(const char* who, int B, int N, int D, const float* Ec, const int* prow, const float* bias) {
  GC_REQUIRE(B > 0 && N > 0 && D > 0 && (long)B * N <= 0x7fffffffL, "%s: bad shape B=%d N=%d D=%d", who, B, N, D);
  GC_REQUIRE(D <= 64 * CMAXK, "%s: hidden width %d (compact rows support up to %d)", who, D, 64 * CMAXK);
  GC_REQUIRE(Ec && prow && bias, "%s: null pointer", who);
  return 0;
}

int cmp_fwd(const CmpE& ce, const float* v, const int* n_valid, float* Ebar, const float* coladd, float* P, float* A, Drop drop,
            int B, int N, int D, hipStream_t st) {
  const bool att = P != nullptr;
  const EdgePlan p = edge_plan_fwd({B, N, D, true, att, false, false, 0});
  GC_REQUIRE(p.lds_ok(), "compact edge pass: N=%d D=%d needs %zu B of LDS", N, D, p.lds);
  ProfScope ps(att ? "edge_fwd_att" : "edge_fwd_mean", st, 0.0);
  const dim3 grid((unsigned)p.grid), block(64 * CW4);
  if (att) hipLaunchKernelGGL(cmp_edge_fwd_kernel<true>, grid, block, p.lds, st, ce, v, n_valid, Ebar, coladd, P, A, drop, N, D);
  else hipLaunchKernelGGL(cmp_edge_fwd_kernel<false>, grid, block, p.lds, st, ce, v, n_valid, Ebar, coladd, P, A, drop, N, D);
  return check_launch("cmp_edge_fwd");
}

int cmp_bwd(const CmpE& ce, const float* v, const int* n_valid, const float* dlogit, const float* dEbar, float* dEc, float* dvpart,
            float* rowbuf, float* dbias, const EdgePlan& p, int B, int N, int D, hipStream_t st) {
  const long BN = (long)B * N;
  float *sd = rowbuf, *cw = rowbuf + BN;
  {
    ProfScope ps("edge_bwd", st, 0.0);
    hipLaunchKernelGGL(cmp_edge_bwd_kernel, dim3((unsigned)p.grid), dim3(64 * CW4), p.lds, st, ce, v, n_valid, dlogit, dEbar, dEc, dvpart, sd, cw, N, D);
    GC_TRY(check_launch("cmp_edge_bwd"));
  }
  ProfScope ps("colsum", st, 0.0);
  hipLaunchKernelGGL(cmp_bias_grad_kernel, dim3(cdiv(D, 64)), dim3(256), 0, st, sd, cw, dEbar, dlogit ? v : nullptr, dbias, BN, D);
  return check_launch("cmp_bias_grad");
}

}  // namespace gc
