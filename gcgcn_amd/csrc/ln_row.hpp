// The LayerNorm row arithmetic of the BERT path: ONE body for res_ln_fwd_kernel / res_ln_bwd_kernel (bert.hip) and the fused
// embeddings stage (bert_embed.hip), so the two cannot drift -- from the same row values they produce the same bits.  One wave owns a
// row; lane l holds columns l + 64 i, i < n = D / 64 <= LNV, in registers (entries at i >= n are zero).  Internal header.
#pragma once
#include "bert.hpp"

namespace gc {

constexpr int LNV = BERT_LN_MAX_D / 64;

// mean and 1 / sqrt(var + eps) of the row; two-pass, biased variance: a constant row has var = 0
__device__ __forceinline__ void ln_row_stats(const float (&v)[LNV], const int n, const int D, float& m, float& r) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LNV; ++i) s += v[i];
  m = wave_sum(s) / (float)D;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < LNV; ++i)
    if (i < n) sq += (v[i] - m) * (v[i] - m);
  r = 1.f / sqrtf(wave_sum(sq) / (float)D + BERT_LN_EPS);
}
__device__ __forceinline__ float ln_row_out(const float v, const float m, const float r, const float w, const float b) {
  return w * ((v - m) * r) + b;
}

// v: the row's LayerNorm input (left holding xhat).  dload(i): the gradient arriving on the output's column l + 64 i; dstore(i, dv):
// takes the gradient of the input's column l + 64 i; each called once per i < n, where the row body has the value.  aw += d * xhat and
// ab += d per column (the weight's and the bias' column sums of the wave's rows).
template <class DLoad, class DStore>
__device__ __forceinline__ void ln_row_bwd(float (&v)[LNV], const DLoad dload, const DStore dstore, const float* __restrict__ weight,
                                           const int n, const int D, const int l, const float m, const float r, float (&aw)[LNV],
                                           float (&ab)[LNV]) {
  float g[LNV];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < LNV; ++i) {
    g[i] = 0.f;
    if (i < n) {
      const float d = dload(i);
      v[i] = (v[i] - m) * r;   // xhat
      g[i] = d * weight[l + 64 * i];
      s1 += g[i], s2 += g[i] * v[i];
      aw[i] += d * v[i], ab[i] += d;
    }
  }
  s1 = wave_sum(s1) / (float)D, s2 = wave_sum(s2) / (float)D;
#pragma unroll
  for (int i = 0; i < LNV; ++i)
    if (i < n) dstore(i, r * (g[i] - s1 - v[i] * s2));
}

// The four waves of a workgroup meet in LDS in a fixed order: part [gridDim.x][2][D] gets this workgroup's column sums.
__device__ __forceinline__ void ln_part_store(float (&sh)[4][2][BERT_LN_MAX_D], const float (&aw)[LNV], const float (&ab)[LNV],
                                              float* __restrict__ part, const int n, const int D, const int wv, const int l) {
#pragma unroll
  for (int i = 0; i < LNV; ++i)
    if (i < n) sh[wv][0][l + 64 * i] = aw[i], sh[wv][1][l + 64 * i] = ab[i];
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * D; c += 256) {
    const int k = c >= D, cc = c - k * D;
    part[(long)blockIdx.x * 2 * D + c] = (sh[0][k][cc] + sh[1][k][cc]) + (sh[2][k][cc] + sh[3][k][cc]);
  }
}

}  // namespace gc
