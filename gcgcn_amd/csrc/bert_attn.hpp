// What the fp32 attention kernels (bert.hip) and the bf16 ones (bert_attn_bf16.hip) share: the dropout decision of an element of the
// virtual [B][H][T][T] probability tensor, the document's penalty shift c_b and its live length.  Internal header.
#pragma once
#include "bert.hpp"

namespace gc {

// keep-scale of element (i, j) of the (b, h) slice of the virtual [B][H][T][T] probability tensor: 1 / (1 - p) or 0
__device__ __forceinline__ float attn_keep(const Drop& d, const uint64_t key, const uint64_t slice_row0, const int i, const int j, const int T) {
  const uint64_t idx = (slice_row0 + (uint64_t)i) * (uint64_t)T + (uint64_t)j;
  return rng_u32(key, idx) >= d.thresh ? d.scale : 0.f;
}

// c_b = the largest penalty of document b's keys (0 without key_bias), the same value in every thread.  The kernels work with
// key_bias - c_b: a softmax does not see a shift common to its keys, and a document whose keys are ALL masked (every penalty -10000)
// would otherwise lose the scores' low bits to the penalty's magnitude (one ulp of 1e4 is 1e-3).  lse is stored relative to c_b.
// Workgroups of 256 threads; holds one barrier.
__device__ __forceinline__ float doc_bias_max(const float* __restrict__ kb, const int T, float* sh) {
  if (!kb) return 0.f;
  float m = -INFINITY;
  for (int j = threadIdx.x; j < T; j += 256) m = fmaxf(m, kb[j]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = m;
  __syncthreads();
  return fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
}

// Token lengths (t_valid [B], row (b, t) is live iff t < t_valid[b]): the document's length clamped to [0, T], a scalar
__device__ __forceinline__ int live_len(const int* __restrict__ t_valid, const int b, const int T) {
  return __builtin_amdgcn_readfirstlane(min(max(t_valid[b], 0), T));
}

}  // namespace gc
