// C = op(A) op(B) (+ bias[col]) (+ add[row, col]) with bf16 operands on the bf16 matrix cores of gfx950 (v_mfma_f32_16x16x32_bf16).
// Internal header.  DESIGN.md section 8.9 ("bf16 matrix products").
//
// Operands and result are fp32 in memory; no bf16 tensor exists outside a workgroup's LDS.  Every operand element is rounded ONCE to
// bf16 (round to nearest even, what tensor.to(torch.bfloat16) does) on its way from global memory into the LDS image; products are
// exact in fp32, accumulation, epilogue and store are fp32.  The storage forms are those of gemm.hpp (a_kc / b_kc, lda / ldb / ldc /
// ldadd mean the same); there is no batching, alpha, relu, rowscale, C2, n_valid or row-block list.  Every M, N, K >= 1 is served:
// interior tiles of 16-byte aligned operands take the unguarded body, every other tile the guarded one (zeros are FED for k >= K and
// for rows / columns outside the views; nothing outside [M][K], [K][N], [M][N] is read or written, the ld padding included).
//
// Split K: where the 64 x 64 tile count leaves compute units idle and K is long, K is cut into `splits` runs of whole 64-deep steps;
// the partial tiles go to ws ([splits][M][N]) and one reduce kernel adds them in split order and runs the epilogue.  No float is
// added atomically: two runs are bitwise equal.  The weights are re-rounded by every tile that stages them (no bf16 scratch).
// Capturable: no host read, no allocation, no synchronisation, the caller's stream.
#pragma once
#include "common.hpp"

namespace gc {

struct GemmBf16Args {
  const float* A = nullptr;
  const float* B = nullptr;
  float* C = nullptr;
  int M = 0, N = 0, K = 0;
  long lda = 0, ldb = 0, ldc = 0;
  int a_kc = 1, b_kc = 0;
  const float* bias = nullptr;   // [N]
  const float* add = nullptr;    // [M][ldadd]
  long ldadd = 0;
  float* ws = nullptr;           // split-K partials, 16-byte aligned
  long ws_elems = 0;
};
inline GemmBf16Args gemm_bf16_stored(int a_kc, int b_kc, const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int N,
                                     int K) {
  GemmBf16Args g;
  g.A = A, g.lda = lda, g.a_kc = a_kc, g.B = B, g.ldb = ldb, g.b_kc = b_kc, g.C = C, g.ldc = ldc, g.M = M, g.N = N, g.K = K;
  return g;
}

// the split factor the launcher takes when the workspace allows it (1: no workspace is needed)
int gemm_bf16_splits(int M, int N, int K);
inline long gemm_bf16_ws_elems(int M, int N, int K) {
  const int s = gemm_bf16_splits(M, N, K);
  return s > 1 ? (long)s * M * N : 0;
}
// A workspace smaller than gemm_bf16_ws_elems (or none) is not an error: K is cut less often, or not at all.
int gemm_bf16(const GemmBf16Args& g, hipStream_t st);

}  // namespace gc
