// C = op(A) op(B) (+ bias[col]) (+ add[row, col]) with bf16 operands on the bf16 matrix cores of gfx950 (v_mfma_f32_16x16x32_bf16).
// Internal header.  DESIGN.md section 8.9 ("bf16 matrix products").
//
// Operands and result are fp32 in memory; no bf16 tensor exists outside a workgroup's LDS.  Every operand element is rounded ONCE to
// bf16 (round to nearest even, what tensor.to(torch.bfloat16) does) on its way from global memory into the LDS image; products are
// exact in fp32, accumulation, epilogue and store are fp32.  The storage forms are those of gemm.hpp (a_kc / b_kc, lda / ldb / ldc /
// ldadd mean the same), and so is the row-block list of a ragged batch (rb / rb_n / rb_mode / rb_zero: below); there is no batching,
// alpha, relu, rowscale, C2 or n_valid.  Every M, N, K >= 1 is served:
// interior tiles of 16-byte aligned operands take the unguarded body, every other tile the guarded one (zeros are FED for k >= K and
// for rows / columns outside the views; nothing outside [M][K], [K][N], [M][N] is read or written, the ld padding included).
//
// Split K: where the 64 x 64 tile count leaves compute units idle and K is long, K is cut into `splits` runs of whole 64-deep steps;
// the partial tiles go to ws ([splits][M][N]) and one reduce kernel adds them in split order and runs the epilogue.  No float is
// added atomically: two runs are bitwise equal.  The weights are re-rounded by every tile that stages them (no bf16 scratch).
// Capturable: no host read, no allocation, no synchronisation, the caller's stream.
//
// Row blocks (gemm.hpp has the list's contract: rb = all 16-row blocks of the [B T]-row tensors, the live ones first, *rb_n of them
// live, both on the device).  The grid, the split factor and the k cut are those of the dense launch; liveness is read by the kernel.
//   rb_mode 1 (a_kc = 1: forward products NT, data gradients NN; M = the document rows): virtual row m is memory row
//     rb[m / 16] * 16 + m % 16 of A, add and C (or the split's slab).  A tile past the live blocks does no arithmetic; a dead block of
//     a partly live tile is fed as zeros; dead blocks are stored as zeros when rb_zero is set and not at all otherwise (the reduce of a
//     split launch does the same and reads no slab row that was never written).  A row's sum runs over k in the dense order, so a live
//     row is bit for bit the dense launch's.
//   rb_mode 2 (a_kc = b_kc = 0: weight gradients TN; K = the document rows): a 64-deep k-step none of whose four blocks is live is
//     SKIPPED -- not fetched, staged or multiplied; every other step runs at its dense position, in the dense order, inside the dense
//     split run.  Live blocks are not gathered into denser steps: that would regroup the 32-deep matrix-instruction sums.  Skipping is
//     exact because both operands hold zeros on every padding row (the caller's contract) and acc + 0 = acc; a run without a live step
//     stores a tile of zeros.
// The launcher KEEPS the list iff all of: rb and rb_n are given; every pointer is 16-byte aligned, every ld a multiple of 4 and
// K % 64 == 0 (the unguarded body's conditions); M % 64 == 0 and N % 64 == 0 (every tile interior; in mode 1 also: whole tiles of four
// list entries); the storage form is the mode's (above); in mode 2 a split run has at most 1024 k-steps (its liveness bitmap).
// Otherwise the list is DROPPED and the product runs dense, which is equally correct by the zero-row argument when the outputs' dead
// rows may be written.  A launch that keeps the list is timed as "gemm_bf16_rb" (its reduce, like every reduce, as "gemm_bf16_reduce").
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
  const int* rb = nullptr;       // row blocks of a ragged batch (above); the entries are clamped to the problem's blocks when read
  const int* rb_n = nullptr;
  int rb_mode = 0, rb_zero = 0;
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
// the rule above: 0 = the launch drops the list (or has none), else g.rb_mode
int gemm_bf16_keeps_rows(const GemmBf16Args& g);

}  // namespace gc
