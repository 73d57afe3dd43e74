// The classifier head's four bilinear passes with bf16 operands on v_mfma_f32_32x32x16_bf16 (head_bf16.hip; DESIGN.md section 8.3,
// "bf16 bilinear passes").  Internal header; head.hip's head_plan decides when these run (option head_matmul = 1) and nothing else calls them.
//
// What is computed (gcgcn_amd.functional.Bf16HeadBilinearFn is the definition the tests hold the kernels to; bf16(.) rounds once to
// nearest even, every sum is fp32, eh / et / dout / the weights are fp32 in memory and no bf16 copy of anything exists outside LDS):
//   mode 1  C[p, r] = sum_ab bf16(eh[p,a] et[p,b]) bf16(W_b[r,a,b]) + sum_k bf16([eh | et][p,k]) bf16(W_c[r,k]) + bias[r]
//   mode 2  C[p, a] = sum_rb bf16(dout[p,r] et[p,b]) bf16(W_b[r,a,b]) + sum_r bf16(dout[p,r]) bf16(W_c[r,a])              (d eh)
//   mode 3  C[p, b] = sum_ra bf16(dout[p,r] eh[p,a]) bf16(W_b[r,a,b]) + sum_r bf16(dout[p,r]) bf16(W_c[r,128 + b])        (d et)
//   dw      dW_b[r,a,b] = sum_p bf16(dout[p,r]) bf16(eh[p,a] et[p,b]),   dW_c[r,:] = sum_p bf16(dout[p,r]) bf16([eh | et][p,:])
// The generated operand is an fp32 product rounded once; the bias is added unrounded in the epilogue.  No float is added atomically
// (two runs are bitwise equal), nothing is read on the host, every launch is capturable.
#pragma once
#include "common.hpp"

namespace gc {

// One pass over the pair rows.  P: the factor indexed by the slow k index (eh; dout padded to 128 columns), Q: the factor whose 128
// values a lane keeps in registers (et; et; eh).  rows_dev / crow / sel_lo / sel_hi: as in head.hip's Bil2 (compacted pair rows: the
// count lives on the device, output row r goes to row crow[r] of C, the launch runs only when sel_lo <= *rows_dev < sel_hi).
struct HeadBf16Pass {
  int mode;   // 1, 2, 3
  const float* P; const float* Q; const float* Wb; const float* Wc; const float* bias;
  float* C;
  int rows, R;
  const int* rows_dev; const int* crow;
  int sel_lo, sel_hi;
};
int head_bf16_pass(const HeadBf16Pass& a, hipStream_t st);
// p[0 .. n) = 0 by a kernel: the padded logits of a compacted batch (DESIGN.md section 8.3 says what was observed with the fp32
// route's hipMemsetAsync under graph replay; its cause is open).
int head_bf16_zero(float* p, long n, hipStream_t st);

// dW_b and dW_c in one launch (130 column tiles: one per a, then the eh and the et half of dW_c).  K = pairs, or *pairs_dev; split
// over up to four workgroups per tile when ws holds the slabs ([splits][R][130 * 128] floats), summed in split order by a reduce.
struct HeadBf16Dw {
  const float* doutp; const float* EH; const float* ET;
  float* dWb; float* dWc;   // [R][128][128], [R][256]
  float* ws; long ws_elems;
  long pairs; int R;
  const int* pairs_dev;
};
int head_bf16_dw_splits(long pairs, int R, long ws_elems);
int head_bf16_dw(const HeadBf16Dw& a, hipStream_t st);

}  // namespace gc
