// The classifier head's bilinear passes with bf16 operands (head_bf16.hpp has the contract).
//
// The idea of head.hip's register-generated kernels carries over: the pair operand never touches LDS.  With k ordered so that the
// index of the register-resident factor is contiguous, a lane's 8-value fragment of v_mfma_f32_32x32x16_bf16 is ONE value of the
// slow factor times 8 consecutive values of the other one, which the lane holds in registers for the whole tile: eight v_mul and
// four packed converts per fragment, and the fragment feeds every column block of the wave.  Only the weight panel goes through
// LDS: fetched as fp32 (coalesced float4 along whichever index is contiguous in memory), rounded by the packed convert while the
// image is written -- [128 columns][64 k + 8 pad] bf16, k contiguous, 144-byte rows as in gemm_bf16.hip (the 16 rows of a fragment
// read fall on 16 disjoint 4-bank groups) -- and re-rounded by every tile that stages it: there is no bf16 copy of the weights.
// A workgroup of four waves owns 128 pair rows and every column; a wave 32 rows and NACC = ceil(columns / 32) accumulators (R = 97:
// a fourth block of which one column is stored; the compiler keeps what a narrower block would save, and the pass stays one body).
// The image is single-buffered: the loads of step s + 1 are issued before the matrix instructions of step s.
#include "head_bf16.hpp"

namespace gc {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int HW = 128;        // width of eh / et
constexpr int TK = 64;         // k-step
constexpr int LP = TK + 8;     // bf16 elements per image row
constexpr int TILE = 128;      // pair rows per workgroup; also the rows of the image
constexpr int DW_TILES = HW + 2;                 // column tiles of the weight-gradient launch: a = 0 .. 127, then dW_c's two halves
constexpr long DW_COLS = (long)DW_TILES * HW;    // columns of one row of a partial slab

// two floats -> two bf16, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ u32x4 pack8(float x0, float x1, float x2, float x3, float x4, float x5, float x6, float x7) {
  return u32x4{pack2(x0, x1), pack2(x2, x3), pack2(x4, x5), pack2(x6, x7)};
}
__device__ __forceinline__ f32x4 ldg4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// A 64-deep panel of an operand that goes through LDS.
//   KC  (stored [rows][k]): image row n is memory row min(n, lim - 1) (rows past the operand repeat its last one; their results are
//        never stored)
//   !KC (stored [k][rows], transposed while the image is written): k rows at and past lim are zeros that are never loaded
struct Panel {
  const float* src;
  long ld;
  int lim;
};

// What a thread holds of a panel between its global loads and its LDS writes.  NB: 32-row blocks of the image that are used.
//   KC : element j = float4 at row (t + 256 j) >> 4, k = 4 ((t + 256 j) & 15) .. + 3              (j < 2 NB)
//   !KC: element i = float4 at k = 8 (t >> 5) + i, rows 4 (t & 31) .. + 3                         (all 128 rows)
template <bool KC, int NB>
__device__ __forceinline__ void fetch(f32x4 (&v)[8], const Panel& p) {
  const int t = threadIdx.x;
  if constexpr (KC) {
#pragma unroll
    for (int j = 0; j < 2 * NB; ++j) {
      const int f = t + 256 * j;
      v[j] = ldg4(p.src + (long)min(f >> 4, p.lim - 1) * p.ld + 4 * (f & 15));
    }
  } else {
    const int k0 = 8 * (t >> 5), r = 4 * (t & 31);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      v[i] = ldg4(p.src + (long)min(k0 + i, p.lim - 1) * p.ld + r);
      if (k0 + i >= p.lim) v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
}
// A KC panel through per-thread element offsets computed once per tile (the main steps of a pass differ in src alone, which is
// uniform: one 32-bit register per element instead of a 64-bit address).
template <int NB>
__device__ __forceinline__ void kc_offsets(unsigned (&off)[8], const long ld, const int lim) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 2 * NB; ++j) {
    const int f = t + 256 * j;
    off[j] = (unsigned)(min(f >> 4, lim - 1) * ld + 4 * (f & 15));
  }
}
template <int NB>
__device__ __forceinline__ void fetch_at(f32x4 (&v)[8], const float* __restrict__ src, const unsigned (&off)[8]) {
#pragma unroll
  for (int j = 0; j < 2 * NB; ++j) v[j] = ldg4(src + off[j]);
}
template <bool KC, int NB>
__device__ __forceinline__ void stage(const f32x4 (&v)[8], __bf16* __restrict__ img) {
  const int t = threadIdx.x;
  if constexpr (KC) {
#pragma unroll
    for (int j = 0; j < 2 * NB; ++j) {
      const int f = t + 256 * j;
      *reinterpret_cast<uint2*>(img + (f >> 4) * LP + 4 * (f & 15)) = make_uint2(pack2(v[j][0], v[j][1]), pack2(v[j][2], v[j][3]));
    }
  } else {   // the transpose: row 4 (t & 31) + c takes component c of the eight k
    const int k0 = 8 * (t >> 5), r = 4 * (t & 31);
#pragma unroll
    for (int c = 0; c < 4; ++c)
      *reinterpret_cast<u32x4*>(img + (r + c) * LP + k0) = pack8(v[0][c], v[1][c], v[2][c], v[3][c], v[4][c], v[5][c], v[6][c], v[7][c]);
  }
}

// the fragment of image row `row` for the matrix instruction's k sub-step m (16 k each): k = 16 m + 8 (lane >> 5) .. + 7
__device__ __forceinline__ bf16x8 frag(const __bf16* __restrict__ img, const int row, const int m, const int lh) {
  return *reinterpret_cast<const bf16x8*>(img + row * LP + 16 * m + 8 * lh);
}

struct PassArgs {
  const float* P; const float* Q; const float* Wb; const float* Wc; const float* bias;
  float* C;
  int rows, R, ncol, ldc;
  const int* rows_dev; const int* crow;
  int sel_lo, sel_hi;
};

// The k sequence of a pass: 2 nA main steps (step 2 i + h: slow index i, half h of the register-resident factor), then the Linear's
// steps -- mode 1: eh's two halves, then et's two (the generated fragment with the factor 1); modes 2 and 3: dout's 64-deep steps.
template <int MODE, int NACC>
__global__ __launch_bounds__(256, 2) void head_bf16_pass_kernel(const PassArgs a) {
  __shared__ __attribute__((aligned(16))) __bf16 img[TILE * LP];
  constexpr bool MAIN_KC = MODE != 3, TAIL_KC = MODE == 1;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, lh = lane >> 5;
  const int m0 = blockIdx.x * TILE, row0 = m0 + 32 * wave;
  const int nrows = a.rows_dev ? *a.rows_dev : a.rows;
  if (m0 >= nrows || (a.rows_dev && (nrows < a.sel_lo || nrows >= a.sel_hi))) return;
  const long row = min(row0 + l31, nrows - 1);   // this lane's pair (clamped: rows past the end are computed and never stored)
  const float* __restrict__ prow = a.P + row * HW;
  const float* __restrict__ qrow = a.Q + row * HW;
  const int nA = MODE == 1 ? HW : a.R;
  const int ntail = MODE == 1 ? 4 : (a.R + TK - 1) / TK;
  const auto main_panel = [&](const int i, const int h) -> Panel {
    if (MODE == 1) return {a.Wb + (long)i * HW + TK * h, (long)HW * HW, a.R};                 // [n = r][k = b] of W_b[., a = i, .]
    if (MODE == 2) return {a.Wb + (long)i * HW * HW + TK * h, HW, HW};                         // [n = a][k = b] of W_b[r = i]
    return {a.Wb + (long)i * HW * HW + (long)TK * h * HW, HW, TK};                             // [k = a][n = b] of W_b[r = i]
  };
  const auto tail_panel = [&](const int u) -> Panel {
    if (MODE == 1) return {a.Wc + TK * u, 2 * HW, a.R};                                        // [n = r][k] of W_c
    return {a.Wc + (long)TK * u * 2 * HW + (MODE == 3 ? HW : 0), 2 * HW, a.R - TK * u};        // [k = r][n] of one half of W_c
  };

  f32x16 acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  // the lane's half of its Q row: q[blk] = Q[row, 16 blk + 8 lh .. + 7], the second factor of k sub-step blk & 3 of half blk >> 2
  f32x4 qa[8], qb[8];
#pragma unroll
  for (int blk = 0; blk < 8; ++blk) qa[blk] = ldg4(qrow + 16 * blk + 8 * lh), qb[blk] = ldg4(qrow + 16 * blk + 8 * lh + 4);

  const auto mfmas = [&](const u32x4 af, const int m) {
#pragma unroll
    for (int j = 0; j < NACC; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af), frag(img, 32 * j + l31, m, lh), acc[j], 0, 0, 0);
  };
  // four sub-steps of the generated operand: pa times half H of the Q row, an fp32 product rounded once
  const auto generated = [&](const float pa, const int H) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const f32x4 x = qa[4 * H + m] * pa, y = qb[4 * H + m] * pa;
      mfmas(pack8(x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]), m);
    }
  };
  // four sub-steps of an operand read as it is: src[16 m + 8 lh .. + 7] of the lane's row
  const auto direct = [&](const float* __restrict__ src) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {   // (a few steps of hundreds: loaded where it is used, not ahead -- the registers are the loop's)
      const f32x4 x = ldg4(src + 16 * m + 8 * lh), y = ldg4(src + 16 * m + 8 * lh + 4);
      mfmas(pack8(x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]), m);
    }
  };

  f32x4 v[8];
  unsigned moff[8];
  if constexpr (MAIN_KC) kc_offsets<NACC>(moff, main_panel(0, 0).ld, main_panel(0, 0).lim);
  const auto fetch_main = [&](const int i, const int h) {
    if constexpr (MAIN_KC) fetch_at<NACC>(v, main_panel(i, h).src, moff);
    else fetch<false, NACC>(v, main_panel(i, h));
  };
  fetch_main(0, 0);
  float pa = prow[0];
  for (int i = 0; i < nA; ++i) {
    const float pn = prow[min(i + 1, nA - 1)];   // the next step's slow factor, requested one step ahead
    __syncthreads();   // the previous step's readers are done with the image
    stage<MAIN_KC, NACC>(v, img);
    __syncthreads();
    fetch_main(i, 1);
    generated(pa, 0);
    __syncthreads();
    stage<MAIN_KC, NACC>(v, img);
    __syncthreads();
    if (i + 1 < nA) fetch_main(i + 1, 0);
    else fetch<TAIL_KC, NACC>(v, tail_panel(0));
    generated(pa, 1);
    pa = pn;
  }
  if constexpr (MODE == 1) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      __syncthreads();
      stage<TAIL_KC, NACC>(v, img);
      __syncthreads();
      if (u + 1 < 4) fetch<TAIL_KC, NACC>(v, tail_panel(u + 1));
      if (u < 2) direct(prow + TK * u);
      else generated(1.f, u - 2);
    }
  } else {
    for (int u = 0; u < ntail; ++u) {
      __syncthreads();
      stage<TAIL_KC, NACC>(v, img);
      __syncthreads();
      if (u + 1 < ntail) fetch<TAIL_KC, NACC>(v, tail_panel(u + 1));
      direct(prow + TK * u);
    }
  }

  // The build's MFMA hazard check wants 19 wait states between a low-precision matrix instruction and the first read of its result
  // on every path; twenty once per tile (gemm_bf16.hip has the argument).
  if constexpr (NACC == 1) asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0]));
  else if constexpr (NACC == 2) asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0]), "+v"(acc[1]));
  else if constexpr (NACC == 3) asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]));
  else asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));

  // lane holds column 32 j + l31 of rows row0 + mfma_row(r, lane)
#pragma unroll
  for (int j = 0; j < NACC; ++j) {
    const int col = 32 * j + l31;
    if (col >= a.ncol) continue;
    const float bias = a.bias ? a.bias[col] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long rw = row0 + mfma_row(r, lane);
      if (rw < nrows) a.C[(a.crow ? (long)a.crow[rw] : rw) * a.ldc + col] = acc[j][r] + bias;
    }
  }
}

struct DwArgs {
  const float* doutp; const float* EH; const float* ET;
  float* dWb; float* dWc; float* part;   // part != NULL: slabs [split][R][DW_COLS]
  long pairs; int R;
  const int* pairs_dev;
};

// Column tile ca of the weight gradients: ca < 128: dW_b[., a = ca, b]; 128 / 129: dW_c[., b] / dW_c[., 128 + b].  A workgroup owns
// every row r (NACC blocks of 32), wave w the columns b = 32 w .. + 31.  The generated operand B[k = pair][n = b] = eh[p, ca] et[p, b]
// (the factor is 1 for dW_c's tiles) is formed in registers from loads that run one k sub-step ahead; dout's 64 pairs of a step go
// through the image, transposed and rounded on the way ([r][pair], the rows past R are zeros of the padded dout).
template <int NACC>
__global__ __launch_bounds__(256, 2) void head_bf16_dw_kernel(const DwArgs a) {
  __shared__ __attribute__((aligned(16))) __bf16 img[TILE * LP];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, lh = lane >> 5;
  const int ca = blockIdx.x, sp = blockIdx.y, bcol = 32 * wave + l31;
  const long npairs = a.pairs_dev ? (long)*a.pairs_dev : a.pairs;
  const long kps = (((npairs + TK - 1) / TK) + gridDim.y - 1) / gridDim.y;   // k-steps of one split
  const long k_begin = sp * kps * TK, k_end = min(npairs, k_begin + kps * TK);
  const int nk = k_end > k_begin ? (int)((k_end - k_begin + TK - 1) / TK) : 0;
  const bool outer = ca < HW;
  const float* __restrict__ X = ca == HW ? a.EH : a.ET;   // the factor indexed by the column
  const long last = npairs - 1;

  f32x16 acc[NACC];
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  // the lane's eight pairs of one k sub-step, first pair p0: e = eh[p, ca] (or 1), q = X[p, b].  Pairs past the end repeat the last
  // one; dout is zero there.
  const auto gen_load = [&](float (&e)[8], float (&q)[8], const long p0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const long p = min(p0 + i, last);
      e[i] = outer ? a.EH[p * HW + ca] : 1.f;
      q[i] = X[p * HW + bcol];
    }
  };
  const auto mm = [&](const float (&e)[8], const float (&q)[8], const int m) {
    const u32x4 bf = pack8(e[0] * q[0], e[1] * q[1], e[2] * q[2], e[3] * q[3], e[4] * q[4], e[5] * q[5], e[6] * q[6], e[7] * q[7]);
#pragma unroll
    for (int j = 0; j < NACC; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(img, 32 * j + l31, m, lh), __builtin_bit_cast(bf16x8, bf), acc[j], 0, 0, 0);
  };

  if (nk > 0) {
    f32x4 v[8];
    float e0[8], q0[8], e1[8], q1[8];
    fetch<false, 4>(v, Panel{a.doutp + k_begin * HW, HW, (int)min(k_end - k_begin, (long)TK)});
    gen_load(e0, q0, k_begin + 8 * lh);
    for (int ks = 0; ks < nk; ++ks) {
      const long p0 = k_begin + (long)ks * TK;
      __syncthreads();
      stage<false, 4>(v, img);
      __syncthreads();
      if (ks + 1 < nk) fetch<false, 4>(v, Panel{a.doutp + (p0 + TK) * HW, HW, (int)min(k_end - p0 - TK, (long)TK)});
      gen_load(e1, q1, p0 + 16 + 8 * lh);
      mm(e0, q0, 0);
      gen_load(e0, q0, p0 + 32 + 8 * lh);
      mm(e1, q1, 1);
      gen_load(e1, q1, p0 + 48 + 8 * lh);
      mm(e0, q0, 2);
      gen_load(e0, q0, p0 + 64 + 8 * lh);   // the next step's first sub-step
      mm(e1, q1, 3);
    }
  }

  if constexpr (NACC == 1) asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0]));
  else if constexpr (NACC == 2) asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0]), "+v"(acc[1]));
  else if constexpr (NACC == 3) asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]));
  else asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]));

  // lane holds column bcol of rows 32 j + mfma_row(r, lane)
  float* __restrict__ o;
  long ldo;
  if (a.part) o = a.part + (long)sp * a.R * DW_COLS + (long)ca * HW + bcol, ldo = DW_COLS;
  else if (outer) o = a.dWb + (long)ca * HW + bcol, ldo = (long)HW * HW;
  else o = a.dWc + (long)(ca - HW) * HW + bcol, ldo = 2 * HW;
#pragma unroll
  for (int j = 0; j < NACC; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int rr = 32 * j + mfma_row(r, lane);
      if (rr < a.R) o[rr * ldo] = acc[j][r];
    }
}

// dW_b / dW_c = the slabs in split order: one thread per element of [R][DW_COLS]
__global__ __launch_bounds__(256) void head_bf16_dw_reduce_kernel(const float* __restrict__ part, float* __restrict__ dWb, float* __restrict__ dWc,
                                                                  const int R, const int splits) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x, n = (long)R * DW_COLS;
  if (e >= n) return;
  float s = 0.f;
  for (int y = 0; y < splits; ++y) s += part[(long)y * n + e];
  const long r = e / DW_COLS, c = e - r * DW_COLS;
  if (c < (long)HW * HW) dWb[r * HW * HW + c] = s;
  else dWc[r * 2 * HW + (c - (long)HW * HW)] = s;
}

__global__ __launch_bounds__(256) void head_bf16_zero_kernel(float* __restrict__ p, const long n) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e < n) p[e] = 0.f;
}

using PassKernel = void (*)(PassArgs);
using DwKernel = void (*)(DwArgs);
const PassKernel fwd_kernels[4] = {head_bf16_pass_kernel<1, 1>, head_bf16_pass_kernel<1, 2>, head_bf16_pass_kernel<1, 3>, head_bf16_pass_kernel<1, 4>};
const DwKernel dw_kernels[4] = {head_bf16_dw_kernel<1>, head_bf16_dw_kernel<2>, head_bf16_dw_kernel<3>, head_bf16_dw_kernel<4>};

}  // namespace

int head_bf16_pass(const HeadBf16Pass& p, hipStream_t st) {
  GC_REQUIRE(p.mode >= 1 && p.mode <= 3 && p.R >= 1 && p.R <= HW && p.rows >= 1, "head_bf16_pass: mode %d, R = %d, %d rows", p.mode, p.R, p.rows);
  GC_REQUIRE(p.P && p.Q && p.Wb && p.Wc && p.C, "head_bf16_pass: null operand");
  PassArgs a;
  a.P = p.P, a.Q = p.Q, a.Wb = p.Wb, a.Wc = p.Wc, a.bias = p.bias, a.C = p.C, a.rows = p.rows, a.R = p.R;
  a.ncol = a.ldc = p.mode == 1 ? p.R : HW;
  a.rows_dev = p.rows_dev, a.crow = p.crow, a.sel_lo = p.sel_lo, a.sel_hi = p.sel_hi;
  const PassKernel kernel = p.mode == 1 ? fwd_kernels[(p.R - 1) / 32] : p.mode == 2 ? head_bf16_pass_kernel<2, 4> : head_bf16_pass_kernel<3, 4>;
  const double flops = 2.0 * p.rows * a.ncol * (double)((p.mode == 1 ? HW : p.R) * HW + (p.mode == 1 ? 2 * HW : p.R));
  GC_LAUNCH_TIMED("head_bf16_bilinear", flops, kernel, dim3((unsigned)cdiv(p.rows, TILE)), dim3(256), 0, st, a);
  return check_launch("head_bf16_pass");
}

int head_bf16_zero(float* p, long n, hipStream_t st) {
  GC_REQUIRE(p && n >= 1 && cdiv(n, 256) >= 1, "head_bf16_zero: bad arguments");
  hipLaunchKernelGGL(head_bf16_zero_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, p, n);
  return check_launch("head_bf16_zero");
}

// Cut K while the 130 tiles do not give every compute unit two workgroups, a run keeps two k-steps and the workspace holds the slabs.
int head_bf16_dw_splits(long pairs, int R, long ws_elems) {
  const long ksteps = cdiv(pairs, TK);
  int s = 1;
  while (s < 4 && ksteps / (2 * s) >= 2 && (long)(2 * s) * R * DW_COLS <= ws_elems) s *= 2;
  return s;
}

int head_bf16_dw(const HeadBf16Dw& d, hipStream_t st) {
  GC_REQUIRE(d.R >= 1 && d.R <= HW && d.pairs >= 1, "head_bf16_dw: R = %d, %ld pairs", d.R, d.pairs);
  GC_REQUIRE(d.doutp && d.EH && d.ET && d.dWb && d.dWc, "head_bf16_dw: null operand");
  const int splits = d.ws ? head_bf16_dw_splits(d.pairs, d.R, d.ws_elems) : 1;
  DwArgs a;
  a.doutp = d.doutp, a.EH = d.EH, a.ET = d.ET, a.dWb = d.dWb, a.dWc = d.dWc, a.part = splits > 1 ? d.ws : nullptr;
  a.pairs = d.pairs, a.R = d.R, a.pairs_dev = d.pairs_dev;
  GC_LAUNCH_TIMED("head_bf16_bilinear", 2.0 * d.R * (double)DW_COLS * (double)d.pairs, dw_kernels[(d.R - 1) / 32], dim3(DW_TILES, splits), dim3(256), 0,
                  st, a);
  GC_TRY(check_launch("head_bf16_dw"));
  if (splits == 1) return 0;
  ProfScope ps("head_bf16_reduce", st);
  hipLaunchKernelGGL(head_bf16_dw_reduce_kernel, dim3(cdiv((long)d.R * DW_COLS, 256)), dim3(256), 0, st, a.part, d.dWb, d.dWc, d.R, splits);
  return check_launch("head_bf16_dw_reduce");
}

}  // namespace gc
