// The token encoder's LSTM layer (EncoderLSTM, glove:377-428): nn.LSTM(input_size, 128, 1, batch_first=True), one or two
// directions, every one of the T padded steps -- or, with per-row lengths (lens), the semantics of a packed sequence: row b is
// active at time t iff t < lens[b]; an inactive step leaves the row's h and c alone and puts 0 into the output; the reverse
// direction of row b starts at t = lens[b] - 1 from h0 / c0.  DESIGN.md section 8.7.
//
//   forward :  gates = X [W_ih_f; W_ih_r]^T + (b_ih + b_hh)      one product of the GEMM layer (gemm_nt + bias)
//              lstm_fwd_kernel                                   the whole time loop, one workgroup per (direction, 16 batch rows)
//   backward:  lstm_bwd_kernel                                   the time loop reversed, same grid: dgates, dh0, dc0
//              lstm_hprev_kernel                                 H_prev = the output shifted one step, h0 at a direction's first step
//              dW_ih = dgates^T X, dW_hh = dgates^T H_prev, dX = dgates W_ih, db = column sums of dgates: GEMM-layer launches
//
// A recurrence workgroup is eight waves.  Wave w owns hidden units [16 w, 16 w + 16) of ALL FOUR gates, so the cell update of a
// unit happens inside one lane and c never leaves the registers.  The wave's slice of W_hh is the B operand of
// v_mfma_f32_16x16x4_f32 and stays in 128 registers for the whole launch; the A operand (h_{t-1}, or dgates_t in the backward) is
// read from a double-buffered LDS image, one __syncthreads() per step.  No workgroup reads what another one of the launch
// writes, nothing is added atomically: two runs are bitwise equal.
//
// Lengths.  The recurrence kernels are templates on LEN; LEN = false (lens == nullptr) is the code without lengths.  With LEN a
// workgroup loops Lt = the largest length among its 16 rows (uniform) instead of T, the reverse direction from t = Lt - 1, and
// zero-fills [Lt, T) of what it owns afterwards, so every element is written by the launch.  Lengths are clamped into [0, T].
// Freezing a row is a select in the cell update; nothing branches around an MFMA.  What the forward leaves unwritten at inactive
// steps (csave, the activated gates) the backward reads only through selects, as it does dout there: NaN in it reaches nothing.
//
// Lane maps of the 16x16x4 form (lane l, c16 = l & 15, q = l >> 4): A[row c16][k q], B[k q][col c16], C/D [row 4 q + r][col c16].
// The sum over k may run in any order as long as A and B agree, so k-step s of lane group q takes k = q * (K / 4) + s: a lane's A
// values are then CONTIGUOUS in the LDS row (ds_read_b128) and the forward's weights contiguous in W_hh's rows.
//
// bf16 recurrence (recurrent = 1; DESIGN.md section 8.7, "bf16 recurrence").  The recurrence kernels are templates on BF as well;
// BF = false is the code above, unchanged.  With BF the two recurrent products -- h_{t-1} W_hh^T forward, dgates_t W_hh backward --
// take bf16 operands on v_mfma_f32_16x16x32_bf16 and accumulate in fp32: the wave's slice of W_hh is rounded once at load (64
// registers instead of 128), the LDS image holds the rounding of h (of dgates_t) and nothing else is rounded -- the input
// projection, the cell update, c, out, the saved gates, csave and the dgates that go to global memory are the fp32 values; the
// cell update, the requests one step ahead and the length selects are the SAME statements for both formats.
// Lane maps of the 16x16x32 form: A[row c16][k 8 q + j], B[k 8 q + j][col c16], j = 0 .. 7 (one ds_read_b128 per lane and
// 32-deep k-block), C/D as above.  A and B use the instruction's own k order.
// The bf16 LDS image (lstm_bf_row): rows of K bf16, K * 2 a multiple of 256 bytes.  ds_read_b128 is served in four groups of 16
// lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32, i.e. rows {0-3, 12-15} of lane group q with rows {4-11} of
// lane group q + 1, over 64 banks = 16 slots of 16 bytes; a lane reads slot (row's first slot + 4 kb + q) mod 16.  A constant
// odd pitch cannot separate the two halves of such a group (row -> slot is then a permutation of all 16 slots, and the q + 1
// rows land one slot further), so the pitch is K * 2 + 32 bytes (2 slots: rows 8 apart share a slot, rows {0-3, 12-15} take the
// eight even slots, rows {4-11} + 1 the eight odd ones).  The 2-byte writes go to 32 banks in halves of 32 lanes: lane groups q
// and q + 1 write rows 4 apart, 16 consecutive units each (8 banks).  Four pitches are a multiple of 32 banks, so rows 4 .. 11
// start another 32 bytes later: the rows of a half are then 8 (q = 0, 1) and 24 (q = 2, 3) banks apart, and the reads keep
// their even slots (2 more for all of rows 4 .. 11).  Neither access conflicts.
#include "lstm.hpp"
#include "gemm.hpp"

namespace gc {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int LH = LSTM_H;
constexpr int LROWS = 16;            // batch rows of a workgroup = rows of an MFMA tile
constexpr int LHS = LH + 4;          // LDS row stride of the h image: rows 4 banks apart
constexpr int LGS = 4 * LH + 4;      // ... of the dgates image
static_assert(2 * LROWS * LGS * sizeof(float) <= 160 * 1024, "LDS of one compute unit");
constexpr int LHB = LH + 16;         // bf16 images: elements per row of the h image (288 bytes) ...
constexpr int LGB = 4 * LH + 16;     // ... and of the dgates image (1056 bytes); rows are placed by lstm_bf_row
constexpr int LSTM_FP32 = 0, LSTM_BF16 = 1;   // the recurrent argument of a call (lstm.hpp)

// element offset of row `row` of a bf16 image of pitch `pitch`: rows 4 .. 11 start 16 elements (32 bytes) later (top of the file)
__device__ __forceinline__ int lstm_bf_row(int row, int pitch) { return row * pitch + 16 * (((row + 4) >> 3) & 1); }
// one rounding to bf16, nearest even (what tensor.to(torch.bfloat16) does)
__device__ __forceinline__ __bf16 lstm_bf(float x) { return static_cast<__bf16>(x); }
// eight consecutive floats -> the eight bf16 of one operand fragment
__device__ __forceinline__ bf16x8 lstm_bf8(const float4 lo, const float4 hi) {
  const f32x2 a = {lo.x, lo.y}, b = {lo.z, lo.w}, c = {hi.x, hi.y}, d = {hi.z, hi.w};
  const bf16x2 pa = __builtin_convertvector(a, bf16x2), pb = __builtin_convertvector(b, bf16x2);
  const bf16x2 pc = __builtin_convertvector(c, bf16x2), pd = __builtin_convertvector(d, bf16x2);
  return bf16x8{pa[0], pa[1], pb[0], pb[1], pc[0], pc[1], pd[0], pd[1]};
}
// The build's MFMA hazard check prices every low-precision matrix instruction as a 16-pass one (19 wait states before its result is
// read); the compiler leaves what this shorter one needs.  Twenty wait states once per step satisfy the stricter count (a step is
// thousands of cycles).  The accumulators are operands of the statement so that no read of them moves in front of it.
__device__ __forceinline__ void lstm_settle(f32x4 (&a)[4]) { asm volatile("s_nop 15\n\ts_nop 3" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3])); }

__device__ __forceinline__ float lstm_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ int lstm_len(const int* __restrict__ lens, int b, int T) {
  const int n = lens[b];
  return n < 0 ? 0 : n > T ? T : n;
}
// the largest length among the workgroup's rows [b0, b0 + 16) that exist: the same value in every lane
__device__ __forceinline__ int lstm_tile_len(const int* __restrict__ lens, int b0, int B, int T) {
  int lt = 0;
  for (int j = 0; j < LROWS && b0 + j < B; ++j) {
    const int n = lstm_len(lens, b0 + j, T);
    lt = n > lt ? n : lt;
  }
  return __builtin_amdgcn_readfirstlane(lt);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------
template <bool LEN, bool BF>
__global__ __launch_bounds__(512) void lstm_fwd_kernel(const float* __restrict__ w_hh, const float* __restrict__ h0,
                                                       const float* __restrict__ c0, float* __restrict__ gates, float* __restrict__ out,
                                                       float* __restrict__ csave, const int* __restrict__ lens, const int B, const int T,
                                                       const int nd) {
  // the h image, double-buffered: fp32 [2][16][LHS], or bf16 [2] x 16 rows placed by lstm_bf_row(., LHB)
  constexpr int IMG = BF ? LROWS * LHB : LROWS * LHS;   // elements of one buffer
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * IMG * (BF ? sizeof(__bf16) : sizeof(float))];
  float* const hbuf = reinterpret_cast<float*>(lds);
  __bf16* const hbf = reinterpret_cast<__bf16*>(lds);
  const int dir = blockIdx.y, b0 = blockIdx.x * LROWS;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c16 = l & 15, q = l >> 4;
  const int u = 16 * w + c16;   // the hidden unit of this lane's accumulator column
  const int wrow = BF ? lstm_bf_row(4 * q, LHB) + u : 4 * q * LHS + u;   // the lane's first row in the image; its rows are
  constexpr int wstep = BF ? LHB : LHS;                                  // 4 q + r, all on one side of lstm_bf_row's shift

  // B operand: W_hh^T[k][g H + u] = W_hh[g H + u][k]; fp32: k = 32 q + s; bf16: k-block kb holds k = 32 kb + 8 q .. + 7, rounded here
  float wr[BF ? 1 : 4][BF ? 1 : 32];
  bf16x8 wb[BF ? 4 : 1][BF ? 4 : 1];
  const float* wd = w_hh + (long)dir * 4 * LH * LH;
  if constexpr (BF) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        const float* wp = wd + (long)(g * LH + u) * LH + 32 * kb + 8 * q;
        wb[g][kb] = lstm_bf8(*reinterpret_cast<const float4*>(wp), *reinterpret_cast<const float4*>(wp + 4));
      }
  } else {
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float4 v = *reinterpret_cast<const float4*>(wd + (long)(g * LH + u) * LH + 32 * q + 4 * j);
        wr[g][4 * j] = v.x, wr[g][4 * j + 1] = v.y, wr[g][4 * j + 2] = v.z, wr[g][4 * j + 3] = v.w;
      }
  }

  // the lane's four rows (C/D map): batch entries b0 + 4 q + r.  Rows past B read zeros (through a clamped address) and store nothing.
  bool valid[4];
  long grow[4], orow[4];   // element offsets of step 0 of the row in gates and in out / csave, this direction's column included
  float c[4];
  float hk[4];   // LEN: the row's h, carried into the next LDS buffer over an inactive step
  int len[4];    // LEN: the row's length
  const int Lt = LEN ? lstm_tile_len(lens, b0, B, T) : T;   // steps of this workgroup
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = b0 + 4 * q + r, bc = b < B ? b : B - 1;
    valid[r] = b < B;
    grow[r] = (long)bc * T * (nd * 4 * LH) + dir * 4 * LH + u;
    orow[r] = (long)bc * T * (nd * LH) + dir * LH + u;
    const long s0 = ((long)dir * B + bc) * LH + u;
    c[r] = valid[r] ? c0[s0] : 0.f;
    hk[r] = valid[r] ? h0[s0] : 0.f;
    if constexpr (BF) hbf[wrow + r * wstep] = lstm_bf(hk[r]);
    else hbuf[wrow + r * wstep] = hk[r];
    len[r] = LEN ? lstm_len(lens, bc, T) : T;
  }
  const long gstep = (long)nd * 4 * LH, ostep = (long)nd * LH;

  float gn[4][4];   // the input projection of the NEXT step, requested one step ahead
  {
    const int t0 = LEN ? (dir && Lt > 0 ? Lt - 1 : 0) : (dir ? T - 1 : 0);   // Lt = 0: nothing runs, the request stays in bounds
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) gn[g][r] = gates[grow[r] + t0 * gstep + g * LH];
  }
  __syncthreads();

  for (int s = 0; s < Lt; ++s) {
    const int t = dir ? Lt - 1 - s : s;
    const int sn = s + 1 < Lt ? s + 1 : s, tn = dir ? Lt - 1 - sn : sn;   // the last step asks for itself again (unused)
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[g][r] = valid[r] ? gn[g][r] : 0.f;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r) gn[g][r] = gates[grow[r] + tn * gstep + g * LH];

    if constexpr (BF) {   // 16 instructions; the four gates' chains interleaved, a dependent one three instructions later
      const __bf16* hp = hbf + (s & 1) * IMG + lstm_bf_row(c16, LHB) + 8 * q;
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(hp + 32 * kb);
#pragma unroll
        for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wb[g][kb], acc[g], 0, 0, 0);
      }
      lstm_settle(acc);
    } else {
      const float* hp = hbuf + (s & 1) * IMG + c16 * LHS + 32 * q;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float4 a = *reinterpret_cast<const float4*>(hp + 4 * j);
        const float av[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e], wr[g][4 * j + e], acc[g], 0, 0, 0);
      }
    }

    const int hn = ((s & 1) ^ 1) * IMG + wrow;   // the lane's first row in the next buffer
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gi = lstm_sigmoid(acc[0][r]), gf = lstm_sigmoid(acc[1][r]), gg = tanhf(acc[2][r]), go = lstm_sigmoid(acc[3][r]);
      if constexpr (LEN) {
        const bool act = t < len[r];
        const float cn = __builtin_fmaf(gf, c[r], gi * gg);   // spelled out: both instantiations round alike
        c[r] = act ? cn : c[r];
        const float h = go * tanhf(cn);
        hk[r] = act ? h : hk[r];
        if constexpr (BF) hbf[hn + r * wstep] = lstm_bf(hk[r]);
        else hbuf[hn + r * wstep] = hk[r];
        if (valid[r]) {
          out[orow[r] + t * ostep] = act ? h : 0.f;
          if (csave && act) {
            float* gp = gates + grow[r] + t * gstep;
            gp[0] = gi, gp[LH] = gf, gp[2 * LH] = gg, gp[3 * LH] = go;
            csave[orow[r] + t * ostep] = cn;
          }
        }
      } else {
        c[r] = __builtin_fmaf(gf, c[r], gi * gg);
        const float h = go * tanhf(c[r]);
        if constexpr (BF) hbf[hn + r * wstep] = lstm_bf(h);
        else hbuf[hn + r * wstep] = h;
        if (valid[r]) {
          out[orow[r] + t * ostep] = h;
          if (csave) {
            float* gp = gates + grow[r] + t * gstep;
            gp[0] = gi, gp[LH] = gf, gp[2 * LH] = gg, gp[3 * LH] = go;
            csave[orow[r] + t * ostep] = c[r];
          }
        }
      }
    }
    __syncthreads();
  }
  if constexpr (LEN) {   // the tile's tail: no row of it is active there
    for (int t = Lt; t < T; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (valid[r]) out[orow[r] + t * ostep] = 0.f;
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------------
// LEN: an inactive step has dgates_t = 0 (LDS image and global memory) and hands dh and dc on unchanged -- the zero LDS row adds
// nothing to the product, so the row keeps its old dh.  c_prev is c0 at the ROW's first step: t = lens[b] - 1 in the reverse
// direction.  Whatever is read at an inactive step (the saved gates, csave, dout: possibly never written, possibly NaN) is
// replaced by 0 through a select, never multiplied by a 0 / 1 flag.
template <bool LEN, bool BF>
__global__ __launch_bounds__(512) void lstm_bwd_kernel(const float* __restrict__ w_hh, const float* __restrict__ c0,
                                                       const float* __restrict__ gates, const float* __restrict__ csave,
                                                       const float* __restrict__ dout, float* __restrict__ dgates, float* __restrict__ dh0,
                                                       float* __restrict__ dc0, const int* __restrict__ lens, const int B, const int T,
                                                       const int nd) {
  // the dgates_t image, double-buffered: fp32 [2][16][LGS], or bf16 [2] x 16 rows placed by lstm_bf_row(., LGB)
  constexpr int IMG = BF ? LROWS * LGB : LROWS * LGS;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * IMG * (BF ? sizeof(__bf16) : sizeof(float))];
  float* const gbuf = reinterpret_cast<float*>(lds);
  __bf16* const gbf = reinterpret_cast<__bf16*>(lds);
  const int dir = blockIdx.y, b0 = blockIdx.x * LROWS;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c16 = l & 15, q = l >> 4;
  const int u = 16 * w + c16;
  const int wrow = BF ? lstm_bf_row(4 * q, LGB) + u : 4 * q * LGS + u;   // as in the forward
  constexpr int wstep = BF ? LGB : LGS;

  // B operand of dh_rec = dgates W_hh: W_hh[k][u] over the 4H gate columns; fp32: k = 128 q + s; bf16: k-block kb holds
  // k = 32 kb + 8 q .. + 7, rounded here (a strided load, once per launch)
  float wr[BF ? 1 : 128];
  bf16x8 wb[BF ? 16 : 1];
  const float* wd = w_hh + (long)dir * 4 * LH * LH;
  if constexpr (BF) {
#pragma unroll
    for (int kb = 0; kb < 16; ++kb)
#pragma unroll
      for (int j = 0; j < 8; ++j) wb[kb][j] = lstm_bf(wd[(long)(32 * kb + 8 * q + j) * LH + u]);
  } else {
#pragma unroll
    for (int s = 0; s < 128; ++s) wr[s] = wd[(long)(128 * q + s) * LH + u];
  }

  bool valid[4];
  long grow[4], orow[4], srow[4];
  int len[4];   // LEN: the row's length, 0 for a row past B (never active)
  const int Lt = LEN ? lstm_tile_len(lens, b0, B, T) : T;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int b = b0 + 4 * q + r, bc = b < B ? b : B - 1;
    valid[r] = b < B;
    grow[r] = (long)bc * T * (nd * 4 * LH) + dir * 4 * LH + u;
    orow[r] = (long)bc * T * (nd * LH) + dir * LH + u;
    srow[r] = ((long)dir * B + bc) * LH + u;
    len[r] = LEN ? (valid[r] ? lstm_len(lens, bc, T) : 0) : T;
  }
  const long gstep = (long)nd * 4 * LH, ostep = (long)nd * LH;

  float dh[4] = {0.f, 0.f, 0.f, 0.f}, dc[4] = {0.f, 0.f, 0.f, 0.f};   // what the later step hands back
  float gt[4][4], ct[4], cp[4], dy[4];                                  // step operands, requested one step ahead
  // step s of this loop undoes forward step Lt - 1 - s, which ran at time t; the forward's previous time is tp.  An inactive
  // row's c_prev address is c0's: t + 1 may lie past the row's end, and the value is dropped anyway.
#define LSTM_BWD_REQUEST(S)                                                                          \
  {                                                                                                  \
    const int fs_ = Lt - 1 - (S), t_ = dir ? Lt - 1 - fs_ : fs_, tp_ = dir ? t_ + 1 : t_ - 1;        \
    _Pragma("unroll") for (int r = 0; r < 4; ++r) {                                                  \
      _Pragma("unroll") for (int g = 0; g < 4; ++g) gt[g][r] = gates[grow[r] + t_ * gstep + g * LH]; \
      ct[r] = csave[orow[r] + t_ * ostep];                                                           \
      const bool first_ = LEN ? (dir ? t_ >= len[r] - 1 : t_ == 0) : fs_ == 0;                       \
      const float* pp_ = first_ ? c0 + srow[r] : csave + orow[r] + tp_ * ostep;                      \
      cp[r] = *pp_;                                                                                  \
      dy[r] = dout[orow[r] + t_ * ostep];                                                            \
    }                                                                                                \
  }
  if (!LEN || Lt > 0) LSTM_BWD_REQUEST(0)

  for (int s = 0; s < Lt; ++s) {
    const int fs = Lt - 1 - s, t = dir ? Lt - 1 - fs : fs;
    const int gw = (s & 1) * IMG;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float gi, gf, gg, go, dyv, cv, cpv;
      const bool act = LEN ? t < len[r] : valid[r];
      if constexpr (LEN) {
        gi = act ? gt[0][r] : 0.f, gf = act ? gt[1][r] : 0.f, gg = act ? gt[2][r] : 0.f, go = act ? gt[3][r] : 0.f;
        dyv = act ? dy[r] : 0.f, cv = act ? ct[r] : 0.f, cpv = act ? cp[r] : 0.f;
      } else {
        const float z = valid[r] ? 1.f : 0.f;
        gi = z * gt[0][r], gf = z * gt[1][r], gg = z * gt[2][r], go = z * gt[3][r];
        dyv = z * dy[r], cv = z * ct[r], cpv = z * cp[r];
      }
      const float dhv = dyv + dh[r];
      const float tc = tanhf(cv);
      const float dcv = dc[r] + dhv * go * (1.f - tc * tc);
      float da_i = dcv * gg * gi * (1.f - gi);
      float da_f = dcv * cpv * gf * (1.f - gf);
      float da_g = dcv * gi * (1.f - gg * gg);
      float da_o = dhv * tc * go * (1.f - go);
      if constexpr (LEN) {
        da_i = act ? da_i : 0.f, da_f = act ? da_f : 0.f, da_g = act ? da_g : 0.f, da_o = act ? da_o : 0.f;
        dc[r] = act ? dcv * gf : dc[r];
      } else {
        dc[r] = dcv * gf;
      }
      if constexpr (BF) {   // the image holds the rounding; global memory (below) the fp32 values
        __bf16* lp = gbf + gw + wrow + r * wstep;
        lp[0] = lstm_bf(da_i), lp[LH] = lstm_bf(da_f), lp[2 * LH] = lstm_bf(da_g), lp[3 * LH] = lstm_bf(da_o);
      } else {
        float* lp = gbuf + gw + wrow + r * wstep;
        lp[0] = da_i, lp[LH] = da_f, lp[2 * LH] = da_g, lp[3 * LH] = da_o;
      }
      if (valid[r]) {
        float* gp = dgates + grow[r] + t * gstep;
        gp[0] = da_i, gp[LH] = da_f, gp[2 * LH] = da_g, gp[3 * LH] = da_o;
      }
    }
    {
      const int sn = s + 1 < Lt ? s + 1 : s;   // the last step asks for itself again (unused)
      LSTM_BWD_REQUEST(sn)
    }
    __syncthreads();

    f32x4 acc[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (BF) {   // 16 instructions on the same four chains: k-block kb goes to chain kb & 3
      const __bf16* ap = gbf + gw + lstm_bf_row(c16, LGB) + 8 * q;
#pragma unroll
      for (int kb = 0; kb < 16; ++kb) {
        const bf16x8 a = *reinterpret_cast<const bf16x8*>(ap + 32 * kb);
        acc[kb & 3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, wb[kb], acc[kb & 3], 0, 0, 0);
      }
      lstm_settle(acc);
    } else {
      const float* ap = gbuf + gw + c16 * LGS + 128 * q;
#pragma unroll
      for (int j = 0; j < 32; ++j) {
        const float4 a = *reinterpret_cast<const float4*>(ap + 4 * j);
        acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, wr[4 * j], acc[0], 0, 0, 0);       // four independent chains: the
        acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, wr[4 * j + 1], acc[1], 0, 0, 0);   // instruction's dependent latency
        acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, wr[4 * j + 2], acc[2], 0, 0, 0);   // exceeds its issue interval
        acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, wr[4 * j + 3], acc[3], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float rec = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
      dh[r] = !LEN || t < len[r] ? rec : dh[r];
    }
  }
#undef LSTM_BWD_REQUEST
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (valid[r]) dh0[srow[r]] = dh[r], dc0[srow[r]] = dc[r];
  if constexpr (LEN) {   // the tile's tail: the gradient products read all B * T rows of dgates
    for (int t = Lt; t < T; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (valid[r]) {
          float* gp = dgates + grow[r] + t * gstep;
          gp[0] = 0.f, gp[LH] = 0.f, gp[2 * LH] = 0.f, gp[3 * LH] = 0.f;
        }
  }
}

// H_prev[b][t][dir H + u] = h of the direction's previous step: out one step back in the direction's own order, h0 at its first step.
// With lengths the reverse direction's first step is t = lens[b] - 1, and every later (padded) t takes h0 too: dgates is zero
// there, so any finite value serves, and out[t + 1] would lie past the row at t = T - 1.  The forward direction's padded rows
// read the output's zeros.
__global__ __launch_bounds__(256) void lstm_hprev_kernel(const float* __restrict__ out, const float* __restrict__ h0, float* __restrict__ hprev,
                                                         const int* __restrict__ lens, const int B, const int T, const int nd) {
  const long n4 = (long)B * T * nd * (LH / 4);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n4) return;
  const int u4 = (int)(i % (LH / 4)), dir = (int)((i / (LH / 4)) % nd);
  const long bt = i / ((LH / 4) * nd);
  const int t = (int)(bt % T);
  const long b = bt / T;
  const int len = lens ? lstm_len(lens, (int)b, T) : T;
  const bool first = dir ? t >= len - 1 : t == 0;
  const float* src = first ? h0 + ((long)dir * B + b) * LH + 4 * u4 : out + (bt + (dir ? 1 : -1)) * ((long)nd * LH) + dir * LH + 4 * u4;
  *reinterpret_cast<float4*>(hprev + 4 * i) = *reinterpret_cast<const float4*>(src);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
int lstm_fwd(int B, int T, int I, int nd, const float* x, const float* w_ih, const float* w_hh, const float* bias, const float* h0,
             const float* c0, float* out, float* gates, float* csave, const int* lens, int recurrent, hipStream_t st) {
  const long BT = (long)B * T;
  const int G = nd * 4 * LH;
  GC_REQUIRE(recurrent == LSTM_FP32 || recurrent == LSTM_BF16, "lstm_fwd: lstm_recurrent = %d (0 = fp32, 1 = bf16)", recurrent);
  GemmArgs g = gemm_nt(x, I, w_ih, I, gates, G, (int)BT, G, I).tagged("lstm_gemm");   // gates = X W_ih^T + b, both directions
  g.bias = bias;
  GC_TRY(gemm(g, st, 0, 1));
  const bool bf = recurrent == LSTM_BF16;
  const auto kernel = lens ? (bf ? lstm_fwd_kernel<true, true> : lstm_fwd_kernel<true, false>)
                           : (bf ? lstm_fwd_kernel<false, true> : lstm_fwd_kernel<false, false>);
  const char* tag = bf ? "lstm_fwd_bf16" : "lstm_fwd";
  GC_LAUNCH_TIMED(tag, 2.0 * BT * G * LH, kernel, dim3(cdiv(B, LROWS), nd), dim3(512), 0, st, w_hh, h0, c0, gates, out, csave, lens, B, T, nd);
  return check_launch(tag);
}

static long lstm_col_elems(int nd) { return (long)COL_RIDE_SLICES * nd * 4 * LH; }
static long lstm_split_elems(int I, int nd) { return gemm_ws_elems((long)nd * 4 * LH, I > LH ? I : LH); }

long lstm_ws_elems(int B, int T, int I, int nd) { return (long)B * T * nd * LH + lstm_split_elems(I, nd) + lstm_col_elems(nd); }

int lstm_bwd(int B, int T, int I, int nd, const float* x, const float* w_ih, const float* w_hh, const float* h0, const float* c0,
             const float* out, const float* gates, const float* csave, const float* dout, float* dgates, float* dx, float* dw_ih,
             float* dw_hh, float* db, float* dh0, float* dc0, float* ws, long ws_elems, const int* lens, int recurrent, hipStream_t st) {
  const long BT = (long)B * T;
  const int G = nd * 4 * LH;
  GC_REQUIRE(recurrent == LSTM_FP32 || recurrent == LSTM_BF16, "lstm_bwd: lstm_recurrent = %d (0 = fp32, 1 = bf16)", recurrent);
  GC_REQUIRE(ws_elems >= lstm_ws_elems(B, T, I, nd), "lstm_bwd: workspace of %ld floats needed", lstm_ws_elems(B, T, I, nd));
  float* hprev = ws;
  float* split = ws + BT * nd * LH;
  const long split_elems = lstm_split_elems(I, nd);
  float* part = split + split_elems;

  const bool bf = recurrent == LSTM_BF16;
  const auto kernel = lens ? (bf ? lstm_bwd_kernel<true, true> : lstm_bwd_kernel<true, false>)
                           : (bf ? lstm_bwd_kernel<false, true> : lstm_bwd_kernel<false, false>);
  const char* tag = bf ? "lstm_bwd_bf16" : "lstm_bwd";
  GC_LAUNCH_TIMED(tag, 2.0 * BT * G * LH, kernel, dim3(cdiv(B, LROWS), nd), dim3(512), 0, st, w_hh, c0, gates, csave, dout, dgates, dh0, dc0,
                  lens, B, T, nd);
  GC_TRY(check_launch(tag));
  {
    ProfScope ps("lstm_hprev", st);
    hipLaunchKernelGGL(lstm_hprev_kernel, dim3(cdiv(BT * nd * (LH / 4), 256)), dim3(256), 0, st, out, h0, hprev, lens, B, T, nd);
    GC_TRY(check_launch("lstm_hprev"));
  }
  // dW_ih = dgates^T X; dW_hh[dir] = dgates[:, dir]^T H_prev[:, dir]; dX = dgates W_ih; db = column sums of dgates (riding)
  GemmArgs gs[3] = {
      gemm_tn(dgates, G, x, I, dw_ih, I, G, I, (int)BT).split_ws(split, split_elems).tagged("lstm_gemm"),
      gemm_tn(dgates, G, hprev, nd * LH, dw_hh, LH, 4 * LH, LH, (int)BT).batch_z2(nd, 4 * LH, LH, 4L * LH * LH).split_ws(split, split_elems).tagged("lstm_gemm"),
      gemm_nn(dgates, G, w_ih, I, dx, I, (int)BT, I, G).split_ws(split, split_elems).tagged("lstm_gemm"),
  };
  const ColRide cr = col_sum(dgates, BT, G, G, db, part);
  return gemm_group(gs, 3, st, &cr);
}

}  // namespace gc
