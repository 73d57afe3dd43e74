// The BERT attention core with bf16 operands (bert.hpp: BERT_ATTN_BF16).  The contract is bert.hip's: packed
// fp32 qkv [B][T][3 D], fp32 ctx / lse / dqkv, key_bias and the c_b shift, t_valid, the dropout index in the virtual [B][H][T][T]
// tensor, one writer per output element.  What changes is the arithmetic of the four products:
//     S = alpha r(q) r(k)^T + penalty,   ctx = r(m o P) r(v),   dP = r(dctx) r(v)^T,   dv = r(m o P)^T r(dctx),
//     dq = alpha r(dS) r(k),   dk = alpha r(dS)^T r(q)                      r(.) = one rounding to bf16, nearest even
// on v_mfma_f32_16x16x32_bf16 with fp32 accumulation; softmax, lse, delta and dS stay fp32.
//
// Tiles.  A workgroup is four waves and OWNS 64 rows -- queries in the forward and in the dq kernel, keys in the dk / dv kernel -- one
// wave 16 of them, and streams the other side in blocks of 64 rows through LDS.  Every product is issued so that the wave's OWN row
// is the matrix instruction's output COLUMN (lane & 15): lane l = (c16, q) then holds, of each 16 x 16 tile of S^T (or of S in the
// dk / dv kernel), the four streamed rows 4 q .. 4 q + 3 of its own row c16.  So
//   - the own side's operand (q, dctx; k, v) is the B fragment of the first products, read once from memory into registers;
//   - the softmax statistics of a query are lane-local up to two shuffles over q (no serial-lane softmax, no LDS round trip);
//   - the tile of P (dS) is, after the packed convert, the B fragment of the second product with no lane movement: elements 0 .. 3 of
//     k-step s come from tile 2 s, elements 4 .. 7 from tile 2 s + 1, i.e. element j of lane group q is streamed row
//     32 s + 16 (j >> 2) + 4 q + (j & 3), and the A fragment of that product (the TRANSPOSED image of v, k, dctx or q) is read in the
//     same order: two 8-byte reads 16 rows apart;
//   - a lane's four accumulator registers of the second product are four consecutive head columns of its own row: float4 stores.
// The streamed block lives in LDS as bf16 images with 144-byte rows (gemm_bf16.hip's pitch): [row][64 d] for the first products,
// [d][64 rows] for the second ones.  Both are written from one fetch, a 4 (rows) x 4 (d) fp32 patch per thread and 64-row step,
// rounded by the packed convert on the way in.
//
// Forward: two passes over the keys.  Pass 1 computes S^T block by block and keeps a running (max, sum) per lane, merged over q at
// the end: lse.  Pass 2 recomputes S^T (the same instructions on the same operands), P = exp(S - lse) UNROUNDED, multiplies by the
// dropout keep-scale, rounds and feeds P v.  Nothing is rescaled, so r(m o P) is the definition's, not a running-maximum variant of it.
// Backward: P recomputed from lse as in bert.hip, delta from bert.hip's row kernel.
//
// Padding.  Rows of a block at or past the document's live length Tl (T without t_valid) are loaded as zeros through a predicate,
// their penalty is -inf (pass 1 / 2, dq) or their probability a selected 0 (dk / dv), rows at or past T are never stored, rows in
// [Tl, T) are stored as zeros.  A workgroup whose 64 rows are all padding stores its zeros and leaves before the first barrier.
#include "bert_attn.hpp"

namespace gc {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int AD = BERT_DH;   // head width = the contraction length of the first products
constexpr int BR = 64;        // rows a workgroup owns, rows of a streamed block
constexpr int LP = 64 + 8;    // bf16 elements per image row
static_assert(AD == 64, "the fragments below are written for a head width of 64");

// two floats -> two bf16, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}
__device__ __forceinline__ bf16x8 frag8(const uint2 lo, const uint2 hi) {
  const uint4 u = make_uint4(lo.x, lo.y, hi.x, hi.y);
  return __builtin_bit_cast(bf16x8, u);
}

// ---- the streamed block ----------------------------------------------------------------------------------------------------------
// Thread t holds rows r0 + 4 (t >> 4) + j, j < 4, columns 4 (t & 15) .. + 3 of a [T][ld] matrix (src = row 0, the head's first
// column); rows at or past Tl are zeros that are never loaded.
struct Patch {
  f32x4 v[4];
};
__device__ __forceinline__ void fetch(Patch& p, const float* __restrict__ src, const long ld, const int r0, const int Tl) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = r0 + 4 * (t >> 4) + j;
    p.v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (r < Tl) p.v[j] = *reinterpret_cast<const f32x4*>(src + (long)r * ld + 4 * (t & 15));
  }
}
// img [row][d]
__device__ __forceinline__ void stage_rows(const Patch& p, __bf16* __restrict__ img) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    *reinterpret_cast<uint2*>(img + (4 * (t >> 4) + j) * LP + 4 * (t & 15)) = make_uint2(pack2(p.v[j][0], p.v[j][1]), pack2(p.v[j][2], p.v[j][3]));
}
// img [d][row]: d = 4 (t & 15) + i takes component i of the thread's four rows
__device__ __forceinline__ void stage_cols(const Patch& p, __bf16* __restrict__ img) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    *reinterpret_cast<uint2*>(img + (4 * (t & 15) + i) * LP + 4 * (t >> 4)) = make_uint2(pack2(p.v[0][i], p.v[1][i]), pack2(p.v[2][i], p.v[3][i]));
}

// ---- fragments -------------------------------------------------------------------------------------------------------------------
// v_mfma_f32_16x16x32_bf16, lane l = (c16 = l & 15, q = l >> 4): A[row c16][k = 8 q + j], B[k = 8 q + j][column c16], j < 8;
// C / D [row 4 q + r][column c16], r < 4.

// The own row's operand: row[0 .. 64) of the head in memory -> the B fragments of k-steps 0 and 1 (d = 32 s + 8 q + j); zeros if !live.
__device__ __forceinline__ void own_frags(bf16x8 (&f)[2], const float* __restrict__ row, const bool live, const int q) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      a = *reinterpret_cast<const f32x4*>(row + 32 * s + 8 * q);
      b = *reinterpret_cast<const f32x4*>(row + 32 * s + 8 * q + 4);
    }
    f[s] = frag8(make_uint2(pack2(a[0], a[1]), pack2(a[2], a[3])), make_uint2(pack2(b[0], b[1]), pack2(b[2], b[3])));
  }
}

// First products: acc[t] = tile t of (the block's rows) x (the own rows), contraction over d.  img [row][d]; own = the B fragments.
// acc[t][r] = element (streamed row 16 t + 4 q + r, own row c16): S^T and dP^T in the forward and the dq kernel (own = a query), S and
// dP in the dk / dv kernel (own = a key).
__device__ __forceinline__ void first_product(f32x4 (&acc)[4], const __bf16* __restrict__ img, const bf16x8 (&own)[2], const int c16, const int q) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(img + (16 * t + c16) * LP + 32 * s + 8 * q);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, own[s], acc[t], 0, 0, 0);
    }
  }
}

// Four tiles of fp32 values x[t][r] (streamed row 16 t + 4 q + r of the own row) -> the B fragments of the second product's two
// k-steps, rounded by the packed convert.
__device__ __forceinline__ void tile_frags(bf16x8 (&f)[2], const f32x4 (&x)[4]) {
#pragma unroll
  for (int s = 0; s < 2; ++s)
    f[s] = frag8(make_uint2(pack2(x[2 * s][0], x[2 * s][1]), pack2(x[2 * s][2], x[2 * s][3])),
                 make_uint2(pack2(x[2 * s + 1][0], x[2 * s + 1][1]), pack2(x[2 * s + 1][2], x[2 * s + 1][3])));
}

// Second products: out[dt] += tile dt of (img^T's d rows) x (own rows), contraction over the block's 64 rows in tile_frags' order.
// img [d][row].  out[dt][r] = element (d = 16 dt + 4 q + r, own row c16).
__device__ __forceinline__ void second_product(f32x4 (&out)[4], const __bf16* __restrict__ img, const bf16x8 (&f)[2], const int c16, const int q) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const __bf16* row = img + (16 * dt + c16) * LP + 32 * s + 4 * q;
      const bf16x8 a = frag8(*reinterpret_cast<const uint2*>(row), *reinterpret_cast<const uint2*>(row + 16));
      out[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, f[s], out[dt], 0, 0, 0);
    }
}

// The build's MFMA hazard check prices every low-precision matrix instruction as a 16-pass one (19 wait states before its result is
// read); the compiler leaves what this shorter one needs.  Twenty wait states behind a batch of products satisfy the stricter count
// (gemm_bf16.hip does the same once per tile).  The accumulators are operands of the statement so that no read of them moves in
// front of it, and the launch bound (two workgroups per SIMD: a budget of 256 registers) keeps them in VGPRs.
__device__ __forceinline__ void settle(f32x4 (&a)[4]) { asm volatile("s_nop 15\n\ts_nop 3" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3])); }
__device__ __forceinline__ void settle(f32x4 (&a)[4], f32x4 (&b)[4]) {
  asm volatile("s_nop 15\n\ts_nop 3" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]));
}

// rows [r0, r0 + 64) x the head's 64 columns of out (row stride ld) = 0, rows at or past T left alone
__device__ __forceinline__ void zero_rows(float* __restrict__ out, const long ld, const int r0, const int T) {
  for (int i = threadIdx.x; i < BR * (AD / 4); i += 256) {
    const int r = r0 + (i >> 4);
    if (r < T) *reinterpret_cast<float4*>(out + (long)r * ld + 4 * (i & 15)) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
// out[dt][r] -> columns 16 dt + 4 q + r of one row
__device__ __forceinline__ void store_row(float* __restrict__ row, const f32x4 (&out)[4], const float scale, const bool live, const int q) {
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const f32x4 v = out[dt];
    *reinterpret_cast<float4*>(row + 16 * dt + 4 * q) =
        live ? make_float4(v[0] * scale, v[1] * scale, v[2] * scale, v[3] * scale) : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// the penalty (minus c_b) of the block's 64 keys into LDS; -inf at or past Tl: such a key's score is -inf, its probability exp(-inf) = 0
__device__ __forceinline__ void stage_penalty(float* __restrict__ Kb, const float* __restrict__ kbias, const float cb, const int k0, const int Tl) {
  if (threadIdx.x < BR) {
    const int key = k0 + threadIdx.x;
    Kb[threadIdx.x] = key < Tl ? (kbias ? kbias[key] - cb : 0.f) : -INFINITY;
  }
}

// ---- forward -------------------------------------------------------------------------------------------------------------------
template <bool LEN>
__global__ __launch_bounds__(256, 2) void bert_attn_bf16_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ key_bias,
                                                                    float* __restrict__ ctx, float* __restrict__ lse, const int T,
                                                                    const int H, const float alpha, const Drop drop,
                                                                    const int* __restrict__ t_valid) {
  __shared__ __attribute__((aligned(16))) __bf16 Ks[BR * LP];   // [key][d]
  __shared__ __attribute__((aligned(16))) __bf16 Vt[BR * LP];   // [d][key]
  __shared__ __attribute__((aligned(16))) float Kb[BR];
  __shared__ float shm[4];
  const int q0 = blockIdx.x * BR, h = blockIdx.y, b = blockIdx.z;
  const int D = H * AD;
  const long ld = 3L * D;
  const float* base = qkv + (long)b * T * ld + h * AD;
  float* cbase = ctx + (long)b * T * D + h * AD;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c16 = l & 15, q = l >> 4;
  const int Tl = LEN ? live_len(t_valid, b, T) : T;
  if (LEN && q0 >= Tl) {   // padding rows only: ctx = 0 (the products behind it read these rows), lse = 0
    zero_rows(cbase, D, q0, T);
    if (threadIdx.x < BR && q0 + threadIdx.x < T) lse[((long)b * H + h) * T + q0 + threadIdx.x] = 0.f;
    return;
  }
  const int nkb = (Tl + BR - 1) / BR;
  const float* kbias = key_bias ? key_bias + (long)b * T : nullptr;
  const float cb = doc_bias_max(kbias, Tl, shm);
  const int i = q0 + 16 * w + c16;   // the lane's query
  bf16x8 qf[2];
  own_frags(qf, base + (long)i * ld, i < Tl, q);

  // pass 1: the row's log-sum-exp.  (m, sum) of the keys this lane has seen; a lane that has seen masked keys only holds (-inf, 0)
  float m = -INFINITY, sum = 0.f;
  Patch pk;
  for (int kb = 0; kb < nkb; ++kb) {
    fetch(pk, base + D, ld, kb * BR, Tl);
    __syncthreads();   // the previous block's readers are done with Ks and Kb
    stage_rows(pk, Ks);
    stage_penalty(Kb, kbias, cb, kb * BR, Tl);
    __syncthreads();
    f32x4 s[4];
    first_product(s, Ks, qf, c16, q);
    settle(s);
    float bm = -INFINITY;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 pen = *reinterpret_cast<const f32x4*>(Kb + 16 * t + 4 * q);
#pragma unroll
      for (int r = 0; r < 4; ++r) s[t][r] = __builtin_fmaf(s[t][r], alpha, pen[r]), bm = fmaxf(bm, s[t][r]);
    }
    const float mn = fmaxf(m, bm), ms = mn == -INFINITY ? 0.f : mn;
    float bs = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) bs += expf(s[t][r] - ms);
    sum = sum * expf(m - ms) + bs, m = mn;
  }
#pragma unroll
  for (int o = 16; o <= 32; o <<= 1) {   // the four lanes of a query; key 0 is live and its penalty finite, so the merged maximum is finite
    const float mo = __shfl_xor(m, o), so = __shfl_xor(sum, o);
    const float mn = fmaxf(m, mo), ms = mn == -INFINITY ? 0.f : mn;
    sum = sum * expf(m - ms) + so * expf(mo - ms), m = mn;
  }
  const float L = __shfl(m + logf(sum), c16);   // one value per query: the merge above may round differently in its four lanes
  if (q == 0 && i < T) lse[((long)b * H + h) * T + i] = i < Tl ? L : 0.f;

  // pass 2: ctx^T = v^T (m o P)^T
  const bool dr = drop.snap != nullptr;
  const uint64_t dk = dr ? drop_key(drop) : 0;
  const uint64_t slice = ((uint64_t)b * H + h) * (uint64_t)T;
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  Patch pv;
  for (int kb = 0; kb < nkb; ++kb) {
    fetch(pk, base + D, ld, kb * BR, Tl);
    fetch(pv, base + 2 * D, ld, kb * BR, Tl);
    __syncthreads();   // the previous block's readers are done with Ks, Vt and Kb
    stage_rows(pk, Ks);
    stage_cols(pv, Vt);
    stage_penalty(Kb, kbias, cb, kb * BR, Tl);
    __syncthreads();
    f32x4 s[4];
    first_product(s, Ks, qf, c16, q);
    settle(s);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 pen = *reinterpret_cast<const f32x4*>(Kb + 16 * t + 4 * q);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float p = expf(__builtin_fmaf(s[t][r], alpha, pen[r]) - L);
        if (dr) p *= attn_keep(drop, dk, slice, i, kb * BR + 16 * t + 4 * q + r, T);
        s[t][r] = p;
      }
    }
    bf16x8 pf[2];
    tile_frags(pf, s);
    second_product(o, Vt, pf, c16, q);
  }
  settle(o);
  if (i < T) store_row(cbase + (long)i * D, o, 1.f, i < Tl, q);
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
// dq of a query block: streams key blocks.  dS_ij = P_ij (keep_ij dP_ij - delta_i), dP^T = v dO^T, dq^T = alpha k^T dS^T.
template <bool LEN>
__global__ __launch_bounds__(256, 2) void bert_attn_bf16_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ key_bias,
                                                                      const float* __restrict__ lse, const float* __restrict__ delta,
                                                                      const float* __restrict__ dctx, float* __restrict__ dqkv,
                                                                      const int T, const int H, const float alpha, const Drop drop,
                                                                      const int* __restrict__ t_valid) {
  __shared__ __attribute__((aligned(16))) __bf16 Ks[BR * LP];   // [key][d]
  __shared__ __attribute__((aligned(16))) __bf16 Vs[BR * LP];   // [key][d]
  __shared__ __attribute__((aligned(16))) __bf16 Kt[BR * LP];   // [d][key]
  __shared__ __attribute__((aligned(16))) float Kb[BR];
  __shared__ float shm[4];
  const int q0 = blockIdx.x * BR, h = blockIdx.y, b = blockIdx.z;
  const int D = H * AD;
  const long ld = 3L * D;
  const float* base = qkv + (long)b * T * ld + h * AD;
  float* obase = dqkv + (long)b * T * ld + h * AD;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c16 = l & 15, q = l >> 4;
  const int Tl = LEN ? live_len(t_valid, b, T) : T;
  if (LEN && q0 >= Tl) {   // padding rows only: dq = 0 (the weight gradient and the bias' column sums read these rows)
    zero_rows(obase, ld, q0, T);
    return;
  }
  const int nkb = (Tl + BR - 1) / BR;
  const bool dr = drop.snap != nullptr;
  const uint64_t dk = dr ? drop_key(drop) : 0;
  const uint64_t slice = ((uint64_t)b * H + h) * (uint64_t)T;
  const float* kbias = key_bias ? key_bias + (long)b * T : nullptr;
  const float cb = doc_bias_max(kbias, Tl, shm);
  const int i = q0 + 16 * w + c16;   // the lane's query; dctx of a padding row is not read
  const bool live = i < Tl;
  bf16x8 qf[2], gf[2];
  own_frags(qf, base + (long)i * ld, live, q);
  own_frags(gf, dctx + ((long)b * T + i) * D + h * AD, live, q);
  const float L = live ? lse[((long)b * H + h) * T + i] : 0.f;
  const float di = live ? delta[((long)b * H + h) * T + i] : 0.f;

  f32x4 dq[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  Patch pk, pv;
  for (int kb = 0; kb < nkb; ++kb) {
    fetch(pk, base + D, ld, kb * BR, Tl);
    fetch(pv, base + 2 * D, ld, kb * BR, Tl);
    __syncthreads();   // the previous block's readers are done with the images
    stage_rows(pk, Ks);
    stage_cols(pk, Kt);
    stage_rows(pv, Vs);
    stage_penalty(Kb, kbias, cb, kb * BR, Tl);
    __syncthreads();
    f32x4 s[4], dp[4];
    first_product(s, Ks, qf, c16, q);
    first_product(dp, Vs, gf, c16, q);
    settle(s, dp);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 pen = *reinterpret_cast<const f32x4*>(Kb + 16 * t + 4 * q);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = expf(__builtin_fmaf(s[t][r], alpha, pen[r]) - L);   // a key at or past Tl: exp(-inf) = 0
        const float dpv = dr ? dp[t][r] * attn_keep(drop, dk, slice, i, kb * BR + 16 * t + 4 * q + r, T) : dp[t][r];
        s[t][r] = p * (dpv - di);
      }
    }
    bf16x8 df[2];
    tile_frags(df, s);
    second_product(dq, Kt, df, c16, q);
  }
  settle(dq);
  if (i < T) store_row(obase + (long)i * ld, dq, alpha, live, q);
}

// dk and dv of a key block: streams query blocks.  The tiles are S and dP themselves, rows = the block's queries, column = the own
// key.  dv^T = dO^T Pd (Pd = the dropped probabilities), dk^T = alpha q^T dS.
template <bool LEN>
__global__ __launch_bounds__(256, 2) void bert_attn_bf16_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ key_bias,
                                                                       const float* __restrict__ lse, const float* __restrict__ delta,
                                                                       const float* __restrict__ dctx, float* __restrict__ dqkv,
                                                                       const int T, const int H, const float alpha, const Drop drop,
                                                                       const int* __restrict__ t_valid) {
  __shared__ __attribute__((aligned(16))) __bf16 Qs[BR * LP];   // [query][d]
  __shared__ __attribute__((aligned(16))) __bf16 Gs[BR * LP];   // dO [query][d]
  __shared__ __attribute__((aligned(16))) __bf16 Qt[BR * LP];   // [d][query]
  __shared__ __attribute__((aligned(16))) __bf16 Gt[BR * LP];   // dO [d][query]
  __shared__ __attribute__((aligned(16))) float Ls[BR];
  __shared__ __attribute__((aligned(16))) float Dl[BR];
  __shared__ float shm[4];
  const int k0 = blockIdx.x * BR, h = blockIdx.y, b = blockIdx.z;
  const int D = H * AD;
  const long ld = 3L * D;
  const float* base = qkv + (long)b * T * ld + h * AD;
  const float* gbase = dctx + (long)b * T * D + h * AD;
  float* obase = dqkv + (long)b * T * ld + h * AD;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c16 = l & 15, q = l >> 4;
  const int Tl = LEN ? live_len(t_valid, b, T) : T;
  if (LEN && k0 >= Tl) {   // padding rows only: dk = dv = 0
    zero_rows(obase + D, ld, k0, T);
    zero_rows(obase + 2 * D, ld, k0, T);
    return;
  }
  const int nqb = (Tl + BR - 1) / BR;
  const bool dr = drop.snap != nullptr;
  const uint64_t dk_ = dr ? drop_key(drop) : 0;
  const uint64_t slice = ((uint64_t)b * H + h) * (uint64_t)T;
  const float* kbias = key_bias ? key_bias + (long)b * T : nullptr;
  const float cb = doc_bias_max(kbias, Tl, shm);
  const int key = k0 + 16 * w + c16;   // the lane's key
  const bool live = key < Tl;
  bf16x8 kf[2], vf[2];
  own_frags(kf, base + (long)key * ld + D, live, q);
  own_frags(vf, base + (long)key * ld + 2 * D, live, q);
  const float kbv = live && kbias ? kbias[key] - cb : 0.f;

  f32x4 dk[4], dv[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f}, dv[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  Patch pq, pg;
  for (int qb = 0; qb < nqb; ++qb) {
    fetch(pq, base, ld, qb * BR, Tl);
    fetch(pg, gbase, D, qb * BR, Tl);   // dctx of a padding row is not read
    __syncthreads();   // the previous block's readers are done with the images, Ls and Dl
    stage_rows(pq, Qs);
    stage_cols(pq, Qt);
    stage_rows(pg, Gs);
    stage_cols(pg, Gt);
    if (threadIdx.x < BR) {
      const int i = qb * BR + threadIdx.x;
      const long o = ((long)b * H + h) * T + i;
      Ls[threadIdx.x] = i < Tl ? lse[o] : 0.f;
      Dl[threadIdx.x] = i < Tl ? delta[o] : 0.f;
    }
    __syncthreads();
    f32x4 s[4], dp[4];
    first_product(s, Qs, kf, c16, q);
    first_product(dp, Gs, vf, c16, q);
    settle(s, dp);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 Lv = *reinterpret_cast<const f32x4*>(Ls + 16 * t + 4 * q);
      const f32x4 dv4 = *reinterpret_cast<const f32x4*>(Dl + 16 * t + 4 * q);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = qb * BR + 16 * t + 4 * q + r;
        const float p = live && i < Tl ? expf(__builtin_fmaf(s[t][r], alpha, kbv) - Lv[r]) : 0.f;
        const float keep = dr ? attn_keep(drop, dk_, slice, i, key, T) : 1.f;
        s[t][r] = p * keep;
        dp[t][r] = p * (dp[t][r] * keep - dv4[r]);
      }
    }
    bf16x8 pf[2], df[2];
    tile_frags(pf, s);
    tile_frags(df, dp);
    second_product(dv, Gt, pf, c16, q);
    second_product(dk, Qt, df, c16, q);
  }
  settle(dk, dv);
  if (key < T) {
    store_row(obase + (long)key * ld + D, dk, alpha, live, q);
    store_row(obase + (long)key * ld + 2 * D, dv, 1.f, live, q);
  }
}

}  // namespace

int bert_attn_bf16_fwd(int B, int T, int H, const float* qkv, const float* key_bias, float* ctx, float* lse, Drop drop, hipStream_t st,
                       const int* t_valid) {
  const float alpha = 1.f / sqrtf((float)AD);
  const auto kernel = t_valid ? bert_attn_bf16_fwd_kernel<true> : bert_attn_bf16_fwd_kernel<false>;
  GC_LAUNCH_TIMED("bert_attn_bf16_fwd", 6.0 * B * H * T * T * AD, kernel, dim3(cdiv(T, BR), H, B), dim3(256), 0, st, qkv, key_bias, ctx, lse, T,
                  H, alpha, drop, t_valid);
  return check_launch("bert_attn_bf16_fwd");
}

int bert_attn_bf16_bwd(int B, int T, int H, const float* qkv, const float* key_bias, const float* lse, const float* delta,
                       const float* dctx, float* dqkv, Drop drop, hipStream_t st, const int* t_valid) {
  const float alpha = 1.f / sqrtf((float)AD);
  const auto kq = t_valid ? bert_attn_bf16_bwd_q_kernel<true> : bert_attn_bf16_bwd_q_kernel<false>;
  GC_LAUNCH_TIMED("bert_attn_bf16_bwd_q", 6.0 * B * H * T * T * AD, kq, dim3(cdiv(T, BR), H, B), dim3(256), 0, st, qkv, key_bias, lse, delta,
                  dctx, dqkv, T, H, alpha, drop, t_valid);
  GC_TRY(check_launch("bert_attn_bf16_bwd_q"));
  const auto kkv = t_valid ? bert_attn_bf16_bwd_kv_kernel<true> : bert_attn_bf16_bwd_kv_kernel<false>;
  GC_LAUNCH_TIMED("bert_attn_bf16_bwd_kv", 8.0 * B * H * T * T * AD, kkv, dim3(cdiv(T, BR), H, B), dim3(256), 0, st, qkv, key_bias, lse, delta,
                  dctx, dqkv, T, H, alpha, drop, t_valid);
  return check_launch("bert_attn_bf16_bwd_kv");
}

}  // namespace gc
