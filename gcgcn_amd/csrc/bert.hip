// The BERT encoder layer (pytorch_pretrained_bert 0.6 modeling.py BertLayer), DESIGN.md section 8.9.
//
//   forward :  qkv = x [Wq; Wk; Wv]^T + b          one product of the GEMM layer (N = 3 D)
//              bert_attn_fwd_kernel                 ctx = dropout(softmax(q k^T / 8 + key_bias)) v, lse; per (document, head, 16 queries)
//              ao = ctx Wo^T                        GEMM layer
//              res_ln_fwd_kernel                    a = LayerNorm(dropout(ao + bo) + x)
//              z = a Wi^T                           GEMM layer
//              bias_gelu_fwd_kernel                 g = gelu(z + bi)
//              o2 = g Wo2^T                         GEMM layer
//              res_ln_fwd_kernel                    y = LayerNorm(dropout(o2 + bo2) + a)
//   backward:  the same chain reversed; every weight gradient is a gemm_tn with split-K workspace in a group launch with the data
//              gradient of the same Linear and the bias gradient as the riding column sum.
//
// The attention kernels.  All four products (q k^T, P v and in the backward dO v^T, dS k / dS^T q / P^T dO) are 16x16 tiles of
// v_mfma_f32_16x16x4_f32 with a contraction length of 64: the head width for the products against k-contiguous rows (tile_nt), a
// streamed block of 64 keys or queries for the others (tile_nn).  A workgroup is four waves and OWNS 16 rows -- queries in the forward
// and in the dq kernel, keys in the dk / dv kernel -- and streams the other side in blocks of 64 rows through LDS; wave w computes
// the 16 x 16 tile of columns [16 w, 16 w + 16) of each 16 x 64 result.  An accumulator tile (C/D map: row 4 q + r, column c16)
// becomes the A operand of the next product (row c16, k contiguous) through an LDS image, never through memory.  B H ceil(T / 16)
// workgroups per launch: 1 536 at B = 4, T = 512, H = 12.
//
// Forward: the query block's whole score rows [16][<= 512] stay in LDS (33 KB), so the softmax is the plain two-pass one and nothing
// is rescaled; keys are streamed once for the scores and values once for the output.  Backward: P_ij = exp(S_ij - lse_i) is
// recomputed block by block, the dropout decision regenerated from the same counter, delta_i = sum_d dO_id O_id precomputed by a
// row kernel.  One workgroup writes each element of dq, dk and dv; nothing is added atomically: two runs are bitwise equal.
//
// Padding.  Rows of a block past T are loaded as zeros through a predicate (never multiplied by 0), keys past T get probability 0
// through a select, rows past T are not stored: what lies behind a buffer's end is never read and never reaches a result.
#include "bert.hpp"
#include "bert_attn.hpp"
#include "ln_row.hpp"
#include "gemm.hpp"
#include "gemm_bf16.hpp"
#include "rowops.hpp"

namespace gc {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int AD = BERT_DH;
constexpr int AS = AD + 4;             // LDS row stride of a [rows][64] image: 16-byte aligned rows, 4 banks apart
constexpr int AQ = 16;                 // rows a workgroup owns
constexpr int AK = 64;                 // rows of a streamed block
constexpr int SS = BERT_MAX_T + 4;     // row stride of the forward's score rows
static_assert((AQ * AS + AK * AS + AQ * SS) * sizeof(float) <= 64 * 1024, "static LDS of the forward kernel");

// rows [r0, r0 + NR) x 64 columns of a [T][ld] matrix (src points at row 0, first column) -> dst [NR][AS]; rows >= T become zeros
template <int NR>
__device__ __forceinline__ void load_rows(float* __restrict__ dst, const float* __restrict__ src, const long ld, const int r0, const int T) {
  for (int i = threadIdx.x; i < NR * (AD / 4); i += 256) {
    const int r = i >> 4, c4 = i & 15;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r0 + r < T) v = *reinterpret_cast<const float4*>(src + (long)(r0 + r) * ld + 4 * c4);
    *reinterpret_cast<float4*>(dst + r * AS + 4 * c4) = v;
  }
}

// Lane maps of the 16x16x4 form (lane l, c16 = l & 15, q = l >> 4): A[row c16][k q], B[k q][col c16], C/D [row 4 q + r][col c16].
// As in lstm.hip, k-step s of lane group q takes k = 16 q + s, so a lane's A values are contiguous in its LDS row.
// X Y^T over k < 64: xrow = the lane's row of X, yrow = the row of Y that is the lane's output column, both k-contiguous.
__device__ __forceinline__ f32x4 tile_nt(const float* xrow, const float* yrow, const int q) {
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};   // two chains: the dependent latency exceeds the issue interval
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4 x = *reinterpret_cast<const float4*>(xrow + 16 * q + 4 * j);
    const float4 y = *reinterpret_cast<const float4*>(yrow + 16 * q + 4 * j);
    a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, y.x, a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, y.y, a1, 0, 0, 0);
    a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, y.z, a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, y.w, a1, 0, 0, 0);
  }
  return a0 + a1;
}
// X Z over k < 64: xrow as above, zcol = column (the lane's output column) of row 0 of Z [64][AS]
__device__ __forceinline__ f32x4 tile_nn(const float* xrow, const float* zcol, const int q) {
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4 x = *reinterpret_cast<const float4*>(xrow + 16 * q + 4 * j);
    const float* z = zcol + (16 * q + 4 * j) * AS;
    a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, z[0], a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, z[AS], a1, 0, 0, 0);
    a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, z[2 * AS], a0, 0, 0, 0);
    a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, z[3 * AS], a1, 0, 0, 0);
  }
  return a0 + a1;
}

// Token lengths (LEN instantiations; t_valid [B], row (b, t) is live iff t < t_valid[b]).  Tl = the document's length clamped to
// [0, T] takes T's place in every predicate -- the rows that are loaded, the keys that get a probability, the streamed loop's end --
// while T keeps the strides and the dropout index.  A workgroup whose 16 rows are all padding stores its zeros and leaves before
// the first barrier; one that holds the document's last live rows stores zeros on the padding rows beside them.  Both decisions
// are uniform per workgroup and made outside the matrix-instruction sequences.  Without LEN the code is what it was.
// (live_len, the penalty shift c_b and the dropout decision: bert_attn.hpp, shared with the bf16 core.)

// ---- forward -------------------------------------------------------------------------------------------------------------------
template <bool LEN>
__global__ __launch_bounds__(256) void bert_attn_fwd_kernel(const float* __restrict__ qkv, const float* __restrict__ key_bias,
                                                            float* __restrict__ ctx, float* __restrict__ lse, const int T, const int H,
                                                            const float alpha, const Drop drop, const int* __restrict__ t_valid) {
  __shared__ __attribute__((aligned(16))) float Qs[AQ * AS];
  __shared__ __attribute__((aligned(16))) float Bs[AK * AS];
  __shared__ __attribute__((aligned(16))) float Ss[AQ * SS];
  const int q0 = blockIdx.x * AQ, h = blockIdx.y, b = blockIdx.z;
  const int D = H * AD;
  const long ld = 3L * D;
  const float* base = qkv + (long)b * T * ld + h * AD;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c16 = l & 15, q = l >> 4;
  const int Tl = LEN ? live_len(t_valid, b, T) : T;
  if (LEN && q0 >= Tl) {   // padding rows only: ctx = 0 (the products behind it read these rows), lse = 0
    for (int i = threadIdx.x; i < AQ * AD; i += 256) {
      const int r = q0 + (i >> 6);
      if (r < T) ctx[((long)b * T + r) * D + h * AD + (i & 63)] = 0.f;
    }
    if (threadIdx.x < AQ && q0 + threadIdx.x < T) lse[((long)b * H + h) * T + q0 + threadIdx.x] = 0.f;
    return;
  }
  const int nkb = (Tl + AK - 1) / AK;
  __shared__ float shm[4];
  const float cb = doc_bias_max(key_bias ? key_bias + (long)b * T : nullptr, Tl, shm);

  load_rows<AQ>(Qs, base, ld, q0, Tl);
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();   // the previous block's readers are done with Bs
    load_rows<AK>(Bs, base + D, ld, kb * AK, Tl);
    __syncthreads();
    const f32x4 s = tile_nt(Qs + c16 * AS, Bs + (16 * w + c16) * AS, q);
    const int key = kb * AK + 16 * w + c16;
    const bool kin = key < Tl;
    const float kbv = kin && key_bias ? key_bias[(long)b * T + key] - cb : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) Ss[(4 * q + r) * SS + key] = kin ? __builtin_fmaf(s[r], alpha, kbv) : -INFINITY;
  }
  __syncthreads();

  {   // softmax of row `row` by 16 consecutive lanes; key 0 exists and the penalty is finite, so the maximum is finite
    const int row = threadIdx.x >> 4, sub = threadIdx.x & 15, Tp = nkb * AK, i = q0 + row;
    float* sr = Ss + row * SS;
    float m = -INFINITY;
    for (int j = sub; j < Tp; j += 16) m = fmaxf(m, sr[j]);
#pragma unroll
    for (int o = 8; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 16));
    float sum = 0.f;
    for (int j = sub; j < Tp; j += 16) sum += expf(sr[j] - m);
#pragma unroll
    for (int o = 8; o; o >>= 1) sum += __shfl_xor(sum, o, 16);
    const float L = m + logf(sum);
    if (sub == 0 && i < T) lse[((long)b * H + h) * T + i] = i < Tl ? L : 0.f;
    const bool dr = drop.snap != nullptr;
    const uint64_t dk = dr ? drop_key(drop) : 0;
    const uint64_t slice = ((uint64_t)b * H + h) * (uint64_t)T;
    for (int j = sub; j < Tp; j += 16) {
      float p = expf(sr[j] - L);
      if (dr) p *= attn_keep(drop, dk, slice, i, j, T);
      sr[j] = p;
    }
  }

  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();   // the probabilities are written; the previous block's readers are done with Bs
    load_rows<AK>(Bs, base + 2 * D, ld, kb * AK, Tl);
    __syncthreads();
    o += tile_nn(Ss + c16 * SS + kb * AK, Bs + 16 * w + c16, q);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = q0 + 4 * q + r;
    if (i < T) ctx[((long)b * T + i) * D + h * AD + 16 * w + c16] = i < Tl ? o[r] : 0.f;
  }
}

// ---- backward ------------------------------------------------------------------------------------------------------------------
// delta [B][H][T] = sum_d dctx * ctx: one wave per (b, t, h)
template <bool LEN>
__global__ __launch_bounds__(256) void bert_attn_delta_kernel(const float* __restrict__ ctx, const float* __restrict__ dctx,
                                                              float* __restrict__ delta, const long n, const int T, const int H,
                                                              const int* __restrict__ t_valid) {
  const long i = (long)blockIdx.x * 4 + (threadIdx.x >> 6);   // (b T + t) H + h
  if (i >= n) return;
  const int l = threadIdx.x & 63;
  const int h = (int)(i % H);
  const long bt = i / H;
  const bool pad = LEN && (int)(bt % T) >= live_len(t_valid, (int)(bt / T), T);   // wave-uniform; dctx of a padding row is not read
  const float s = pad ? 0.f : wave_sum(ctx[i * AD + l] * dctx[i * AD + l]);
  if (l == 0) delta[((bt / T) * H + h) * T + bt % T] = s;
}

// dq of a query block: streams key blocks.  dS_ij = P_ij (keep_ij dP_ij - delta_i), dP = dO v^T, dq = alpha dS k.
template <bool LEN>
__global__ __launch_bounds__(256) void bert_attn_bwd_q_kernel(const float* __restrict__ qkv, const float* __restrict__ key_bias,
                                                              const float* __restrict__ lse, const float* __restrict__ delta,
                                                              const float* __restrict__ dctx, float* __restrict__ dqkv, const int T,
                                                              const int H, const float alpha, const Drop drop,
                                                              const int* __restrict__ t_valid) {
  __shared__ __attribute__((aligned(16))) float Qs[AQ * AS];
  __shared__ __attribute__((aligned(16))) float Gs[AQ * AS];    // dO
  __shared__ __attribute__((aligned(16))) float Ks[AK * AS];
  __shared__ __attribute__((aligned(16))) float Vs[AK * AS];
  __shared__ __attribute__((aligned(16))) float Ds[AQ * AS];    // dS of the block
  __shared__ float Ls[AQ], Dl[AQ];
  const int q0 = blockIdx.x * AQ, h = blockIdx.y, b = blockIdx.z;
  const int D = H * AD;
  const long ld = 3L * D;
  const float* base = qkv + (long)b * T * ld + h * AD;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c16 = l & 15, q = l >> 4;
  const int Tl = LEN ? live_len(t_valid, b, T) : T;
  if (LEN && q0 >= Tl) {   // padding rows only: dq = 0 (the weight gradient and the bias' column sums read these rows)
    for (int i = threadIdx.x; i < AQ * AD; i += 256) {
      const int r = q0 + (i >> 6);
      if (r < T) dqkv[((long)b * T + r) * ld + h * AD + (i & 63)] = 0.f;
    }
    return;
  }
  const int nkb = (Tl + AK - 1) / AK;
  const bool dr = drop.snap != nullptr;
  const uint64_t dk = dr ? drop_key(drop) : 0;
  const uint64_t slice = ((uint64_t)b * H + h) * (uint64_t)T;
  __shared__ float shm[4];
  const float cb = doc_bias_max(key_bias ? key_bias + (long)b * T : nullptr, Tl, shm);

  load_rows<AQ>(Qs, base, ld, q0, Tl);
  load_rows<AQ>(Gs, dctx + (long)b * T * D + h * AD, D, q0, Tl);
  if (threadIdx.x < AQ) {
    const int i = q0 + threadIdx.x;
    const long o = ((long)b * H + h) * T + i;
    Ls[threadIdx.x] = i < Tl ? lse[o] : 0.f;
    Dl[threadIdx.x] = i < Tl ? delta[o] : 0.f;
  }
  f32x4 dq = {0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < nkb; ++kb) {
    __syncthreads();   // the previous block's readers are done with Ks and Ds
    load_rows<AK>(Ks, base + D, ld, kb * AK, Tl);
    load_rows<AK>(Vs, base + 2 * D, ld, kb * AK, Tl);
    __syncthreads();
    const f32x4 s = tile_nt(Qs + c16 * AS, Ks + (16 * w + c16) * AS, q);
    const f32x4 dp = tile_nt(Gs + c16 * AS, Vs + (16 * w + c16) * AS, q);
    const int key = kb * AK + 16 * w + c16;
    const bool kin = key < Tl;
    const float kbv = kin && key_bias ? key_bias[(long)b * T + key] - cb : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * q + r, i = q0 + row;
      const float p = kin && i < Tl ? expf(__builtin_fmaf(s[r], alpha, kbv) - Ls[row]) : 0.f;
      const float dpv = dr ? dp[r] * attn_keep(drop, dk, slice, i, key, T) : dp[r];
      Ds[row * AS + 16 * w + c16] = p * (dpv - Dl[row]);
    }
    __syncthreads();
    dq += tile_nn(Ds + c16 * AS, Ks + 16 * w + c16, q);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = q0 + 4 * q + r;
    if (i < T) dqkv[((long)b * T + i) * ld + h * AD + 16 * w + c16] = i < Tl ? dq[r] * alpha : 0.f;
  }
}

// dk and dv of a key block: streams query blocks.  The tiles are the transposes: S^T = k q^T, dP^T = v dO^T, rows = the block's keys.
// dv = Pd^T dO (Pd = the dropped probabilities), dk = alpha dS^T q.
template <bool LEN>
__global__ __launch_bounds__(256) void bert_attn_bwd_kv_kernel(const float* __restrict__ qkv, const float* __restrict__ key_bias,
                                                               const float* __restrict__ lse, const float* __restrict__ delta,
                                                               const float* __restrict__ dctx, float* __restrict__ dqkv, const int T,
                                                               const int H, const float alpha, const Drop drop,
                                                               const int* __restrict__ t_valid) {
  __shared__ __attribute__((aligned(16))) float Ks[AQ * AS];
  __shared__ __attribute__((aligned(16))) float Vs[AQ * AS];
  __shared__ __attribute__((aligned(16))) float Qs[AK * AS];
  __shared__ __attribute__((aligned(16))) float Gs[AK * AS];    // dO
  __shared__ __attribute__((aligned(16))) float Ps[AQ * AS];    // Pd^T of the block
  __shared__ __attribute__((aligned(16))) float Ds[AQ * AS];    // dS^T of the block
  __shared__ float Ls[AK], Dl[AK];
  const int k0 = blockIdx.x * AQ, h = blockIdx.y, b = blockIdx.z;
  const int D = H * AD;
  const long ld = 3L * D;
  const float* base = qkv + (long)b * T * ld + h * AD;
  const float* gbase = dctx + (long)b * T * D + h * AD;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c16 = l & 15, q = l >> 4;
  const int Tl = LEN ? live_len(t_valid, b, T) : T;
  if (LEN && k0 >= Tl) {   // padding rows only: dk = dv = 0
    for (int i = threadIdx.x; i < AQ * AD; i += 256) {
      const int r = k0 + (i >> 6);
      if (r < T) {
        float* o = dqkv + ((long)b * T + r) * ld + h * AD + (i & 63);
        o[D] = 0.f, o[2 * D] = 0.f;
      }
    }
    return;
  }
  const int nqb = (Tl + AK - 1) / AK;
  const bool dr = drop.snap != nullptr;
  const uint64_t dk_ = dr ? drop_key(drop) : 0;
  const uint64_t slice = ((uint64_t)b * H + h) * (uint64_t)T;

  __shared__ float shm[4];
  const float cb = doc_bias_max(key_bias ? key_bias + (long)b * T : nullptr, Tl, shm);
  load_rows<AQ>(Ks, base + D, ld, k0, Tl);
  load_rows<AQ>(Vs, base + 2 * D, ld, k0, Tl);
  float kbv[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int key = k0 + 4 * q + r;
    kbv[r] = key < Tl && key_bias ? key_bias[(long)b * T + key] - cb : 0.f;
  }
  f32x4 dk = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f};
  for (int qb = 0; qb < nqb; ++qb) {
    __syncthreads();   // the previous block's readers are done with Qs, Gs, Ps, Ds, Ls, Dl
    load_rows<AK>(Qs, base, ld, qb * AK, Tl);
    load_rows<AK>(Gs, gbase, D, qb * AK, Tl);
    if (threadIdx.x < AK) {
      const int i = qb * AK + threadIdx.x;
      const long o = ((long)b * H + h) * T + i;
      Ls[threadIdx.x] = i < Tl ? lse[o] : 0.f;
      Dl[threadIdx.x] = i < Tl ? delta[o] : 0.f;
    }
    __syncthreads();
    const f32x4 st = tile_nt(Ks + c16 * AS, Qs + (16 * w + c16) * AS, q);
    const f32x4 dpt = tile_nt(Vs + c16 * AS, Gs + (16 * w + c16) * AS, q);
    const int qi = 16 * w + c16, i = qb * AK + qi;
    const float Li = Ls[qi], di = Dl[qi];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * q + r, key = k0 + row;
      const float p = key < Tl && i < Tl ? expf(__builtin_fmaf(st[r], alpha, kbv[r]) - Li) : 0.f;
      const float keep = dr ? attn_keep(drop, dk_, slice, i, key, T) : 1.f;
      Ps[row * AS + qi] = p * keep;
      Ds[row * AS + qi] = p * (dpt[r] * keep - di);
    }
    __syncthreads();
    dv += tile_nn(Ps + c16 * AS, Gs + 16 * w + c16, q);
    dk += tile_nn(Ds + c16 * AS, Qs + 16 * w + c16, q);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int key = k0 + 4 * q + r;
    if (key < T) {
      float* o = dqkv + ((long)b * T + key) * ld + h * AD + 16 * w + c16;
      o[D] = key < Tl ? dk[r] * alpha : 0.f;
      o[2 * D] = key < Tl ? dv[r] : 0.f;
    }
  }
}

int bert_attn_fwd(int B, int T, int H, const float* qkv, const float* key_bias, float* ctx, float* lse, Drop drop, hipStream_t st,
                  const int* t_valid, int attn) {
  if (attn == BERT_ATTN_BF16) return bert_attn_bf16_fwd(B, T, H, qkv, key_bias, ctx, lse, drop, st, t_valid);
  const float alpha = 1.f / sqrtf((float)AD);
  const auto kernel = t_valid ? bert_attn_fwd_kernel<true> : bert_attn_fwd_kernel<false>;
  GC_LAUNCH_TIMED("bert_attn_fwd", 4.0 * B * H * T * T * AD, kernel, dim3(cdiv(T, AQ), H, B), dim3(256), 0, st, qkv, key_bias, ctx, lse, T, H,
                  alpha, drop, t_valid);
  return check_launch("bert_attn_fwd");
}

int bert_attn_bwd(int B, int T, int H, const float* qkv, const float* key_bias, const float* ctx, const float* lse, const float* dctx,
                  float* dqkv, float* delta, Drop drop, hipStream_t st, const int* t_valid, int attn) {
  const float alpha = 1.f / sqrtf((float)AD);
  const long n = (long)B * T * H;
  {   // delta comes from the stored fp32 ctx, unrounded, at either setting of attn
    ProfScope ps("bert_attn_delta", st);
    const auto kd = t_valid ? bert_attn_delta_kernel<true> : bert_attn_delta_kernel<false>;
    hipLaunchKernelGGL(kd, dim3(cdiv(n, 4)), dim3(256), 0, st, ctx, dctx, delta, n, T, H, t_valid);
    GC_TRY(check_launch("bert_attn_delta"));
  }
  if (attn == BERT_ATTN_BF16) return bert_attn_bf16_bwd(B, T, H, qkv, key_bias, lse, delta, dctx, dqkv, drop, st, t_valid);
  const auto kq = t_valid ? bert_attn_bwd_q_kernel<true> : bert_attn_bwd_q_kernel<false>;
  GC_LAUNCH_TIMED("bert_attn_bwd_q", 6.0 * B * H * T * T * AD, kq, dim3(cdiv(T, AQ), H, B), dim3(256), 0, st, qkv, key_bias, lse, delta, dctx,
                  dqkv, T, H, alpha, drop, t_valid);
  GC_TRY(check_launch("bert_attn_bwd_q"));
  const auto kkv = t_valid ? bert_attn_bwd_kv_kernel<true> : bert_attn_bwd_kv_kernel<false>;
  GC_LAUNCH_TIMED("bert_attn_bwd_kv", 8.0 * B * H * T * T * AD, kkv, dim3(cdiv(T, AQ), H, B), dim3(256), 0, st, qkv, key_bias, lse, delta, dctx,
                  dqkv, T, H, alpha, drop, t_valid);
  return check_launch("bert_attn_bwd_kv");
}

// ---- LayerNorm(dropout(x + bias) + res) ------------------------------------------------------------------------------------------
// One wave per row; lane l holds columns l + 64 i, i < D / 64 <= 16, in registers.  Two-pass variance: a constant row has var = 0.
// The row arithmetic itself is ln_row.hpp's, shared with the fused embeddings stage (bert_embed.hip).
__device__ __forceinline__ void ln_input(float (&v)[LNV], const float* __restrict__ x, const float* __restrict__ bias,
                                         const float* __restrict__ res, const long row, const int D, const int l, const Drop& drop,
                                         const uint64_t dk) {
  const int n = D >> 6;
#pragma unroll
  for (int i = 0; i < LNV; ++i) {
    v[i] = 0.f;
    if (i < n) {
      const int c = l + 64 * i;
      const long o = row * D + c;
      float t = x[o];
      if (bias) t += bias[c];
      if (drop.snap) t = rng_u32(dk, (uint64_t)o) >= drop.thresh ? t * drop.scale : 0.f;
      if (res) t += res[o];
      v[i] = t;
    }
  }
}

// Token lengths (t_valid, T; rows = B T): the wave of a padding row stores zeros -- y, which the next product and the weight
// gradient behind it read on every row, and mean / rstd -- and reads nothing: what x and res hold there (the rows a row-block
// product left unwritten) never reaches a result.
__global__ __launch_bounds__(256) void res_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ bias,
                                                         const float* __restrict__ res, const float* __restrict__ weight,
                                                         const float* __restrict__ lnb, float* __restrict__ y, float* __restrict__ mean,
                                                         float* __restrict__ rstd, const long rows, const int D, const Drop drop,
                                                         const int* __restrict__ t_valid, const int T) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;   // wave-uniform
  const int l = threadIdx.x & 63, n = D >> 6;
  if (t_valid && (int)(row % T) >= live_len(t_valid, (int)(row / T), T)) {   // wave-uniform
    for (int i = 0; i < n; ++i) y[row * D + l + 64 * i] = 0.f;
    if (l == 0 && mean) mean[row] = 0.f, rstd[row] = 0.f;
    return;
  }
  const uint64_t dk = drop.snap ? drop_key(drop) : 0;
  float v[LNV];
  ln_input(v, x, bias, res, row, D, l, drop, dk);
  float m, r;
  ln_row_stats(v, n, D, m, r);
#pragma unroll
  for (int i = 0; i < LNV; ++i)
    if (i < n) {
      const int c = l + 64 * i;
      y[row * D + c] = ln_row_out(v[i], m, r, weight[c], lnb[c]);
    }
  if (l == 0 && mean) mean[row] = m, rstd[row] = r;
}

// Stage 1 of the backward: workgroup g takes rows 4 g + w, 4 (g + G) + w, ...; every wave sums dy * xhat and dy of its rows per column in
// registers, the four waves meet in LDS in a fixed order: part [G][2][D].
__global__ __launch_bounds__(256) void res_ln_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ bias,
                                                         const float* __restrict__ res, const float* __restrict__ weight,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         float* __restrict__ dx, float* __restrict__ dres, float* __restrict__ part,
                                                         const long rows, const int D, const Drop drop, const int* __restrict__ t_valid,
                                                         const int T) {
  __shared__ float sh[4][2][BERT_LN_MAX_D];
  const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, n = D >> 6;
  const uint64_t dk = drop.snap ? drop_key(drop) : 0;
  float aw[LNV], ab[LNV];
#pragma unroll
  for (int i = 0; i < LNV; ++i) aw[i] = 0.f, ab[i] = 0.f;
  for (long row = (long)blockIdx.x * 4 + wv; row < rows; row += (long)gridDim.x * 4) {
    if (t_valid && (int)(row % T) >= live_len(t_valid, (int)(row / T), T)) {   // a padding row (wave-uniform): dy there counts as zero and
      for (int i = 0; i < n; ++i) {                                            // is not read; dx = dres = 0, nothing joins the column sums
        const long o = row * D + l + 64 * i;
        if (dres) dres[o] = 0.f;
        dx[o] = 0.f;
      }
      continue;
    }
    float v[LNV];
    ln_input(v, x, bias, res, row, D, l, drop, dk);
    const float m = mean[row], r = rstd[row];
    const auto dstore = [&](const int i, const float dv) {
      const long o = row * D + l + 64 * i;
      if (dres) dres[o] = dv;
      dx[o] = drop.snap ? (rng_u32(dk, (uint64_t)o) >= drop.thresh ? dv * drop.scale : 0.f) : dv;
    };
    ln_row_bwd(v, [&](const int i) { return dy[row * D + l + 64 * i]; }, dstore, weight, n, D, l, m, r, aw, ab);
  }
  ln_part_store(sh, aw, ab, part, n, D, wv, l);
}
// Stage 2: the G row groups in order
__global__ __launch_bounds__(256) void res_ln_bwd_reduce_kernel(const float* __restrict__ part, const int G, const int D,
                                                                float* __restrict__ dweight, float* __restrict__ dlnb) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= 2 * D) return;
  float s = 0.f;
  for (int g = 0; g < G; ++g) s += part[(long)g * 2 * D + c];
  if (c < D) dweight[c] = s;
  else dlnb[c - D] = s;
}

int res_ln_bwd_reduce(const float* part, int G, int D, float* dweight, float* dlnb, hipStream_t st) {
  hipLaunchKernelGGL(res_ln_bwd_reduce_kernel, dim3(cdiv(2 * D, 256)), dim3(256), 0, st, part, G, D, dweight, dlnb);
  return check_launch("res_ln_bwd_reduce");
}

int res_ln_fwd(long rows, int D, const float* x, const float* bias, const float* res, const float* weight, const float* lnb, float* y,
               float* mean, float* rstd, Drop drop, hipStream_t st, const int* t_valid, int T) {
  ProfScope ps("bert_res_ln_fwd", st);
  hipLaunchKernelGGL(res_ln_fwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, x, bias, res, weight, lnb, y, mean, rstd, rows, D, drop, t_valid,
                     t_valid ? T : 1);
  return check_launch("res_ln_fwd");
}

int res_ln_bwd(long rows, int D, const float* dy, const float* x, const float* bias, const float* res, const float* weight,
               const float* mean, const float* rstd, float* dx, float* dres, float* dweight, float* dlnb, float* part, Drop drop,
               hipStream_t st, const int* t_valid, int T) {
  const int G = (int)std::min<long>(BERT_LN_PARTS, cdiv(rows, 4));
  ProfScope ps("bert_res_ln_bwd", st);
  hipLaunchKernelGGL(res_ln_bwd_kernel, dim3(G), dim3(256), 0, st, dy, x, bias, res, weight, mean, rstd, dx, dres, part, rows, D, drop,
                     t_valid, t_valid ? T : 1);
  GC_TRY(check_launch("res_ln_bwd"));
  return res_ln_bwd_reduce(part, G, D, dweight, dlnb, st);
}

// ---- erf GELU with the bias ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_f(float z) { return z * 0.5f * (1.f + erff(z * 0.70710678118654752f)); }
__device__ __forceinline__ float gelu_df(float z) {
  return 0.5f * (1.f + erff(z * 0.70710678118654752f)) + z * 0.39894228040143268f * expf(-0.5f * z * z);
}
// LEN (t_valid, T; rows = B T): an element of a padding row becomes zero -- g and dz are read on every row by the weight gradients
// and the bias' column sum -- and neither x nor dy is read there.
template <bool BWD, bool LEN>
__global__ __launch_bounds__(256) void bias_gelu_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ bias,
                                                        float* __restrict__ out, const long n4, const int C4, const int* __restrict__ t_valid,
                                                        const int T) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    if constexpr (LEN) {
      const long row = i / C4;
      if ((int)(row % T) >= min(max(t_valid[row / T], 0), T)) {
        reinterpret_cast<float4*>(out)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        continue;
      }
    }
    float4 z = reinterpret_cast<const float4*>(x)[i];
    if (bias) {
      const float4 bv = reinterpret_cast<const float4*>(bias)[i % C4];
      z.x += bv.x, z.y += bv.y, z.z += bv.z, z.w += bv.w;
    }
    float4 o;
    if constexpr (BWD) {
      const float4 d = reinterpret_cast<const float4*>(dy)[i];
      o = make_float4(d.x * gelu_df(z.x), d.y * gelu_df(z.y), d.z * gelu_df(z.z), d.w * gelu_df(z.w));
    } else {
      o = make_float4(gelu_f(z.x), gelu_f(z.y), gelu_f(z.z), gelu_f(z.w));
    }
    reinterpret_cast<float4*>(out)[i] = o;
  }
}
int bias_gelu_fwd(long rows, int C, const float* x, const float* bias, float* y, hipStream_t st, const int* t_valid, int T) {
  const long n4 = rows * C / 4;
  ProfScope ps("bert_gelu_fwd", st);
  const auto kernel = t_valid ? bias_gelu_kernel<false, true> : bias_gelu_kernel<false, false>;
  hipLaunchKernelGGL(kernel, dim3((int)std::min<long>(cdiv(n4, 256), 4096)), dim3(256), 0, st, (const float*)nullptr, x, bias, y, n4, C / 4,
                     t_valid, T);
  return check_launch("bias_gelu_fwd");
}
int bias_gelu_bwd(long rows, int C, const float* dy, const float* x, const float* bias, float* dx, hipStream_t st, const int* t_valid, int T) {
  const long n4 = rows * C / 4;
  ProfScope ps("bert_gelu_bwd", st);
  const auto kernel = t_valid ? bias_gelu_kernel<true, true> : bias_gelu_kernel<true, false>;
  hipLaunchKernelGGL(kernel, dim3((int)std::min<long>(cdiv(n4, 256), 4096)), dim3(256), 0, st, dy, x, bias, dx, n4, C / 4, t_valid, T);
  return check_launch("bias_gelu_bwd");
}

// ---- one encoder layer -----------------------------------------------------------------------------------------------------------
namespace {
struct Saved {   // views into the forward's saved buffer (bert.hpp)
  float *qkv, *ctx, *lse, *ao, *a, *z, *g, *o2, *mean1, *rstd1, *mean2, *rstd2;
  long total;
};
long up4(long n) { return (n + 3) & ~3L; }   // every view stays 16-byte aligned
Saved saved_views(float* base, int B, int T, int D, int H, int Dff) {
  const long R = (long)B * T;
  Saved s;
  long o = 0;
  auto take = [&](long n) {
    float* p = base + o;
    o += up4(n);
    return p;
  };
  s.qkv = take(R * 3 * D), s.ctx = take(R * D), s.lse = take((long)B * H * T), s.ao = take(R * D), s.a = take(R * D);
  s.z = take(R * Dff), s.g = take(R * Dff), s.o2 = take(R * D);
  s.mean1 = take(R), s.rstd1 = take(R), s.mean2 = take(R), s.rstd2 = take(R);
  s.total = o;
  return s;
}
struct Work {   // the backward's workspace
  float *t1, *t2, *t3, *big, *delta, *split, *colpart, *lnpart;
  long split_elems, total;
};
constexpr int COL_PART_SLICES = 128;   // what a stand-alone column sum may use (rowops.hip), at least COL_RIDE_SLICES
Work work_views(float* base, int B, int T, int D, int H, int Dff) {
  const long R = (long)B * T;
  const int W = Dff > 3 * D ? Dff : 3 * D;
  Work w;
  long o = 0;
  auto take = [&](long n) {
    float* p = base + o;
    o += up4(n);
    return p;
  };
  w.t1 = take(R * D), w.t2 = take(R * D), w.t3 = take(R * D), w.big = take(R * W), w.delta = take((long)B * H * T);
  w.split_elems = gemm_ws_elems(W, D);
  w.split = take(w.split_elems), w.colpart = take((long)COL_PART_SLICES * W), w.lnpart = take(res_ln_ws_elems(D));
  w.total = o;
  return w;
}
}  // namespace

long bert_layer_saved_elems(int B, int T, int D, int H, int Dff) { return saved_views(nullptr, B, T, D, H, Dff).total; }
long bert_layer_ws_elems(int B, int T, int D, int H, int Dff) { return work_views(nullptr, B, T, D, H, Dff).total; }

// Token lengths (t_valid; bert.hpp has the contract).  On the fp32 route every product runs on the live 16-row blocks where the
// launcher serves the list (rowblk, gcgcn_row_blocks(B, T, t_valid); gemm_plan decides, per problem) and dense elsewhere.  Either way
// is correct because no product's padding rows are read unguarded: the kernel BEHIND each product is length-aware and stores the
// zeros that the next product, the weight gradients (which sum over the padding rows of a partly live block, or over all of them
// when dense) and the bias' column sums read --
//   forward :  qkv -> attention core (loads live rows only; ctx = 0),  ao -> LayerNorm (a = 0),  z -> GELU (g = 0),  o2 -> LayerNorm (y = 0)
//   backward:  dy -> LayerNorm (d o2 = d a = 0),  dg -> GELU (dz = 0),  da -> LayerNorm (d ao = dx' = 0),  dctx -> attention core (dqkv = 0)
// -- and dx, which leaves the layer, is zero-stored on the dead blocks by the product itself (rb_zero); on a partly live block and on
// the dense route it is dqkv Wqkv + dx' = 0 W + 0.
namespace {
GemmArgs on_rows(GemmArgs g, const int* rowblk, int mode, int zero_dead = 0) {
  if (rowblk) g.rb = rowblk + ROWBLK_HDR, g.rb_n = rowblk, g.rb_mode = mode, g.rb_zero = zero_dead;
  return g;
}

// One Linear of the layer, y [M][N] = x [M][K] w[N][K]^T + b, on the route that matmul names; the chains below are written once.
// BERT_MM_FP32: the GEMM layer.  BERT_MM_BF16: the same products on the bf16 matrix cores (gemm_bf16.hpp); everything between the
// products is the same fp32 code, the dropout sites and their indices included.  The bf16 products take the row-block list the way
// the fp32 ones do -- mode 1 forward and on the data gradients (rb_zero where dx leaves the layer), mode 2 on the weight gradients,
// which SKIP the 64-deep steps without a live block and otherwise sum in the dense order -- where their launcher serves it
// (gemm_bf16.hpp has the rule) and run dense elsewhere, and everywhere when option bf16_rows (GCGCN_BF16_ROWS, default 1) is 0.
// Either way gives the same bits: x is zero-stored by the caller and every other operand by the length-aware kernel in front of the
// product, bf16(0) = 0, so a dense dx is 0 W + 0 exactly and a skipped step would have added zeros.  The bf16 route's bias gradients
// are the exact fp32 column sums of the fp32 gradient tensors, launched stand-alone and dense (rowops' colsum through colpart: two
// launches per bias where the fp32 route has none of its own).
GemmBf16Args on_rows(GemmBf16Args g, const int* rowblk, int mode, int zero_dead = 0) {
  if (rowblk && option("bf16_rows", 1) != 0) g.rb = rowblk + ROWBLK_HDR, g.rb_n = rowblk, g.rb_mode = mode, g.rb_zero = zero_dead;
  return g;
}
struct Linear {
  int matmul, M;
  const int* rb;    // the live row blocks, or nullptr = dense
  const Work* wk;   // the backward's split-K and column-sum slices (the forward has none)
  hipStream_t st;

  int fwd(float* y, const float* x, const float* w, const float* bias, int N, int K) const {
    if (matmul == BERT_MM_BF16) {
      GemmBf16Args g = on_rows(gemm_bf16_stored(1, 1, x, K, w, K, y, N, M, N, K), rb, 1);
      g.bias = bias;
      return gemm_bf16(g, st);
    }
    GemmArgs g = on_rows(gemm_nt(x, K, w, K, y, N, M, N, K).tagged("bert_gemm"), rb, 1);
    g.bias = bias;
    return gemm(g, st, 0, 1);
  }
  // dw = dy^T x,  dx = dy w (+ add),  db = column sums of dy.  zero_dead: dx leaves the layer, the product zero-stores its dead blocks.
  int bwd(const float* dy, const float* x, const float* w, float* dw, float* dx, const float* add, float* db, int N, int K,
          int zero_dead = 0) const {
    if (matmul == BERT_MM_BF16) {
      GemmBf16Args gw = on_rows(gemm_bf16_stored(0, 0, dy, N, x, K, dw, K, N, K, M), rb, 2);
      gw.ws = wk->split, gw.ws_elems = wk->split_elems;
      GC_TRY(gemm_bf16(gw, st));
      GemmBf16Args gx = on_rows(gemm_bf16_stored(1, 0, dy, N, w, K, dx, K, M, K, N), rb, 1, zero_dead);
      gx.add = add, gx.ldadd = K, gx.ws = wk->split, gx.ws_elems = wk->split_elems;
      GC_TRY(gemm_bf16(gx, st));
      return colsum(dy, nullptr, db, M, N, N, 1, 0, 0, 0, 0, wk->colpart, st);
    }
    // one group launch: a weight gradient sums over the live row blocks (mode 2), a data gradient computes them (mode 1), the bias
    // gradient rides along as a column sum
    GemmArgs gs[2] = {on_rows(gemm_tn(dy, N, x, K, dw, K, N, K, M).split_ws(wk->split, wk->split_elems).tagged("bert_gemm"), rb, 2),
                      on_rows(gemm_nn(dy, N, w, K, dx, K, M, K, N).split_ws(wk->split, wk->split_elems).tagged("bert_gemm"), rb, 1, zero_dead)};
    if (add) gs[1].add = add, gs[1].ldadd = K;
    const ColRide cr = col_sum(dy, M, N, N, db, wk->colpart);
    return gemm_group(gs, 2, st, &cr);
  }
};
const int* live_blocks(const int* tv, int T, const int* rowblk) { return tv && T % 16 == 0 ? rowblk : nullptr; }
}  // namespace

int bert_layer_fwd(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const BertLayerParams& p, float* y,
                   float* saved, const void* snap, float p_attn, float p_hidden, hipStream_t st, const int* tv, const int* rowblk, int matmul,
                   int attn) {
  const long R = (long)B * T;
  const Saved s = saved_views(saved, B, T, D, H, Dff);
  const Linear lin = {matmul, (int)R, live_blocks(tv, T, rowblk), nullptr, st};
  GC_TRY(lin.fwd(s.qkv, x, p.wqkv, p.bqkv, 3 * D, D));
  GC_TRY(bert_attn_fwd(B, T, H, s.qkv, key_bias, s.ctx, s.lse, make_drop(snap, SALT_BERT_ATTN, p_attn), st, tv, attn));
  GC_TRY(lin.fwd(s.ao, s.ctx, p.wo, nullptr, D, D));
  GC_TRY(res_ln_fwd(R, D, s.ao, p.bo, x, p.ln1w, p.ln1b, s.a, s.mean1, s.rstd1, make_drop(snap, SALT_BERT_AO, p_hidden), st, tv, T));
  GC_TRY(lin.fwd(s.z, s.a, p.wi, nullptr, Dff, D));
  GC_TRY(bias_gelu_fwd(R, Dff, s.z, p.bi, s.g, st, tv, T));
  GC_TRY(lin.fwd(s.o2, s.g, p.wo2, nullptr, D, Dff));
  return res_ln_fwd(R, D, s.o2, p.bo2, s.a, p.ln2w, p.ln2b, y, s.mean2, s.rstd2, make_drop(snap, SALT_BERT_OUT, p_hidden), st, tv, T);
}

int bert_layer_bwd(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const BertLayerParams& p,
                   const float* saved, const float* dy, float* dx, const BertLayerGrads& d, float* ws, long ws_elems, const void* snap,
                   float p_attn, float p_hidden, hipStream_t st, const int* tv, const int* rowblk, int matmul, int attn) {
  const long R = (long)B * T;
  const Saved s = saved_views(const_cast<float*>(saved), B, T, D, H, Dff);
  const Work w = work_views(ws, B, T, D, H, Dff);
  GC_REQUIRE(ws_elems >= w.total, "bert_layer_bwd: workspace of %ld floats needed", w.total);
  const Linear lin = {matmul, (int)R, live_blocks(tv, T, rowblk), &w, st};

  // y = LN2(dropout(o2 + bo2) + a):  t1 = d o2, t2 = d a (the residual's share)
  GC_TRY(res_ln_bwd(R, D, dy, s.o2, p.bo2, s.a, p.ln2w, s.mean2, s.rstd2, w.t1, w.t2, d.ln2w, d.ln2b, w.lnpart,
                    make_drop(snap, SALT_BERT_OUT, p_hidden), st, tv, T));
  // o2 = g Wo2^T:  dWo2 = t1^T g, big = dg = t1 Wo2, dbo2 = column sums of t1
  GC_TRY(lin.bwd(w.t1, s.g, p.wo2, d.wo2, w.big, nullptr, d.bo2, D, Dff));
  GC_TRY(bias_gelu_bwd(R, Dff, w.big, s.z, p.bi, w.big, st, tv, T));   // big = dz
  // z = a Wi^T:  dWi = big^T a, t3 = da = big Wi + t2, dbi = column sums of big
  GC_TRY(lin.bwd(w.big, s.a, p.wi, d.wi, w.t3, w.t2, d.bi, Dff, D));
  // a = LN1(dropout(ao + bo) + x):  t1 = d ao, t2 = dx (the residual's share)
  GC_TRY(res_ln_bwd(R, D, w.t3, s.ao, p.bo, x, p.ln1w, s.mean1, s.rstd1, w.t1, w.t2, d.ln1w, d.ln1b, w.lnpart,
                    make_drop(snap, SALT_BERT_AO, p_hidden), st, tv, T));
  // ao = ctx Wo^T:  dWo = t1^T ctx, t3 = dctx = t1 Wo, dbo = column sums of t1
  GC_TRY(lin.bwd(w.t1, s.ctx, p.wo, d.wo, w.t3, nullptr, d.bo, D, D));
  GC_TRY(bert_attn_bwd(B, T, H, s.qkv, key_bias, s.ctx, s.lse, w.t3, w.big, w.delta, make_drop(snap, SALT_BERT_ATTN, p_attn), st, tv,
                       attn));   // big = dqkv
  // qkv = x Wqkv^T + b:  dWqkv = big^T x, dx = big Wqkv + t2 (it leaves the layer), dbqkv = column sums of big
  return lin.bwd(w.big, x, p.wqkv, d.wqkv, dx, w.t2, d.bqkv, 3 * D, D, 1);
}

}  // namespace gc
