// The BERT encoder layer (pytorch_pretrained_bert 0.6 BertLayer) and its three non-GEMM pieces: the masked attention core,
// y = LayerNorm(dropout(x + bias) + res), and the erf GELU with its bias (bert.hip).  Internal header.  DESIGN.md section 8.9.
#pragma once
#include "common.hpp"

namespace gc {

constexpr int BERT_DH = 64;        // the head width the attention kernels serve (768 / 12; every published BERT size has it)
constexpr int BERT_MAX_T = 512;    // the forward kernel keeps a query block's whole score rows in LDS
constexpr int BERT_LN_MAX_D = 1024;
constexpr float BERT_LN_EPS = 1e-12f;

// dropout sites: three per layer (each layer call has its own rng snapshot), one after the embeddings' LayerNorm
constexpr uint64_t SALT_BERT_ATTN = 0x42415431ull;   // on P, index = offset in the virtual [B][H][T][T] tensor
constexpr uint64_t SALT_BERT_AO = 0x42414f31ull;     // on attention.output.dense(ctx) + bias, index = offset in [B T][D]
constexpr uint64_t SALT_BERT_OUT = 0x424f5531ull;    // on output.dense(i) + bias, index = offset in [B T][D]

// ---- token lengths (include/gcgcn.h) -------------------------------------------------------------------------
// Every function below takes an optional t_valid (int32 [B] on the device, clamped to [0, T]; with the row functions also T, rows = B T):
// row (b, t) is live iff t < t_valid[b].  Live rows: what the function computes for document b alone at T = t_valid[b].  Padding rows:
// outputs (ctx, lse, dqkv, y, mean, rstd, dx, dres, gelu's out) are stored as exactly 0, inputs there (qkv, dctx, x, res, dy) are not read.
// nullptr: the code as it was.  Dropout indices do not change: T keeps the strides.
// ---- attention core on packed qkv [B][T][3 D], D = H * 64: row (b, t) holds q | k | v, head h in columns [64 h, 64 h + 64) of each.
// S = q k^T * alpha + key_bias[b][key] (key_bias [B][T] or nullptr), P = dropout(softmax over keys), ctx [B][T][D] = P v,
// lse [B][H][T] = log sum_j exp(S_ij - c_b), c_b = max_j key_bias[b][j] (0 without key_bias): the row's log-sum-exp relative to the
// document's largest penalty, which keeps a document whose keys are all masked at full precision.  Nothing of size [T][T] is written
// to memory.
// With t_valid: keys at or past t_valid[b] have probability exactly 0, c_b is the largest penalty of the document's LIVE keys.
// attn: BERT_ATTN_FP32 = the kernels of bert.hip, launch for launch what they were; BERT_ATTN_BF16 = the same contract with the four
// matrix products on bf16 operands (bert_attn_bf16.hip): q, k, v and dctx rounded once on their way into LDS or registers, P and dS
// when they become operands, fp32 accumulation, softmax, lse, delta and dS in fp32; the dropout mask is bit for bit the same.
constexpr int BERT_ATTN_FP32 = 0, BERT_ATTN_BF16 = 1;
int bert_attn_fwd(int B, int T, int H, const float* qkv, const float* key_bias, float* ctx, float* lse, Drop drop, hipStream_t st,
                  const int* t_valid = nullptr, int attn = BERT_ATTN_FP32);
// dqkv [B][T][3 D] = dq | dk | dv.  delta: [B][H][T] floats of scratch (sum_d dctx * ctx).  P is recomputed from q, k and lse and
// the dropout mask from the same Drop; one workgroup writes each element of dq (per query block) and of dk / dv (per key block).
int bert_attn_bwd(int B, int T, int H, const float* qkv, const float* key_bias, const float* ctx, const float* lse, const float* dctx,
                  float* dqkv, float* delta, Drop drop, hipStream_t st, const int* t_valid = nullptr, int attn = BERT_ATTN_FP32);
// the bf16 core's launches (bert_attn_bf16.hip); bert_attn_fwd / bert_attn_bwd dispatch to them, the backward after the delta kernel.
// ctx and dqkv must be 16-byte aligned.
int bert_attn_bf16_fwd(int B, int T, int H, const float* qkv, const float* key_bias, float* ctx, float* lse, Drop drop, hipStream_t st,
                       const int* t_valid);
int bert_attn_bf16_bwd(int B, int T, int H, const float* qkv, const float* key_bias, const float* lse, const float* delta,
                       const float* dctx, float* dqkv, Drop drop, hipStream_t st, const int* t_valid);

// ---- y [rows][D] = weight * (v - mean) / sqrt(var + 1e-12) + lnb,  v = dropout(x + bias) + res; bias, res, dropout each optional.
// D a multiple of 64, <= 1024.  mean / rstd [rows]: written when given (the backward reads them).  Dropout index = row * D + col.
int res_ln_fwd(long rows, int D, const float* x, const float* bias, const float* res, const float* weight, const float* lnb, float* y,
               float* mean, float* rstd, Drop drop, hipStream_t st, const int* t_valid = nullptr, int T = 0);
constexpr int BERT_LN_PARTS = 128;   // row groups of the backward's first stage
inline long res_ln_ws_elems(int D) { return 2L * BERT_LN_PARTS * D; }
// dx = gradient of x (and of bias, row by row), dres (optional) = gradient of res, dweight / dlnb by a two-stage column sum through
// part (res_ln_ws_elems(D) floats): stage 1 sums fixed row groups, stage 2 the groups in order.
int res_ln_bwd(long rows, int D, const float* dy, const float* x, const float* bias, const float* res, const float* weight,
               const float* mean, const float* rstd, float* dx, float* dres, float* dweight, float* dlnb, float* part, Drop drop,
               hipStream_t st, const int* t_valid = nullptr, int T = 0);
// stage 2 alone: dweight / dlnb from part [G][2][D], the G row groups in order (the fused embeddings stage writes its own stage 1)
int res_ln_bwd_reduce(const float* part, int G, int D, float* dweight, float* dlnb, hipStream_t st);

// ---- y = gelu(x + bias[col]), gelu(z) = z * 0.5 * (1 + erf(z / sqrt 2)); n = rows * C elements, C % 4 == 0; bias optional.
int bias_gelu_fwd(long rows, int C, const float* x, const float* bias, float* y, hipStream_t st, const int* t_valid = nullptr, int T = 0);
int bias_gelu_bwd(long rows, int C, const float* dy, const float* x, const float* bias, float* dx, hipStream_t st,   // dx may be dy
                  const int* t_valid = nullptr, int T = 0);

// ---- one encoder layer ---------------------------------------------------------------------------------------------------------
// wqkv [3 D][D] / bqkv [3 D]: query | key | value stacked (one product instead of three).  Linear weights are [out][in].
struct BertLayerParams {
  const float *wqkv, *bqkv, *wo, *bo, *ln1w, *ln1b, *wi, *bi, *wo2, *bo2, *ln2w, *ln2b;
};
struct BertLayerGrads {
  float *wqkv, *bqkv, *wo, *bo, *ln1w, *ln1b, *wi, *bi, *wo2, *bo2, *ln2w, *ln2b;
};
// What the forward keeps for the backward, in this order (floats, R = B T, Dff = the intermediate size): qkv [R][3 D], ctx [R][D],
// lse [B][H][T], ao [R][D] (attention.output.dense without bias), a [R][D] (first LayerNorm), z [R][Dff] (intermediate.dense without
// bias), g [R][Dff] (gelu), o2 [R][D] (output.dense without bias), mean1, rstd1, mean2, rstd2 [R] each: 7 D + 2 Dff + H + 4 per token
// beside the layer's input x (another D) and output y, which the caller holds anyway.
long bert_layer_saved_elems(int B, int T, int D, int H, int Dff);
long bert_layer_ws_elems(int B, int T, int D, int H, int Dff);   // the backward's workspace
// t_valid: x must be zero on padding rows (the caller's, as for the graph blocks' X); y and dx are exactly zero there, dy there is
// not read.  rowblk: gcgcn_row_blocks(B, T, t_valid) (T a multiple of 16) or nullptr -- the products then run on the live 16-row blocks
// wherever the GEMM launcher serves the list, dense elsewhere; the results obey the same contract either way.
// matmul: BERT_MM_FP32 = the fp32-MFMA GEMM layer, launch for launch what it was; BERT_MM_BF16 = the twelve Linear products with bf16
// operands (gemm_bf16.hpp: fp32 in memory, rounded once on the way into LDS, fp32 accumulation), on the live row blocks of rowblk where
// that launcher serves the list (bit for bit the dense products; option bf16_rows = 0 runs them dense), the bias gradients as
// stand-alone fp32 column sums.  The saved state and the workspace are the same either way.
// attn: the attention core's selector (above), independent of matmul.
constexpr int BERT_MM_FP32 = 0, BERT_MM_BF16 = 1;
int bert_layer_fwd(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const BertLayerParams& p, float* y,
                   float* saved, const void* snap, float p_attn, float p_hidden, hipStream_t st, const int* t_valid = nullptr,
                   const int* rowblk = nullptr, int matmul = BERT_MM_FP32, int attn = BERT_ATTN_FP32);
int bert_layer_bwd(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const BertLayerParams& p,
                   const float* saved, const float* dy, float* dx, const BertLayerGrads& g, float* ws, long ws_elems, const void* snap,
                   float p_attn, float p_hidden, hipStream_t st, const int* t_valid = nullptr, const int* rowblk = nullptr,
                   int matmul = BERT_MM_FP32, int attn = BERT_ATTN_FP32);

}  // namespace gc
