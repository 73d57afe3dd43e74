// The BERT graph model's own glue either side of the shared tail (include/gcgcn_bert_frontend.h, symbols gcbf_*).  DESIGN.md section 8.8.
//
// The folded context pair: linear_re over cat(states, entity_embed[document_pos], ner_emb[document_ner]) with weight = W1 | W2 | W3 is
//   pre[b, t] = states[b, t] W1^T + bias + F2[document_pos[b, t]] + F3[document_ner[b, t]],   F2 = coref_w W2^T,  F3 = ner_w W3^T
// so the concatenated [B T][Dw + Dc + Dn] tensor exists in neither direction and the large product runs at K = Dw.
//   gcbf_context_fwd :  gemm_group              the two fold products F2, F3 (tiny; W2 / W3 read in place at the weight's leading dimension)
//                       context_fwd_ld          frontend.hip's pair with the weight at ldb = Dw + Dc + Dn and context_fwd_kernel<true>, which
//                                               adds the two gathered 128-wide rows in front of tanh (the pooling workgroups as well)
//   gcbf_context_bwd :  context_bwd_ld          frontend.hip's: context_bwd_kernel -> dpre; dW1 = dpre^T states at ldc = Dw + Dc + Dn,
//                                               dstates = dpre W1, dbias riding as the column sum
//                       embed_bwd, twice        frontend.hip's owner-computes scheme on dpre, once per table at width 128 and no padding
//                                               row: dF2 [P][128], dF3 [R][128], every token counted
//                       gemm_group              dweight[:, Dw:Dw+Dc] = dF2^T coref_w, dweight[:, Dw+Dc:] = dF3^T ner_w, dcoref = dF2 W2, dner = dF3 W3
//                       bfe_pad_rows_kernel     the two padding rows of dcoref / dner: exact zeros
// The [CLS] logit tail:
//   gcbf_logit_bias_fwd :  bfe_logit_bias_kernel   one streaming pass, 16 bytes a thread where the flat tensor allows (a vector may straddle
//                                                  two pairs, as loss.hip's backward: R = 97 rows are not 16-byte aligned)
//   gcbf_logit_bias_bwd :  bfe_dcls_rows_kernel    part[b, i, :] = sum_j dout[b, i, j, :], j in two interleaved halves, each ascending
//                          bfe_dcls_sum_kernel     dcls[b, :] = sum_i part[b, i, :], i ascending
// Every output element has one writer and a fixed order, no float is added atomically, nothing reads back to the host: two runs are
// bitwise equal and both pairs are capturable.
#include "../../include/gcgcn_bert_frontend.h"
#include "frontend.hpp"
#include "gemm.hpp"

namespace gc {

struct BfeArgs {
  int B, T, N, Dw, Dc, Dn, P, R;
  const float* states;
  const int64_t *pos_ids, *ner_ids;
  const float *coref_w, *ner_w, *weight, *node_pos;
  int K() const { return Dw + Dc + Dn; }
};

static int bfe_context_fwd(const BfeArgs& a, const float* bias, float* fold, float* pre, float* ctx, float* node_feat, hipStream_t st) {
  const int K = a.K();
  float *f2 = fold, *f3 = fold + (long)a.P * FE_HD;
  const GemmArgs gs[2] = {
      gemm_nt(a.coref_w, a.Dc, a.weight + a.Dw, K, f2, FE_HD, a.P, FE_HD, a.Dc).tagged("bfe_fold"),
      gemm_nt(a.ner_w, a.Dn, a.weight + a.Dw + a.Dc, K, f3, FE_HD, a.R, FE_HD, a.Dn).tagged("bfe_fold"),
  };
  GC_TRY(gemm_group(gs, 2, st));
  const ContextFold fo = {a.pos_ids, a.ner_ids, f2, f3, a.P, a.R};
  return context_fwd_ld(a.B, a.T, a.N, a.Dw, a.states, a.weight, K, bias, a.node_pos, pre, ctx, node_feat, st, &fo);
}

// grid 2: workgroup 0 zeroes row cpad of dcoref, workgroup 1 row npad of dner (a negative index: the table has no padding row)
__global__ __launch_bounds__(256) void bfe_pad_rows_kernel(float* __restrict__ dcoref, const int Dc, const int cpad, float* __restrict__ dner,
                                                           const int Dn, const int npad) {
  float* row = blockIdx.x == 0 ? dcoref + (long)cpad * Dc : dner + (long)npad * Dn;
  const int w = blockIdx.x == 0 ? Dc : Dn, pad = blockIdx.x == 0 ? cpad : npad;
  if (pad < 0) return;
  for (int c = threadIdx.x; c < w; c += 256) row[c] = 0.f;
}

// The backward's workspace (floats, each view 16-byte aligned): dpre [B T][128] | dF2 [P][128] | dF3 [R][128] | context_bwd's | embed_bwd's
namespace {
long up4(long n) { return (n + 3) & ~3L; }
EmbedTables fold_table(const int64_t* ids, float* df, int rows) {
  EmbedTables tb;
  tb.t[0] = EmbedTable{ids, nullptr, df, rows, FE_HD, -1};
  tb.t[1] = tb.t[2] = EmbedTable{nullptr, nullptr, nullptr, 0, 0, -1};
  return tb;
}
struct BfeWs {
  float *dpre, *df2, *df3, *ctxws;
  long ctx_elems;
  char* embed;
  long embed_bytes, total;
};
BfeWs bfe_ws(void* base, int B, int T, int Dw, int P, int R) {
  const long rows = (long)B * T;
  BfeWs w;
  long off = 0;
  auto take = [&](long elems) {
    float* p = (float*)base + off;
    off += up4(elems);
    return p;
  };
  w.ctx_elems = context_ws_elems(Dw);
  w.dpre = take(rows * FE_HD), w.df2 = take((long)P * FE_HD), w.df3 = take((long)R * FE_HD), w.ctxws = take(w.ctx_elems);
  w.embed = (char*)base + 4 * off;
  w.embed_bytes = std::max(embed_ws_bytes(rows, fold_table(nullptr, nullptr, P)), embed_ws_bytes(rows, fold_table(nullptr, nullptr, R)));
  w.total = 4 * off + w.embed_bytes;
  return w;
}
}  // namespace

static int bfe_context_bwd(const BfeArgs& a, const float* ctx, const float* dctx, const float* dnode, int cpad, int npad, float* dstates,
                           float* dweight, float* dbias, float* dcoref, float* dner, void* ws, long ws_bytes, hipStream_t st) {
  const int K = a.K();
  const BfeWs w = bfe_ws(ws, a.B, a.T, a.Dw, a.P, a.R);
  GC_REQUIRE(ws_bytes >= w.total, "bert_context_bwd: workspace of %ld bytes needed", w.total);
  GC_TRY(context_bwd_ld(a.B, a.T, a.N, a.Dw, a.states, a.weight, K, a.node_pos, ctx, dctx, dnode, w.dpre, dstates, dweight, dbias, w.ctxws,
                        w.ctx_elems, st));
  GC_TRY(embed_bwd(a.B, a.T, fold_table(a.pos_ids, w.df2, a.P), w.dpre, nullptr, w.embed, w.embed_bytes, st, nullptr, 1));
  GC_TRY(embed_bwd(a.B, a.T, fold_table(a.ner_ids, w.df3, a.R), w.dpre, nullptr, w.embed, w.embed_bytes, st, nullptr, 1));
  const float *w2 = a.weight + a.Dw, *w3 = a.weight + a.Dw + a.Dc;
  const GemmArgs gs[4] = {
      gemm_tn(w.df2, FE_HD, a.coref_w, a.Dc, dweight + a.Dw, K, FE_HD, a.Dc, a.P).tagged("bfe_fold"),
      gemm_tn(w.df3, FE_HD, a.ner_w, a.Dn, dweight + a.Dw + a.Dc, K, FE_HD, a.Dn, a.R).tagged("bfe_fold"),
      gemm_nn(w.df2, FE_HD, w2, K, dcoref, a.Dc, a.P, a.Dc, FE_HD).tagged("bfe_fold"),
      gemm_nn(w.df3, FE_HD, w3, K, dner, a.Dn, a.R, a.Dn, FE_HD).tagged("bfe_fold"),
  };
  GC_TRY(gemm_group(gs, 4, st));
  if (cpad < 0 && npad < 0) return 0;
  hipLaunchKernelGGL(bfe_pad_rows_kernel, dim3(2), dim3(256), 0, st, dcoref, a.Dc, cpad, dner, a.Dn, npad);
  return check_launch("bert_context_pad_rows");
}

// ---- the [CLS] logit tail ------------------------------------------------------------------------------------------------------
// a thread owns VEC consecutive floats of the flat [B N N R] tensor; the pair (b, i, j) is worked out once and stepped where a row ends
template <int VEC>
__global__ __launch_bounds__(256) void bfe_logit_bias_kernel(const float* __restrict__ logits, const float* __restrict__ cls,
                                                             const int* __restrict__ n_valid, float* __restrict__ out, const int N,
                                                             const int R, const long total) {
  const long e0 = ((long)blockIdx.x * 256 + threadIdx.x) * VEC;
  if (e0 >= total) return;
  float x[VEC];
  if constexpr (VEC == 4) {
    const float4 v = *reinterpret_cast<const float4*>(logits + e0);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
  } else {
    x[0] = logits[e0];
  }
  unsigned pair = (unsigned)e0 / (unsigned)R;   // total < 2^31 (the C entry checks)
  int r = (int)((unsigned)e0 - pair * (unsigned)R);
  bool live = false;
  int b = 0;
  const auto place = [&]() {
    const unsigned row = pair / (unsigned)N;
    const int j = (int)(pair - row * (unsigned)N);
    b = (int)(row / (unsigned)N);
    const int i = (int)(row - (unsigned)b * (unsigned)N);
    const int nv = n_valid ? min(max(n_valid[b], 0), N) : N;
    live = i < nv && j < nv;
  };
  place();
#pragma unroll
  for (int u = 0; u < VEC; ++u) {
    if (live) x[u] += cls[(long)b * R + r];
    if (++r == R && u + 1 < VEC) {
      r = 0, ++pair;
      place();   // past the end of the tensor only in lanes whose remaining elements do not exist (VEC == 4: total % 4 == 0, none)
    }
  }
  if constexpr (VEC == 4) *reinterpret_cast<float4*>(out + e0) = make_float4(x[0], x[1], x[2], x[3]);
  else out[e0] = x[0];
}

static int bfe_logit_bias_fwd(int B, int N, int R, const float* logits, const float* cls, const int* n_valid, float* out, hipStream_t st) {
  const long total = (long)B * N * N * R;
  auto al = [](const void* p) { return (((uintptr_t)p) & 15) == 0; };
  if (total % 4 == 0 && al(logits) && al(out))
    GC_LAUNCH_TIMED("bfe_logit_bias", 8.0 * total, bfe_logit_bias_kernel<4>, dim3(cdiv(total / 4, 256)), dim3(256), 0, st, logits, cls, n_valid,
                    out, N, R, total);
  else
    GC_LAUNCH_TIMED("bfe_logit_bias", 8.0 * total, bfe_logit_bias_kernel<1>, dim3(cdiv(total, 256)), dim3(256), 0, st, logits, cls, n_valid, out,
                    N, R, total);
  return check_launch("logit_bias_fwd");
}

// grid (N, B), 256 threads = 2 halves x 128 columns: part[b, i, r] = (sum of the even j < nv, ascending) + (sum of the odd ones);
// rows i >= nv are neither written nor read
__global__ __launch_bounds__(256) void bfe_dcls_rows_kernel(const float* __restrict__ dout, const int* __restrict__ n_valid,
                                                            float* __restrict__ part, const int N, const int R) {
  __shared__ float odd[128];
  const int i = blockIdx.x, b = blockIdx.y, half = threadIdx.x >> 7, c = threadIdx.x & 127;
  const int nv = n_valid ? min(max(n_valid[b], 0), N) : N;
  if (i >= nv) return;   // the whole workgroup
  const float* rows = dout + ((long)b * N + i) * N * R;
  for (int r0 = 0; r0 < R; r0 += 128) {
    const int r = r0 + c;
    float acc = 0.f;
    if (r < R) {
      int j = half;
      for (; j + 6 < nv; j += 8) {   // four rows in flight
        const float v0 = rows[(long)j * R + r], v1 = rows[(long)(j + 2) * R + r], v2 = rows[(long)(j + 4) * R + r],
                    v3 = rows[(long)(j + 6) * R + r];
        acc += v0, acc += v1, acc += v2, acc += v3;
      }
      for (; j < nv; j += 2) acc += rows[(long)j * R + r];
    }
    if (half == 1) odd[c] = acc;
    __syncthreads();
    if (half == 0 && r < R) part[((long)b * N + i) * R + r] = acc + odd[c];
    __syncthreads();   // the next 128 columns rewrite odd
  }
}
// grid (R / 256 rounded up, B)
__global__ __launch_bounds__(256) void bfe_dcls_sum_kernel(const float* __restrict__ part, const int* __restrict__ n_valid,
                                                           float* __restrict__ dcls, const int N, const int R) {
  const int r = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (r >= R) return;
  const int nv = n_valid ? min(max(n_valid[b], 0), N) : N;
  float s = 0.f;
  for (int i = 0; i < nv; ++i) s += part[((long)b * N + i) * R + r];
  dcls[(long)b * R + r] = s;
}

static int bfe_logit_bias_bwd(int B, int N, int R, const float* dout, const int* n_valid, float* dcls, float* part, hipStream_t st) {
  GC_LAUNCH_TIMED("bfe_dcls_rows", 4.0 * B * N * N * R, bfe_dcls_rows_kernel, dim3(N, B), dim3(256), 0, st, dout, n_valid, part, N, R);
  GC_TRY(check_launch("logit_bias_bwd_rows"));
  hipLaunchKernelGGL(bfe_dcls_sum_kernel, dim3(cdiv(R, 256), B), dim3(256), 0, st, part, n_valid, dcls, N, R);
  return check_launch("logit_bias_bwd_sum");
}

}  // namespace gc

// ---- the C boundary ------------------------------------------------------------------------------------------------------------
using namespace gc;

static bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

static int bfe_shape_ok(const char* who, int B, int T, int N, int Dw, int Dc, int Dn, int P, int R) {
  GC_REQUIRE(B >= 1 && T >= 1 && N >= 1 && B <= 65535, "%s: bad shape B=%d T=%d N=%d", who, B, T, N);
  GC_REQUIRE(Dw >= 1 && Dc >= 1 && Dn >= 1, "%s: a width below 1 (Dw=%d Dc=%d Dn=%d)", who, Dw, Dc, Dn);
  GC_REQUIRE(P >= 1 && R >= 1, "%s: bad tables P=%d R=%d", who, P, R);
  GC_REQUIRE((long)B * T <= 0x7fffff00L && (long)B * T * (Dw > FE_HD ? Dw : FE_HD) <= 0x7fffffffL && (long)B * N * T <= 0x7fffffffL &&
                 (long)Dw + Dc + Dn <= 0x7fffffL && (long)P * FE_HD <= 0x7fffffffL && (long)R * FE_HD <= 0x7fffffffL,
             "%s: B=%d T=%d N=%d Dw=%d P=%d R=%d is too large", who, B, T, N, Dw, P, R);
  return 0;
}
static int bfe_tail_ok(const char* who, int B, int N, int R) {
  GC_REQUIRE(B >= 1 && N >= 1 && R >= 1, "%s: bad shape B=%d N=%d R=%d", who, B, N, R);
  GC_REQUIRE(B <= 65535 && (long)B * N * N * R <= 0x7fffffffL, "%s: B=%d N=%d R=%d is too large (B N N R < 2^31)", who, B, N, R);
  return 0;
}

extern "C" int64_t gcbf_context_ws_bytes(int B, int T, int N, int Dw, int Dc, int Dn, int P, int R) {
  if (bfe_shape_ok("gcbf_context_ws_bytes", B, T, N, Dw, Dc, Dn, P, R)) return -1;
  return bfe_ws(nullptr, B, T, Dw, P, R).total;
}

extern "C" int gcbf_context_fwd(int B, int T, int N, int Dw, int Dc, int Dn, int P, int R, const float* states, const int64_t* document_pos,
                                const int64_t* document_ner, const float* coref_w, const float* ner_w, const float* weight, const float* bias,
                                const float* node_pos, float* fold, float* pre, float* ctx, float* node_feat, void* stream) {
  GC_TRY(bfe_shape_ok("gcbf_context_fwd", B, T, N, Dw, Dc, Dn, P, R));
  GC_REQUIRE(states && document_pos && document_ner && coref_w && ner_w && weight && bias && node_pos && fold && pre && ctx && node_feat,
             "gcbf_context_fwd: null pointer");
  GC_REQUIRE(al16(fold) && al16(pre) && al16(ctx), "gcbf_context_fwd: fold, pre and ctx must be 16-byte aligned");
  GC_REQUIRE(pre != ctx, "gcbf_context_fwd: ctx aliases pre (the pooling reads pre while ctx is being written)");
  const BfeArgs a = {B, T, N, Dw, Dc, Dn, P, R, states, document_pos, document_ner, coref_w, ner_w, weight, node_pos};
  return bfe_context_fwd(a, bias, fold, pre, ctx, node_feat, (hipStream_t)stream);
}

extern "C" int gcbf_context_bwd(int B, int T, int N, int Dw, int Dc, int Dn, int P, int R, const float* states, const int64_t* document_pos,
                                const int64_t* document_ner, const float* coref_w, const float* ner_w, const float* weight,
                                const float* node_pos, const float* ctx, const float* dctx, const float* dnode_feat, int coref_padding_idx,
                                int ner_padding_idx, float* dstates, float* dweight, float* dbias, float* dcoref, float* dner, void* ws,
                                int64_t ws_bytes, void* stream) {
  GC_TRY(bfe_shape_ok("gcbf_context_bwd", B, T, N, Dw, Dc, Dn, P, R));
  GC_REQUIRE(states && document_pos && document_ner && coref_w && ner_w && weight && node_pos && ctx && dctx && dnode_feat && dstates &&
                 dweight && dbias && dcoref && dner,
             "gcbf_context_bwd: null pointer");
  GC_REQUIRE(coref_padding_idx < P && ner_padding_idx < R, "gcbf_context_bwd: padding index %d / %d outside its table (P=%d R=%d)",
             coref_padding_idx, ner_padding_idx, P, R);
  GC_REQUIRE(ws && al16(ws) && ws_bytes >= gcbf_context_ws_bytes(B, T, N, Dw, Dc, Dn, P, R),
             "gcbf_context_bwd: a 16-byte aligned workspace of %lld bytes needed (gcbf_context_ws_bytes)",
             (long long)gcbf_context_ws_bytes(B, T, N, Dw, Dc, Dn, P, R));
  const BfeArgs a = {B, T, N, Dw, Dc, Dn, P, R, states, document_pos, document_ner, coref_w, ner_w, weight, node_pos};
  return bfe_context_bwd(a, ctx, dctx, dnode_feat, coref_padding_idx, ner_padding_idx, dstates, dweight, dbias, dcoref, dner, ws, ws_bytes,
                         (hipStream_t)stream);
}

extern "C" int64_t gcbf_logit_bias_ws_bytes(int B, int N, int R) {
  if (bfe_tail_ok("gcbf_logit_bias_ws_bytes", B, N, R)) return -1;
  return (int64_t)sizeof(float) * B * N * R;
}

extern "C" int gcbf_logit_bias_fwd(int B, int N, int R, const float* logits, const float* cls, const int32_t* n_valid, float* out,
                                   void* stream) {
  GC_TRY(bfe_tail_ok("gcbf_logit_bias_fwd", B, N, R));
  GC_REQUIRE(logits && cls && out, "gcbf_logit_bias_fwd: null pointer");
  return bfe_logit_bias_fwd(B, N, R, logits, cls, n_valid, out, (hipStream_t)stream);
}

extern "C" int gcbf_logit_bias_bwd(int B, int N, int R, const float* dout, const int32_t* n_valid, float* dcls, void* ws, int64_t ws_bytes,
                                   void* stream) {
  GC_TRY(bfe_tail_ok("gcbf_logit_bias_bwd", B, N, R));
  GC_REQUIRE(dout && dcls, "gcbf_logit_bias_bwd: null pointer");
  GC_REQUIRE(ws && al16(ws) && ws_bytes >= gcbf_logit_bias_ws_bytes(B, N, R),
             "gcbf_logit_bias_bwd: a 16-byte aligned workspace of %lld bytes needed (gcbf_logit_bias_ws_bytes)",
             (long long)gcbf_logit_bias_ws_bytes(B, N, R));
  return bfe_logit_bias_bwd(B, N, R, dout, n_valid, dcls, (float*)ws, (hipStream_t)stream);
}
