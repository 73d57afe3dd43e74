// The embeddings stage in front of the BERT encoder layers, fused (include/gcgcn_bert_embed.h, symbols gcbe_*).  DESIGN.md section 8.9.
//
//   gcbe_fwd :  bemb_fwd_kernel        one wave per token row: the word row by id, the position row and the type row are loaded
//                                      together, summed as (w + p) + s, normalised with ln_row.hpp's row body, dropped and stored once;
//                                      a padding row stores zeros and reads neither ids nor tables.  emb never reaches memory.
//   gcbe_bwd :  bemb_bwd_kernel        gathers the row again; demb [B T][D] = the LayerNorm's backward of dy times the regenerated
//                                      dropout factor (zero on padding rows); the weight's and bias' column sums of fixed row groups
//               res_ln_bwd_reduce      bert.hip's second stage: the groups in order -> dln_w, dln_b
//               embed_bwd              frontend.hip's owner-computes scheme on the word table alone: memset of the touched flags,
//                                      embed_bwd_chunk_kernel<LEN> (256 tokens sorted by id, runs summed in ascending position),
//                                      embed_bwd_rows_kernel (one wave per table row, chunks ascending; untouched rows zero-filled)
//               bemb_pos_kernel        one wave per (position row, 64 columns): the documents in ascending b; rows >= T zero-filled
//               bemb_type_kernel       stage 1: a fixed group of consecutive tokens per workgroup, per type row the tokens in order
//               bemb_type_sum_kernel   stage 2: the groups in order
//
// Every element of every output has one writer, no float is added atomically, the orders depend on (B, T) and the ids' positions
// alone: two runs are bitwise equal.  Nothing reads back to the host: capturable, and a replay follows new ids and lengths.
// Every table access is predicated on 0 <= id < rows.
#include "../../include/gcgcn_bert_embed.h"
#include "bert_embed.hpp"
#include "bert_attn.hpp"
#include "frontend.hpp"
#include "ln_row.hpp"

namespace gc {

// emb of row (b, t) into the lane's registers: (word[id] + pos[t]) + type[tt], the three loads of a column issued together
__device__ __forceinline__ void bemb_gather(float (&v)[LNV], const BertEmbedArgs& a, const long row, const int t, const int l) {
  const int n = a.D >> 6;
  const int64_t id = a.ids[row], ty = a.tts[row];
  const bool okw = id >= 0 && id < a.V, oks = ty >= 0 && ty < a.Ty;   // ids are validated by the caller; a bad one reads nothing
  const float* wr = a.word + (okw ? id : 0) * (long)a.D;
  const float* pr = a.pos + (long)t * a.D;
  const float* sr = a.type + (oks ? ty : 0) * (long)a.D;
#pragma unroll
  for (int i = 0; i < LNV; ++i) {
    v[i] = 0.f;
    if (i < n) {
      const int c = l + 64 * i;
      const float w = okw ? wr[c] : 0.f, p = pr[c], s = oks ? sr[c] : 0.f;
      v[i] = (w + p) + s;
    }
  }
}

__global__ __launch_bounds__(256) void bemb_fwd_kernel(const BertEmbedArgs a, float* __restrict__ y, float* __restrict__ mean,
                                                       float* __restrict__ rstd, const long rows, const Drop drop) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;   // wave-uniform
  const int l = threadIdx.x & 63, D = a.D, n = D >> 6;
  const int b = (int)(row / a.T), t = (int)(row % a.T);
  if (a.t_valid && t >= live_len(a.t_valid, b, a.T)) {   // wave-uniform
    for (int i = 0; i < n; ++i) y[row * D + l + 64 * i] = 0.f;
    if (l == 0) mean[row] = 0.f, rstd[row] = 0.f;
    return;
  }
  const uint64_t dk = drop.snap ? drop_key(drop) : 0;
  float v[LNV];
  bemb_gather(v, a, row, t, l);
  float m, r;
  ln_row_stats(v, n, D, m, r);
#pragma unroll
  for (int i = 0; i < LNV; ++i)
    if (i < n) {
      const int c = l + 64 * i;
      const long o = row * D + c;
      const float x = ln_row_out(v[i], m, r, a.lnw[c], a.lnb[c]);
      y[o] = drop.snap ? (rng_u32(dk, (uint64_t)o) >= drop.thresh ? x * drop.scale : 0.f) : x;
    }
  if (l == 0) mean[row] = m, rstd[row] = r;
}

// Stage 1 of the backward, res_ln_bwd_kernel's shape: workgroup g takes rows 4 g + w, 4 (g + G) + w, ...; part [G][2][D]
__global__ __launch_bounds__(256) void bemb_bwd_kernel(const BertEmbedArgs a, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                       const float* __restrict__ dy, float* __restrict__ demb, float* __restrict__ part,
                                                       const long rows, const Drop drop) {
  __shared__ float sh[4][2][BERT_LN_MAX_D];
  const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, D = a.D, n = D >> 6;
  const uint64_t dk = drop.snap ? drop_key(drop) : 0;
  float aw[LNV], ab[LNV];
#pragma unroll
  for (int i = 0; i < LNV; ++i) aw[i] = 0.f, ab[i] = 0.f;
  for (long row = (long)blockIdx.x * 4 + wv; row < rows; row += (long)gridDim.x * 4) {
    const int b = (int)(row / a.T), t = (int)(row % a.T);
    if (a.t_valid && t >= live_len(a.t_valid, b, a.T)) {   // a padding row (wave-uniform): dy and the ids there are not read
      for (int i = 0; i < n; ++i) demb[row * D + l + 64 * i] = 0.f;
      continue;
    }
    float v[LNV];
    bemb_gather(v, a, row, t, l);
    const float m = mean[row], r = rstd[row];
    const auto dload = [&](const int i) {   // dy times the dropout factor, regenerated from the counter
      const long o = row * D + l + 64 * i;
      const float g = dy[o];
      return drop.snap ? (rng_u32(dk, (uint64_t)o) >= drop.thresh ? g * drop.scale : 0.f) : g;
    };
    ln_row_bwd(v, dload, [&](const int i, const float dv) { demb[row * D + l + 64 * i] = dv; }, a.lnw, n, D, l, m, r, aw, ab);
  }
  ln_part_store(sh, aw, ab, part, n, D, wv, l);
}

// grid (Pmax, slices of 4 x 64 columns): dpos[t] = sum over the documents, b ascending, of the live rows (b, t)
__global__ __launch_bounds__(256) void bemb_pos_kernel(const float* __restrict__ demb, const int* __restrict__ t_valid, float* __restrict__ dpos,
                                                       const int B, const int T, const int D) {
  const int t = blockIdx.x, c = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 64 + (threadIdx.x & 63);
  if (c >= D) return;   // wave-uniform
  float acc = 0.f;
  if (t < T)
    for (int b = 0; b < B; ++b)
      if (!t_valid || t < live_len(t_valid, b, T)) acc += demb[((long)b * T + t) * D + c];
  dpos[(long)t * D + c] = acc;
}

// grid (G, D / 256 rounded up): workgroup g owns tokens [g per, (g + 1) per); part [G][Ty][D], every cell written
__global__ __launch_bounds__(256) void bemb_type_kernel(const float* __restrict__ demb, const int64_t* __restrict__ tts,
                                                        const int* __restrict__ t_valid, float* __restrict__ part, const long rows,
                                                        const int per, const int T, const int D, const int Ty) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= D) return;
  const long r0 = (long)blockIdx.x * per, r1 = r0 + per < rows ? r0 + per : rows;
  for (int ty = 0; ty < Ty; ++ty) {
    float acc = 0.f;
    for (long row = r0; row < r1; ++row) {   // the tests are the same in every thread
      if (t_valid && (int)(row % T) >= live_len(t_valid, (int)(row / T), T)) continue;
      if (tts[row] == ty) acc += demb[row * D + c];
    }
    part[((long)blockIdx.x * Ty + ty) * D + c] = acc;
  }
}
__global__ __launch_bounds__(256) void bemb_type_sum_kernel(const float* __restrict__ part, float* __restrict__ dtype, const int G,
                                                            const long cells) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= cells) return;
  float s = 0.f;
  for (int g = 0; g < G; ++g) s += part[(long)g * cells + i];
  dtype[i] = s;
}

int bert_embed_fwd(const BertEmbedArgs& a, float* y, float* mean, float* rstd, Drop drop, hipStream_t st) {
  const long rows = (long)a.B * a.T;
  GC_LAUNCH_TIMED("bert_embed_fwd", 4.0 * rows * a.D * 4, bemb_fwd_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, a, y, mean, rstd, rows,
                  drop);
  return check_launch("bert_embed_fwd");
}

// The workspace: demb [B T][D] | LayerNorm partials | type partials [G][Ty][D] (floats, each view 16-byte aligned) | embed_bwd's own
namespace {
long up4(long n) { return (n + 3) & ~3L; }
int type_groups(long rows) { return (int)std::min<long>(BEMB_TYPE_GROUPS, cdiv(rows, 32)); }
EmbedTables word_table(const BertEmbedArgs& a, float* dword) {
  EmbedTables tb;
  tb.t[0] = EmbedTable{a.ids, a.word, dword, a.V, a.D, -1};
  tb.t[1] = tb.t[2] = EmbedTable{nullptr, nullptr, nullptr, 0, 0, -1};
  return tb;
}
struct BembWs {
  float *demb, *lnpart, *typart;
  char* embed;
  long embed_bytes, total;
};
BembWs bemb_ws(void* base, int B, int T, int D, int V, int Ty) {
  const long rows = (long)B * T;
  BertEmbedArgs a{};
  a.V = V, a.D = D;
  BembWs w;
  long off = 0;
  auto take = [&](long elems) {
    float* p = (float*)base + off;
    off += up4(elems);
    return p;
  };
  w.demb = take(rows * D), w.lnpart = take(res_ln_ws_elems(D)), w.typart = take((long)type_groups(rows) * Ty * D);
  w.embed = (char*)base + 4 * off;
  w.embed_bytes = embed_ws_bytes(rows, word_table(a, nullptr));
  w.total = 4 * off + w.embed_bytes;
  return w;
}
}  // namespace

long bert_embed_ws_bytes(int B, int T, int D, int V, int Ty) { return bemb_ws(nullptr, B, T, D, V, Ty).total; }

int bert_embed_bwd(const BertEmbedArgs& a, const float* mean, const float* rstd, const float* dy, float* dword, float* dpos, float* dtype,
                   float* dlnw, float* dlnb, void* ws, long ws_bytes, Drop drop, hipStream_t st) {
  const long rows = (long)a.B * a.T;
  const int D = a.D;
  const BembWs w = bemb_ws(ws, a.B, a.T, D, a.V, a.Ty);
  GC_REQUIRE(ws_bytes >= w.total, "bert_embed_bwd: workspace of %ld bytes needed", w.total);
  const int G = (int)std::min<long>(BERT_LN_PARTS, cdiv(rows, 4));
  GC_LAUNCH_TIMED("bert_embed_bwd", 4.0 * rows * D * 5, bemb_bwd_kernel, dim3(G), dim3(256), 0, st, a, mean, rstd, dy, w.demb, w.lnpart, rows,
                  drop);
  GC_TRY(check_launch("bert_embed_bwd"));
  GC_TRY(res_ln_bwd_reduce(w.lnpart, G, D, dlnw, dlnb, st));
  GC_TRY(embed_bwd(a.B, a.T, word_table(a, dword), w.demb, nullptr, w.embed, w.embed_bytes, st, a.t_valid, 1));
  GC_LAUNCH_TIMED("bert_embed_pos", 4.0 * (rows + a.Pmax) * D, bemb_pos_kernel, dim3(a.Pmax, cdiv(D, 256)), dim3(256), 0, st, w.demb, a.t_valid,
                  dpos, a.B, a.T, D);
  GC_TRY(check_launch("bert_embed_pos"));
  const int TG = type_groups(rows), per = cdiv(rows, TG);
  GC_LAUNCH_TIMED("bert_embed_type", 4.0 * rows * D, bemb_type_kernel, dim3(TG, cdiv(D, 256)), dim3(256), 0, st, w.demb, a.tts, a.t_valid,
                  w.typart, rows, per, a.T, D, a.Ty);
  GC_TRY(check_launch("bert_embed_type"));
  const long cells = (long)a.Ty * D;
  hipLaunchKernelGGL(bemb_type_sum_kernel, dim3(cdiv(cells, 256)), dim3(256), 0, st, w.typart, dtype, TG, cells);
  return check_launch("bert_embed_type_sum");
}

}  // namespace gc

// ---- the C boundary ------------------------------------------------------------------------------------------------------------
using namespace gc;

static bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

static int bemb_shape_ok(const char* who, int B, int T, int D, int V, int Pmax, int Ty) {
  GC_REQUIRE(D >= 64 && D % 64 == 0 && D <= BERT_LN_MAX_D, "%s: D = %d (a multiple of 64, at most %d)", who, D, BERT_LN_MAX_D);
  GC_REQUIRE(B >= 1 && T >= 1 && (long)B * T * D <= 0x7fffffffL, "%s: bad shape B=%d T=%d (B T D < 2^31)", who, B, T);
  GC_REQUIRE(V >= 1 && Ty >= 1 && Pmax >= 1, "%s: bad tables V=%d Pmax=%d Ty=%d", who, V, Pmax, Ty);
  GC_REQUIRE(T <= Pmax, "%s: T = %d exceeds the position table's %d rows", who, T, Pmax);
  return 0;
}
static int bemb_drop_ok(const char* who, const void* snap, float p) {
  GC_REQUIRE(p >= 0.f && p < 1.f, "%s: p=%f out of [0,1)", who, p);
  GC_REQUIRE(!(p > 0.f) || snap, "%s: dropout without an rng snapshot", who);
  return 0;
}
static BertEmbedArgs bemb_args(int B, int T, int D, int V, int Pmax, int Ty, const int64_t* input_ids, const int64_t* token_type_ids,
                               const float* word_w, const float* pos_w, const float* type_w, const float* ln_w, const float* ln_b,
                               const int32_t* t_valid) {
  return BertEmbedArgs{B, T, D, V, Pmax, Ty, input_ids, token_type_ids, word_w, pos_w, type_w, ln_w, ln_b, t_valid};
}

extern "C" int64_t gcbe_ws_bytes(int B, int T, int D, int V, int Pmax, int Ty) {
  if (bemb_shape_ok("gcbe_ws_bytes", B, T, D, V, Pmax, Ty)) return -1;
  return bert_embed_ws_bytes(B, T, D, V, Ty);
}

extern "C" int gcbe_fwd(int B, int T, int D, int V, int Pmax, int Ty, const int64_t* input_ids, const int64_t* token_type_ids,
                        const float* word_w, const float* pos_w, const float* type_w, const float* ln_w, const float* ln_b,
                        const int32_t* t_valid, float* y, float* mean, float* rstd, const void* rng_snap, float p, void* stream) {
  GC_TRY(bemb_shape_ok("gcbe_fwd", B, T, D, V, Pmax, Ty));
  GC_TRY(bemb_drop_ok("gcbe_fwd", rng_snap, p));
  GC_REQUIRE(input_ids && token_type_ids && word_w && pos_w && type_w && ln_w && ln_b && y && mean && rstd, "gcbe_fwd: null pointer");
  return bert_embed_fwd(bemb_args(B, T, D, V, Pmax, Ty, input_ids, token_type_ids, word_w, pos_w, type_w, ln_w, ln_b, t_valid), y, mean, rstd,
                        make_drop(rng_snap, SALT_BERT_EMB, p), (hipStream_t)stream);
}

extern "C" int gcbe_bwd(int B, int T, int D, int V, int Pmax, int Ty, const int64_t* input_ids, const int64_t* token_type_ids,
                        const float* word_w, const float* pos_w, const float* type_w, const float* ln_w, const int32_t* t_valid,
                        const float* mean, const float* rstd, const float* dy, float* dword, float* dpos, float* dtype, float* dln_w,
                        float* dln_b, void* ws, int64_t ws_bytes, const void* rng_snap, float p, void* stream) {
  GC_TRY(bemb_shape_ok("gcbe_bwd", B, T, D, V, Pmax, Ty));
  GC_TRY(bemb_drop_ok("gcbe_bwd", rng_snap, p));
  GC_REQUIRE(input_ids && token_type_ids && word_w && pos_w && type_w && ln_w && mean && rstd && dy && dword && dpos && dtype && dln_w &&
                 dln_b,
             "gcbe_bwd: null pointer");
  GC_REQUIRE(ws && al16(ws) && ws_bytes >= gcbe_ws_bytes(B, T, D, V, Pmax, Ty),
             "gcbe_bwd: a 16-byte aligned workspace of %lld bytes needed (gcbe_ws_bytes)", (long long)gcbe_ws_bytes(B, T, D, V, Pmax, Ty));
  return bert_embed_bwd(bemb_args(B, T, D, V, Pmax, Ty, input_ids, token_type_ids, word_w, pos_w, type_w, ln_w, nullptr, t_valid), mean, rstd,
                        dy, dword, dpos, dtype, dln_w, dln_b, ws, ws_bytes, make_drop(rng_snap, SALT_BERT_EMB, p), (hipStream_t)stream);
}
