// The token front end of the two models, either side of the BiLSTM (glove:282-298, bert:275-290).  DESIGN.md section 8.8.
//
//   embed_fwd  :  embed_fwd_kernel          x = word_emb[document] | entity_embed[document_pos] | ner_emb[document_ner], times the
//                                           locked-dropout factor scale[b][i]; one wave per token, a plain copy
//   embed_bwd  :  memset of the touched flags
//                 embed_bwd_chunk_kernel    a chunk of 256 consecutive tokens is sorted by (id, position) in LDS; every run of equal
//                                           ids is summed in ascending position in pieces of at most 32 rows -> partial rows
//                 embed_bwd_rows_kernel     one wave per table row: untouched rows are zero-filled; a touched row finds its range in
//                                           every chunk's sorted ids (binary search) and adds the pieces, chunks and pieces ascending
//   context_fwd:  pre = h W^T + b           one product of the GEMM layer (gemm_nt + bias)
//                 context_fwd_kernel        ctx = tanh(pre) elementwise; trailing workgroups pool node_feat = node_pos tanh(pre),
//                                           visiting only the non-zeros of a node_pos row, in ascending t
//   context_bwd:  context_bwd_kernel        dpre = (dctx + node_pos^T dnode_feat) (1 - ctx^2), each token's sum in ascending n
//                 dW = dpre^T h, dh = dpre W, db = column sums of dpre: one gemm_group launch, the column sum riding
//   context_fwd_ld / context_bwd_ld: the same two with the weight (and its gradient) at a leading dimension of its own, and
//                 context_fwd_kernel<true> adding two gathered 128-wide fold rows in front of tanh: the BERT model's folded pair
//                 (bert_frontend.hip), which reads W1 in place inside linear_re's [128][Dw + Dc + Dn] weight
//
// No workgroup reads what another one of the same launch writes (the pooling workgroups recompute tanh(pre) instead of reading
// ctx), no float is added atomically and no order is handed out by an atomic: the only shared writes are the touched flags, every
// writer storing the same 1.  Two runs are bitwise equal.  Nothing reads back to the host: capturable.
#include "frontend.hpp"
#include "gemm.hpp"
#include <limits.h>

namespace gc {

constexpr int FE_CHUNK = 256;   // tokens of a chunk = one workgroup's sort
constexpr int FE_PIECE = 32;    // sorted tokens one wave sums; a run crossing a piece boundary leaves one partial row per piece
constexpr int FE_NONE = INT_MAX;   // the key of a token that adds nothing: past the end, a padding id, an id outside the table

struct EmbedWs {
  int* touched;   // [rows of table 0 | 1 | 2]: the row has a partial row somewhere
  int* sid;       // [3][chunks * 256]: each chunk's keys, ascending
  float* part;    // [chunks * 256][I]: the partial row of the piece ending at sorted index e of chunk k is row k * 256 + e
  long toff[3];
  long nsorted;   // chunks * 256
};

__device__ __forceinline__ int fe_coff(const EmbedTables& tb, int i) { return i == 0 ? 0 : i == 1 ? tb.t[0].width : tb.t[0].width + tb.t[1].width; }

// ---- embeddings, forward ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void embed_fwd_kernel(const EmbedTables tb, const float* __restrict__ scale, float* __restrict__ x,
                                                        const long n, const int T, const int I) {
  const long tok = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (tok >= n) return;
  const float* sc = scale ? scale + (tok / T) * I : nullptr;
  float* xr = x + tok * I;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const EmbedTable& t = tb.t[i];
    const int64_t id = t.ids[tok];
    const bool ok = id >= 0 && id < t.rows;   // ids are validated by the caller; a bad one reads nothing
    const float* src = t.w + (ok ? id : 0) * t.width;
    const int coff = fe_coff(tb, i);
    for (int c = lane; c < t.width; c += 64) {
      float v = ok ? src[c] : 0.f;
      if (sc) v *= sc[coff + c];
      xr[coff + c] = v;
    }
  }
}

int embed_fwd(int B, int T, const EmbedTables& tb, const float* scale, float* x, hipStream_t st) {
  const long n = (long)B * T;
  const int I = tb.width();
  GC_LAUNCH_TIMED("fe_embed_fwd", 8.0 * n * I, embed_fwd_kernel, dim3(cdiv(n, 4)), dim3(256), 0, st, tb, scale, x, n, T, I);
  return check_launch("embed_fwd");
}

// ---- embeddings, backward --------------------------------------------------------------------------------------------------
// grid (chunks, column tiles of 64, tables), 512 threads = 8 waves x 32 sorted tokens.  LEN (t_valid [B]; the BERT embeddings stage):
// a token at or past its document's length adds nothing, and neither its id nor its row of dx is read.
template <bool LEN>
__global__ __launch_bounds__(512) void embed_bwd_chunk_kernel(const EmbedTables tb, const EmbedWs ws, const float* __restrict__ dx,
                                                              const float* __restrict__ scale, const long n, const int T, const int I,
                                                              const int* __restrict__ t_valid) {
  __shared__ __attribute__((aligned(16))) int s_id[FE_CHUNK];
  __shared__ int s_sid[FE_CHUNK], s_pos[FE_CHUNK], s_b[FE_CHUNK];
  const int ti = blockIdx.z, ct = blockIdx.y, t = threadIdx.x;
  const EmbedTable& tab = tb.t[ti];
  if (ct * 64 >= tab.width) return;
  const long k = blockIdx.x;

  int id = FE_NONE;
  if (t < FE_CHUNK) {
    const long pos = k * FE_CHUNK + t;
    if (pos < n && (!LEN || (int)(pos % T) < min(max(t_valid[pos / T], 0), T))) {
      const int64_t v = tab.ids[pos];
      if (v >= 0 && v < tab.rows && v != tab.pad) id = (int)v;
    }
    s_id[t] = id;
  }
  __syncthreads();
  if (t < FE_CHUNK) {
    int rank = 0;   // keys (id, t) below this token's
    for (int j = 0; j < FE_CHUNK; j += 4) {
      const int4 q = *reinterpret_cast<const int4*>(s_id + j);
      rank += (q.x < id || (q.x == id && j < t)) + (q.y < id || (q.y == id && j + 1 < t)) + (q.z < id || (q.z == id && j + 2 < t)) +
              (q.w < id || (q.w == id && j + 3 < t));
    }
    const long pos = k * FE_CHUNK + t;
    s_sid[rank] = id, s_pos[rank] = t, s_b[rank] = (int)(pos / T);
    if (ct == 0) {
      ws.sid[ti * ws.nsorted + k * FE_CHUNK + rank] = id;
      if (id != FE_NONE) __hip_atomic_store(ws.touched + ws.toff[ti] + id, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();

  const int w = t >> 6, lane = t & 63, col = ct * 64 + lane, e0 = w * FE_PIECE;
  const bool colok = col < tab.width;
  const int coff = fe_coff(tb, ti) + col;
  float v[FE_PIECE];
#pragma unroll
  for (int i = 0; i < FE_PIECE; ++i) {
    const int e = e0 + i;
    const bool ok = colok && s_sid[e] != FE_NONE;
    v[i] = ok ? dx[(k * FE_CHUNK + s_pos[e]) * I + coff] : 0.f;
    if (ok && scale) v[i] *= scale[(long)s_b[e] * I + coff];
  }
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < FE_PIECE; ++i) {
    const int e = e0 + i, key = s_sid[e];
    acc += v[i];
    if (i == FE_PIECE - 1 || s_sid[e + 1] != key) {   // the run, or this wave's piece of it, ends here
      if (colok && key != FE_NONE) ws.part[(k * FE_CHUNK + e) * I + coff] = acc;
      acc = 0.f;
    }
  }
}

// grid (rows / 4, 1, tables): one wave per table row
__global__ __launch_bounds__(256) void embed_bwd_rows_kernel(const EmbedTables tb, const EmbedWs ws, const int chunks, const int I) {
  const int ti = blockIdx.z, lane = threadIdx.x & 63;
  const EmbedTable& tab = tb.t[ti];
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= tab.rows) return;
  float* out = tab.dw + row * tab.width;
  if (!ws.touched[ws.toff[ti] + row]) {
    for (int c = lane; c < tab.width; c += 64) out[c] = 0.f;
    return;
  }
  const int* sid = ws.sid + ti * ws.nsorted;
  const int coff = fe_coff(tb, ti), key = (int)row;
  for (int cg = 0; cg < tab.width; cg += 256) {   // four column tiles of 64 per sweep over the chunks
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < chunks; c0 += 64) {
      int lo = 0, hi = 0;   // [lo, hi): where chunk c0 + lane holds this row's id
      if (c0 + lane < chunks) {
        const int* s = sid + (long)(c0 + lane) * FE_CHUNK;
        int a = 0, b = FE_CHUNK;
        while (a < b) {
          const int m = (a + b) >> 1;
          if (s[m] < key) a = m + 1; else b = m;
        }
        lo = a, b = FE_CHUNK;
        while (a < b) {
          const int m = (a + b) >> 1;
          if (s[m] <= key) a = m + 1; else b = m;
        }
        hi = a;
      }
      unsigned long long mask = __ballot(hi > lo);
      while (mask) {
        const int j = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        const int clo = __shfl(lo, j), chi = __shfl(hi, j);
        const float* p = ws.part + (long)(c0 + j) * FE_CHUNK * I + coff + cg + lane;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (cg + 64 * q + lane >= tab.width) continue;
          for (int e = clo | (FE_PIECE - 1); e < chi - 1; e += FE_PIECE) acc[q] += p[(long)e * I + 64 * q];   // pieces that end at a wave's edge
          acc[q] += p[(long)(chi - 1) * I + 64 * q];                                                           // the piece that ends the run
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (cg + 64 * q + lane < tab.width) out[cg + 64 * q + lane] = acc[q];
  }
}

static long up4(long v) { return (v + 3) & ~3L; }
static EmbedWs embed_ws(long n, const EmbedTables& tb, void* base) {
  EmbedWs w;
  const long chunks = (n + FE_CHUNK - 1) / FE_CHUNK;
  w.nsorted = chunks * FE_CHUNK;
  w.toff[0] = 0, w.toff[1] = tb.t[0].rows, w.toff[2] = (long)tb.t[0].rows + tb.t[1].rows;
  const long nt = up4(w.toff[2] + tb.t[2].rows);
  w.touched = (int*)base;
  w.sid = w.touched + nt;
  w.part = (float*)(w.sid + 3 * w.nsorted);
  return w;
}
long embed_ws_bytes(long n, const EmbedTables& tb) {
  const long nsorted = (n + FE_CHUNK - 1) / FE_CHUNK * FE_CHUNK;
  const long ints = up4((long)tb.t[0].rows + tb.t[1].rows + tb.t[2].rows) + 3 * nsorted;
  return 4 * (ints + nsorted * tb.width());
}

int embed_bwd(int B, int T, const EmbedTables& tb, const float* dx, const float* scale, void* wsp, long ws_bytes, hipStream_t st,
              const int* t_valid, int ntab) {
  const long n = (long)B * T;
  const int I = tb.width();
  GC_REQUIRE(ws_bytes >= embed_ws_bytes(n, tb), "embed_bwd: workspace of %ld bytes needed", embed_ws_bytes(n, tb));
  const EmbedWs ws = embed_ws(n, tb, wsp);
  const int chunks = (int)(ws.nsorted / FE_CHUNK);
  int wmax = 1, rmax = 1;
  for (int i = 0; i < ntab; ++i) wmax = tb.t[i].width > wmax ? tb.t[i].width : wmax, rmax = tb.t[i].rows > rmax ? tb.t[i].rows : rmax;
  {
    ProfScope ps("fe_embed_flags", st);
    GC_REQUIRE(hipMemsetAsync(ws.touched, 0, (char*)ws.sid - (char*)ws.touched, st) == hipSuccess, "embed_bwd: memset failed");
  }
  const auto chunk_kernel = t_valid ? embed_bwd_chunk_kernel<true> : embed_bwd_chunk_kernel<false>;
  GC_LAUNCH_TIMED("fe_embed_chunk", 8.0 * n * I, chunk_kernel, dim3(chunks, cdiv(wmax, 64), ntab), dim3(512), 0, st, tb, ws, dx, scale, n, T,
                  I, t_valid);
  GC_TRY(check_launch("embed_bwd_chunk"));
  double bytes = 0;
  for (int i = 0; i < ntab; ++i) bytes += 4.0 * tb.t[i].rows * tb.t[i].width;
  GC_LAUNCH_TIMED("fe_embed_rows", bytes + 4.0 * n * I, embed_bwd_rows_kernel, dim3(cdiv(rmax, 4), 1, ntab), dim3(256), 0, st, tb, ws, chunks, I);
  return check_launch("embed_bwd_rows");
}

// ---- linear_re + tanh + entity pooling ---------------------------------------------------------------------------------------
// the first `ew` workgroups: ctx = tanh(pre), four floats a thread; the others: one wave per entity row of node_pos.
// FOLD (the BERT model's folded pair, bert_frontend.hip): both read pre[b, t] + f2[pos_ids[b, t]] + f3[ner_ids[b, t]] in place of pre.
__device__ __forceinline__ const float* fold_row(const int64_t* __restrict__ ids, const float* __restrict__ f, const int rows, const long tok,
                                                 bool& ok) {
  const int64_t id = ids[tok];
  ok = id >= 0 && id < rows;
  return f + (ok ? id : 0) * FE_HD;
}
template <bool FOLD>
__global__ __launch_bounds__(256) void context_fwd_kernel(const float* __restrict__ pre, const float* __restrict__ node_pos,
                                                          float* __restrict__ ctx, float* __restrict__ node_feat, const int ew, const long BT,
                                                          const int T, const int N, const long BN, const ContextFold fo) {
  if ((int)blockIdx.x < ew) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= BT * (FE_HD / 4)) return;
    float4 v = reinterpret_cast<const float4*>(pre)[i];
    if constexpr (FOLD) {
      const int c4 = (int)(i & (FE_HD / 4 - 1));
      bool ok2, ok3;
      const float* r2 = fold_row(fo.pos_ids, fo.f2, fo.P, i / (FE_HD / 4), ok2);
      const float* r3 = fold_row(fo.ner_ids, fo.f3, fo.R, i / (FE_HD / 4), ok3);
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 a = ok2 ? reinterpret_cast<const float4*>(r2)[c4] : zero, b = ok3 ? reinterpret_cast<const float4*>(r3)[c4] : zero;
      v.x = (v.x + a.x) + b.x, v.y = (v.y + a.y) + b.y, v.z = (v.z + a.z) + b.z, v.w = (v.w + a.w) + b.w;
    }
    v.x = tanhf(v.x), v.y = tanhf(v.y), v.z = tanhf(v.z), v.w = tanhf(v.w);
    reinterpret_cast<float4*>(ctx)[i] = v;
    return;
  }
  const long pid = (long)(blockIdx.x - ew) * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (pid >= BN) return;
  const float* np = node_pos + pid * T;
  const float* rows = pre + (pid / N) * T * FE_HD;
  float a0 = 0.f, a1 = 0.f;
  for (int t0 = 0; t0 < T; t0 += 64) {
    const float wt = t0 + lane < T ? np[t0 + lane] : 0.f;
    unsigned long long mask = __ballot(wt != 0.f);
    while (mask) {
      const int j = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const float wj = __shfl(wt, j);
      const float* r = rows + (long)(t0 + j) * FE_HD;
      float p0 = r[lane], p1 = r[64 + lane];
      if constexpr (FOLD) {
        bool ok2, ok3;
        const long tok = (pid / N) * T + t0 + j;
        const float* r2 = fold_row(fo.pos_ids, fo.f2, fo.P, tok, ok2);
        const float* r3 = fold_row(fo.ner_ids, fo.f3, fo.R, tok, ok3);
        p0 = (p0 + (ok2 ? r2[lane] : 0.f)) + (ok3 ? r3[lane] : 0.f);
        p1 = (p1 + (ok2 ? r2[64 + lane] : 0.f)) + (ok3 ? r3[64 + lane] : 0.f);
      }
      a0 += wj * tanhf(p0), a1 += wj * tanhf(p1);
    }
  }
  node_feat[pid * FE_HD + lane] = a0, node_feat[pid * FE_HD + 64 + lane] = a1;
}

int context_fwd_ld(int B, int T, int N, int K, const float* h, const float* w, long ldw, const float* bias, const float* node_pos, float* pre,
                   float* ctx, float* node_feat, hipStream_t st, const ContextFold* fold) {
  const long BT = (long)B * T, BN = (long)B * N;
  GemmArgs g = gemm_nt(h, K, w, ldw, pre, FE_HD, (int)BT, FE_HD, K).tagged("fe_gemm");
  g.bias = bias;
  GC_TRY(gemm(g, st, 0, 1));
  const int ew = cdiv(BT * (FE_HD / 4), 256);
  const ContextFold fo = fold ? *fold : ContextFold{nullptr, nullptr, nullptr, nullptr, 0, 0};
  GC_LAUNCH_TIMED("fe_ctx_fwd", 8.0 * BT * FE_HD + 4.0 * BN * T, (fold ? context_fwd_kernel<true> : context_fwd_kernel<false>),
                  dim3(ew + cdiv(BN, 4)), dim3(256), 0, st, pre, node_pos, ctx, node_feat, ew, BT, T, N, BN, fo);
  return check_launch("context_fwd");
}
int context_fwd(int B, int T, int N, int K, const float* h, const float* w, const float* bias, const float* node_pos, float* pre,
                float* ctx, float* node_feat, hipStream_t st) {
  return context_fwd_ld(B, T, N, K, h, w, K, bias, node_pos, pre, ctx, node_feat, st);
}

// grid (tiles of 64 tokens, B), 256 threads: thread (half, col) owns the sums of the tile's tokens j with j % 2 == half at column col
__global__ __launch_bounds__(256) void context_bwd_kernel(const float* __restrict__ node_pos, const float* __restrict__ ctx,
                                                          const float* __restrict__ dctx, const float* __restrict__ dnode,
                                                          float* __restrict__ dpre, const int T, const int N) {
  __shared__ float acc[64 * FE_HD];
  const int t0 = blockIdx.x * 64, b = blockIdx.y;
  const int col = threadIdx.x & (FE_HD - 1), half = threadIdx.x >> 7, lane = threadIdx.x & 63;
  for (int j = half; j < 64; j += 2) acc[j * FE_HD + col] = 0.f;   // a thread reads and writes its own cells only: no barrier
  for (int nn = 0; nn < N; ++nn) {
    const long en = (long)b * N + nn;
    const float wt = t0 + lane < T ? node_pos[en * T + t0 + lane] : 0.f;
    unsigned long long mask = __ballot(wt != 0.f);   // the same in all four waves
    if (!mask) continue;
    const float dn = dnode[en * FE_HD + col];
    while (mask) {
      const int j = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const float wj = __shfl(wt, j);
      if ((j & 1) == half) acc[j * FE_HD + col] += wj * dn;
    }
  }
  for (int j = half; j < 64 && t0 + j < T; j += 2) {
    const long i = ((long)b * T + t0 + j) * FE_HD + col;
    const float c = ctx[i];
    dpre[i] = (dctx[i] + acc[j * FE_HD + col]) * (1.f - c * c);
  }
}

static long context_col_elems() { return (long)COL_RIDE_SLICES * FE_HD; }
long context_ws_elems(int K) { return gemm_ws_elems(FE_HD, K) + context_col_elems(); }

int context_bwd_ld(int B, int T, int N, int K, const float* h, const float* w, long ldw, const float* node_pos, const float* ctx,
                   const float* dctx, const float* dnode, float* dpre, float* dh, float* dw, float* db, float* ws, long ws_elems,
                   hipStream_t st) {
  const long BT = (long)B * T;
  GC_REQUIRE(ws_elems >= context_ws_elems(K), "context_bwd: workspace of %ld floats needed", context_ws_elems(K));
  const long split_elems = gemm_ws_elems(FE_HD, K);
  float* part = ws + split_elems;
  GC_LAUNCH_TIMED("fe_ctx_bwd", 16.0 * BT * FE_HD + 4.0 * B * N * T, context_bwd_kernel, dim3(cdiv(T, 64), B), dim3(256), 0, st, node_pos, ctx,
                  dctx, dnode, dpre, T, N);
  GC_TRY(check_launch("context_bwd"));
  GemmArgs gs[2] = {
      gemm_tn(dpre, FE_HD, h, K, dw, ldw, FE_HD, K, (int)BT).split_ws(ws, split_elems).tagged("fe_gemm"),
      gemm_nn(dpre, FE_HD, w, ldw, dh, K, (int)BT, K, FE_HD).split_ws(ws, split_elems).tagged("fe_gemm"),
  };
  const ColRide cr = col_sum(dpre, BT, FE_HD, FE_HD, db, part);
  return gemm_group(gs, 2, st, &cr);
}
int context_bwd(int B, int T, int N, int K, const float* h, const float* w, const float* node_pos, const float* ctx, const float* dctx,
                const float* dnode, float* dpre, float* dh, float* dw, float* db, float* ws, long ws_elems, hipStream_t st) {
  return context_bwd_ld(B, T, N, K, h, w, K, node_pos, ctx, dctx, dnode, dpre, dh, dw, db, ws, ws_elems, st);
}

}  // namespace gc
