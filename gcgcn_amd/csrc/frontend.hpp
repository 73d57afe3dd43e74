// The token front end either side of the BiLSTM (frontend.hip): the three embedding gathers with the locked-dropout factor, and
// linear_re + tanh + entity pooling.  DESIGN.md section 8.8.  Internal header.
#pragma once
#include "common.hpp"

namespace gc {

constexpr int FE_HD = 128;   // the width of the token states the context pair serves (both reference models hard-code it)

// The three tables in the column order of x: word_emb[document] | entity_embed[document_pos] | ner_emb[document_ner].
// ids int64 [B * T]; w / dw [rows][width]; pad: the row whose gradient stays zero, -1 for none.
struct EmbedTable {
  const int64_t* ids;
  const float* w;   // forward
  float* dw;        // backward
  int rows, width, pad;
};
struct EmbedTables {
  EmbedTable t[3];
  int width() const { return t[0].width + t[1].width + t[2].width; }
};

// x [B * T][I] = the gathered rows side by side, times scale [B][I] where given (one factor per batch entry and feature).
int embed_fwd(int B, int T, const EmbedTables& tb, const float* scale, float* x, hipStream_t st);

// Bytes of workspace embed_bwd needs (touched flags per table row, the chunks' sorted ids, the chunks' partial rows).
long embed_ws_bytes(long n, const EmbedTables& tb);
// dw of every table, fully written, from dx [B * T][I] (times scale): each row summed by one owner in ascending token position.
// t_valid (int32 [B] on the device, or nullptr): token (b, t) with t >= t_valid[b] adds nothing; its ids and its row of dx are not read.
// ntab: the leading tables the launches visit (the BERT embeddings stage hands over its word table alone, the others with no rows).
int embed_bwd(int B, int T, const EmbedTables& tb, const float* dx, const float* scale, void* ws, long ws_bytes, hipStream_t st,
              const int* t_valid = nullptr, int ntab = 3);

// pre [B * T][128] = h W^T + b (scratch the caller owns), ctx = tanh(pre), node_feat [B][N][128] = node_pos [B][N][T] ctx.
int context_fwd(int B, int T, int N, int K, const float* h, const float* w, const float* bias, const float* node_pos, float* pre,
                float* ctx, float* node_feat, hipStream_t st);

// The folded pair of the BERT model (bert_frontend.hip): the projection runs on the encoder states alone, and the two small tables
// arrive folded through it, f2 [P][128] and f3 [R][128]: pre[b, t] + f2[pos_ids[b, t]] + f3[ner_ids[b, t]], in this association, is
// what tanh sees.  An id outside its table adds nothing (callers validate their ids).
struct ContextFold {
  const int64_t* pos_ids;   // [B * T]
  const int64_t* ner_ids;
  const float* f2;
  const float* f3;
  int P, R;
};
// context_fwd with the weight read in place at leading dimension ldw >= K (its first K columns), and the fold rows where given
int context_fwd_ld(int B, int T, int N, int K, const float* h, const float* w, long ldw, const float* bias, const float* node_pos, float* pre,
                   float* ctx, float* node_feat, hipStream_t st, const ContextFold* fold = nullptr);

long context_ws_elems(int K);
// dpre [B * T][128] = (dctx + node_pos^T dnode_feat) (1 - ctx^2) (scratch the caller owns); dw = dpre^T h, dh = dpre W, db = column sums.
int context_bwd(int B, int T, int N, int K, const float* h, const float* w, const float* node_pos, const float* ctx, const float* dctx,
                const float* dnode, float* dpre, float* dh, float* dw, float* db, float* ws, long ws_elems, hipStream_t st);
// ... with w and dw at leading dimension ldw >= K: the first K columns of a wider weight are read, and of its gradient written
int context_bwd_ld(int B, int T, int N, int K, const float* h, const float* w, long ldw, const float* node_pos, const float* ctx,
                   const float* dctx, const float* dnode, float* dpre, float* dh, float* dw, float* db, float* ws, long ws_elems,
                   hipStream_t st);

}  // namespace gc
