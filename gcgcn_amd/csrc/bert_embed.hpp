// The embeddings stage in front of the BERT encoder layers (bert_embed.hip): gathers, sum, LayerNorm, dropout, length select, and the
// backward with owner-computed table gradients.  include/gcgcn_bert_embed.h states the contract.  Internal header.  DESIGN.md section 8.9.
#pragma once
#include "bert.hpp"

namespace gc {

constexpr uint64_t SALT_BERT_EMB = 0x42454d31ull;   // the dropout after the embeddings' LayerNorm, index = offset in [B T][D]
constexpr int BEMB_TYPE_GROUPS = 64;                // token groups of the type table's first stage, at least 32 tokens each

struct BertEmbedArgs {
  int B, T, D, V, Pmax, Ty;
  const int64_t *ids, *tts;
  const float *word, *pos, *type, *lnw, *lnb;
  const int* t_valid;   // or nullptr
};

int bert_embed_fwd(const BertEmbedArgs& a, float* y, float* mean, float* rstd, Drop drop, hipStream_t st);
long bert_embed_ws_bytes(int B, int T, int D, int V, int Ty);
int bert_embed_bwd(const BertEmbedArgs& a, const float* mean, const float* rstd, const float* dy, float* dword, float* dpos, float* dtype,
                   float* dlnw, float* dlnb, void* ws, long ws_bytes, Drop drop, hipStream_t st);

}  // namespace gc
