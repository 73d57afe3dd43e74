/* The embeddings-stage extension of libgcgcn_hip.so: the stage in front of the BERT encoder layers -- three table gathers, their sum,
 * LayerNorm, dropout and the length select -- as one forward launch, and its backward with owner-computed table gradients
 * (csrc/bert_embed.hip; gcgcn_amd.functional.bert_embeddings).
 *
 * A header and a symbol prefix of its own (gcbe_), as include/gcgcn_optim.h has: include/gcgcn.h is the core ABI, whose recorded
 * symbol table (tests/golden/abi_signatures.json) this extension leaves exactly as it is; its own table is recorded in
 * tests/golden/abi_signatures_bert_embed.json and held by tests/test_bert_embed_cpu.py (declared == recorded == exported).
 * gcgcn_amd/_lib.py binds both.  The calls follow the core's conventions: int status (0 = ok, message from gcgcn_last_error),
 * every device pointer as void* to the binding, the stream last. */
#ifndef GCGCN_BERT_EMBED_H
#define GCGCN_BERT_EMBED_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* input_ids, token_type_ids: int64 [B][T].  word_w [V][D], pos_w [Pmax][D], type_w [Ty][D], ln_w / ln_b [D], all fp32.
 * t_valid: int32 [B] on the device or NULL; row (b, t) is live iff t_valid is NULL or t < t_valid[b] (clamped to [0, T]).
 * D a multiple of 64, at most 1024; 1 <= T <= Pmax; B T D < 2^31.
 *   emb[b][t] = (word_w[input_ids[b][t]] + pos_w[t]) + type_w[token_type_ids[b][t]]          in this association
 *   x = ln_w * (emb - mean) / sqrt(var + 1e-12) + ln_b                                       gcgcn_res_ln_fwd's row arithmetic
 *   y = x, or with p > 0: x * keep / (1 - p), keep from rng_snap with the salt of the embeddings' site (0x42454D31) and the
 *       element's offset in [B][T][D]: the mask gcgcn_dropout draws from the same arguments
 * Padding rows: y, mean and rstd are exactly 0; neither the ids nor (backward) dy are read there, and they add nothing to any
 * gradient.  An id outside its table is never dereferenced (it counts as a row of zeros, and adds to no gradient); callers
 * validate their ids.  emb is not stored: the backward gathers it again.
 * gcbe_bwd: dword [V][D], dpos [Pmax][D], dtype [Ty][D] are written in full (rows nobody refers to, and dpos rows at or past T, get
 * 0), dln_w / dln_b [D].  Every sum has one writer and a fixed order: dword rows in ascending b T + t (the scheme of
 * gcgcn_embed_bwd), dpos rows in ascending b, dtype rows through 64 fixed token groups and then the groups in order, dln_w / dln_b as
 * gcgcn_res_ln_bwd does.  No float atomics, no host read, allocation or synchronisation: capturable, and a captured call follows new
 * ids and lengths in the same buffers.
 * ws: device memory, 16-byte aligned, ws_bytes >= gcbe_ws_bytes(B, T, D, V, Pmax, Ty) (-1: bad arguments). */
int64_t gcbe_ws_bytes(int B, int T, int D, int V, int Pmax, int Ty);
int gcbe_fwd(int B, int T, int D, int V, int Pmax, int Ty, const int64_t* input_ids, const int64_t* token_type_ids, const float* word_w,
             const float* pos_w, const float* type_w, const float* ln_w, const float* ln_b, const int32_t* t_valid, float* y, float* mean,
             float* rstd, const void* rng_snap, float p, void* stream);
int gcbe_bwd(int B, int T, int D, int V, int Pmax, int Ty, const int64_t* input_ids, const int64_t* token_type_ids, const float* word_w,
             const float* pos_w, const float* type_w, const float* ln_w, const int32_t* t_valid, const float* mean, const float* rstd,
             const float* dy, float* dword, float* dpos, float* dtype, float* dln_w, float* dln_b, void* ws, int64_t ws_bytes,
             const void* rng_snap, float p, void* stream);

#ifdef __cplusplus
}
#endif
#endif
