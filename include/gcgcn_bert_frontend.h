/* The BERT graph model's extension of libgcgcn_hip.so: what GraphCNN_multihead_bert_gate_cls computes either side of the shared tail
 * beside its encoder -- the folded context pair in front (linear_re over cat(states, entity_embed, ner_emb), tanh, entity pooling,
 * without the concatenated tensor) and the [CLS] logit tail behind (csrc/bert_frontend.hip; gcgcn_amd.functional.bert_token_context
 * and pair_logit_bias).
 *
 * A header and a symbol prefix of its own (gcbf_), as include/gcgcn_bert_embed.h has: include/gcgcn.h is the core ABI, whose recorded
 * symbol table (tests/golden/abi_signatures.json) this extension leaves exactly as it is; its own table is recorded in
 * tests/golden/abi_signatures_bert_frontend.json and held by tests/test_bert_frontend_cpu.py (declared == recorded == exported).
 * gcgcn_amd/_lib.py binds both.  The calls follow the core's conventions: int status (0 = ok, message from gcgcn_last_error),
 * every device pointer as void* to the binding, the stream last. */
#ifndef GCGCN_BERT_FRONTEND_H
#define GCGCN_BERT_FRONTEND_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The folded context pair.  states [B][T][Dw]; document_pos, document_ner int64 [B][T]; coref_w [P][Dc]; ner_w [R][Dn];
 * weight [128][Dw + Dc + Dn] = W1 | W2 | W3 by columns, read in place; bias [128]; node_pos [B][N][T].  All fp32.
 *   F2 [P][128] = coref_w W2^T,  F3 [R][128] = ner_w W3^T                                         (fold: (P + R) * 128 floats, scratch)
 *   pre [B][T][128] = states W1^T + bias                                                          (scratch the caller owns)
 *   ctx [B][T][128] = tanh((pre + F2[document_pos]) + F3[document_ner]),  node_feat [B][N][128] = node_pos ctx
 * which is tanh(linear(cat(states, coref_w[document_pos], ner_w[document_ner]))) and its pooling without the concatenated tensor.
 * An id outside its table is never dereferenced (it adds nothing); callers validate their ids.
 * gcbf_context_bwd: dctx [B][T][128], dnode_feat [B][N][128] -> dstates [B][T][Dw], dweight [128][Dw + Dc + Dn], dbias [128],
 * dcoref [P][Dc], dner [R][Dn], all written in full.  dF2 / dF3 (the per-id sums of dpre's rows, the scheme of gcgcn_embed_bwd:
 * each row by one owner in ascending b T + t) count every token, the padding ids included, so dweight sees them as torch's does;
 * rows coref_padding_idx of dcoref and ner_padding_idx of dner (-1: none) are then written as exact zeros.  No float atomics, no
 * host read, allocation or synchronisation: bit-reproducible and capturable.
 * ws: device memory, 16-byte aligned, ws_bytes >= gcbf_context_ws_bytes(...) (-1: bad arguments). */
int64_t gcbf_context_ws_bytes(int B, int T, int N, int Dw, int Dc, int Dn, int P, int R);
int gcbf_context_fwd(int B, int T, int N, int Dw, int Dc, int Dn, int P, int R, const float* states, const int64_t* document_pos,
                     const int64_t* document_ner, const float* coref_w, const float* ner_w, const float* weight, const float* bias,
                     const float* node_pos, float* fold, float* pre, float* ctx, float* node_feat, void* stream);
int gcbf_context_bwd(int B, int T, int N, int Dw, int Dc, int Dn, int P, int R, const float* states, const int64_t* document_pos,
                     const int64_t* document_ner, const float* coref_w, const float* ner_w, const float* weight, const float* node_pos,
                     const float* ctx, const float* dctx, const float* dnode_feat, int coref_padding_idx, int ner_padding_idx,
                     float* dstates, float* dweight, float* dbias, float* dcoref, float* dner, void* ws, int64_t ws_bytes, void* stream);

/* The [CLS] logit tail.  logits, out [B][N][N][R]; cls [B][R]; n_valid int32 [B] on the device or NULL (every entity exists).
 *   out[b][i][j][:] = logits[b][i][j][:] + cls[b][:]  where i, j < n_valid[b] (clamped to [0, N]), logits[b][i][j][:] elsewhere
 * in one launch; out may be logits.  B N N R < 2^31.
 * gcbf_logit_bias_bwd: dcls [B][R] = the sum of dout over the pairs i, j < n_valid[b], in two stages with one writer each and a
 * fixed order (j ascending in two interleaved halves per row i, then i ascending): bit-reproducible, no atomics.  The gradient of
 * logits is dout itself.  ws: gcbf_logit_bias_ws_bytes(B, N, R) bytes (-1: bad arguments), 16-byte aligned. */
int64_t gcbf_logit_bias_ws_bytes(int B, int N, int R);
int gcbf_logit_bias_fwd(int B, int N, int R, const float* logits, const float* cls, const int32_t* n_valid, float* out, void* stream);
int gcbf_logit_bias_bwd(int B, int N, int R, const float* dout, const int32_t* n_valid, float* dcls, void* ws, int64_t ws_bytes,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif
