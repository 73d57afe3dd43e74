/* The record route of the edge-feature producer: gcgcn_producer_fwd / _bwd / _bwd_det of include/gcgcn.h with the three dense
 * [B][N][N][S][T] byte tensors (sen, pos_h, pos_t) replaced by the packed slot records they are tensorised from
 * (csrc/producer_rec.hip; gcgcn_amd.functional.edge_features(slot_records=...)).
 *
 * A header and a symbol prefix of its own (gcpr_), as include/gcgcn_optim.h and include/gcgcn_bert_embed.h have: include/gcgcn.h is
 * the core ABI, whose recorded symbol table (tests/golden/abi_signatures.json) and version this extension leave exactly as they are;
 * its own table is recorded in tests/golden/abi_signatures_producer_rec.json and held by tests/test_producer_rec_cpu.py (declared ==
 * recorded == exported).  gcgcn_amd/_lib.py binds both.  The calls follow the core's conventions: int status (0 = ok, message from
 * gcgcn_last_error), every device pointer as void* to the binding, the stream last. */
#ifndef GCGCN_PRODUCER_REC_H
#define GCGCN_PRODUCER_REC_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* records: int32 [n_records][10] on the device (NULL only with n_records == 0), one row per (edge, sentence slot) as
 * gcgcn_amd.data.collate uploads them and gcgcn_tensorise reads them:  doc, u, v, j, s0, s1, h0, h1, t0, t1.
 * Contract: the call computes exactly -- bit for bit -- what the dense entry computes on the tensors gcgcn_tensorise writes from the
 * same records with the same (B, N, S, T, dis_plus):
 *   - a record with u >= N, v >= N or j >= S is dropped (so is one with a negative index or a doc outside [0, B));
 *   - its token range is [max(s0, 0), min(s1, T)); an empty range is dropped;
 *   - a slot is live iff token 0 lies in its range (the reference's padding test, glove:305); other slots contribute nothing;
 *   - token t of a live slot is unmasked iff it lies in the range; its distance ids are pos_id(t, h0, h1, dis_plus) and
 *     pos_id(t, t0, t1, dis_plus) truncated to a byte and clamped to [0, ND - 1];
 *   - entities at or past n_valid[b] are padding, as in the dense entries.
 * (doc, u, v, j) must be UNIQUE in a table (gcgcn_amd.data.pack_document guarantees it): each live record owns one compact row.
 * The order of the records does not matter: compact rows and pairs are numbered by ascending slot index ((b N + u) N + v) S + j,
 * as the dense entries number them (bits scattered with integer atomic OR, the dense entries' scan, then each live record stores its
 * index at its row).  Everything else -- arguments, buffers, capacities, the live-count words {live slots, live pairs, over
 * capacity, 0} and the NaN poisoning when the capacities are too small, E == NULL for compact rows, dE / dEc, the deterministic
 * backward's detbuf -- is what include/gcgcn.h says of the dense entries.  ibuf / fbuf / bbuf are sized by gcgcn_producer_sizes
 * (whose int32 count includes the row -> record map), detbuf by gcgcn_producer_det_elems.  The backward entries take the records
 * and the buffers of the forward call they follow.
 * No host read, stream synchronisation or float atomic beyond the dense entries' own; capturable.
 * Refused before any launch: a null pointer, a negative count or capacity, T > 2048, S outside 1..31, a negative scratch_elems,
 * det_elems smaller than gcgcn_producer_det_elems. */
int gcpr_producer_fwd(int B, int N, int S, int T, int Hd, int P, int ND, const float* ctx, int n_records, const int32_t* records,
                      int dis_plus, const float* node, const float* dis_table, const int32_t* n_valid, const float* flat,
                      int64_t cap_rows, int64_t cap_pairs, int32_t* ibuf, float* fbuf, float* scratch, int64_t scratch_elems, float* E,
                      void* stream);
int gcpr_producer_bwd(int B, int N, int S, int T, int Hd, int P, int ND, const float* ctx, int n_records, const int32_t* records,
                      int dis_plus, const float* node, const float* dis_table, const int32_t* n_valid, const float* flat,
                      int64_t cap_rows, int64_t cap_pairs, int32_t* ibuf, float* fbuf, float* bbuf, const float* dE, const float* dEc,
                      float* dctx, float* dnode, float* ddis_table, float* dflat, void* stream);
int gcpr_producer_bwd_det(int B, int N, int S, int T, int Hd, int P, int ND, const float* ctx, int n_records, const int32_t* records,
                          int dis_plus, const float* node, const float* dis_table, const int32_t* n_valid, const float* flat,
                          int64_t cap_rows, int64_t cap_pairs, int32_t* ibuf, float* fbuf, float* bbuf, const float* dE,
                          const float* dEc, float* dctx, float* dnode, float* ddis_table, float* dflat, float* detbuf, int64_t det_elems,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif
