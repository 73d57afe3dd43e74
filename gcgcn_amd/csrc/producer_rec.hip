// The edge-feature producer on the packed slot records (include/gcgcn_producer_rec.h): the route of csrc/producer.hip without the
// three dense [B,N,N,S,T] byte tensors.  data.collate uploads one int32 row per (edge, sentence slot) -- doc, u, v, j, s0, s1, h0, h1,
// t0, t1 -- and gcgcn_tensorise expands them into sen / pos_h / pos_t (3 x 144 MB at B = 32, N = 42, S = 5, T = 512, zero-filled and
// scattered every step), from which producer.hip then recovers what the record states outright: which slots hold token 0, each live
// slot's token range, and position ids that are a closed form of (t, mention bounds).  Here the record table is the input.
//
//   index      prod_rec_bits     one thread per record: a live record ORs bit j into pair_bits[(b N + u) N + v] (integer atomic:
//                                exact and order-free; pair_bits is zeroed by a memset node first)
//              prod_rec_index_a  the dense route's pass A (producer_slots.hpp) reading those bits instead of S mask bytes per pair;
//                                padding entities are masked here, as there
//              prod_index_b      the dense route's pass B, unchanged: rows, pairs, counts, the over-capacity flag
//              prod_rec_rows     one thread per record: a live record of a real pair stores its index at
//                                row_rec[pair_row0 + popc(bits & ((1 << j) - 1))] -- the row the dense route gives its slot
//   word fwd / bwd rows / bwd tok   the dense route's bodies (producer_slots.hpp) on RecSlots: the row's record is fetched once,
//                                its range and mention bounds sit in registers, only [r0, r1) is visited
// Everything else (score table, GEMMs, sentence attention, expand / poison, the table backward, both backward variants) is
// prod_fwd / prod_bwd of producer.hip itself, which branch on ProdSrc::rec at those three places.  Compact rows are numbered alike
// and every row runs the same arithmetic in the same order, so the two routes agree bit for bit.
//
// (doc, u, v, j) is unique in a table: each compact row then has exactly one writer in prod_rec_rows.  No workgroup reads what another
// workgroup of its launch writes; no host read, synchronisation or float atomic is added.
#include "gemm.hpp"
#include "rowops.hpp"
#include "producer_slots.hpp"

namespace gc {

__global__ __launch_bounds__(256) void prod_rec_bits_kernel(const int* __restrict__ records, int n_records, int* __restrict__ pair_bits,
                                                            int B, int N, int S, int T) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_records) return;
  const int* rec = records + (long)i * REC_W;
  const RecSlot q = rec_slot(rec, B, N, S, T);
  if (q.live) atomicOr(pair_bits + q.pair, 1 << rec[3]);
}

__global__ __launch_bounds__(256) void prod_rec_index_a_kernel(const int* __restrict__ n_valid, ProdIdx ix, int N) {
  prod_index_a_body([&](long pp) { return ix.pair_bits[pp]; }, n_valid, ix, N);
}

// after pass B: pair_bits holds the live slots of real pairs only (all zero when the capacities are too small), pair_row0 the
// pair's first global row
__global__ __launch_bounds__(256) void prod_rec_rows_kernel(const int* __restrict__ records, int n_records, ProdIdx ix,
                                                            int* __restrict__ row_rec, int B, int N, int S, int T) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_records) return;
  const int* rec = records + (long)i * REC_W;
  const RecSlot q = rec_slot(rec, B, N, S, T);
  if (!q.live) return;
  const int j = rec[3], bits = ix.pair_bits[q.pair];
  if (bits >> j & 1) row_rec[ix.pair_row0[q.pair] + __popc(bits & ((1 << j) - 1))] = i;
}

template <int HC>
__global__ __launch_bounds__(64 * PW) void prod_rec_word_fwd_kernel(const float* __restrict__ ctx, const int* __restrict__ records,
                                                                    const int* __restrict__ row_rec, int dis_plus,
                                                                    const float* __restrict__ table, ProdIdx ix, float* __restrict__ CW,
                                                                    float* __restrict__ stats, int N, int S, int T, int Hd, int ND) {
  extern __shared__ float wsm[];
  prod_word_fwd_body<HC>(RecSlots{records, row_rec, dis_plus}, wsm, ctx, table, ix, CW, stats, N, S, T, Hd, ND);
}

template <int HC>
__global__ __launch_bounds__(64 * PW) void prod_rec_word_bwd_rows_kernel(const float* __restrict__ ctx, const int* __restrict__ records,
                                                                         const int* __restrict__ row_rec, int dis_plus,
                                                                         const float* __restrict__ table, const float* __restrict__ stats,
                                                                         const float* __restrict__ dCW, ProdIdx ix, float* __restrict__ dots,
                                                                         int N, int S, int T, int Hd, int ND) {
  extern __shared__ float wsm[];
  prod_word_bwd_rows_body<HC>(RecSlots{records, row_rec, dis_plus}, wsm, ctx, table, stats, dCW, ix, dots, N, S, T, Hd, ND);
}

// one workgroup per (document, token): "does this live row cover t" is t against the row's row_rng, nothing else
template <int HC>
__global__ __launch_bounds__(64 * PW) void prod_rec_word_bwd_tok_kernel(const float* __restrict__ ctx, const int* __restrict__ records,
                                                                        const int* __restrict__ row_rec, int dis_plus,
                                                                        const float* __restrict__ table, const float* __restrict__ stats,
                                                                        const float* __restrict__ dCW, const float* __restrict__ dots,
                                                                        ProdIdx ix, float* __restrict__ dtable, float* __restrict__ dctx,
                                                                        int T, int Hd, int ND) {
  extern __shared__ float sm[];
  prod_word_bwd_tok_body<HC>(RecSlots{records, row_rec, dis_plus}, sm, ctx, table, stats, dCW, dots, ix, dtable, dctx, T, Hd, ND);
}

int prod_rec_index(const ProdSrc& src, const int* n_valid, ProdIdx ix, int B, int N, int S, int T, long cap_rows, long cap_pairs,
                   hipStream_t st) {
  GC_REQUIRE(S >= 1 && S <= 31, "producer: %d sentence slots per pair (1..31 supported)", S);
  GC_REQUIRE((long)B * N * N * S < (1L << 31), "producer: B*N*N*S exceeds 32-bit slot indices");
  ProfScope ps("prod_index", st);
  GC_REQUIRE(hipMemsetAsync(ix.pair_bits, 0, sizeof(int) * (size_t)B * N * N, st) == hipSuccess, "producer: memset failed");
  if (src.n_records > 0) {
    hipLaunchKernelGGL(prod_rec_bits_kernel, dim3(cdiv(src.n_records, 256)), dim3(256), 0, st, src.records, src.n_records, ix.pair_bits, B,
                       N, S, T);
    GC_TRY(check_launch("prod_rec_bits"));
  }
  hipLaunchKernelGGL(prod_rec_index_a_kernel, dim3(B), dim3(256), 0, st, n_valid, ix, N);
  GC_TRY(check_launch("prod_rec_index_a"));
  GC_TRY(prod_index_b(n_valid, ix, B, N, S, cap_rows, cap_pairs, st));
  if (src.n_records > 0) {
    hipLaunchKernelGGL(prod_rec_rows_kernel, dim3(cdiv(src.n_records, 256)), dim3(256), 0, st, src.records, src.n_records, ix, src.row_rec,
                       B, N, S, T);
    GC_TRY(check_launch("prod_rec_rows"));
  }
  return 0;
}

int prod_rec_word_fwd(const ProdSrc& src, const float* ctx, const float* table, ProdIdx ix, float* CW, float* stats, int N, int S, int T,
                      int Hd, int ND, hipStream_t st) {
  PROD_LAUNCH(prod_rec_word_fwd_kernel, Hd, dim3(PGRID), dim3(64 * PW), (size_t)PW * T * sizeof(float), st, ctx, src.records,
              (const int*)src.row_rec, src.dis_plus, table, ix, CW, stats, N, S, T, Hd, ND);
  return check_launch("prod_rec_word_fwd");
}

int prod_rec_word_bwd(const ProdSrc& src, const float* ctx, const float* table, const float* stats, const float* dCW, ProdIdx ix,
                      float* dots, float* dtable, float* dctx, int B, int N, int S, int T, int Hd, int ND, hipStream_t st) {
  PROD_LAUNCH(prod_rec_word_bwd_rows_kernel, Hd, dim3(PGRID), dim3(64 * PW), (size_t)PW * (T + Hd) * sizeof(float), st, ctx, src.records,
              (const int*)src.row_rec, src.dis_plus, table, stats, dCW, ix, dots, N, S, T, Hd, ND);
  GC_TRY(check_launch("prod_rec_word_bwd_rows"));
  PROD_LAUNCH(prod_rec_word_bwd_tok_kernel, Hd, dim3((unsigned)((long)B * T)), dim3(64 * PW), sizeof(float) * PW * (size_t)(Hd + ND), st,
              ctx, src.records, (const int*)src.row_rec, src.dis_plus, table, stats, dCW, dots, ix, dtable, dctx, T, Hd, ND);
  return check_launch("prod_rec_word_bwd_tok");
}

}  // namespace gc

// =====================================================================================================================
// C ABI (include/gcgcn_producer_rec.h)
// =====================================================================================================================
#include "../../include/gcgcn_producer_rec.h"

using namespace gc;

// Everything the three entries refuse alike, before anything is launched.
static int rec_check(const char* who, int B, int N, int S, int T, int Hd, int P, int ND, int n_records, const int32_t* records,
                     int64_t cap_rows, int64_t cap_pairs) {
  GC_REQUIRE(B > 0 && N > 0 && T > 0 && Hd >= 1 && Hd <= 64 * HCLIM && P > 0 && ND > 0, "%s: bad shape", who);
  GC_REQUIRE(S >= 1 && S <= 31, "%s: %d sentence slots per pair (1..31 supported)", who, S);
  GC_REQUIRE(T <= 2048, "%s: T=%d tokens (at most 2048: the word attention keeps a slot's weights in LDS)", who, T);
  GC_REQUIRE(n_records >= 0, "%s: negative record count n_records=%d", who, n_records);
  GC_REQUIRE(n_records == 0 || records, "%s: null pointer records", who);
  GC_REQUIRE(((uintptr_t)records & 7) == 0, "%s: records is not 8-byte aligned", who);
  GC_REQUIRE(cap_rows >= 0 && cap_pairs >= 0 && cap_rows < (1L << 30) && cap_pairs < (1L << 30), "%s: bad capacities", who);
  return 0;
}

static ProdSrc rec_src(int n_records, const int32_t* records, int dis_plus, const ProdBound& o) {
  ProdSrc src;
  src.rec = true, src.n_records = n_records, src.records = records, src.dis_plus = dis_plus, src.row_rec = o.row_rec;
  return src;
}

extern "C" {

int gcpr_producer_fwd(int B, int N, int S, int T, int Hd, int P, int ND, const float* ctx, int n_records, const int32_t* records,
                      int dis_plus, const float* node, const float* dis_table, const int32_t* n_valid, const float* flat,
                      int64_t cap_rows, int64_t cap_pairs, int32_t* ibuf, float* fbuf, float* scratch, int64_t scratch_elems, float* E,
                      void* stream) {
  GC_TRY(rec_check("gcpr_producer_fwd", B, N, S, T, Hd, P, ND, n_records, records, cap_rows, cap_pairs));
  GC_REQUIRE(ctx && node && dis_table && flat && ibuf && fbuf, "gcpr_producer_fwd: null pointer");   // E == NULL: compact
  GC_REQUIRE(!scratch || scratch_elems >= 0, "gcpr_producer_fwd: short workspace: scratch_elems=%ld", (long)scratch_elems);
  const ProdBound o = prod_bind(ibuf, fbuf, nullptr, false, B, N, S, T, Hd, P, ND, cap_rows, cap_pairs);
  return prod_fwd(B, N, S, T, Hd, P, ND, ctx, rec_src(n_records, records, dis_plus, o), node, dis_table, n_valid, flat, o.ix, cap_rows,
                  cap_pairs, o.w, E, scratch, scratch ? scratch_elems : 0, (hipStream_t)stream);
}

int gcpr_producer_bwd(int B, int N, int S, int T, int Hd, int P, int ND, const float* ctx, int n_records, const int32_t* records,
                      int dis_plus, const float* node, const float* dis_table, const int32_t* n_valid, const float* flat,
                      int64_t cap_rows, int64_t cap_pairs, int32_t* ibuf, float* fbuf, float* bbuf, const float* dE, const float* dEc,
                      float* dctx, float* dnode, float* ddis_table, float* dflat, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  GC_TRY(rec_check("gcpr_producer_bwd", B, N, S, T, Hd, P, ND, n_records, records, cap_rows, cap_pairs));
  GC_REQUIRE(ctx && node && dis_table && flat && ibuf && fbuf && bbuf && (dE || dEc) && dctx && dnode && ddis_table && dflat,
             "gcpr_producer_bwd: null pointer");
  const ProdBound o = prod_bind(ibuf, fbuf, bbuf, true, B, N, S, T, Hd, P, ND, cap_rows, cap_pairs);
  if (n_valid && dE) GC_TRY(prod_wpair(n_valid, o.g.wpair, B, N, st));
  return prod_bwd(B, N, S, T, Hd, P, ND, ctx, rec_src(n_records, records, dis_plus, o), node, dis_table, n_valid, flat, o.ix, cap_rows,
                  cap_pairs, o.w, dE, o.g, dctx, dnode, ddis_table, dflat, o.scratch, prod_scratch_elems(B, N, T, Hd), st,
                  dE ? nullptr : dEc);
}

int gcpr_producer_bwd_det(int B, int N, int S, int T, int Hd, int P, int ND, const float* ctx, int n_records, const int32_t* records,
                          int dis_plus, const float* node, const float* dis_table, const int32_t* n_valid, const float* flat,
                          int64_t cap_rows, int64_t cap_pairs, int32_t* ibuf, float* fbuf, float* bbuf, const float* dE,
                          const float* dEc, float* dctx, float* dnode, float* ddis_table, float* dflat, float* detbuf, int64_t det_elems,
                          void* stream) {
  hipStream_t st = (hipStream_t)stream;
  GC_TRY(rec_check("gcpr_producer_bwd_det", B, N, S, T, Hd, P, ND, n_records, records, cap_rows, cap_pairs));
  GC_REQUIRE(ctx && node && dis_table && flat && ibuf && fbuf && bbuf && (dE || dEc) && dctx && dnode && ddis_table && dflat,
             "gcpr_producer_bwd_det: null pointer");
  GC_REQUIRE(detbuf, "gcpr_producer_bwd_det: null pointer detbuf");
  GC_REQUIRE(((uintptr_t)detbuf & 15) == 0, "gcpr_producer_bwd_det: detbuf is not 16-byte aligned");
  GC_REQUIRE(det_elems >= prod_det_elems(Hd, cap_pairs),
             "gcpr_producer_bwd_det: short workspace: det_elems=%ld is smaller than gcgcn_producer_det_elems (%ld)", (long)det_elems,
             prod_det_elems(Hd, cap_pairs));
  const ProdBound o = prod_bind(ibuf, fbuf, bbuf, true, B, N, S, T, Hd, P, ND, cap_rows, cap_pairs);
  if (n_valid && dE) GC_TRY(prod_wpair(n_valid, o.g.wpair, B, N, st));
  return prod_bwd(B, N, S, T, Hd, P, ND, ctx, rec_src(n_records, records, dis_plus, o), node, dis_table, n_valid, flat, o.ix, cap_rows,
                  cap_pairs, o.w, dE, o.g, dctx, dnode, ddis_table, dflat, o.scratch, prod_scratch_elems(B, N, T, Hd), st,
                  dE ? nullptr : dEc, true, detbuf);
}

}  // extern "C"
