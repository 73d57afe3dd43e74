// Batched fp32 GEMM on the exact-f32 matrix cores of gfx950 (v_mfma_f32_32x32x2_f32) with the
// fused epilogues the graph-convolution stack needs.  Internal header (host launcher + args).
#pragma once
#include "common.hpp"

namespace gc {

// C[z] = epilogue( alpha * opA(A[z]) * opB(B[z]) )          z = z1 * batch2 + z2
// A problem is described by one of three constructors, named after how the operands are STORED (gemm_nn / gemm_nt / gemm_tn
// below the struct; they launch nothing), then whatever recurs is attached (split_ws, batch_z1 / batch_z2, tagged) and the
// epilogue fields are assigned:
//   NN : A[M][K], B[K][N]   C = A B      activations times a [K][N] weight; every data gradient dX = dY W
//   NT : A[M][K], B[N][K]   C = A B^T    Y = X W^T with a Linear's [out][in] weight; Q_h Q_h^T; dM We^T
//   TN : A[K][M], B[K][N]   C = A^T B    K = the row dimension of both operands: every weight gradient dW = dY^T X
//   a_kc : A is stored [M][K] (k contiguous: NN, NT);  else A is stored [K][M] (TN)        -- set by the constructors,
//   b_kc : B is stored [N][K] (k contiguous: NT);      else B is stored [K][N] (NN, TN)    -- by nobody else
// epilogue, in this order (every pointer optional):
//   v  = alpha * acc
//   v += add[row * ldadd + col]            (batch strided)
//   v += bias[col]
//   v += rowadd[row]                       (batch strided)
//   v *= rowscale[row]                     (batch strided)
//   v  = max(v, 0)           if relu
//   v += C[row, col]         if accumulate
//   v  = 0                   if the row is a padding row (n_valid given)
//   C[row, col] = v
//   C2[row, col] = dropout(v) + add2[row * ldadd2 + col]     if C2 (dropout index = element
//                                                             offset inside the C2 buffer, plus drop_base)
//   C2[row, col] = 0         if the row is a padding row: add2 is NOT added there (C2 leaves the block, as api.hip's `out`:
//                                                             its padding rows are zero like C's)
struct GemmArgs {
  const float* A = nullptr;
  const float* B = nullptr;
  float* C = nullptr;
  int M = 0, N = 0, K = 0;
  long lda = 0, ldb = 0, ldc = 0;
  int a_kc = 1, b_kc = 0;
  int batch1 = 1, batch2 = 1;
  long sA1 = 0, sA2 = 0, sB1 = 0, sB2 = 0, sC1 = 0, sC2 = 0;
  float alpha = 1.f;
  const float* add = nullptr;
  long ldadd = 0, sAdd1 = 0, sAdd2 = 0;
  const float* bias = nullptr;
  const float* rowadd = nullptr;
  long sRa1 = 0, sRa2 = 0;
  const float* rowscale = nullptr;
  long sRs1 = 0, sRs2 = 0;
  int relu = 0;
  int accumulate = 0;
  float* C2 = nullptr;
  long ldc2 = 0, sC21 = 0, sC22 = 0;
  const float* add2 = nullptr;
  long ldadd2 = 0, sAdd21 = 0, sAdd22 = 0;
  Drop drop = {nullptr, 0, 0, 1.f};
  long drop_base = 0;  // added to the C2 element offset to form the dropout index (C2 may be a shifted view)
  // ragged documents: output row r of batch (z1, z2) belongs to document
  // z1 * nv_zdoc + r / nv_rows and is a padding row iff r % nv_rows >= n_valid[doc].
  const int* n_valid = nullptr;
  int nv_rows = 1, nv_zdoc = 0;
  const char* tag = "gemm_single";  // name seen by the per-kernel timer (gemm_kernel launches; groups: "gemm_group")
  // Ragged batches: run on the entity rows that exist.  The [B N]-row tensors stay padded in memory; `rb` lists their 16-row
  // blocks, LIVE blocks first (block r of document b is live iff 16 r < n_valid[b]), then the dead ones; *rb_n = number of
  // live blocks (device).  Interior, 16-byte aligned problems only (the launcher drops rb otherwise: the dense product is
  // equally correct, padding rows hold zeros).
  //   rb_mode 1: M is the document-row dimension -- virtual row m of this problem is row rb[m / 16] * 16 + m % 16 of A
  //              ([M][K], a_kc = 1) and of every row-indexed epilogue operand and output.  Tiles past the live blocks do no
  //              arithmetic; they store zeros when rb_zero is set (outputs that leave the block: their padding rows must be
  //              zero) and nothing otherwise (workspaces whose dead rows nobody reads).
  //   rb_mode 2: K is the document-row dimension (weight gradients; both operands [K][.], a_kc = b_kc = 0): only the live
  //              blocks are summed over.
  const int* rb = nullptr;
  const int* rb_n = nullptr;
  int rb_mode = 0, rb_zero = 0;
  // split-K workspace (optional): partial sums [splits][batch][M][N]
  float* ws = nullptr;
  long ws_elems = 0;
  // filled by the launcher
  short vecA = 0, vecB = 0;
  int splits = 1, ksplit = 0;
  int widen = 1;   // rb_mode 1, splits > 1: a launch of a ragged batch may cut K up to `widen` times finer ON THE DEVICE, with the tile
                   // workgroups its dead rows leave idle (split_width, gemm_body.hpp); the workspace holds splits * widen slabs

  // What recurs beside the product itself; each returns *this, so a description reads gemm_tn(...).split_ws(...).tagged(...)
  __host__ __device__ GemmArgs& split_ws(float* w, long elems) { return ws = w, ws_elems = elems, *this; }
  __host__ __device__ GemmArgs& tagged(const char* t) { return tag = t, *this; }
  // the two batch levels (z = z1 * batch2 + z2) with the strides of A, B and C; epilogue operands keep their own stride fields
  __host__ __device__ GemmArgs& batch_z1(int n, long sA, long sB, long sC) { return batch1 = n, sA1 = sA, sB1 = sB, sC1 = sC, *this; }
  __host__ __device__ GemmArgs& batch_z2(int n, long sA, long sB, long sC) { return batch2 = n, sA2 = sA, sB2 = sB, sC2 = sC, *this; }
};

// The storage forms (see the top of this file).  gemm_stored takes the two flags as data: for the C ABI's gcgcn_gemm /
// gcgcn_gemm_dyn, whose callers hand them in, and for nobody else.
__host__ __device__ inline GemmArgs gemm_stored(int a_kc, int b_kc, const float* A, long lda, const float* B, long ldb, float* C, long ldc,
                                                int M, int N, int K) {
  GemmArgs g;
  g.A = A, g.lda = lda, g.a_kc = a_kc;
  g.B = B, g.ldb = ldb, g.b_kc = b_kc;
  g.C = C, g.ldc = ldc;
  g.M = M, g.N = N, g.K = K;
  return g;
}
__host__ __device__ inline GemmArgs gemm_nn(const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int N, int K) {
  return gemm_stored(1, 0, A, lda, B, ldb, C, ldc, M, N, K);
}
__host__ __device__ inline GemmArgs gemm_nt(const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int N, int K) {
  return gemm_stored(1, 1, A, lda, B, ldb, C, ldc, M, N, K);
}
__host__ __device__ inline GemmArgs gemm_tn(const float* A, long lda, const float* B, long ldb, float* C, long ldc, int M, int N, int K) {
  return gemm_stored(0, 0, A, lda, B, ldb, C, ldc, M, N, K);
}

// Enqueue on `stream`.  tile: 0 or 1 = the 64x64 block body (the only one; the two 128x128 bodies of earlier rounds lost every
// A/B on this path's products and are gone).
// splits: 0 = pick (needs g.ws), 1 = none, n = split K n ways (partials in g.ws, then one
// deterministic reduce + epilogue kernel).
int gemm(const GemmArgs& g, hipStream_t stream, int tile = 0, int splits = 0);

// A column sum riding in a group launch: out[c] = sum_{r < R} X[r * ld + c]  (bias gradients).  Stage 1 (COL_RIDE_SLICES
// row slices -> part[slice][C]) runs in extra workgroups of the GEMM launch, stage 2 in extra workgroups of its
// split-K reduce: the two launches of a stand-alone column sum disappear.  part: COL_RIDE_SLICES * C floats.
// A ColRide is one of three things, and callers build it with the constructor of that name (the kernels tell them apart by
// `ready_slices`, which only the constructors write):
//   col_sum(X, R, ld, C, out, part)   the whole column sum: stage 1 in the launch, stage 2 in its reduce or with the caller
//   .stage2(slices)                   of such a sum whose part[slices][C] an earlier launch (or the chain kernel) filled: only
//                                     stage 2 rides, in the trailing workgroups of the group launch itself
//   head_sum(W, H, D, out)            not a column sum but the sum over H interleaved blocks (heads) of D columns, in trailing
//                                     workgroups of the launch: out[k * D + c] = sum_{h < H} W[(k * H + h) * D + c], k, c < D
constexpr int COL_RIDE_SLICES = 64;
struct ColRide {
  const float* X = nullptr;
  float* out = nullptr;
  float* part = nullptr;
  long R = 0, ld = 0;
  int C = 0;
  int ready_slices = 0;  // 0: col_sum, > 0: stage2 (the slices to sum; X unused), < 0: head_sum
  ColRide stage2(int slices) const {
    ColRide c = *this;
    c.ready_slices = slices;
    return c;
  }
};
inline ColRide col_sum(const float* X, long R, long ld, int C, float* out, float* part) {
  ColRide c;
  c.X = X, c.out = out, c.part = part, c.R = R, c.ld = ld, c.C = C;
  return c;
}
inline ColRide head_sum(const float* W, int H, int D, float* out) {
  ColRide c;
  c.X = W, c.out = out, c.R = H, c.ld = D, c.C = D * D, c.ready_slices = -1;
  return c;
}
// Stage 2 as a launch of its own (nothing was left to carry it): out[c] = the sum of c.part's ready_slices slices, in order
int col_sum_stage2_launch(const ColRide& c, hipStream_t stream);

// Up to NP independent problems carried by one launch.
template <int NP>
struct GemmGroupT {
  static constexpr int MAXP = NP;
  GemmArgs p[NP];
  int tile_begin[NP + 1];  // first workgroup of each problem, a multiple of 8 (see gemm_group_kernel)
  int tile_count[NP];      // 64x64 tiles of each problem (the domain of the XCD remap)
  int tile_first[NP];      // this launch carries tiles [tile_first, tile_first + tile_take) of the problem's (remapped) list:
  int tile_take[NP];       // a parked problem may be split over two carrying launches
  int red_begin[NP + 1];
  int nprob;
  ColRide col;  // col.X == nullptr: nothing rides
};
// MultiHeadAttention's backward core (mha_body.hpp: dA, P, Q -> dQ per (document, head)) riding in a group launch of the
// convolution that follows the attention: `count` = B * H pairs, spread evenly through the launch's tile list.
struct MhaPass {
  const float* Q = nullptr;
  const float* P = nullptr;
  const float* dA = nullptr;
  float* dQ = nullptr;
  int N = 0, D = 0, H = 0, dh = 0, kchunk = 0, count = 0;
  float alpha = 1.f;
  Drop drop = {nullptr, 0, 0, 1.f};
};
using GemmGroup = GemmGroupT<9>;   // gemm_group launches and the edge pass carrying parked problems
using GemmGroup4 = GemmGroupT<4>;  // passengers of a chain launch (kernel arguments stay small)
// col_later (optional): if the launch needs no split-K reduce, stage 2 of the riding column sum is NOT launched on its own;
// *col_later is set and the caller finishes it inside a later kernel of its own (col_ride_stage2_block).
int gemm_group(const GemmArgs* probs, int n, hipStream_t stream, const ColRide* col = nullptr, bool* col_later = nullptr,
               const MhaPass* mha = nullptr);
int gemm_group_mha_chunk(int dh);   // the pairs' LDS images fit the group kernel's with this head-feature chunk, or 0 (attn_plan_bwd)

// ---- deferred problems ------------------------------------------------------------------------------------------
// Weight-gradient products are needed by nobody before the end of backward, while later launches of the same
// backward leave the matrix pipes idle (the edge-tensor stream of GATAttention's backward is HBM-bound).  A block can
// park such a product in the DeferQueue of its backward pass (host memory, owned by the caller: one queue per pass, no
// process-wide state); the next launch that can carry passengers takes them along as extra workgroups, unsplit (their
// full K runs inside one workgroup: no reduce launch).  Whoever parks a problem must keep its operands alive until
// gemm_flush_deferred() or a carrying launch has been enqueued.
// Only interior, 16-byte aligned shapes are parked (gemm_defer returns false otherwise: launch it now).
struct DeferQueue {
  static constexpr int CAP = 32;
  GemmArgs p[CAP];
  int done[CAP] = {};  // tiles of p[i] already carried by an earlier launch
  int n = 0;
  // second stages of riding column sums (bias gradients: ColRide::stage2, the partials are in memory) that nobody
  // needs before the end of backward either: the next carrying edge pass sums them in a trailing workgroup, or the flush does
  static constexpr int COLCAP = 4;
  ColRide col2[COLCAP];
  int ncol2 = 0;
};
bool gemm_defer(DeferQueue* q, const GemmArgs& g);  // q == nullptr: never parks
bool gemm_defer_col2(DeferQueue* q, const ColRide& c);          // c: a .stage2(); false: run it now
bool gemm_take_deferred_col2(DeferQueue* q, ColRide& out);      // pops one parked second stage
// Move up to MAXP parked problems into gg (longest K first, per-problem XCD-aligned tile ranges); returns the number
// of workgroups (0: nothing parked).  flops (optional) accumulates 2MNK of the taken problems.
int gemm_take_deferred(DeferQueue* q, GemmGroup& gg, double* flops);
// Same for a chain launch: a workgroup of 512 threads runs ONE tile, its two tile teams splitting K (the partial sums meet
// in LDS).  Takes at most `max_wgs` tiles, longest problems first; a problem may be taken partially -- the rest of its
// tiles waits for a later carrier.
int gemm_take_deferred_pairs(DeferQueue* q, GemmGroup4& gg, double* flops, long max_wgs, bool small_first = false);
// Launch whatever is still parked as ordinary group launches (end of backward without a carrying launch).
int gemm_flush_deferred(DeferQueue* q, hipStream_t stream);

// The deterministic reduce + epilogue over g.splits partial slabs in g.ws (every split launch of gemm.hip, and tile kernels defined
// outside it); `what` names the launch in an error message.
int splitk_reduce(const GemmArgs& g, hipStream_t st, const char* what = "gemm_splitk_reduce");

// ---- one dimension known only on the device ------------------------------------------------------------------
// Products over a data-dependent selection of rows (the live sentence slots / entity pairs of the edge-feature producer,
// producer.hip): the row count lives in device memory, the host only knows an upper bound `cap`.  A fixed grid of
// persistent workgroups walks the tile list computed from *cnt, so no host synchronisation and no worst-case grid.
//   dyn = 1: M = *cnt  (rows of A and of C; g.M is ignored)
//   dyn = 2: K = *cnt  (rows of both operands -- weight gradients; g.K is ignored); split-K over a factor chosen from
//            `cap`, partials through g.ws + the deterministic reduce.
// Interior shapes (N, and M or K, multiples of 64 / 32; 16-byte aligned) take the unguarded tile body with the count
// rounded UP to a multiple of 64: operand buffers must be readable that far, C writable that far (dyn = 1), and for
// dyn = 2 at least one operand's rows in [*cnt, roundup64(*cnt)) must be zero.  Other shapes take the guarded body
// with the exact count.
int gemm_dyn(const GemmArgs& g, const int* cnt, int dyn, long cap, hipStream_t st);
// The weight gradient (dyn = 2: gw) and the data gradient (dyn = 1: gx) of one Linear layer on the same device-side row count, in one
// launch (+ the weight gradient's reduce).
int gemm_dyn_pair(const GemmArgs& gw, const GemmArgs& gx, const int* cnt, long cap, hipStream_t st);
// ... and two weight gradients of the same shape over the same rows (dyn = 2 both; one reduce launch for both)
int gemm_dyn_pair_ww(const GemmArgs& ga, const GemmArgs& gb, const int* cnt, long cap, hipStream_t st);
// ... and two products whose M is the same device-side row count (dyn = 1 both)
int gemm_dyn_pair_xx(const GemmArgs& ga, const GemmArgs& gb, const int* cnt, long cap, hipStream_t st);

// Floats of split-K workspace that lets every GEMM of a [rows x cols]-sized problem split freely.
inline long gemm_ws_elems(long rows, long cols) {
  long need = 16 * rows * cols;
  const long cap = 16L << 20;   // 64 MB (r5: two split + device-widened K = 3072 data gradients of cfg 3 need 12.6 M floats)
  return need < cap ? need : cap;
}

}  // namespace gc
