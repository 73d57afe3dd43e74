/* gcgcn.h -- C ABI of libgcgcn_hip.so: the CAGGC + MAGGC graph-convolution hot path of GCGCN
 * as hand-written HIP kernels for gfx950 (MI355X).
 *
 * The reference (Huiweizhou/GCGCN) has no FFI: its boundary for this path is the nn.Module
 * protocol of five Python classes in models/GCGCN_glove.py:18-168 (code-identical copies in
 * models/GraphCNN_multihead_bert_gate_cls.py:18-172).  Each entry point below replaces the
 * forward (or autograd backward) of one of those classes and cites it.  gcgcn_amd/functional.py
 * binds these with ctypes; INTEGRATION.md shows the binding a maintainer of the reference adds.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp32 (unless typed otherwise), row-major, dense;
 *   - B documents, N entity slots per document, D feature width, L sub-layers, H heads,
 *     gh = D / L, dh = D / H, M = B * N;
 *   - n_valid: optional int32[B]; entities >= n_valid[b] are padding (their rows of X must be
 *     zero; their outputs and gradients are zero).  NULL = every document has N entities;
 *   - the caller owns all memory (inputs, outputs, saved-for-backward, workspace); the library
 *     keeps no device memory and never synchronises: work is enqueued on `stream`
 *     (a hipStream_t) and is hipGraph-capturable;
 *   - return value 0 = ok, otherwise gcgcn_last_error() describes the failure (thread-local);
 *   - dropout: rng_snap is a device int64[2] {seed, counter} written by gcgcn_rng_next at
 *     forward time; NULL (or p == 0) = eval mode.  Backward takes the same snapshot.
 *
 * Parameter buffers ("flat") hold one block's parameters contiguously in the layout the
 * kernels want; gcgcn_*_layout report offsets (in floats).  Gradient buffers use the same
 * layout, so a block's gradient is one contiguous all-reduce bucket.
 */
#ifndef GCGCN_H
#define GCGCN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int gcgcn_version(void);            /* ABI version, currently 7 */
const char* gcgcn_last_error(void); /* message of the last failing call on this thread */

/* Run-time switches for A/B tests.  "chain": 1 (default) = the per-(doc, head) products of a conv run inside the
 * chain kernels, 0 = one batched launch per product.  "mha_core": 1 (default) = graphs of N <= 64 entities take the
 * one-workgroup-per-(doc, head) attention kernels, 0 = batched GEMM + row softmax for every N.  Results are identical
 * up to fp32 summation order.  "head_v1" (-1 = by problem size), "head_bil3", "head_bil3_bwd", "head_dw3",
 * "head_compact", "chain_t", "chain_big" and "split_widen" select kernel generations (the five head options take effect in
 * csrc/head.hip head_plan and nowhere else: gcgcn_debug_head_plan shows the result; "split_widen" in csrc/gemm.hip gemm_plan and
 * nowhere else: gcgcn_debug_gemm_plan); "head_matmul" is no switch but the matmul argument of the calling thread's NEXT
 * classifier-head call (see gcgcn_head_fwd: taken by that call, no environment variable, nothing lasting), and "lstm_recurrent" likewise the recurrent argument of its NEXT LSTM call (see gcgcn_lstm_fwd); "group_dump" (0 = off) prints what
 * every GEMM launch is made of on stderr.  Each name also reads the environment variable GCGCN_<NAME> once when nobody set
 * it (GCGCN_CHAIN=0, GCGCN_HEAD_V1=1, ...: DESIGN.md section 6 lists them).  Any other name fails. */
int gcgcn_set_option(const char* name, int value);

/* ---- ragged batches: the entity rows that exist (ABI v5; v7: one list serves every product) ------------------------------- */
/* The reference runs one UNPADDED document per call (config/Config.py:339-354): its products have n rows.  A padded batch
 * [B, N, .] with n_valid has sum_b n_b real rows of B N.  gcgcn_row_blocks lists the 16-row blocks of the [B N]-row tensors,
 * the LIVE ones first (block r of document b is live iff 16 r < n_valid[b]; ascending), the dead ones behind them:
 *   out = int32[gcgcn_row_blocks_ints(B, N)] = {live blocks, 0, 0, 0 | B N / 16 blocks};
 * N must be a multiple of 16.  Given as `rowblk` to gcgcn_gcn_fwd / _bwd and gcgcn_mha_fwd / _bwd (NULL = dense), the
 * node-phase products of the block -- X WnX, Ebar We, X Wq, the output projection, every data gradient -- run on the live
 * blocks only (four to a 64-row tile), and every weight gradient (K = the document rows) sums over the live blocks only (two
 * to a k-tile; lists of up to 512 blocks, B N <= 8192 -- longer ones run dense); the tensors keep their padded layout,
 * outputs that leave the block (out, dX, dEbar, Q) are zero on
 * padding rows as always.  Everything stays on the device (no host read; the list is rebuilt by every replay of a captured
 * step).  A block whose shape the column-strip chain kernels do not serve (N > 64, or a width they are not instantiated for)
 * ignores the list and computes every row, as does a forward / backward pair without n_valid.  The SAME list must be given
 * to a block's forward and backward. */
int64_t gcgcn_row_blocks_ints(int B, int N);
int gcgcn_row_blocks(int B, int N, const int32_t* n_valid, int32_t* out, void* stream);

/* ---- per-kernel timing for roofline reports (bench.py) ------------------------------------------- */
/* While active, every kernel launch whose name starts with kernel_prefix ("edge_bwd", "edge_fwd",
 * "edge_bcast", "gemm", "softmax", ...) is bracketed by hipEvents on its launch stream (at most
 * `capacity` launches).  prof_stop synchronises those events and returns their summed duration, their
 * count and (optional) the work they did: executed flops for GEMM kernels, algorithmic HBM bytes for the
 * edge kernels.  Not thread-safe; keep it off while capturing a hipGraph. */
int gcgcn_prof_start(const char* kernel_prefix, int capacity);
int gcgcn_prof_enable(int on); /* pause (0) / resume (1) between prof_start and prof_stop: sample some steps only */
int gcgcn_prof_stop(double* total_ms, int* launches, double* work);

/* ---- dropout RNG state (replaces torch's global CUDA generator used by nn.Dropout) ------- */
/* snaps[i] <- {state.seed, state.counter + i} for i < count; state.counter += count.
 * state: device int64[2] {seed, counter}; snaps: device int64[2 * count].  One launch serves `count`
 * dropout-using forward calls (each takes its own 2-word snapshot). */
int gcgcn_rng_next(void* state, void* snaps, int count, void* stream);
/* keep[i] = 1 iff element i of dropout site (snap, salt, p) is kept.  Test/debug aid. */
int gcgcn_dropout_keep(uint8_t* keep, int64_t n, const void* rng_snap, uint64_t salt, float p, void* stream);
/* y = dropout(x); calling it on a gradient with the same snapshot is the backward.
 * Replaces self.dropout in the hop glue, GCGCN_glove.py:341. */
int gcgcn_dropout(const float* x, float* y, int64_t n, const void* rng_snap, uint64_t salt, float p, void* stream);

/* salts of the dropout sites inside the blocks */
#define GCGCN_SALT_GAT 0x47415431ull
#define GCGCN_SALT_MHA 0x4d484131ull
#define GCGCN_SALT_GCN 0x47434e31ull
#define GCGCN_SALT_GLUE 0x474c5531ull

/* ---- GATAttention (CAGGC adjacency)  GCGCN_glove.py:144-168 -------------------------------- */
/* D = att_input_dim (width of node_feat and edge_feat), Dh = hidden_dim (rows of the three nn.Linear(att_input_dim,
 * hidden_dim), glove:148-150; wt = nn.Linear(3 * hidden_dim, 1), glove:151).
 * flat = [W_h Dh*D | b_h Dh | W_t Dh*D | b_t Dh | W_r Dh*D | b_r Dh | wt 3Dh | wt_bias 1]
 * out[0..7] = offsets of those eight pieces, out[8] = total floats. */
int gcgcn_gat_layout(int D, int Dh, int64_t* out9);

/* forward(node_feat X[B,N,D], edge_feat E[B,N,N,D], mask ignored as in the reference):
 *   P[B,N,N]    softmax_j(u.x_j + v.e_ij + c)            (saved for backward)
 *   A[B,N,N]    dropout(P); may be NULL when rng_snap is NULL (then A == P)
 *   Ebar[B,N,D] mean_j E[b,i,j,:]  -- by-product of the single pass over E, consumed by the
 *               GraphConvolution that follows (GCGCN_glove.py:40-41 commuted)
 *   uvc[2D+1], s[B,N]  folded projection and node scores (saved for backward) */
/* rng_state / rng_snaps / rng_count: optional (NULL, NULL, 0).  When given, the call also performs
 * gcgcn_rng_next(rng_state, rng_snaps, rng_count) inside its first kernel, BEFORE anything reads rng_snap (which may
 * point into rng_snaps): a hop loop draws the snapshots of all its dropout sites without a launch of its own.
 * mask: NULL (default: the reference DISCARDS its masked_fill result, glove:163-164, so its mask is a no-op), or a
 * uint8/bool [B,N,N] whose non-zero entries get energy -100000 before the softmax: the paper-faithful partially
 * connected adjacency, an explicit opt-in (GATAttention(apply_mask=True)).  The backward needs no mask where a row keeps an
 * unmasked real column: its masked entries have P == 0 exactly, hence a zero logit gradient.  A row whose real columns are
 * ALL masked comes out uniform, and masked_fill passes no gradient through it: the caller of gcgcn_gat_bwd clears that row
 * of dA (functional.GatFn does).
 * uvc_valid != 0: uvc already holds the folded projection of THESE parameters (a function of flat only: the caller may
 * keep it while flat is unchanged -- inference, several documents per optimiser step); the fold kernel is skipped. */
int gcgcn_gat_fwd(int B, int N, int D, int Dh, const float* X, const float* E, const int32_t* n_valid, const float* flat,
                  const void* rng_snap, float p, float* uvc, float* s, float* P, float* A, float* Ebar, void* rng_state,
                  void* rng_snaps, int rng_count, const uint8_t* mask, int uvc_valid, void* stream);

/* backward.  dA[B,N,N], dEbar[B,N,D] (NULL = zero), dX_in[B,N,D] (NULL = zero: gradient node_feat has
 * already collected from its other consumers -- the convolution of the same hop -- added here instead of
 * by a separate kernel) -> dX[B,N,D], dE[B,N,N,D] (NULL = not wanted), dflat.  Workspace: dlogit[B,N,N], ds[B,N], dvpart[B*N*D], duvc[2D+1],
 * scratch[gcgcn_gat_bwd_scratch(B,N,D)]. */
int64_t gcgcn_gat_bwd_scratch(int B, int N, int D);
/* defer_queue: NULL, or the gcgcn_defer queue of this backward pass (below): weight-gradient products parked in it by
 * gcgcn_gcn_bwd / gcgcn_mha_bwd calls that ran earlier in the pass ride in this call's HBM-bound edge pass. */
int gcgcn_gat_bwd(int B, int N, int D, int Dh, const float* X, const float* E, const int32_t* n_valid, const float* flat,
                  const void* rng_snap, float p, const float* uvc, const float* P, const float* dA, const float* dEbar,
                  const float* dX_in, float* dX, float* dE, float* dflat, float* dlogit, float* ds, float* dvpart,
                  float* duvc, float* scratch, void* defer_queue, void* stream);

/* ---- edge mean alone (MAGGC hop: E enters only through GraphConv's mean, glove:40-41) ------ */
int gcgcn_edge_mean_fwd(int B, int N, int D, const float* E, const int32_t* n_valid, float* Ebar, void* stream);
int gcgcn_edge_mean_bwd(int B, int N, int D, const float* dEbar, const int32_t* n_valid, float* dE, void* stream);

/* ---- MultiHeadAttention (MAGGC adjacency)  GCGCN_glove.py:122-142 -------------------------- */
/* flat = [Wq D*D (rows h*dh.. = linears_q.h.weight) | bq D]; linears_k.* never enter (the
 * reference projects keys with linears_q, glove:136-137).  out = {oWq, obq, total}. */
int gcgcn_mha_layout(int D, int64_t* out3);
/* forward(node_feat X[B,N,D]) -> A[B,H,N,N] = dropout(P), P = softmax(Q_h Q_h^T / sqrt(dh));
 * saved: Q[B,N,D], P[B,H,N,N].  A may be NULL when rng_snap is NULL.
 * scratch[gcgcn_mha_scratch(B,N,D)] floats (split-K partials, column-sum partials); may be NULL
 * (then no GEMM is split). */
int64_t gcgcn_mha_scratch(int B, int N, int D);
int gcgcn_mha_fwd(int B, int N, int D, int H, const float* X, const int32_t* n_valid, const float* flat,
                  const void* rng_snap, float p, float* Q, float* P, float* A, float* scratch, const int32_t* rowblk, void* stream);
/* backward.  dX_in[B,N,D] (NULL = zero) as in gcgcn_gat_bwd.  Workspace: dS[B,H,N,N], dQ[B,N,D],
 * scratch[gcgcn_mha_scratch].  defer_queue (may be NULL): dWq is parked as described at gcgcn_gcn_bwd, and so is the second
 * stage of dbq's column sums (its 64 partial rows live in `scratch`: a later gcgcn_gat_bwd given the same queue sums them in a
 * trailing workgroup of its edge pass, or the flush does) -- keep X, dQ, scratch and dflat alive until the flush. */
int gcgcn_mha_bwd(int B, int N, int D, int H, const float* X, const float* flat, const void* rng_snap, float p,
                  const float* Q, const float* P, const float* dA, const float* dX_in, float* dX, float* dflat,
                  float* dS, float* dQ, float* scratch, void* defer_queue, int core_done, const int32_t* rowblk, void* stream);
/* core_done = 1: dQ already holds the attention core's gradient (gcgcn_gcn_bwd with a gcgcn_mha_hook computed it) */

/* ---- GraphConvolution (H = 1) / MultiGraphConvolution  GCGCN_glove.py:52-120 --------------- */
/* flat = [WnX D x H*D | We D x H*D | Wd | Wlin D x H*D | blin D]
 *   WnX[:, (h*L+l)*gh ..] = graphconv.{h*L+l}.weights_node[:D]     (X part of the dense connection)
 *   We [:, (h*L+l)*gh ..] = graphconv.{h*L+l}.weights_edge
 *   Wd: for h, for l = 1..L-1: graphconv.{h*L+l}.weights_node[D:]  ([l*gh, gh], the Y_0..Y_{l-1} part)
 *   Wlin, blin = linear_layer.weight / .bias
 * out = {oWnX, oWe, oWd, oWlin, oblin, total, wd_floats_per_head}. */
int gcgcn_gcn_layout(int D, int L, int H, int64_t* out7);
/* forward(node_feat X[B,N,D], mean edge feature Ebar[B,N,D], adjacency A[B,H,N,N]) -> out[B,N,D].
 * saved for backward: Pn, Y, HO (each [B,N,H*D]) and rinv[B,H,N].  Workspace: G[B,N,H*D],
 * scratch[gcgcn_gcn_scratch(B,N,D,H)] (split-K / column-sum partials; NULL = never split). */
int64_t gcgcn_gcn_scratch(int B, int N, int D, int H);
/* An edge-tensor pass that depends on nothing the block computes may ride along with it: the NEXT hop's
 * edge mean (forward; == gcgcn_edge_mean_fwd(B,N,D,in=E,n_valid,out=Ebar)) and its backward
 * (== gcgcn_edge_mean_bwd(B,N,D,in=dEbar,n_valid,out=dE)).  The dependent per-(doc, head) part of a block
 * is latency-bound and, for few documents x heads, occupies a fraction of the chip; the HBM-bound pass
 * runs in extra workgroups of that same launch (or as its own launch when that is not possible).  The
 * result is complete when the call's work is.  NULL = nothing rides. */
typedef struct gcgcn_edge_ride {
  int32_t B, N, D;
  const float* in;
  const int32_t* n_valid; /* may be NULL */
  float* out;
} gcgcn_edge_ride;
/* out_rng_snap / out_p: the hop's output dropout x <- dropout(block(x)) (glove:341, site GCGCN_SALT_GLUE) applied
 * in the epilogue of the block's last product; NULL / 0 = the plain block output.  gcgcn_gcn_bwd given the same
 * pair takes dout = gradient of the DROPPED output.
 * wsum[D,D] (may be NULL; H > 1 only): sum over heads of linear_layer.weight's column blocks, a function of the parameters
 * alone that rides in this call's first launch; gcgcn_gcn_bwd given the same buffer skips the launch that would sum it. */
/* A whole MAGGC hop in one call pair (glove:336-337: MultiHeadAttention, then MultiGraphConvolution on its adjacencies).
 * The attention's work rides inside the convolution's launches: forward, the query projection Q = X Wq^T + bq is one more
 * problem of the first group launch (node / edge terms), the attention core (Q -> P, A) follows it and the chain reads
 * A (or P when there is no dropout) -- the `A` argument of gcgcn_gcn_fwd is ignored; backward, the attention core
 * (dA, P, Q -> dQ) runs as passenger workgroups of the convolution's last group launch, and gcgcn_mha_bwd is then called
 * with core_done = 1 for the rest (dX = dQ Wq + dX_in, dWq, dbq).  Needs a graph of at most 64 entities and head width
 * D / H a multiple of 4 (gcgcn_maggc_fusable); results equal the separate calls bit for bit.  Where a chain kernel that
 * keeps its pair in LDS serves the shape, the forward core runs in that kernel's prologue instead of a launch; heads wider
 * than 64 features keep the backward core as a launch of its own (its scratch does not fit a tile workgroup's LDS). */
typedef struct gcgcn_mha_hook {
  const float* flat_q;  /* MultiHeadAttention's flat parameters [Wq D*D | bq D] (gcgcn_mha_layout) */
  float* Q;             /* [B,N,D]   forward: out; backward: in */
  float* P;             /* [B,H,N,N] forward: out; backward: in */
  float* A;             /* [B,H,N,N] forward: out (NULL without dropout) */
  float* dQ;            /* [B,N,D]   backward: out */
  const void* rng_snap; /* the attention's dropout snapshot (site GCGCN_SALT_MHA), NULL = eval */
  float p;
} gcgcn_mha_hook;
int gcgcn_maggc_fusable(int N, int D, int H);
int gcgcn_gcn_fwd(int B, int N, int D, int L, int H, const float* X, const float* Ebar, const float* A,
                  const int32_t* n_valid, const float* flat, const void* rng_snap, float p, const void* out_rng_snap,
                  float out_p, float* out, float* Pn, float* Y, float* HO, float* rinv, float* G, float* wsum, float* scratch,
                  const gcgcn_edge_ride* ride, const gcgcn_mha_hook* mha, const int32_t* rowblk, void* stream);
/* backward.  dout[B,N,D] -> dX, dEbar [B,N,D], dA[B,H,N,N], dflat.
 * Workspace: W1, W2, W3 (each [B,N,H*D]), drow[B,H,N], dXres[B,N,D], dout_m[B,N,D] (only used
 * when n_valid != NULL or out_rng_snap != NULL), scratch[gcgcn_gcn_scratch]. */
int gcgcn_gcn_bwd(int B, int N, int D, int L, int H, const float* X, const float* Ebar, const float* A,
                  const int32_t* n_valid, const float* flat, const void* rng_snap, float p, const void* out_rng_snap,
                  float out_p, const float* Pn, const float* Y, const float* HO, const float* rinv, const float* wsum,
                  const float* dout, float* dX, float* dEbar,
                  float* dA, float* dflat, float* W1, float* W2, float* W3, float* drow, float* dXres, float* dout_m,
                  float* scratch, const gcgcn_edge_ride* ride, const gcgcn_mha_hook* mha, void* defer_queue, const int32_t* rowblk,
                  void* stream);
/* defer_queue != NULL: the block's weight-gradient products (dWlin, dWnX, dWe, dWd: nobody needs them before the end
 * of backward) are not launched by this call but parked in that queue -- a small host-side object the caller creates
 * per backward pass (no process-wide state: concurrent passes, models and devices never share one).  A later
 * gcgcn_gat_bwd (or a long gcgcn_gcn_bwd chain launch) given the same queue carries them as extra workgroups of a launch
 * whose matrix pipes are idle.  Until then the caller must keep X, Ebar, Y, HO, dout (dout_m), W2, W3 and dflat of this
 * call alive, and must call gcgcn_defer_flush(queue, stream) at the end of the pass (it launches what is still parked;
 * no-op otherwise).  The parked parts of dflat are complete only after that.  Destroying a queue forgets what is
 * parked in it without launching anything (a pass that failed half-way). */
void* gcgcn_defer_create(void);
void gcgcn_defer_destroy(void* queue);
int gcgcn_defer_count(const void* queue);
int gcgcn_defer_flush(void* queue, void* stream);

/* ---- GraphConv, the leaf layer  GCGCN_glove.py:18-50 ------------------------------------------ */
/* forward(inputs X[B,N,Din], mean edge feature Ebar[B,N,De], adjacency A[B,N,N]):
 *   out[B,N,Dout] = (Ebar We + A X Wn (+ bias)) / (rowsum(A) + [rowsum == 0])
 * We[De,Dout] = weights_edge, Wn[Din,Dout] = weights_node, bias[Dout] or NULL.  Saved: T = X Wn, rinv[B,N].
 * (Inside GraphConvolution / MultiGraphConvolution this layer is fused into gcgcn_gcn_fwd.) */
int gcgcn_graphconv_fwd(int B, int N, int Din, int De, int Dout, const float* X, const float* Ebar, const float* A,
                        const float* We, const float* Wn, const float* bias, float* out, float* T, float* rinv,
                        float* scratch, void* stream);
/* backward.  Workspace: dS, dT [B,N,Dout], drow[B,N], scratch[gcgcn_gcn_scratch(B,N,max(Din,Dout),1)].
 * dbias may be NULL. */
int gcgcn_graphconv_bwd(int B, int N, int Din, int De, int Dout, const float* X, const float* Ebar, const float* A,
                        const float* We, const float* Wn, const float* out, const float* T, const float* rinv,
                        const float* dout, float* dX, float* dEbar, float* dA, float* dWe, float* dWn, float* dbias,
                        float* dS, float* dT, float* drow, float* scratch, void* stream);

/* ---- trainer loss  config/Config.py:302,355-366 ---------------------------- */
/* loss[b] = sum_{h != t < n} mean_r BCE(sigmoid(logits[b,h,t,r]), labels[b,h,t,r]) / (n^2 - n), n = n_valid[b] or N:
 * what the trainer's double Python loop of nn.BCELoss calls computes per document (ATen arithmetic: logs clamped at
 * -100).  logits, labels [B,N,N,R]; workspace part[B*N].  A document with n < 2 yields NaN like the reference. */
int gcgcn_pair_bce_fwd(int B, int N, int R, const float* logits, const float* labels, const int32_t* n_valid, float* loss,
                       float* part, void* stream);
/* dlogits[B,N,N,R] = dloss[b] * d loss[b] / d logits (dloss NULL = ones); zero on the diagonal and on padding. */
int gcgcn_pair_bce_bwd(int B, int N, int R, const float* logits, const float* labels, const int32_t* n_valid,
                       const float* dloss, float* dlogits, void* stream);
/* The trainer's accuracy bookkeeping (config/Config.py:376-393) over the same logits / labels [B,N,N,R], without the host
 * copy.  For every document b, n = clamp(n_valid[b], 0, N) (NULL: N), and every ordered pair h != t, both < n:
 *   p = 1 / (1 + expf(-x)),  q = 1 / (1 + expf(-p))   (fp32; the reference applies the sigmoid at :355 and again at :377),
 *   r* = the FIRST maximum of q over 0..R-1 (numpy's argmax: saturated logits tie and the lowest index wins, so this is
 *   not the argmax of the logits),  hit = labels[b,h,t,r*] == 1,  na = labels[b,h,t,0] == 1.
 * counters (device int64[8], ADDED to, never overwritten): [0]/[1] acc_NA correct/total (pairs with na), [2]/[3] acc_not_NA
 * correct/total, [4]/[5] acc_total correct/total, [6] pairs whose row holds a NaN (counted here and in no other counter),
 * [7] documents seen (B per call).  One launch, integer atomics only: the result is exact and independent of their order. */
int gcgcn_pair_stats(int B, int N, int R, const float* logits, const float* labels, const int32_t* n_valid, int64_t* counters,
                     void* stream);

/* ---- trainer evaluation  config/Config.py:432-561 (test), config/Config_bert.py:488-656 (ignore-train-facts curve) ---------
 * The reference copies every document's probabilities to the host, appends one Python tuple per (head, tail, relation != NA),
 * sorts the list by score, and walks it for the precision/recall curve, F1, theta and AUC.  Here that is three device stages
 * over 64-bit records; a record's ORDINAL is its position in the reference's append order.
 *   record = (0x3fffffff - bits(p)) << 34 | ordinal << 2 | (label != 0) << 1 | flag      (ascending = the ranking)
 * with p = 1 / (1 + expf(-logit)) in fp32 and flag the pair's sticky in-train flag: the OR over 1 <= k' <= k of
 * label[k'] && in_train[k'] (Config_bert.py:545-562).
 *
 * Workspace bytes of the rank and curve stages for n_records records of which n_keep are kept.  An ordinal has 32 bits: more
 * than 2^32 - 1 records (or a negative count) returns -1 with a message in the last-error buffer; nothing ever wraps. */
int64_t gcgcn_eval_ws_bytes(int64_t n_records, int64_t n_keep);
/* One workgroup per (document, head entity) row of logits / labels [B,N,N,R] (fp32; in_train uint8 [B,N,N,R] or NULL).
 * Only the first n_valid[b] (NULL: N) entities form pairs.  Pair (i, j != i) of document b writes its R - 1 records at
 * doc_base[b] + ((i (n - 1) + j') (R - 1)) + (k - 1), j' = j with the diagonal skipped; doc_base (device int64[B]) is the
 * caller's running exclusive prefix of n (n - 1) (R - 1).  records has room for `capacity` (<= 2^32 - 1) records.
 * counters (device int64[8], ADDED to): top1_acc, na_recall, na_correct, total_recall, total_correct, have_label as
 * Config.py:487-505 (argmax = first maximum of the probabilities), then the number of pairs holding a NaN probability and the
 * number of pairs with a record at or past `capacity` (such records are not written). */
int gcgcn_eval_scan(int B, int N, int R, const float* logits, const float* labels, const uint8_t* in_train, const int32_t* n_valid,
                    const int64_t* doc_base, uint64_t* records, int64_t capacity, int64_t* counters, void* stream);
/* Stable least-significant-digit radix sort of records[0, n) (which must be in ordinal order, as the scan leaves them) by
 * score, in this library's own kernels; digits that all records share are skipped.  records is not modified; the ranked copy
 * is left in ws at byte offset *sorted_off (host).  Reads one 4 KiB histogram back: SYNCHRONISES the stream. */
int gcgcn_eval_rank(const uint64_t* records, int64_t n, void* ws, int64_t ws_bytes, int64_t* sorted_off, void* stream);
/* Curve over ranked[0, m), m <= n_records, with total_recall = counters[3] (1 when 0):
 *   pr_y[i] = fp32(correct_i / (i + 1)), pr_x[i] = fp32(correct_i / total_recall)    (fp64 quotients),
 *   ign_pr_y[i] (NULL: not stored) = 0 if correct_in_train_i == correct_i, else
 *                 fp32((correct_i - correct_in_train_i) / (i + 1 - correct_in_train_i)),
 *   f1_arr = 2 pr_x pr_y / (pr_x + pr_y + 1e-20) in fp32; trapezoids in fp64, summed in index order.
 * result (device double[16]): f1, f1_pos (first argmax), theta = score at f1_pos, p = pr_x[f1_pos], r = pr_y[f1_pos] (named
 * as the reference names them), w (f1_pos when input_theta == -1, else the last i with score_i > input_theta, else 0),
 * f1_arr[w], auc, ign_f1, ign_auc, total_recall as used.  ws / ws_bytes / n_records as given to the rank stage. */
int gcgcn_eval_curve(const uint64_t* ranked, int64_t m, int64_t n_records, const int64_t* counters, double input_theta,
                     float* pr_x, float* pr_y, float* ign_pr_y, double* result, void* ws, int64_t ws_bytes, void* stream);

/* ---- edge-feature producer  GCGCN_glove.py:171-214 and the call sequence :300-330 ------------ */
/* Builds E = context_sent_att[B,N,N,Hd] -- the edge tensor the blocks above consume -- from the token states:
 * WordAttention (glove:171-190) on the head- and tail-side distance embeddings, Linear(2Hd, Hd) (linear_word_att),
 * SentenceAttention (glove:193-214) on the head- and tail-side node embeddings, Linear(2Hd, Hd) (linear_sentence_att).
 *   ctx[B,T,Hd]        token states (context_output, glove:292)
 *   sen[B,N,N,S,T]     uint8 / bool: token t belongs to sentence slot s of pair (i, j)   (sen_matrix)
 *   pos_h, pos_t       [B,N,N,S,T] distance ids 0..ND-1 (pos_matrix_h / _t), element width pos_bytes in {8, 4, 1}
 *   node[B,N,Hd]       entity features (node_feat);  dis_table[ND,P] = dis_embed.weight
 * Nothing of size [N,N,S,T,Hd] is materialised (the reference's 2.3 GB per document): the word score is a [ND,T] table per
 * document; only LIVE sentence slots -- those containing token 0, the only ones the reference's padding test
 * ~sen_matrix[...,0:1] (glove:305) does not zero out, forward and backward -- are computed, compacted into rows whose
 * count stays on the device.  The reference's divisor (number of PADDED slots + 1e-10, glove:205,212) is reproduced.
 * flat = [word_attention.attention_sent W,b | .attention_pos W,b | .attention_all w,b | linear_word_att W,b |
 *         sentence_attention.attention_sent W,b | .attention_pos W,b | .attention_all w,b | linear_sentence_att W,b],
 * every matrix in the reference's [out, in] layout; out17 = the 16 offsets + total.
 * Capacities: cap_rows >= live slots, cap_pairs >= pairs with a live slot (gcgcn_producer_count reports both; anything
 * beyond a capacity is NOT computed: ibuf[sizes[3] + 2] becomes 1 and every real pair of E is written as NaN, so an
 * undersized capacity is loud even inside a captured hipGraph).  Buffers (caller-owned): ibuf int32[sizes[0]], fbuf
 * float[sizes[1]] (written by forward, read by backward), bbuf float[sizes[2]] (backward workspace) from
 * gcgcn_producer_sizes.  Reproducibility: the forward is bit-reproducible.  In gcgcn_producer_bwd two small sums -- the
 * gradient of the per-entity node terms and of the sentence attention's vector / bias -- are scatter-added with fp32 atomics,
 * so dnode, dctx and dflat are reproducible up to summation order; every other sum (ctx, the score table, the weight
 * gradients) is computed by its owner in a fixed order.  gcgcn_producer_bwd_det computes those two sums by their owners
 * too (no float atomics anywhere): every output is bit-reproducible from run to run, for the dense and the compact entry. */
int gcgcn_producer_layout(int Hd, int P, int64_t* out17);
int gcgcn_producer_count(int B, int N, int S, int T, const uint8_t* sen, const int32_t* n_valid, int32_t* counts2, void* stream);
int gcgcn_producer_sizes(int B, int N, int S, int T, int Hd, int P, int ND, int64_t cap_rows, int64_t cap_pairs, int64_t* out7);
/* out7 = {ibuf elements, fbuf elements, bbuf elements, offset of int32 {live rows, live pairs, over capacity, 0} in ibuf,
 *         offset of pair_prow int32[B,N,N] in ibuf, offset of the compact rows Ec[rows, Hd] in fbuf, rows of Ec}
 * Compact mode: gcgcn_producer_fwd with E == NULL leaves E unwritten; the hop's graph blocks read Ec / pair_prow / the bias
 * of linear_sentence_att directly (gcgcn_*_compact below) and hand gcgcn_producer_bwd dEc instead of dE (dE == NULL; rows
 * of dEc beyond the live pairs must be zero; the bias gradient is produced by the consumers, not here). */
int gcgcn_producer_fwd(int B, int N, int S, int T, int Hd, int P, int ND, const float* ctx, const uint8_t* sen, const void* pos_h,
                       const void* pos_t, int pos_bytes, const float* node, const float* dis_table, const int32_t* n_valid,
                       const float* flat, int64_t cap_rows, int64_t cap_pairs, int32_t* ibuf, float* fbuf, float* scratch,
                       int64_t scratch_elems, float* E, void* stream);
/* dE[B,N,N,Hd] -> dctx[B,T,Hd], dnode[B,N,Hd], ddis_table[ND,P], dflat (layout of flat). */
int gcgcn_producer_bwd(int B, int N, int S, int T, int Hd, int P, int ND, const float* ctx, const uint8_t* sen, const void* pos_h,
                       const void* pos_t, int pos_bytes, const float* node, const float* dis_table, const int32_t* n_valid,
                       const float* flat, int64_t cap_rows, int64_t cap_pairs, int32_t* ibuf, float* fbuf, float* bbuf,
                       const float* dE, const float* dEc, float* dctx, float* dnode, float* ddis_table, float* dflat, void* stream);
/* The bit-reproducible backward (opt-in): the arguments and results of gcgcn_producer_bwd plus one workspace.  Each live pair's
 * wave stores its head- and tail-side node-term rows (dnpair[rows of Ec][2][Hd]) and each workgroup its partial of the attention
 * vector / bias gradient (2048 x (Hd + 1)); one wave per entity then sums its pairs' rows in pair-index order and one small
 * kernel sums the partials in a fixed order.  Three launches instead of one launch and two memsets; no host read, capturable.
 * *out of gcgcn_producer_det_elems (host; no GPU needed) = floats of detbuf = rows of Ec x 2 Hd + 2048 (Hd + 1), each piece
 * rounded up to 16 bytes.  detbuf must be non-null, 16-byte aligned and hold det_elems >= that many floats: anything else is
 * refused (gcgcn_last_error) before a kernel is launched.  Its contents need not be initialised and are not kept. */
int gcgcn_producer_det_elems(int B, int N, int Hd, int64_t cap_pairs, int64_t* out);
int gcgcn_producer_bwd_det(int B, int N, int S, int T, int Hd, int P, int ND, const float* ctx, const uint8_t* sen, const void* pos_h,
                           const void* pos_t, int pos_bytes, const float* node, const float* dis_table, const int32_t* n_valid,
                           const float* flat, int64_t cap_rows, int64_t cap_pairs, int32_t* ibuf, float* fbuf, float* bbuf,
                           const float* dE, const float* dEc, float* dctx, float* dnode, float* ddis_table, float* dflat,
                           float* detbuf, int64_t det_elems, void* stream);

/* ---- consumers of the compact rows: a hop's graph blocks without a dense E (compact.hip) -------------------------------
 * e_ij = Ec[prow[b,i,j]] where prow >= 0, else bias.  Mean-only hop (MultiGraphConvolution's edge term): Ebar = mean_j e_ij;
 * backward dEc[prow] = dEbar_i / n, dbias = sum (dead pairs of row)/n dEbar_i.  Attention hop: gcgcn_gat_fwd / _bwd with the
 * edge pass reading e_ij (no opt-in mask); dEc and dbias instead of dE.  rowbuf: float[2 B N]; scratch of the attention
 * backward: gcgcn_gat_bwd_compact_scratch(B,N,D) floats.  D <= 512.  Every sum in a fixed order. */
int gcgcn_edge_mean_fwd_compact(int B, int N, int D, const float* Ec, const int32_t* prow, const float* bias, const int32_t* n_valid,
                                float* Ebar, void* stream);
int gcgcn_edge_mean_bwd_compact(int B, int N, int D, const int32_t* prow, const int32_t* n_valid, const float* dEbar, float* dEc,
                                float* dbias, float* rowbuf, void* stream);
int gcgcn_gat_fwd_compact(int B, int N, int D, int Dh, const float* X, const float* Ec, const int32_t* prow, const float* bias,
                          const int32_t* n_valid, const float* flat, const void* rng_snap, float p, float* uvc, float* s, float* P,
                          float* A, float* Ebar, void* rng_state, void* rng_snaps, int rng_count, int uvc_valid, void* stream);
int64_t gcgcn_gat_bwd_compact_scratch(int B, int N, int D);
int gcgcn_gat_bwd_compact(int B, int N, int D, int Dh, const float* X, const float* Ec, const int32_t* prow, const float* bias,
                          const int32_t* n_valid, const float* flat, const void* rng_snap, float p, const float* uvc, const float* P,
                          const float* dA, const float* dEbar, const float* dX_in, float* dX, float* dEc, float* dbias, float* dflat,
                          float* dlogit, float* ds, float* dvpart, float* duvc, float* scratch, void* stream);

/* ---- classifier head  GCGCN_glove.py:306-307, 344-358 ------------------------------------------------ */
/* logits[B,N,N,R] = bili_layer_01(eh, et) + classification_layer_01(cat(eh, et)) with
 *   eh[i,j] = tanh(dense_layer(cat(feats[j], ner_emb[type[j]], dis_embed[dis_plus + rel[i,j]])))   (column entity)
 *   et[i,j] = tanh(dense_layer(cat(feats[i], ner_emb[type[i]], dis_embed[dis_plus - rel[i,j]])))   (row entity)
 * feats: host array of nf device pointers, the model's node_feats list (each [B,N,Hd]); node_type int64[B,N] in 0..6;
 * node_relative_pos int64[B,N,N]; ner_emb[7,Pt] (padding_idx 0: its row 0 gets no gradient), dis_table[ND,Pr].
 * The hidden width of eh / et is 128 (hard-coded in the reference, glove:234); R <= 128.
 * flat = [dense_layer W [128, nf Hd + Pt + Pr] | b | classification_layer_01 W [R,256] | b | bili_layer_01 b [R] |
 *         bili_layer_01 W [R,128,128]], pieces 16-byte aligned; out7 = 6 offsets + total.
 * The bilinear form runs on the fp32 MFMA with the per-pair outer product eh (x) et generated in registers: no
 * [pairs, 16384] operand and no [N,N,F] concatenations exist.  Buffers: fbuf float[sizes[0]] (forward, kept for backward),
 * bbuf float[sizes[1]] (backward workspace), ibuf int32[sizes[2]] (pair index of a ragged batch; only touched when n_valid is
 * given) from gcgcn_head_sizes.  Deterministic (no atomics).
 * n_valid (ABI v5): the reference runs these lines on ONE unpadded document (n x n pairs).  With n_valid the pair passes run on
 * the pairs that exist only -- rows of eh / et / their gradients compacted on the device (row off[b] + i n_b + j, off = prefix
 * sums of n_b^2; no host read, capturable), 2 x 128 x 128 x R flops per existing pair and pass instead of per pair slot of the
 * padded batch -- and logits of pairs with a padding entity are exactly zero.  n_valid == NULL: every slot is computed.
 * Padding contents: node_type / node_relative_pos of padding slots may hold any id in range, dlogits of padding pairs anything
 * (NaN included); no real result depends on them, and dfeats of padding entities are exactly zero.  The feats rows of padding
 * entities must be FINITE: the dense layer's weight gradient is dUT^T feats over all B N rows with dUT exactly zero on the
 * padding rows (0 x finite = 0, 0 x NaN = NaN), and for R outside 65..97 every pair slot is computed from them.
 * dis_table: 2 dis_plus + 1 <= ND <= 32 rows (the backward pass keeps one table of partial sums per id in LDS); both entry
 * points refuse more. */
int gcgcn_head_layout(int Hd, int nf, int Pt, int Pr, int R, int64_t* out7);
int gcgcn_head_sizes(int B, int N, int R, int ND, int64_t* out3);
int gcgcn_head_fwd(int B, int N, int Hd, int nf, int Pt, int Pr, int R, int ND, int dis_plus, const float* const* feats,
                   const int64_t* node_type, const int64_t* node_relative_pos, const float* ner_emb, const float* dis_table,
                   const int32_t* n_valid, const float* flat, float* fbuf, int32_t* ibuf, float* logits, void* stream);
/* dlogits[B,N,N,R] (entries of padding entities ignored when n_valid is given) -> dfeats (nf pointers, [B,N,Hd] each),
 * dner_emb[7,Pt], ddis_table[ND,Pr], dflat.  n_valid / fbuf / ibuf: the forward call's. */
int gcgcn_head_bwd(int B, int N, int Hd, int nf, int Pt, int Pr, int R, int ND, int dis_plus, const float* const* feats,
                   const int64_t* node_type, const int64_t* node_relative_pos, const float* ner_emb, const float* dis_table,
                   const int32_t* n_valid, const float* flat, float* fbuf, int32_t* ibuf, float* bbuf, const float* dlogits,
                   float* const* dfeats, float* dner_emb, float* ddis_table, float* dflat, void* stream);
/* Opt-in bf16 operands for the four bilinear passes (csrc/head_bf16.hip): the call takes one more
 * argument, matmul (0 = fp32, 1 = bf16), which travels beside the argument list: gcgcn_set_option("head_matmul", v) hands v to the
 * calling THREAD's next gcgcn_head_fwd / gcgcn_head_bwd / gcgcn_debug_head_plan call, which takes it (whatever it then returns) and
 * leaves 0 behind.  A call that was not announced runs fp32, exactly as before: the value is per thread and per call, no environment
 * variable is read, no other thread sees it and nothing lasting selects the arithmetic.  Any value but 0 and 1 is refused by the call
 * that takes it, before a launch.  Both calls of a pair are announced with the same value.  The argument lists, the buffers and their
 * sizes do not change.  (Entry points with matmul in their own argument list would be the plainer interface; none is added here.)
 * With 1 the forward pass, d eh, d et and d W_b /
 * d W_c run on v_mfma_f32_32x32x16_bf16 -- the generated operand (eh[p,a] et[p,b]; dout[p,r] et[p,b]; dout[p,r] eh[p,a]) is an fp32
 * product rounded once to bf16 (nearest even), eh | et, dout and the weights are rounded once on their way into the instruction, every
 * sum is fp32, the bias is added unrounded and its gradient is the column sum of the unrounded dlogits
 * (gcgcn_amd.functional.Bf16HeadBilinearFn is the definition).  Everything else -- the dense layer, the tables, tanh and its backward,
 * the compaction -- is the fp32 code; no bf16 copy of a weight exists in memory, the padding contract above holds, no float is added
 * atomically and both calls are capturable. */

/* ---- device-side tensorisation of packed documents  config/Config.py:162-233 -------------------------- */
/* Expands the packed records of a batch (gcgcn_amd/data.py; all int32, device memory) into the dense inputs of the
 * reference's forward, batched and padded to (N entities, S sentence slots, T tokens), in ONE launch.  Outputs must be
 * zero-filled by the caller.
 *   slots[n_slots][10]   doc, u, v, slot j, sentence start, end, head mention start, end, tail mention start, end
 *                        -> sen[B,N,N,S,T] (uint8 0/1), pos_h / pos_t [B,N,N,S,T] (uint8 distance ids: dis_plus +- the
 *                        bucket dis2idx of the distance to the head / tail mention, Config.py:106-116, 190-203)
 *   edges[n_edges][3]    doc, u, v -> adj[B,N,N] = 1                                     (Config.py:183)
 *   labels[n_labels][4]  doc, h, t, r -> label_matrix[B,N,N,R] = 1
 *   mentions[n][2], mention_node[n][4] = (doc, entity, mentions of that entity, index inside the entity), sorted by
 *                        (doc, entity, index) -> node_pos[B,N,T] (each mention span ASSIGNED 1 / length in order, the row
 *                        scaled by 1 / mentions, float64 arithmetic, Config.py:170-175) and node_relative_pos[B,N,N]
 *                        (signed bucket of the difference of the first mention starts, Config.py:206-215)
 *   n_valid[B]           entities per document;  first_start[B,N] start of each entity's first mention */
int gcgcn_tensorise(int B, int N, int S, int T, int R, int dis_plus, int n_slots, const int32_t* slots, int n_edges,
                    const int32_t* edges, int n_labels, const int32_t* labels, int n_mentions, const int32_t* mentions,
                    const int32_t* mention_node, const int32_t* n_valid, const int32_t* first_start, float* adj, uint8_t* sen, uint8_t* pos_h,
                    uint8_t* pos_t, float* node_pos, int64_t* node_relative_pos, float* label_matrix, void* stream);

/* ---- test hook: how tile passengers are placed among the rows of a carrying launch (csrc/common.hpp Spread) ---------
 * kind[x] / ordinal[x] for every workgroup index x < n_tiles + n_others: 1 / tile number or 0 / row number.  Host-only. */
int gcgcn_debug_spread(int64_t n_tiles, int64_t n_others, int64_t cohort, int64_t pct, int32_t* kind, int32_t* ordinal);

/* ---- test hook: which chain kernel a gcgcn_gcn_fwd (bwd = 0) / gcgcn_gcn_bwd (bwd = 1) call of this shape gets -------
 * Evaluates the plan function the two entry points call (csrc/chain.hip chain_plan_fwd / _bwd) under the current options.
 * ragged: n_valid given; ride / hook / scratch: those arguments given; misalign: bit 0 the per-(document, head) tensors,
 * bit 1 dout / dXres / dout_m, bit 2 the ride's in / out, bit 3 flat are NOT 16-byte aligned.
 * out[6] = kind (0 one launch per product, 1 generic chain kernels, 2 gcn_chain_s_*, 3 gcn_chain_t_*), aligned (kind 1),
 * full (kind 3), fuse (backward computes dHO / dXres), attention (forward runs the core), ride (the edge pass is a
 * passenger of the chain launch).  Host-only. */
int gcgcn_debug_chain_plan(int bwd, int B, int N, int D, int L, int H, int ragged, int ride, int hook, int scratch,
                           int misalign, int32_t* out);

/* ---- test hook: which kernels a gcgcn_head_fwd / gcgcn_head_bwd call of this shape gets ------------------------------
 * Evaluates the plan function the two entry points call (csrc/head.hip head_plan) under the current options.  ragged: n_valid
 * given.  out[6] = compact (the pair passes run on the pairs that exist), the forward pass and the d eh / d et passes (0
 * head_gemm_kernel, 1 head_bil2_kernel: 64-pair tiles, 2 head_bil3_kernel: 128-pair tiles), d W_b (0 head_gemm_kernel<4>, 1
 * head_dw_kernel), then for the forward and the d eh / d et passes whether both launch shapes are issued and the device-side
 * pair count selects one.  A call announced with gcgcn_set_option("head_matmul", 1) (see gcgcn_head_fwd; this call takes the
 * announcement like a head call) answers 3, 3, 2 for the kernels (head_bf16_pass_kernel for the passes, head_bf16_dw_kernel for d W_b
 * and d W_c; one launch of 128-pair tiles per pass, so the last two answers are 0); announced with any other value but 0 it fails.
 * Not announced, its answers are what they were.  Host-only. */
int gcgcn_debug_head_plan(int B, int N, int R, int ragged, int32_t* out);

/* ---- test hook: which launch a pass over the edge tensor gets ----------------------------------------------------------
 * Evaluates the plan functions the edge launchers call (csrc/edge_plan.hpp, csrc/edge.hip: edge_plan_fwd / _bwd / _bcast, then
 * edge_plan_carry with what the defer queue would hand over).  pass: 0 forward, 1 backward, 2 the mean's backward alone; compact:
 * the producer's compact rows instead of a dense E; att: GATAttention's pass (forward: P is wanted; backward: a logit gradient
 * comes in -- a dense backward always has one); has_dE / has_dEbar: those operands given; misalign: bit 0 E, bit 1 v, bit 2 dE,
 * bit 3 dEbar, bit 4 Ebar are NOT 16-byte aligned; parked_tiles: tile workgroups parked in the queue (0: nothing), any_rb: one of
 * them walks row blocks, col_C: columns of a parked column-sum second stage (0: none).  ragged is accepted and decides nothing.
 * out[17] = vec (4 / 1), att, dlogit route (0 passengers of the edge pass, 1 one gat_dlogit launch, 2 three launches), slices,
 * ngat, dynamic LDS bytes, lds_ok, carry_ok, RB, grid, col_base, ncolwg, the Spread's na / cohort / stride, scratch floats, offset of
 * the compact row buffer in them.  -1: does not apply.  Host-only. */
int gcgcn_debug_edge_plan(int pass, int compact, int B, int N, int D, int ragged, int att, int has_dE, int has_dEbar, int misalign,
                          int parked_tiles, int any_rb, int col_C, int32_t* out);

/* ---- test hook: where the core of MultiHeadAttention runs ---------------------------------------------------------------
 * Evaluates the plan functions gcgcn_mha_fwd / gcgcn_mha_bwd (hook = 0) and gcgcn_gcn_fwd / gcgcn_gcn_bwd with a gcgcn_mha_hook
 * (hook = 1) call (csrc/attn_plan.hpp, csrc/mha_core.hip: attn_plan_fwd / _bwd) under the current "mha_core" option.
 * chain_attends: the forward hook's chain kernel runs the core (gcgcn_debug_chain_plan's attention); core_done: gcgcn_mha_bwd's;
 * misalign bit 0 puts Q off a 16-byte boundary, bit 1 dQ.  out[4] = route (0 batched GEMMs + softmax, 1 a mha_core launch, 2 the
 * chain workgroups' prologue, 3 passengers of the convolution's last group launch, 4 nothing: dQ arrived), the head-feature chunk
 * of that route's kernel (0: none), gcgcn_maggc_fusable, refused (0; a hook the entry point fails on: 1 a shape the core does not
 * serve, 2 a misaligned Q / dQ -- route and chunk are then -1).  Host-only. */
int gcgcn_debug_attn_plan(int bwd, int N, int D, int H, int hook, int chain_attends, int core_done, int misalign, int32_t* out);

/* ---- test hook: the output stage of the convolution's backward -----------------------------------------------------------
 * Evaluates the two plan functions gcgcn_gcn_bwd calls for its output projection's backward (csrc/gcn_plan.hpp: OutBwdPlan,
 * OutBwdCol2; csrc/api.hip: out_bwd_plan, out_bwd_plan_col2).  fuse: gcgcn_debug_chain_plan's; scratch, wsum_fwd, ragged (n_valid),
 * odrop (output dropout) and drop (the block's dropout): whether the call has them; dxres_misaligned: dXres off a 16-byte boundary;
 * front_reduced: the group launch in front of the chain had a split-K reduce (not read where there is no such launch).
 * out[10] = mask (0 none, 1 a mask_rows launch, 2 in the chain), wsum (0 none, 1 the forward call's, 2 summed here), fold (0 none,
 * 1 one head, 2 several heads), fold_drop, head_sum_launch, dwlin (0 offered in front of the chain, 1 behind it), col1 (stage 1 of
 * the dblin column sums: 0 in the chain, 1 the front launch, 2 the back launch, 3 a colsum launch of its own), the slices the chain
 * leaves (2 B, else 0); then col2 (stage 2: 0 the front launch's reduce, 1 trailing workgroups of head_sum_drop_bwd, 2 of the back
 * launch, 3 the back launch's reduce, 4 done with stage 1) and the slices the back launch's ride sums (else 0).  fuse without
 * scratch fails, as in gcgcn_gcn_bwd.  Host-only. */
int gcgcn_debug_out_bwd_plan(int fuse, int B, int N, int D, int H, int scratch, int wsum_fwd, int ragged, int odrop, int drop,
                             int dxres_misaligned, int front_reduced, int32_t* out);

/* ---- test hook: what the GEMM launcher decides for a problem ----------------------------------------------------------
 * Evaluates the plan function every launcher of csrc/gemm.hip calls (gemm_plan) under the current options, on made-up operand
 * addresses.  form: 0 a single launch (splits: the caller's request), 1 a member of a group launch of group_work tile-k-steps,
 * 2 parking, 3 / 4 M / K is a device-side count of at most cap; 5, 6, 7: the pairs gemm_dyn_pair, _ww, _xx over prob_a and prob_b.
 * A problem is int64[13]: M, N, K, a_kc, b_kc, lda, ldb, ldc, batch1, batch2, row-block mode, workspace elements (0: none),
 * misalign (bit 0 A, bit 1 B, bit 2 the workspace are NOT 16-byte aligned).
 * out[26]: for prob_a in out[0..11], for a pair's prob_b in out[12..23]: ok, interior, splits, ksplit, widen, kept row-block mode,
 * vecA, vecB, tiles, reduce launch, zero-fill launch, grid of a device-side form (a pair that is not fused: the plans of the two
 * gemm_dyn calls that run instead); out[24] = the pair runs fused, out[25] = its gridW.  -1: does not apply.  Host-only. */
int gcgcn_debug_gemm_plan(int form, const int64_t* prob_a, const int64_t* prob_b, int splits, int64_t group_work, int64_t cap,
                          int32_t* out);

/* ---- test hook: run what the GEMM launcher launches -------------------------------------------------------------------
 * The run-side twin of gcgcn_debug_gemm_plan: n <= 40 problems are built from flat rows with the named constructors of csrc/gemm.hpp
 * and handed to the launchers the library itself calls.  form: 0 gemm() on each problem with the caller's tile / splits; 1 one
 * gemm_group launch over all n (n = 0 with a ride: the ride alone); 2 gemm_defer of each problem into a DeferQueue local to the
 * call -- a problem that is refused runs through gemm() at once, as the library's callers do -- then gemm_flush_deferred; 5, 6, 7
 * gemm_dyn_pair, _ww, _xx over problems 0 and 1 on the device-side count *cnt <= cap (the numbering of gcgcn_debug_gemm_plan).
 * Problem i is
 *   probs + 40 i, int64[40]: [0..12] the 13 integers of gcgcn_debug_gemm_plan in their order (M, N, K, a_kc, b_kc, lda, ldb, ldc,
 *     batch1, batch2, row-block mode, workspace ELEMENTS, unused); [13..18] sA1, sA2, sB1, sB2, sC1, sC2; [19..21] ldadd, sAdd1,
 *     sAdd2; [22..25] sRa1, sRa2, sRs1, sRs2; [26..28] ldc2, sC21, sC22; [29..31] ldadd2, sAdd21, sAdd22; [32] relu; [33] accumulate;
 *     [34] nv_rows; [35] nv_zdoc; [36] rb_zero; [37] drop_base; [38] the dropout salt; [39] unused;
 *   scal + 2 i, float[2]: alpha, dropout p (0: no dropout);
 *   ptrs + 14 i, 14 device pointers: A, B, C, add, bias, rowadd, rowscale, C2, add2, n_valid, rb, rb_n, ws, rng_snap (all but the
 *     first three may be NULL; rb / rb_n are gcgcn_row_blocks' out + 4 / out and are required when the row-block mode is not 0).
 * ride (form 1; NULL or ride[0] = 0: nothing rides), int64[6]: kind (1 col_sum, 2 col_sum(...).stage2(slices), 3 head_sum), R (head_sum:
 * H), ld (head_sum: D), C, slices, and whether gemm_group is given a col_later to report into; ride_ptrs: X (head_sum: W), out, part.
 * out, int32[2 + 2 n]: out[0] the return code of the launch (form 0: the first failing gemm(); form 2: of the flush), out[1] whether
 * col_later was set, and per problem out[2 + 2 i] whether gemm_defer accepted it and out[3 + 2 i] the return code of its own gemm()
 * call; -1: does not apply.  Returns the first non-zero code.  Allocates nothing and reads no device memory on the host. */
int gcgcn_debug_gemm_run(int form, int n, const int64_t* probs, const float* scal, const void* const* ptrs, const int64_t* ride,
                         const void* const* ride_ptrs, int tile, int splits, const int32_t* cnt, int64_t cap, int32_t* out, void* stream);

/* ---- raw batched GEMM (exposed for unit tests and benchmarks of the MFMA kernel) ----------- */
/* C[z] = alpha * opA(A[z]) opB(B[z]);  a_kc: A stored [M][K] else [K][M];  b_kc: B stored [N][K]
 * else [K][N];  z < batch with element strides sA, sB, sC;  tile: 0 or 1 = 64x64 block tiles (the only body; other values are refused);
 * splits: 0 auto, 1 none, n = split K n ways through ws[ws_elems] (>= n*batch*M*N floats);
 * bias[N] optional, relu/accumulate flags. */
int gcgcn_gemm(int M, int N, int K, const float* A, int64_t lda, int a_kc, const float* B, int64_t ldb, int b_kc,
               float* C, int64_t ldc, int batch, int64_t sA, int64_t sB, int64_t sC, float alpha, const float* bias,
               int relu, int accumulate, int tile, int splits, float* ws, int64_t ws_elems, void* stream);

/* The same product with ONE dimension read from device memory (exposed for unit tests; used by the edge-feature producer for
 * its compacted rows): dyn = 1: M = *count, dyn = 2: K = *count (the M / K argument is ignored); cap = a host-side upper bound of
 * *count.  Interior shapes run the unguarded tile body on the count rounded up to 64: operand buffers must be readable (C
 * writable, dyn = 1) that far, and for dyn = 2 at least one operand's rows in [*count, roundup64) must be zero. */
int gcgcn_gemm_dyn(int M, int N, int K, const float* A, int64_t lda, int a_kc, const float* B, int64_t ldb, int b_kc, float* C,
                   int64_t ldc, const float* bias, int accumulate, const int32_t* count, int dyn, int64_t cap, float* ws,
                   int64_t ws_elems, void* stream);

/* ---- the trainer's optimiser step (config/Config.py:300, 372-373: torch.optim.Adam, no weight decay) -------------------
 * ONE launch over n_tensors parameter tensors.  table (device memory): n_tensors records of 56 bytes
 *   { float* p; const float* g; float* m; float* v; int64 numel; int64 block_begin; float step_size; float inv_bc2_sqrt; }
 * sorted by block_begin, where a tensor owns ceil(numel / 1024) consecutive workgroups starting at block_begin,
 * step_size = lr / (1 - beta1^t) and inv_bc2_sqrt = 1 / sqrt(1 - beta2^t) with t the tensor's own step count (torch skips a
 * parameter whose .grad is None and does not advance its t).  Arithmetic as torch.optim.Adam's single-tensor path. */
int gcgcn_adam_step(int n_tensors, const void* table, int64_t total_blocks, double beta1, double beta2, double eps, void* stream);

/* The same step with everything that changes from step to step read on the device, so that a hipGraph which holds the call
 * trains when it is replayed.  The table keeps its 56-byte records, but their last 8 bytes are `float* step`: the tensor's own
 * step counter, an fp32 device scalar (torch.optim.Adam(capturable=True)'s state["step"]).  One call, on `stream`:
 *   1. max_norm > 0 only: total = sqrt(sum g^2) over every element of every tensor of the table (fp32, one partial per
 *      workgroup in ws, added in a fixed order: bit-reproducible, no float atomics); *grad_norm = total (the norm BEFORE
 *      clipping; grad_norm may be NULL); coef = min(1, max_norm / (total + 1e-6)), torch.nn.utils.clip_grad_norm_'s formula.
 *      A non-finite norm propagates into the parameters (torch's error_if_nonfinite=False).
 *   2. per tensor: *step += 1; step_size = *lr / (1 - beta1^t) and inv_bc2_sqrt = 1 / sqrt(1 - beta2^t) in double, rounded to
 *      fp32, into ws.  lr is an fp32 device scalar.
 *   3. gcgcn_adam_step's update with g * coef in place of g.  The gradients themselves are NOT modified.
 * At most three launches (two when max_norm <= 0); no host read, no allocation, no stream synchronisation.  ws: device memory,
 * 16-byte aligned, ws_bytes >= gcgcn_adam_ws_bytes(n_tensors, total_blocks); its contents need not survive between calls. */
int64_t gcgcn_adam_ws_bytes(int n_tensors, int64_t total_blocks);
int gcgcn_adam_step_dev(int n_tensors, const void* table, int64_t total_blocks, double beta1, double beta2, double eps,
                        const float* lr, double max_norm, void* ws, int64_t ws_bytes, float* grad_norm, void* stream);

/* ---- the token encoder's LSTM layer (EncoderLSTM, glove:377-428) ----------------------------------------------------------
 * One nn.LSTM(I, H, 1, batch_first=True) layer with nd = 1 or 2 directions over ALL T padded steps, gate order i, f, g, o,
 * gates = x W_ih^T + b_ih + h W_hh^T + b_hh.  H = 128 is served; any other width is refused.  The directions' parameters are
 * stacked: w_ih [nd * 4H][I], w_hh [nd * 4H][H], bias [nd * 4H] = b_ih + b_hh; h0 / c0 [nd][B][H]; x [B][T][I].
 * gcgcn_lstm_fwd: out [B][T][nd * H]; gates [B * T][nd * 4H] is always needed (the input projection); with csave [B][T][nd * H]
 * given, gates ends up holding the activated gates and csave the cell states, which is what gcgcn_lstm_bwd reads; csave = NULL
 * (no-grad / eval) keeps nothing.  One GEMM launch + one recurrence launch.
 * gcgcn_lstm_bwd: dout [B][T][nd * H] (must not alias out) -> dgates [B * T][nd * 4H] (scratch the caller owns), dx [B][T][I],
 * dw_ih / dw_hh / db stacked like the parameters (db is the gradient of b_ih and of b_hh), dh0 / dc0 [nd][B][H] PER BATCH ROW
 * (a broadcast initial state sums them over B).  ws: 16-byte aligned, gcgcn_lstm_ws_bytes(B, T, I, H, nd) bytes (-1: refused).
 * No workgroup waits for another and nothing is added atomically: results are bit-reproducible.  Capturable.
 * gcgcn_lstm_fwd_len / gcgcn_lstm_bwd_len: the same calls with per-row lengths, lens = device int32 [B] or NULL (NULL: every row
 * has length T; gcgcn_lstm_fwd / gcgcn_lstm_bwd are these with NULL).  The semantics are those of a packed sequence padded back to
 * T: row b is active at time t iff t < lens[b]; an inactive step leaves the row's h and c as they are; the reverse direction of row
 * b takes its first step at t = lens[b] - 1 from h0 / c0.  The kernels clamp every length into [0, T] (callers check the range;
 * a bad value cannot address out of bounds).  Written: EVERY element of out (exactly 0 at t >= lens[b]) and, in the backward, of
 * dgates (0 there, hence dx exactly 0 there), dx, the parameter gradients, dh0, dc0; no memset is needed.  gates and csave are NOT
 * written at inactive steps, and the backward lets neither them nor dout at those positions reach any result (NaN included).
 * x must be finite at padded positions (it is multiplied by the zero dgates).  Both calls of a pair take the same lens.
 * The four calls take one more argument, recurrent (0 = fp32, 1 = bf16), which travels beside the argument list as the head's
 * matmul does: gcgcn_set_option("lstm_recurrent", v) hands v to the calling thread's NEXT gcgcn_lstm_fwd / _fwd_len / _bwd /
 * _bwd_len, which takes it first -- whatever it then returns -- and leaves 0 behind: no environment variable, nothing lasting,
 * another thread never sees it, and a call nobody announced runs fp32 exactly as before.  Any value but 0 and 1 is refused
 * (gcgcn_last_error).  With 1 the two recurrent products take bf16 operands on the bf16 matrix cores and accumulate in fp32, r(.)
 * being one rounding to bf16, nearest even:  forward  gates_t = (x_t W_ih^T + bias) + r(h_{t-1}) r(W_hh)^T  (h0 is rounded like any
 * other h);  backward  dh_rec = r(dgates_t) r(W_hh).  Nothing stored is rounded: out, gates, csave and dgates are the fp32 values, the
 * input projection and dw_ih / dw_hh / dx / db are the same fp32 products on them, and lens means what it means above.  Both calls
 * of a pair take the same recurrent.  gcgcn_lstm_ws_bytes does not depend on it. */
int64_t gcgcn_lstm_ws_bytes(int B, int T, int I, int H, int nd);
int gcgcn_lstm_fwd(int B, int T, int I, int H, int nd, const float* x, const float* w_ih, const float* w_hh, const float* bias,
                   const float* h0, const float* c0, float* out, float* gates, float* csave, void* stream);
int gcgcn_lstm_bwd(int B, int T, int I, int H, int nd, const float* x, const float* w_ih, const float* w_hh, const float* h0,
                   const float* c0, const float* out, const float* gates, const float* csave, const float* dout, float* dgates,
                   float* dx, float* dw_ih, float* dw_hh, float* db, float* dh0, float* dc0, void* ws, int64_t ws_bytes, void* stream);
int gcgcn_lstm_fwd_len(int B, int T, int I, int H, int nd, const float* x, const float* w_ih, const float* w_hh, const float* bias,
                       const float* h0, const float* c0, float* out, float* gates, float* csave, const int* lens, void* stream);
int gcgcn_lstm_bwd_len(int B, int T, int I, int H, int nd, const float* x, const float* w_ih, const float* w_hh, const float* h0,
                       const float* c0, const float* out, const float* gates, const float* csave, const float* dout, float* dgates,
                       float* dx, float* dw_ih, float* dw_hh, float* db, float* dh0, float* dc0, void* ws, int64_t ws_bytes,
                       const int* lens, void* stream);

/* ---- the token front end, either side of the BiLSTM (glove:282-298, bert:275-290) -------------------------------------------
 * Embeddings.  x [B][T][I], I = Dw + Dc + Dn, = word_emb[document] | entity_embed[document_pos] | ner_emb[document_ner] in that
 * column order; tables word_w [V][Dw], coref_w [P][Dc], ner_w [R][Dn]; ids int64 [B][T] inside their table (the caller checks:
 * an id outside its table reads zeros and adds to no gradient).  scale [B][I] or NULL: every element is multiplied by
 * scale[b][i], the locked-dropout factor shared by all T steps.  Without a scale x is a plain copy of the table rows.
 * gcgcn_embed_bwd: dx [B][T][I] (and the same scale) -> dword [V][Dw], dcoref [P][Dc], dner [R][Dn], every row written, zeros
 * included (no memset is needed); the row at coref_padding_idx / ner_padding_idx (-1: none) is exactly zero, word_emb has no
 * padding row.  Each row is summed by one owner in ascending token position b * T + t, in pieces of at most 32 tokens inside
 * chunks of 256 consecutive tokens, the pieces added in ascending position.  Three launches and a memset of the workspace's
 * flags; the workspace's contents need not survive between calls.
 * Context.  gcgcn_context_fwd: h [B][T][K], w [Hd][K], bias [Hd], node_pos [B][N][T] -> ctx [B][T][Hd] = tanh(h w^T + bias) and
 * node_feat [B][N][Hd] = sum_t node_pos[b][n][t] ctx[b][t][:] in ascending t over the non-zeros of the row (a row of zeros
 * gives zeros).  pre [B][T][Hd] is scratch the caller owns (the product before the tanh; it must not alias ctx).  One GEMM
 * launch + one launch.  gcgcn_context_bwd: dctx [B][T][Hd], dnode_feat [B][N][Hd] -> dpre [B][T][Hd] (scratch the caller owns)
 * = (dctx + sum_n node_pos[b][n][t] dnode_feat[b][n][:], ascending n) (1 - ctx^2), then dh [B][T][K], dw [Hd][K], db [Hd]:
 * one launch + one GEMM group launch (+ its split-K reduce).  node_pos gets no gradient.  Hd = 128 is served.
 * ws: 16-byte aligned, gcgcn_frontend_ws_bytes bytes: enough for gcgcn_embed_bwd at these tables (V = 0: leave them out) and
 * for gcgcn_context_bwd at inner width K (K = 0: leave it out); -1: refused.
 * Refused before anything is launched: a null pointer (scale excepted), B, T, N, K, a table's rows or a width below 1,
 * Hd != 128, a workspace that is too small or not 16-byte aligned, pre or ctx not 16-byte aligned.
 * No workgroup waits for another, no float is added atomically: results are bit-reproducible.  Capturable. */
int64_t gcgcn_frontend_ws_bytes(int B, int T, int V, int P, int R, int Dw, int Dc, int Dn, int K);
int gcgcn_embed_fwd(int B, int T, int V, int P, int R, int Dw, int Dc, int Dn, const int64_t* document, const int64_t* document_pos,
                    const int64_t* document_ner, const float* word_w, const float* coref_w, const float* ner_w, const float* scale,
                    float* x, void* stream);
int gcgcn_embed_bwd(int B, int T, int V, int P, int R, int Dw, int Dc, int Dn, const int64_t* document, const int64_t* document_pos,
                    const int64_t* document_ner, const float* dx, const float* scale, int coref_padding_idx, int ner_padding_idx,
                    float* dword, float* dcoref, float* dner, void* ws, int64_t ws_bytes, void* stream);
int gcgcn_context_fwd(int B, int T, int N, int K, int Hd, const float* h, const float* w, const float* bias, const float* node_pos,
                      float* pre, float* ctx, float* node_feat, void* stream);
int gcgcn_context_bwd(int B, int T, int N, int K, int Hd, const float* h, const float* w, const float* node_pos, const float* ctx,
                      const float* dctx, const float* dnode_feat, float* dpre, float* dh, float* dw, float* db, void* ws,
                      int64_t ws_bytes, void* stream);

/* ---- the BERT encoder layer (pytorch_pretrained_bert 0.6 BertLayer; bert.hip) --------------------------
 * Attention core on PACKED qkv [B][T][3 D], D = H * dh: row (b, t) holds q | k | v, head h in columns [dh h, dh h + dh) of each.
 *   S = q k^T / sqrt(dh) + key_bias[b][key]      key_bias [B][T] (the additive penalty, finite) or NULL
 *   P = dropout(softmax over keys of S)          element (b, h, i, j) draws index ((b H + h) T + i) T + j of site (rng_snap, salt)
 *   ctx [B][T][D] = P v, heads concatenated;  lse [B][H][T] = log sum_j exp(S_ij - c_b), c_b = max_j key_bias[b][j] (0 without
 *   key_bias): the log-sum-exp of the row is lse + c_b.  The kernels subtract c_b from the penalties first (a softmax does not see a
 *   shift common to its keys), so a document whose keys are ALL masked keeps the scores' low bits.
 * gcgcn_bert_attn_bwd: dctx [B][T][D] -> dqkv [B][T][3 D] = dq | dk | dv; delta: [B][H][T] floats of scratch.  P is recomputed from q, k
 * and lse, the dropout decisions from the same (rng_snap, salt, p); no [T][T] tensor is written to memory in either direction.
 * dh = 64 and T <= 512 are served; anything else is refused (gcgcn_last_error).  rng_snap may be NULL when p = 0.
 * y = LayerNorm(dropout(x + bias) + res) over rows of D (a multiple of 64, <= 1024), biased variance, eps = 1e-12: bias [D], res
 * [rows][D] and the dropout (p = 0) are each optional; dropout index = row D + col.  mean / rstd [rows]: both or neither; the
 * backward needs them.  gcgcn_res_ln_bwd: dx (the gradient of x; its column sums are the gradient of bias), dres (or NULL),
 * dweight / dlnb [D] by a two-stage column sum in a fixed order through ws (gcgcn_res_ln_ws_bytes(D) bytes).
 * y = gelu(x + bias[col]) with gelu(z) = z / 2 (1 + erf(z / sqrt 2)), C a multiple of 4, bias [C] or NULL; dx may alias dy.
 * One encoder layer.  params / grads: HOST arrays of GCGCN_BERT_LAYER_PARAMS device pointers, in this order (Linear weights [out][in]):
 *   wqkv [3 D][D] (query | key | value stacked), bqkv [3 D], attention.output.dense weight [D][D], bias [D], attention.output.LayerNorm
 *   weight, bias [D], intermediate.dense weight [Dff][D], bias [Dff], output.dense weight [D][Dff], bias [D], output.LayerNorm weight, bias.
 * x, y, dy, dx [B][T][D].  saved: gcgcn_bert_layer_ws_bytes(..., 0) bytes the forward fills and the backward reads (7 D + 2 Dff + H + 4
 * floats per token, beside the layer's input x); ws: gcgcn_bert_layer_ws_bytes(..., 1) bytes of scratch for the backward.  -1: the shape is refused.  Three dropout
 * sites with salts of their own draw from one rng_snap: P (p_attn), the two Linear outputs in front of the LayerNorms (p_hidden).
 * Nothing is allocated, the host never waits: capturable.  No float is added atomically: results are bit-reproducible. */
#define GCGCN_BERT_LAYER_PARAMS 12
#define GCGCN_SALT_BERT_ATTN 0x42415431ull
#define GCGCN_SALT_BERT_AO 0x42414f31ull
#define GCGCN_SALT_BERT_OUT 0x424f5531ull
#define GCGCN_SALT_BERT_EMB 0x42454d31ull /* the embeddings' dropout, after their LayerNorm (gcgcn_amd.BertModel: gcgcn_dropout) */
int gcgcn_bert_attn_fwd(int B, int T, int H, int dh, const float* qkv, const float* key_bias, float* ctx, float* lse, const void* rng_snap,
                        uint64_t salt, float p, void* stream);
int gcgcn_bert_attn_bwd(int B, int T, int H, int dh, const float* qkv, const float* key_bias, const float* ctx, const float* lse,
                        const float* dctx, float* dqkv, float* delta, const void* rng_snap, uint64_t salt, float p, void* stream);
int64_t gcgcn_res_ln_ws_bytes(int D);
int gcgcn_res_ln_fwd(int64_t rows, int D, const float* x, const float* bias, const float* res, const float* weight, const float* lnb,
                     float* y, float* mean, float* rstd, const void* rng_snap, uint64_t salt, float p, void* stream);
int gcgcn_res_ln_bwd(int64_t rows, int D, const float* dy, const float* x, const float* bias, const float* res, const float* weight,
                     const float* mean, const float* rstd, float* dx, float* dres, float* dweight, float* dlnb, void* ws, int64_t ws_bytes,
                     const void* rng_snap, uint64_t salt, float p, void* stream);
int gcgcn_bias_gelu_fwd(int64_t rows, int C, const float* x, const float* bias, float* y, void* stream);
int gcgcn_bias_gelu_bwd(int64_t rows, int C, const float* dy, const float* x, const float* bias, float* dx, void* stream);
int64_t gcgcn_bert_layer_ws_bytes(int B, int T, int D, int H, int Dff, int which);
int gcgcn_bert_layer_fwd(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const float* const* params, float* y,
                         void* saved, int64_t saved_bytes, const void* rng_snap, float p_attn, float p_hidden, void* stream);
int gcgcn_bert_layer_bwd(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const float* const* params,
                         const void* saved, int64_t saved_bytes, const float* dy, float* dx, float* const* grads, void* ws, int64_t ws_bytes,
                         const void* rng_snap, float p_attn, float p_hidden, void* stream);

/* ---- the same with per-document token lengths -----------------------------------------------------------------
 * t_valid: int32 [B] on the device, 0 <= t_valid[b] <= T (values outside are clamped).  Row (b, t) is LIVE iff t < t_valid[b].  The layout
 * stays padded; T keeps every stride and every dropout index (the offset in the virtual [B][H][T][T] and [B T][D] tensors), so the
 * length path and the prefix-mask path draw the same keep decisions on live elements from one snapshot.
 *  1. Live rows: outputs, saved state and gradients are what the entry point without _len computes for document b alone at T = t_valid[b]
 *     with no mask.  Keys at or past t_valid[b] have probability exactly 0.  key_bias may still be given (holes inside the live prefix) and
 *     keeps its meaning; c_b is then the largest penalty of the document's live keys.
 *  2. Padding rows: every output row (ctx, lse, dqkv, y, mean, rstd, dx, dres, gelu's output; the layer's y and dx) is exactly 0.0f.
 *     Gradients arriving there (dctx, dy) are not read: they may hold anything, NaN included.  The LAYER's input x must be zero on padding
 *     rows; the caller owns this (gcgcn_amd.BertModel guarantees it whatever token ids sit there).  The stand-alone row functions read
 *     nothing of a padding row.
 *  3. t_valid[b] == 0: the document contributes nothing and produces zeros; no softmax over an empty key set is formed.
 *  4. No host read, no allocation, capturable: a captured call replayed after t_valid was overwritten in place computes the new lengths.
 *     No float atomics: bit-reproducible.
 *  5. No result depends on memory the call did not write.  A weight gradient sums over the padding rows of a partly live 16-row block (on
 *     the dense route: over all padding rows), so every kernel whose output such a sum reads stores zeros there.
 * The grids do not depend on the lengths (fixed for capture): a workgroup of the attention kernels whose 16 rows are all padding stores
 * its zeros and leaves, the others stream ceil(t_valid[b] / 64) blocks instead of ceil(T / 64).
 * gcgcn_bert_layer_*_len: rowblk = the list gcgcn_row_blocks(B, T, t_valid) built (T a multiple of 16; build it once per model forward and
 * hand it to every layer and its backward), or NULL.  With it the four forward products compute, the data gradients compute and the weight
 * gradients sum over the live 16-row blocks only.  The GEMM launcher drops the list per problem on shapes it does not serve -- B T or a
 * width that is no multiple of 64, more than 512 blocks for a weight gradient (B T > 8192), unaligned operands, launches too small to
 * gain -- and T % 16 != 0 has no list at all: those products run dense and the results obey the same contract. */
int gcgcn_bert_attn_fwd_len(int B, int T, int H, int dh, const float* qkv, const float* key_bias, const int32_t* t_valid, float* ctx,
                            float* lse, const void* rng_snap, uint64_t salt, float p, void* stream);
int gcgcn_bert_attn_bwd_len(int B, int T, int H, int dh, const float* qkv, const float* key_bias, const int32_t* t_valid, const float* ctx,
                            const float* lse, const float* dctx, float* dqkv, float* delta, const void* rng_snap, uint64_t salt, float p,
                            void* stream);
int gcgcn_res_ln_fwd_len(int64_t rows, int D, const float* x, const float* bias, const float* res, const float* weight, const float* lnb,
                         const int32_t* t_valid, int T, float* y, float* mean, float* rstd, const void* rng_snap, uint64_t salt, float p,
                         void* stream);
int gcgcn_res_ln_bwd_len(int64_t rows, int D, const float* dy, const float* x, const float* bias, const float* res, const float* weight,
                         const float* mean, const float* rstd, const int32_t* t_valid, int T, float* dx, float* dres, float* dweight,
                         float* dlnb, void* ws, int64_t ws_bytes, const void* rng_snap, uint64_t salt, float p, void* stream);
int gcgcn_bias_gelu_fwd_len(int64_t rows, int C, const float* x, const float* bias, const int32_t* t_valid, int T, float* y, void* stream);
int gcgcn_bias_gelu_bwd_len(int64_t rows, int C, const float* dy, const float* x, const float* bias, const int32_t* t_valid, int T, float* dx,
                            void* stream);
int gcgcn_bert_layer_fwd_len(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const int32_t* t_valid,
                             const int32_t* rowblk, const float* const* params, float* y, void* saved, int64_t saved_bytes,
                             const void* rng_snap, float p_attn, float p_hidden, void* stream);
int gcgcn_bert_layer_bwd_len(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const int32_t* t_valid,
                             const int32_t* rowblk, const float* const* params, const void* saved, int64_t saved_bytes, const float* dy,
                             float* dx, float* const* grads, void* ws, int64_t ws_bytes, const void* rng_snap, float p_attn, float p_hidden,
                             void* stream);

/* ---- opt-in bf16 matrix products (gemm_bf16.hip) --------------------------------------------------------------
 * gcgcn_gemm_bf16: C [M][N] = op(A) op(B) + bias[col] + add[row][col] (bias [N], add [M][ldadd], each or both NULL) for the storage
 * forms of gcgcn_gemm: a_kc = 1: A is stored [M][K], else [K][M]; b_kc = 1: B is stored [N][K], else [K][N]; NN (1, 0), NT (1, 1) and
 * TN (0, 0) are served.  Operands and result are fp32 in memory.  Every operand element is rounded once to bf16, round to nearest even
 * (what tensor.to(torch.bfloat16) does), on its way into the workgroup's LDS; the products run on v_mfma_f32_16x16x32_bf16, the
 * accumulation, the epilogue (bias, then add) and the store are fp32.  Every M, N, K >= 1 is served; nothing outside the [M][K], [K][N],
 * [M][N] views is read or written, the ld padding included.  Long K on few tiles is cut into runs whose partial tiles go through ws
 * (gcgcn_gemm_bf16_ws_bytes(M, N, K) bytes, 16-byte aligned; 0: ws may be NULL) and are added in a fixed order: no float atomics, two
 * runs are bitwise equal.  Capturable: no host read, no allocation, no synchronisation.
 * gcgcn_bert_layer_fwd_mm / gcgcn_bert_layer_bwd_mm: the _len entry points (t_valid and rowblk may both be NULL: every row is live)
 * with a selector for the twelve Linear products.  matmul = 0: the fp32 GEMM layer, launch for launch what the entry points above
 * run.  matmul = 1: bf16 operands as above -- everything else (attention core, LayerNorms, GELU, dropout sites and indices, saved
 * state, workspace sizes) is unchanged, the bias gradients are exact fp32 column sums, and with rowblk the products run on the live
 * 16-row blocks where their launcher serves the list (whole 64-row tiles of 16-byte aligned operands; dense elsewhere): forward
 * products and data gradients compute the live blocks, weight gradients skip the 64-deep steps without a live block.  The results are
 * bit for bit those of the dense products (gcgcn_set_option("bf16_rows", 0) / GCGCN_BF16_ROWS=0 runs those), and the padding-row
 * contract of the _len entry points holds.  Both calls of a pair take the same matmul. */
int64_t gcgcn_gemm_bf16_ws_bytes(int M, int N, int K);
int gcgcn_gemm_bf16(int a_kc, int b_kc, const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int M, int N, int K,
                    const float* bias, const float* add, int64_t ldadd, void* ws, int64_t ws_bytes, void* stream);
int gcgcn_bert_layer_fwd_mm(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const int32_t* t_valid,
                            const int32_t* rowblk, const float* const* params, float* y, void* saved, int64_t saved_bytes,
                            const void* rng_snap, float p_attn, float p_hidden, void* stream, int matmul);
int gcgcn_bert_layer_bwd_mm(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const int32_t* t_valid,
                            const int32_t* rowblk, const float* const* params, const void* saved, int64_t saved_bytes, const float* dy,
                            float* dx, float* const* grads, void* ws, int64_t ws_bytes, const void* rng_snap, float p_attn, float p_hidden,
                            void* stream, int matmul);

/* ---- opt-in bf16 attention core (bert_attn_bf16.hip) -----------------------------------------------------------
 * gcgcn_bert_attn_fwd_mx / gcgcn_bert_attn_bwd_mx: the argument lists of gcgcn_bert_attn_*_len (t_valid may be NULL: every row is
 * live) plus a selector.  attn = 0: the fp32 core, launch for launch and bit for bit what the entry points above run.  attn = 1: the
 * four matrix products of the core take bf16 operands on v_mfma_f32_16x16x32_bf16, with r(.) one rounding to bf16, nearest even:
 *     S = r(q) r(k)^T / 8 + key_bias,  P = softmax(S) (fp32, unrounded),  Pd = keep / (1 - p) o P,  ctx = r(Pd) r(v),  lse as above;
 *     delta = sum_d dctx ctx (fp32, from the stored ctx),  dPd = r(dctx) r(v)^T,  dS = P o (keep / (1 - p) o dPd - delta),
 *     dv = r(Pd)^T r(dctx),  dq = r(dS) r(k) / 8,  dk = r(dS)^T r(q) / 8.
 * q, k, v and dctx are rounded once on their way into LDS or registers, P and dS when they become operands; every accumulation, the
 * softmax, lse, delta and dS are fp32; qkv, ctx, lse, dctx and dqkv stay fp32 in memory in the layouts above.  Everything else of the
 * contract holds unchanged: dh = 64, T <= 512, key_bias and the c_b shift (a document whose keys are all masked keeps a finite
 * softmax), the five points of the token lengths (grids independent of the lengths; a workgroup whose 64 rows are all padding stores
 * its zeros and leaves), the dropout index in the virtual [B][H][T][T] tensor -- from one snapshot and salt attn = 1 draws bit for bit
 * the mask attn = 0 draws --, nothing of size [T][T] in memory, one writer per output element, no float atomics, capturable.
 * With attn = 1, ctx (forward) and dqkv (backward) must be 16-byte aligned as well.  Any other attn is refused.
 * gcgcn_bert_layer_fwd_mx / gcgcn_bert_layer_bwd_mx: the _mm argument lists plus attn behind matmul; the two selectors are
 * independent, the saved state and the workspace sizes do not depend on either.  Both calls of a pair take the same selectors. */
int gcgcn_bert_attn_fwd_mx(int B, int T, int H, int dh, const float* qkv, const float* key_bias, const int32_t* t_valid, float* ctx,
                           float* lse, const void* rng_snap, uint64_t salt, float p, void* stream, int attn);
int gcgcn_bert_attn_bwd_mx(int B, int T, int H, int dh, const float* qkv, const float* key_bias, const int32_t* t_valid, const float* ctx,
                           const float* lse, const float* dctx, float* dqkv, float* delta, const void* rng_snap, uint64_t salt, float p,
                           void* stream, int attn);
int gcgcn_bert_layer_fwd_mx(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const int32_t* t_valid,
                            const int32_t* rowblk, const float* const* params, float* y, void* saved, int64_t saved_bytes,
                            const void* rng_snap, float p_attn, float p_hidden, void* stream, int matmul, int attn);
int gcgcn_bert_layer_bwd_mx(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const int32_t* t_valid,
                            const int32_t* rowblk, const float* const* params, const void* saved, int64_t saved_bytes, const float* dy,
                            float* dx, float* const* grads, void* ws, int64_t ws_bytes, const void* rng_snap, float p_attn, float p_hidden,
                            void* stream, int matmul, int attn);

#ifdef __cplusplus
}
#endif
#endif /* GCGCN_H */
