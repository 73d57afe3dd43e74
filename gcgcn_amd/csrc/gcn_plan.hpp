// The per-(document, head) products of the densely connected GraphConv stack, described once and
// used twice: by the host (one batched launch per product: ChainPlan::NONE) and by the chain kernels
// (chain.hip: one persistent workgroup per (b, h) runs them back to back).  Below them: ChainQuery /
// ChainPlan, the one decision which of the two, and which chain kernel, a convolution call gets.
//
// Tensors are [B*N, H, L, gh] row-major (row stride HD = H*D, D = L*gh); A is [B, H, N, N];
// z1 = document, z2 = head.  Reference: GraphConv.forward glove:36-50 inside the dense loops of
// GraphConvolution.forward glove:70-76 / MultiGraphConvolution.forward glove:102-113.
#pragma once
#include "gemm.hpp"
#include "mha_body.hpp"

namespace gc {

// An edge-tensor streaming pass that depends on nothing the chain computes (the NEXT hop's mean_j E forward, its
// dE = dEbar / n backward).  A chain launch of few (doc, head) pairs leaves most compute units idle, and the chain
// is latency-bound where the pass is HBM-bound: the pass rides in extra workgroups of the same launch.
struct EdgeRide {
  int kind;  // 0 none, 1: out[B,N,D] = mean_j in[B,N,N,D], 2: out[B,N,N,D] = in[B,N,D] / n
  int B, N, D;
  const float* in;
  const int* n_valid;
  float* out;
};

struct GcnCtx {
  int B, N, D, L, H, gh;
  EdgeRide ride;
  // forward with MultiHeadAttention's core computed by the chain workgroup itself (LDS-resident kernels, gcgcn_mha_hook):
  // A_h = dropout(softmax(alpha Q_h Q_h^T)) goes straight into the adjacency image; P and A are still written for backward
  struct MhaFwd {
    const float* Q;   // NULL: the adjacency comes from c.A
    float* P;
    float* A;         // NULL without dropout (the chain then uses P)
    float alpha;
    Drop drop;
    int dh, kchunk;
  } mha;
  Spread carry;      // backward launches: how the tile passengers are placed among the riding rows (common.hpp)
  long HD, oWd, wd_head;
  const float* X;
  const float* A;
  const float* flat;
  const int* n_valid;
  Drop drop;
  // forward: G (edge term) in, Pn/Y/HO/rinv out
  const float* G;
  float* Pn;
  float* Y;
  float* HO;
  float* rinv;
  // backward
  float* dYa;   // running gradient of Y (starts as dropout_bwd(dHO))
  float* dM;    // gradient of G_l + A_h Pn_l
  float* dP;    // gradient of Pn_l
  float* dA;
  float* drow;  // gradient of the normaliser's row sum
  // backward with the output projection's input gradient computed by the chain itself (chain.hip, fused kernels):
  // dHO = dout Wlin per (document, head) instead of a launch of its own, dXres = sum_h dHO_h = dout (sum_h Wlin_h)
  const float* dout;   // [B*N, D]   gradient of the block's output; with dout_m set: as it arrives, the chain zeroes the
                       //            padding rows (n_valid) and undoes the output dropout (odrop) while it stages the rows
  float* dout_m;       // [B*N, D] or NULL: the masked gradient, written back for the products that need it later (dWlin)
  Drop odrop;
  const float* Wsum;   // [D, D]     sum over heads of Wlin's column blocks (H > 1)
  float* dXres;        // [B*N, D]
  float* colpart;      // [2 B, D] or NULL: column sums of dout over each half of a document's rows (bias gradient, stage 1)
  long oWlin;
  __host__ __device__ long wd_off(int l) const { return oWd + (long)gh * gh * l * (l - 1) / 2; }
};

// Pn_l += [Y_0 .. Y_{l-1}] Wd_l          (dense connection, glove:73 / 110), l >= 1
__host__ __device__ inline GemmArgs plan_fwd_dense(const GcnCtx& c, int l) {
  const long sb = (long)c.N * c.HD, sh = (long)c.L * c.gh;
  GemmArgs g = gemm_nn(c.Y, c.HD, c.flat + c.wd_off(l), c.gh, c.Pn + (long)l * c.gh, c.HD, c.N, c.gh, l * c.gh);
  g.batch_z1(c.B, sb, 0, sb).batch_z2(c.H, sh, c.wd_head, sh);
  g.splits = 1;
  g.accumulate = 1;
  g.tag = "gemm_dense";
  return g;
}

// Y_l = relu((G_l + A_h Pn_l) * rinv);  HO_l = dropout(Y_l) + X_l      (glove:42-50, 71-76)
__host__ __device__ inline GemmArgs plan_fwd_agg(const GcnCtx& c, int l) {
  const long off = (long)l * c.gh, sb = (long)c.N * c.HD, sh = (long)c.L * c.gh;
  GemmArgs g = gemm_nn(c.A, c.N, c.Pn + off, c.HD, c.Y + off, c.HD, c.N, c.gh, c.N);
  g.batch_z1(c.B, (long)c.H * c.N * c.N, sb, sb).batch_z2(c.H, (long)c.N * c.N, sh, sh);
  g.splits = 1;
  g.add = c.G + off, g.ldadd = c.HD, g.sAdd1 = sb, g.sAdd2 = sh;
  g.rowscale = c.rinv, g.sRs1 = (long)c.H * c.N, g.sRs2 = c.N;
  g.relu = 1;
  g.C2 = c.HO + off, g.ldc2 = c.HD, g.sC21 = sb, g.sC22 = sh;
  g.add2 = c.X + off, g.ldadd2 = c.D, g.sAdd21 = (long)c.N * c.D, g.sAdd22 = 0;
  g.drop = c.drop, g.drop_base = off;  // dropout index = element offset inside HO
  g.tag = "gemm_agg";
  return g;
}

// dPn_l = A_h^T dM_l
__host__ __device__ inline GemmArgs plan_bwd_dP(const GcnCtx& c, int l) {
  const long off = (long)l * c.gh, sb = (long)c.N * c.HD, sh = (long)c.L * c.gh;
  GemmArgs g = gemm_tn(c.A, c.N, c.dM + off, c.HD, c.dP + off, c.HD, c.N, c.gh, c.N);
  g.batch_z1(c.B, (long)c.H * c.N * c.N, sb, sb).batch_z2(c.H, (long)c.N * c.N, sh, sh);
  g.splits = 1;
  g.tag = "gemm_dP";
  return g;
}

// dA_h (+)= dM_l Pn_l^T ; the normaliser's gradient drow[i] is added to every column on the last pass (l == 0)
__host__ __device__ inline GemmArgs plan_bwd_dA(const GcnCtx& c, int l) {
  const long off = (long)l * c.gh, sb = (long)c.N * c.HD, sh = (long)c.L * c.gh;
  GemmArgs g = gemm_nt(c.dM + off, c.HD, c.Pn + off, c.HD, c.dA, c.N, c.N, c.N, c.gh);
  g.batch_z1(c.B, sb, sb, (long)c.H * c.N * c.N).batch_z2(c.H, sh, sh, (long)c.N * c.N);
  g.splits = 1;
  g.accumulate = (l != c.L - 1);
  if (l == 0) g.rowadd = c.drow, g.sRa1 = (long)c.H * c.N, g.sRa2 = c.N;
  g.tag = "gemm_dA";
  return g;
}

// dY_{0..l-1} += dPn_l Wd_l^T, l >= 1
__host__ __device__ inline GemmArgs plan_bwd_dY(const GcnCtx& c, int l) {
  const long sb = (long)c.N * c.HD, sh = (long)c.L * c.gh;
  GemmArgs g = gemm_nt(c.dP + (long)l * c.gh, c.HD, c.flat + c.wd_off(l), c.gh, c.dYa, c.HD, c.N, l * c.gh, c.gh);
  g.batch_z1(c.B, sb, 0, sb).batch_z2(c.H, sh, c.wd_head, sh);
  g.splits = 1;
  g.accumulate = 1;
  g.tag = "gemm_dY";
  return g;
}

// ---- which chain kernel serves a convolution call -------------------------------------------------------------------------
// Decided ONCE per gcgcn_gcn_fwd / _bwd call, by chain_plan_fwd / _bwd (chain.hip), from a ChainQuery that holds everything the
// decision may depend on; the ChainPlan travels BESIDE the GcnCtx (a kernel argument, whose layout it must not move) to
// gcn_chain_fwd / _bwd and on to the column-strip launchers, which select the kernel from it and ask nothing again.
struct ChainQuery {
  int B, N, D, L, H, gh;
  long HD, oWd, wd_head, oWlin;
  const float* flat;
  bool ragged;    // n_valid given
  bool scratch;   // the call has workspace (the fused backward parks its column sums there)
  bool hook;      // forward: the attention core is left to this call (gcgcn_mha_hook)
  EdgeRide ride;  // the passenger the caller offers (kind 0: none)
  const void *A, *Pn, *Y;               // operands whose alignment matters: both directions,
  const void *G, *HO, *X;               // forward,
  const void *dYa, *dM, *dP, *dA;       // backward,
  const void *dout, *dXres, *dout_m;    // the fused output projection's (dout_m: NULL or the masked gradient's workspace)
  int chain, chain_big, chain_t;        // the options of the same names
};
struct ChainPlan {
  enum Kind { NONE, GENERIC, S, T };   // one launch per product | gcn_chain_fwd/bwd_kernel | gcn_chain_s_* | gcn_chain_t_*
  int kind = NONE;
  bool aligned = false;     // GENERIC: the <ALIGNED> instantiation
  bool full = false;        // T: the FULL instantiation (every document fills all four 16-row blocks: N == 64, no n_valid)
  bool fuse = false;        // backward, S / T: the chain computes dHO = dout Wlin and dXres itself (c.dout, c.dXres, c.Wsum)
  bool attention = false;   // forward, S / T: the chain runs the attention core in its prologue (c.mha)
  bool ride = false;        // the offered edge pass is a passenger of the chain launch (c.ride)
};
inline bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
ChainPlan chain_plan_fwd(const ChainQuery& q);
ChainPlan chain_plan_bwd(const ChainQuery& q);

// ---- the output projection's backward (the first half of gcgcn_gcn_bwd) ----------------------------------------------------
// Decided ONCE per call by out_bwd_plan (api.hip), after the chain plan: where dout is masked / un-dropped, where sum_h Wlin_h
// comes from, whether the head sum and the dropout backward fold into the group launch in front of the chain, which launch dWlin
// is offered to, and where the two stages of dblin's column sums run.  Stage 2 also depends on whether the front launch had a
// split-K reduce, which gemm_group reports: out_bwd_plan_col2 is the second pure step.
struct OutBwdQuery {
  bool fuse;            // ChainPlan::fuse; it implies `scratch` (chain_plan_bwd fuses with workspace alone; gcgcn_gcn_bwd checks)
  int B, N, D, H;
  bool scratch;         // the call has workspace
  bool wsum_fwd;        // the forward call left sum_h Wlin_h
  bool ragged;          // n_valid given
  bool odrop, drop;     // the output dropout / the block's dropout is on
  bool dxres_aligned;   // dXres on a 16-byte boundary
};
struct OutBwdPlan {
  enum Mask { MASK_NONE, MASK_LAUNCH, MASK_CHAIN };       // nothing to mask | a mask_rows launch | the chain, while it stages dout
  enum Wsum { WSUM_NONE, WSUM_FORWARD, WSUM_HERE };       // not needed | the forward call's | a mask_rows launch into dYa's buffer
  enum Fold { FOLD_NONE, FOLD_ONE_HEAD, FOLD_HEADS };     // - | dHO is the head sum: written to dXres | + the product dout (sum_h Wlin_h)
  enum DWlin { DWLIN_FRONT, DWLIN_BACK };                 // offered to the queue or the launch in front of the chain | behind it
  enum Col1 { COL1_CHAIN, COL1_FRONT, COL1_BACK, COL1_OWN_LAUNCH };   // stage 1 of dblin's sums (OWN_LAUNCH: a colsum, both stages)
  int mask, wsum, fold;
  bool fold_drop;       // a fold whose epilogue also writes dY = dropout_bwd(dHO) (one head: always; more: with dropout on)
  bool head_sum_launch; // not fused, no fold: head_sum_drop_bwd follows the front launch
  int dwlin, col1;
  int chain_slices;     // COL1_CHAIN: the slices the chain leaves (2 B), else 0
};
struct OutBwdCol2 {
  enum Where { FRONT_REDUCE, HEAD_SUM_KERNEL, BACK_LAUNCH, BACK_REDUCE, DONE };
  int where;
  int back_ready_slices;   // BACK_LAUNCH: the slices the back launch's ColRide::stage2 sums; else 0 (BACK_REDUCE: the whole sum rides)
};

// Each kernel generation answers for itself only, next to its kernels: "I serve this input" (shape + alignment), and for the
// LDS-resident ones whether the backward can fuse the output projection's gradient / the forward can run the attention core.
// Called from chain_plan_fwd / _bwd and from nowhere else; the preference between generations lives there.
bool chain_g_aligned(const ChainQuery& q, bool bwd);                       // chain.hip: generic kernels, <ALIGNED> or not
bool chain_s_serves(const ChainQuery& q, bool bwd);                        // chain.hip: gcn_chain_s_*
bool chain_s_fuses(const ChainQuery& q);
bool chain_s_attends(const ChainQuery& q);
bool chain_t_serves(const ChainQuery& q, bool bwd, bool ride);            // chain_t.hip: gcn_chain_t_* (ride: q.ride comes along)
bool chain_t_fuses(const ChainQuery& q);
bool chain_t_attends(const ChainQuery& q);
bool chain_can_carry(const EdgeRide& r);                                   // chain.hip: a passenger every chain kernel can take

// chain_t.hip (host side) + chain_t.hpp / chain_t_u0..3.hip (kernels): LDS-resident chain kernels for N <= 64 and the instantiated (gh, L) pairs
int gcn_chain_t_fwd(const GcnCtx& c, const ChainPlan& p, dim3 grid, double flops, hipStream_t st);
int gcn_chain_t_bwd(const GcnCtx& c, const ChainPlan& p, double flops, hipStream_t st, DeferQueue* carry);

// chain.hip
Spread chain_carry_spread(const GcnCtx& c, int n_tile_workgroups);
int gcn_chain_fwd(const GcnCtx& c, const ChainPlan& p, hipStream_t st);
int gcn_chain_bwd(const GcnCtx& c, const ChainPlan& p, hipStream_t st, DeferQueue* carry = nullptr);

}  // namespace gc
