// Attention core of MultiHeadAttention for small graphs (N <= 64 entities, the DocRED regime).
//
// Per (document b, head h) the reference computes  A = dropout(softmax(Q_h Q_h^T / sqrt(dh)))  (glove:136-140; the
// keys reuse the query projection).  With N <= 64 the whole N x N score matrix of one (b, h) fits in LDS, so one
// workgroup produces P and A straight from Q_h -- scores never touch HBM -- and, backward, turns dA into
// dQ_h = alpha (dS + dS^T) Q_h without materialising dS; both products run on the fp32 MFMA from LDS operands.  Replaces three launches forward (batched score GEMM at
// 64x64x32 per problem, softmax) and three backward (softmax gradient, two batched 64x32x64 GEMMs).
// Larger graphs take the generic GEMM + row-softmax path in api.hip.
#include "attn_plan.hpp"
#include "rowops.hpp"

namespace gc {

__global__ __launch_bounds__(256) void mha_core_fwd_kernel(const float* __restrict__ Q, const int* __restrict__ n_valid,
                                                           float* __restrict__ P, float* __restrict__ A, int N, int D, int H,
                                                           int dh, int kchunk, float alpha, Drop drop) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  mha_core_fwd_body(sm, blockIdx.x, Q, n_valid, P, A, N, D, H, dh, kchunk, alpha, drop, threadIdx.x, true, nullptr, 0, 4);
}

__global__ __launch_bounds__(256) void mha_core_bwd_kernel(const float* __restrict__ Q, const float* __restrict__ P,
                                                           const float* __restrict__ dA, float* __restrict__ dQ, int N, int D,
                                                           int H, int dh, int kchunk, float alpha, Drop drop) {
  extern __shared__ __attribute__((aligned(16))) float sm[];
  mha_core_bwd_body(sm, blockIdx.x, Q, P, dA, dQ, N, D, H, dh, kchunk, alpha, drop);
}

// The core serves graphs of at most MT entities whose heads are whole float4s (load_q_chunk)
static bool mha_core_ok(const AttnQuery& q) {
  return q.N >= 1 && q.N <= MT && q.H >= 1 && q.D % q.H == 0 && (q.D / q.H) % 4 == 0 && q.D % 4 == 0;
}
unsigned attn_misalign(const void* Q, const void* dQ) { return (al16(Q) ? 0u : ATTN_MIS_Q) | (al16(dQ) ? 0u : ATTN_MIS_DQ); }

// option mha_core = 0 sends small graphs through the generic batched-GEMM + row-softmax path as well (A/B testing of this file),
// and takes the hook away with it: the fused hop has no other form of the core.
static bool attn_fusable(const AttnQuery& q) { return q.mha_core != 0 && mha_core_ok(q); }
int attn_hook_refusal(const AttnQuery& q) {
  return !q.hook ? ATTN_SERVED : !attn_fusable(q) ? ATTN_REFUSED_SHAPE : q.mis ? ATTN_REFUSED_ALIGN : ATTN_SERVED;
}

// A (served) hook takes `hooked_route`; a stand-alone call takes the core where it serves the call, the GEMMs elsewhere
static AttnPlan attn_plan(const AttnQuery& q, int hooked_route, int hooked_chunk) {
  AttnPlan p;
  p.fusable = attn_fusable(q);
  if (q.hook) p.route = hooked_route, p.kchunk = hooked_chunk;
  else if (p.fusable && !q.mis) p.route = AttnPlan::CORE, p.kchunk = mha_chunk(q.D / q.H);   // small graph: scores stay in LDS
  return p;
}

AttnPlan attn_plan_fwd(const AttnQuery& q) {
  // in the chain workgroups' prologue where the shape's chain kernel can do that, as a launch of its own inside the hook otherwise
  return attn_plan(q, q.chain_attends ? AttnPlan::CHAIN : AttnPlan::CORE, q.H >= 1 ? mha_chunk(q.D / q.H) : 0);
}

AttnPlan attn_plan_bwd(const AttnQuery& q) {
  if (!q.hook && q.core_done) {  // dQ arrived with the call (computed by gcgcn_gcn_bwd with a gcgcn_mha_hook)
    AttnPlan p;
    p.fusable = attn_fusable(q), p.route = AttnPlan::DONE;
    return p;
  }
  // as passenger workgroups of the convolution's last group launch where a (document, head) pair's scratch fits the tile kernel's
  // LDS (head width <= 64: cfg 1 / cfg 2's 16 and 32), as a launch of its own in front of it otherwise (cfg 3's 192: the group
  // launch grew by more than the launch it saved, see gemm_group_mha_chunk)
  const int dh = q.H >= 1 ? q.D / q.H : 0, ride = q.hook ? gemm_group_mha_chunk(dh) : 0;
  return attn_plan(q, ride ? AttnPlan::GROUP : AttnPlan::CORE, ride ? ride : mha_chunk(dh));
}

int mha_core_fwd(const GcnCtx::MhaFwd& m, const int* n_valid, int B, int N, int D, int H, hipStream_t st) {
  ProfScope ps("mha_core_fwd", st);
  hipLaunchKernelGGL(mha_core_fwd_kernel, dim3(B * H), dim3(256), mha_lds_bytes_of(m.kchunk), st, m.Q, n_valid, m.P, m.A, N, D, H, m.dh,
                     m.kchunk, m.alpha, m.drop);
  return check_launch("mha_core_fwd");
}

int mha_core_bwd(const MhaPass& mp, hipStream_t st) {
  ProfScope ps("mha_core_bwd", st);
  hipLaunchKernelGGL(mha_core_bwd_kernel, dim3(mp.count), dim3(256), mha_lds_bytes_of(mp.kchunk), st, mp.Q, mp.P, mp.dA, mp.dQ, mp.N, mp.D,
                     mp.H, mp.dh, mp.kchunk, mp.alpha, mp.drop);
  return check_launch("mha_core_bwd");
}

}  // namespace gc
