// Where the core of MultiHeadAttention runs -- P = softmax(alpha Q_h Q_h^T), A = dropout(P) forward, dQ from dA backward: decided
// ONCE per call, by the pure functions below (mha_core.hip), from an AttnQuery that holds everything the decision may depend on.
// The four entry points that run attention (api.hip: gcgcn_mha_fwd / _bwd, and gcgcn_gcn_fwd / _bwd with a gcgcn_mha_hook) make the
// query, plan, and switch on the route; the plan's kchunk is the one the route's kernel gets (GcnCtx::mha, MhaPass).
// gcgcn_debug_attn_plan shows the result (tests/test_host_cpu.py pins it).  Host only: nothing here is a kernel argument.
#pragma once
#include "../../include/gcgcn.h"
#include "gcn_plan.hpp"

namespace gc {

enum AttnMisalign { ATTN_MIS_Q = 1, ATTN_MIS_DQ = 2 };
unsigned attn_misalign(const void* Q, const void* dQ);   // NULL counts as aligned

struct AttnQuery {
  int N, D, H;
  unsigned mis;         // AttnMisalign bits of the operands that exist
  bool hook;            // the call is the convolution's (gcgcn_mha_hook), not gcgcn_mha_fwd / _bwd
  bool chain_attends;   // forward hook: ChainPlan::attention -- the call's chain kernel can run the core in its prologue
  bool core_done;       // gcgcn_mha_bwd: dQ arrived with the call
  int mha_core;         // the option of the same name
};

struct AttnPlan {
  enum Route {
    GEMM = 0,    // batched GEMMs + softmax_fwd | softmax_bwd + two batched GEMMs: any N
    CORE = 1,    // a mha_core_fwd / mha_core_bwd launch
    CHAIN = 2,   // forward hook: the prologue of the chain S / chain T workgroups (GcnCtx::mha)
    GROUP = 3,   // backward hook: passenger workgroups of the convolution's last group launch (MhaPass)
    DONE = 4     // gcgcn_mha_bwd: nothing to run
  };
  int route = GEMM;
  int kchunk = 0;         // head-feature chunk of the route's kernel (CORE, CHAIN, GROUP), else 0
  bool fusable = false;   // gcgcn_maggc_fusable: a hook may be offered for this (N, D, H)
};

// A hook (q.hook) on a shape the core does not serve, or on a misaligned Q / dQ, is an error of gcgcn_gcn_fwd / _bwd: they ask this
// first -- it depends on nothing the chain plan decides -- and plan only a hook that is served.  No hook: served.
enum AttnRefusal { ATTN_SERVED = 0, ATTN_REFUSED_SHAPE = 1, ATTN_REFUSED_ALIGN = 2 };
int attn_hook_refusal(const AttnQuery& q);
AttnPlan attn_plan_fwd(const AttnQuery& q);
AttnPlan attn_plan_bwd(const AttnQuery& q);

// The core's operands `c` with its parameters, set here and nowhere else, in whichever struct the route hands to its kernel:
// GcnCtx::MhaFwd (forward: a launch of its own, or the chain's prologue) or MhaPass (backward: a launch of its own, or passengers
// of a group launch)
template <class Core>
inline Core attn_core(Core c, int D, int H, const AttnPlan& plan, const void* rng_snap, float p) {
  c.dh = D / H, c.kchunk = plan.kchunk, c.alpha = 1.f / sqrtf((float)c.dh), c.drop = make_drop(rng_snap, GCGCN_SALT_MHA, p);
  return c;
}

inline MhaPass mha_pass(const float* Q, const float* P, const float* dA, float* dQ, int B, int N, int D, int H) {
  MhaPass mp;
  mp.Q = Q, mp.P = P, mp.dA = dA, mp.dQ = dQ, mp.N = N, mp.D = D, mp.H = H, mp.count = B * H;
  return mp;
}

// The CORE route's launches (mha_core.hip), on the same two structs the CHAIN and GROUP routes hand to their kernels
int mha_core_fwd(const GcnCtx::MhaFwd& m, const int* n_valid, int B, int N, int D, int H, hipStream_t st);
int mha_core_bwd(const MhaPass& mp, hipStream_t st);

}  // namespace gc
