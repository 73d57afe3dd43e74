// Which launch a pass over the edge tensor gets: decided ONCE per call, by the pure functions below (edge.hip), from an EdgeQuery
// that holds everything the decision may depend on -- shapes, alignment bits, which optional operands exist -- and, for the
// backward pass that carries parked weight-gradient tiles, a summary of what the defer queue handed over.  The launchers
// (edge_fwd / edge_bwd / edge_bcast in edge.hip, cmp_fwd / cmp_bwd in compact.hip) validate, plan and launch what the plan
// names; the GATAttention entry points (api.hip) read the dlogit route and the scratch layout from the same plan.
// gcgcn_debug_edge_plan shows the result (tests/test_host_cpu.py pins it).  Host only: nothing here is a kernel argument.
#pragma once
#include "common.hpp"

namespace gc {

enum EdgeMisalign { EDGE_MIS_E = 1, EDGE_MIS_V = 2, EDGE_MIS_DE = 4, EDGE_MIS_DEBAR = 8, EDGE_MIS_EBAR = 16 };
unsigned edge_misalign(const void* E, const void* v, const void* dE, const void* dEbar, const void* Ebar);   // NULL counts as aligned

struct EdgeQuery {
  int B, N, D;
  bool compact;             // the operand is CmpE, not a dense E
  bool att;                 // forward: P is wanted; backward: a logit gradient comes in (GATAttention), not the mean alone
  bool has_dE, has_dEbar;   // dense backward: the optional operands
  unsigned mis;             // EdgeMisalign bits of the operands that exist
};

struct EdgePlan {
  enum Route { RIDE = 0, ONE = 1, THREE = 2 };   // passengers of the edge pass | one gat_dlogit launch | softmax_bwd + colsum + node_score_bwd
  // kernel choice
  bool compact = false, att = false;
  int vec = 1;            // dense kernels: the <4> (16-byte) or the <1> instantiation; the compact kernels have one form
  int route = -1;         // GATAttention backward: how dlogit / ds / dX are produced (Route); -1: no attention term
  int slices = -1;        // RIDE / ONE: feature slices per document (gat_dlogit_slices)
  int ngat = 0;           // RIDE: passenger workgroups in front of the entity rows (B * slices)
  // resources
  size_t lds = 0;         // dynamic LDS of the launch, bytes
  size_t lds_limit = 0;   // what the launcher checks it against (0: the pass has no check; its bound on D keeps it small)
  bool lds_ok() const { return lds_limit == 0 || lds <= lds_limit; }
  // carrying (dense backward)
  bool carry_ok = false;  // parked weight-gradient tiles may ride: 16-byte rows, and a row's LDS fits the tile's static image
  int ntile = 0, ncolwg = 0, col_base = 0;   // edge_plan_carry: tile workgroups, workgroups of a parked column sum's second stage
  bool RB = false;                            // and their first index (0: none); a carried product walks row blocks
  long grid = 0;          // workgroups of the launch: entity rows + ngat (+ ntile + ncolwg)
  Spread spread = {0, 0, 0};
  // scratch of a GATAttention backward call, floats (-1: not one)
  long scratch = -1;      // what gcgcn_gat_bwd_scratch / gcgcn_gat_bwd_compact_scratch return
  long rowbuf_off = -1;   // compact: where cmp_bwd's row buffer [2 B N] starts inside it
};

EdgePlan edge_plan_fwd(const EdgeQuery& q);
EdgePlan edge_plan_bwd(const EdgeQuery& q);     // eligibility only: carry_ok, nothing taken yet
EdgePlan edge_plan_bcast(const EdgeQuery& q);   // the mean alone: dense edge_bcast; compact = edge_plan_bwd without attention
// The grid of a carrying launch, once gemm_take_deferred has popped `ntile` tile workgroups (0: nothing rides, p stays as it is);
// any_rb: one of the taken problems walks row blocks; col_C: width of the parked column-sum second stage taken with them, or 0.
void edge_plan_carry(EdgePlan& p, int ntile, bool any_rb, int col_C);

}  // namespace gc
