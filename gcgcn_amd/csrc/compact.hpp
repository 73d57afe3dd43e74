// Consumers of the edge-feature producer's compact rows (compact.hip): the operand and the launchers.
#pragma once
#include "edge_plan.hpp"

namespace gc {

constexpr int CW4 = 4;     // waves per workgroup
constexpr int CMAXK = 8;   // columns per lane: D <= 64 * CMAXK

struct CmpE {
  const float* Ec;     // [Q, D] compact rows
  const int* prow;     // [B, N, N]: row of Ec, or -1
  const float* bias;   // [D]
};

int cmp_check(const char* who, int B, int N, int D, const float* Ec, const int* prow, const float* bias);
int cmp_fwd(const CmpE& ce, const float* v, const int* n_valid, float* Ebar, const float* coladd, float* P, float* A, Drop drop,
            int B, int N, int D, hipStream_t st);
// plan: edge_plan_bwd's (GATAttention) or edge_plan_bcast's (the mean alone: v, dlogit, dvpart NULL), made by the caller
int cmp_bwd(const CmpE& ce, const float* v, const int* n_valid, const float* dlogit, const float* dEbar, float* dEc, float* dvpart,
            float* rowbuf, float* dbias, const EdgePlan& plan, int B, int N, int D, hipStream_t st);

}  // namespace gc
