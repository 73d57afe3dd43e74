// C ABI of libgcgcn_hip.so (include/gcgcn.h): host-side orchestration of the HIP kernels for
// each block of the CAGGC/MAGGC path.  Every function only enqueues work on the caller's stream.
#include "../../include/gcgcn.h"

#include <stdarg.h>
#include <string.h>

#include <new>
#include <vector>

#include <stdlib.h>

#include "attn_plan.hpp"
#include "compact.hpp"
#include "gat_body.hpp"
#include "gemm.hpp"
#include "lstm.hpp"
#include "frontend.hpp"
#include "bert.hpp"
#include "gemm_bf16.hpp"
#include "rowops.hpp"

namespace gc {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return 2;
  }
  return 0;
}

// ---- per-kernel timing ---------------------------------------------------------------------------
static struct {
  bool on = false;
  char filter[48] = "";
  std::vector<hipEvent_t> ev;  // pairs: start, stop
  int used = 0;                // pairs recorded
  double work = 0;             // summed work of the recorded launches
} g_prof;

ProfScope::ProfScope(const char* tag, hipStream_t s, double work) : slot(-1), st(s) {
  if (!g_prof.on || strncmp(tag, g_prof.filter, strlen(g_prof.filter)) != 0) return;
  if (2 * (g_prof.used + 1) > (int)g_prof.ev.size()) return;  // ring full: stop recording
  slot = g_prof.used++;
  g_prof.work += work;
  (void)hipEventRecord(g_prof.ev[2 * slot], st);
}
ProfScope::~ProfScope() {
  if (slot >= 0) (void)hipEventRecord(g_prof.ev[2 * slot + 1], st);
}
bool prof_events(const char* tag, double work, hipEvent_t* start, hipEvent_t* stop) {
  if (!g_prof.on || strncmp(tag, g_prof.filter, strlen(g_prof.filter)) != 0) return false;
  if (2 * (g_prof.used + 1) > (int)g_prof.ev.size()) return false;  // ring full: stop recording
  const int slot = g_prof.used++;
  g_prof.work += work;
  *start = g_prof.ev[2 * slot], *stop = g_prof.ev[2 * slot + 1];
  return true;
}

struct GcnLayout {
  long oWnX, oWe, oWd, oWlin, oblin, total, wd_head;
  int gh;
  long wd_off(int h, int l) const { return oWd + h * wd_head + (long)gh * gh * l * (l - 1) / 2; }
};
static GcnLayout gcn_layout(int D, int L, int H) {
  GcnLayout y;
  y.gh = D / L;
  const long DHD = (long)D * H * D;
  y.wd_head = (long)y.gh * y.gh * L * (L - 1) / 2;
  y.oWnX = 0;
  y.oWe = DHD;
  y.oWd = 2 * DHD;
  y.oWlin = y.oWd + H * y.wd_head;
  y.oblin = y.oWlin + DHD;
  y.total = y.oblin + D;
  return y;
}

static int check_dims(const char* who, int B, int N, int D, int L, int H) {
  GC_REQUIRE(B > 0 && N > 0 && D > 0, "%s: bad shape B=%d N=%d D=%d", who, B, N, D);
  GC_REQUIRE(L > 0 && D % L == 0, "%s: D=%d not divisible by layer_num=%d", who, D, L);
  GC_REQUIRE(H > 0 && D % H == 0, "%s: D=%d not divisible by head_num=%d", who, D, H);
  return 0;
}

// Workspace of one block call: [split-K partials / column-sum partials | partials of a riding column sum]
static long col_ride_elems(int D) { return (long)COL_RIDE_SLICES * D; }
static long gemm_scratch_elems(int B, int N, int D, int H) {
  const long a = colsum_scratch_elems((long)B * N, D, 1);
  const long rows = (long)B * N > D ? (long)B * N : D;
  const long b = gemm_ws_elems(rows, (long)H * D);
  return a > b ? a : b;
}
static long scratch_elems(int B, int N, int D, int H) { return gemm_scratch_elems(B, N, D, H) + col_ride_elems(D); }

// Run-time A/B switches.  option("head_v1", -1) reads gcgcn_set_option's value if one was set, else the environment
// variable GCGCN_HEAD_V1 (read once), else the default.  Every knob a test has to flip lives here, so that one process
// can run both sides of an A/B; the knobs whose A/B is settled are constants at their use.
struct Opt {
  const char* name;
  int value;
  bool resolved;
};
static Opt g_opts[] = {{"head_v1", 0, false},      {"head_bil3", 0, false}, {"head_bil3_bwd", 0, false}, {"head_dw3", 0, false},
                       {"head_compact", 0, false}, {"chain_t", 0, false},   {"chain_big", 0, false},     {"split_widen", 0, false},
                       {"chain", 0, false},        {"mha_core", 0, false},  {"group_dump", 0, false},
                       {"bf16_rows", 0, false}};   // 0: the BERT layer's bf16 products ignore the row-block list (bert.hip's on_rows reads it)
int option(const char* name, int dflt) {
  for (Opt& o : g_opts) {
    if (strcmp(o.name, name) != 0) continue;
    if (!o.resolved) {
      char env[64] = "GCGCN_";
      size_t n = strlen(env);
      for (const char* c = name; *c && n + 1 < sizeof(env); ++c) env[n++] = (char)((*c >= 'a' && *c <= 'z') ? *c - 32 : *c);
      env[n] = 0;
      const char* e = getenv(env);
      o.value = e ? atoi(e) : dflt;
      o.resolved = true;
    }
    return o.value;
  }
  return dflt;
}
// "head_matmul" is not one of the switches above: it is an ARGUMENT of the next head call, handed over beside the call's list.
// gcgcn_set_option("head_matmul", v) stores v for the calling THREAD; the next gcgcn_head_fwd / gcgcn_head_bwd / gcgcn_debug_head_plan
// on that thread takes it and leaves 0 behind.  Nothing process-wide and nothing lasting selects the arithmetic: no environment
// variable is read, another thread never sees the value, and a call that nobody announced runs fp32.
static thread_local int g_head_matmul_next = 0;
int head_matmul_take() {
  const int v = g_head_matmul_next;
  g_head_matmul_next = 0;
  return v;
}
// "lstm_recurrent" travels the same way: the recurrent argument (0 = fp32, 1 = bf16 operands) of the calling thread's next
// gcgcn_lstm_fwd / _fwd_len / _bwd / _bwd_len, which takes it first -- whatever it then returns -- and leaves 0 behind.
static thread_local int g_lstm_recurrent_next = 0;
int lstm_recurrent_take() {
  const int v = g_lstm_recurrent_next;
  g_lstm_recurrent_next = 0;
  return v;
}
static bool set_opt(const char* name, int value) {
  if (strcmp(name, "head_matmul") == 0) {
    g_head_matmul_next = value;
    return true;
  }
  if (strcmp(name, "lstm_recurrent") == 0) {
    g_lstm_recurrent_next = value;
    return true;
  }
  for (Opt& o : g_opts)
    if (strcmp(o.name, name) == 0) {
      o.value = value, o.resolved = true;
      return true;
    }
  return false;
}

// What attn_plan_fwd / _bwd (mha_core.hip) decide on: the one place option mha_core (GCGCN_MHA_CORE) is read
static AttnQuery make_attn_query(int N, int D, int H, const void* Q, const void* dQ, bool hook, bool chain_attends, bool core_done) {
  return AttnQuery{N, D, H, attn_misalign(Q, dQ), hook, chain_attends, core_done, option("mha_core", 1)};
}

// gcgcn_edge_ride -> EdgeRide (kind 1: edge mean forward, 2: its backward); NULL = no passenger
static int make_ride(const char* who, const gcgcn_edge_ride* ride, int kind, EdgeRide& r) {
  memset(&r, 0, sizeof(r));
  if (!ride) return 0;
  GC_REQUIRE(ride->B > 0 && ride->N > 0 && ride->D > 0 && ride->in && ride->out, "%s: bad edge ride B=%d N=%d D=%d", who,
             ride->B, ride->N, ride->D);
  GC_REQUIRE((long)ride->B * ride->N <= 0x3fffffffL, "%s: edge ride too large", who);
  r.kind = kind, r.B = ride->B, r.N = ride->N, r.D = ride->D;
  r.in = ride->in, r.n_valid = ride->n_valid, r.out = ride->out;
  return 0;
}

// Row blocks of a ragged batch (gcgcn_row_blocks) on one GEMM problem: mode 1 = M is the document-row dimension, 2 = K is.
// (both walk the same list of live 16-row blocks: mode 1 four at a time as a 64-row tile, mode 2 two at a time as a k-tile)
static void use_rows(GemmArgs& g, const int* rowblk, int mode, int zero_dead = 0) {
  if (!rowblk) return;
  g.rb = rowblk + ROWBLK_HDR, g.rb_n = rowblk;
  g.rb_mode = mode, g.rb_zero = zero_dead;
}

// The row-block list of a call, or NULL where the call does not walk the live row blocks (dense batch, or a graph size whose
// documents are not whole 16-row blocks)
static const int* live_rows(const int32_t* rowblk, int N, bool ragged) {
  return (rowblk && ragged && N % 16 == 0 && N >= 32) ? rowblk : nullptr;
}

// What chain_plan_fwd / _bwd (chain.hip) decide on, apart from the direction's own operands (set by the caller)
static ChainQuery make_query(int B, int N, int D, int L, int H, const GcnLayout& y, const float* flat, bool ragged, bool scratch,
                             bool hook, const EdgeRide& ride, const void* A, const void* Pn, const void* Y) {
  ChainQuery q = ChainQuery();
  q.B = B, q.N = N, q.D = D, q.L = L, q.H = H, q.gh = y.gh;
  q.HD = (long)H * D, q.oWd = y.oWd, q.wd_head = y.wd_head, q.oWlin = y.oWlin;
  q.flat = flat, q.ragged = ragged, q.scratch = scratch, q.hook = hook, q.ride = ride;
  q.A = A, q.Pn = Pn, q.Y = Y;
  q.chain = option("chain", 1), q.chain_big = option("chain_big", 0), q.chain_t = option("chain_t", 1);
  return q;
}

static GcnCtx make_ctx(int B, int N, int D, int L, int H, const GcnLayout& y, const float* X, const float* A,
                       const float* flat, const int* n_valid, Drop drop) {
  GcnCtx c;
  memset(&c, 0, sizeof(c));
  c.B = B, c.N = N, c.D = D, c.L = L, c.H = H, c.gh = y.gh;
  c.HD = (long)H * D, c.oWd = y.oWd, c.wd_head = y.wd_head;
  c.X = X, c.A = A, c.flat = flat, c.n_valid = n_valid, c.drop = drop;
  return c;
}

// ---- GATAttention's node phase around the edge pass, once for dense E and for compact rows -------------------------------------
struct EdgeOperand {   // the edge tensor of a GATAttention call: dense E[B, N, N, D], or compact rows (E == nullptr)
  const float* E;
  CmpE ce;
};

// uvc = the folded projections (unless the caller kept them from an earlier call with the same parameters), s = u . x + c.
// The rng draw, if asked for, rides in whichever of the two launches comes first.
static int gat_node_fwd(const float* X, const float* flat, float* uvc, float* s, long M, int D, int Dh, int uvc_valid, void* rng_state,
                        void* rng_snaps, int rng_count, hipStream_t st) {
  if (!uvc_valid) {
    GC_TRY(gat_fold_fwd(flat, uvc, D, Dh, st, rng_state, rng_snaps, rng_count));  // + gcgcn_rng_next, if asked to
    return node_score_fwd(X, uvc, s, M, D, st);
  }
  return node_score_fwd(X, uvc, s, M, D, st, rng_state, rng_snaps, rng_count);
}

// dlogit by the plan's route, the edge pass on either operand (dE: dE[B, N, N, D], or dEc with dbias for compact rows), then
// du / dv / dc and the fold's backward
static int gat_bwd(const EdgeOperand& eo, int B, int N, int D, int Dh, const float* X, const int* n_valid, const float* flat, Drop drop,
                   const float* uvc, const float* P, const float* dA, const float* dEbar, const float* dX_in, float* dX, float* dE,
                   float* dbias, float* dflat, float* dlogit, float* ds, float* dvpart, float* duvc, float* scratch, DeferQueue* dq,
                   hipStream_t st) {
  const bool compact = eo.E == nullptr;
  const long M = (long)B * N;
  const float* v = uvc + D;
  const EdgePlan plan = edge_plan_bwd({B, N, D, compact, true, dE != nullptr, dEbar != nullptr,
                                       compact ? 0u : edge_misalign(eo.E, v, dE, dEbar, nullptr)});
  const GatTail tail{P, dA, uvc, dX_in, ds, dX, drop, B, plan.slices};
  if (plan.route == EdgePlan::ONE) {
    GC_TRY(gat_dlogit(P, dA, uvc, dX_in, dlogit, ds, dX, B, N, D, plan.slices, drop, st));
  } else if (plan.route == EdgePlan::THREE) {
    GC_TRY(softmax_bwd(P, dA, dlogit, M, N, drop, st));
    // ds[b, j] = sum_i dlogit[b, i, j]
    GC_TRY(colsum(dlogit, nullptr, ds, N, N, N, B, (long)N * N, 0, N, 0, nullptr, st));
    GC_TRY(node_score_bwd(ds, uvc, dX_in, dX, M, D, st));
  }  // RIDE: dlogit, ds and dX = ds u + dX_in ride in the dense edge pass below (`tail`; dlogit is never stored)
  if (compact)
    GC_TRY(cmp_bwd(eo.ce, v, n_valid, dlogit, dEbar, dE, dvpart, scratch + plan.rowbuf_off, dbias, plan, B, N, D, st));
  else
    GC_TRY(edge_bwd(eo.E, v, n_valid, dlogit, dEbar, dE, dvpart, plan, B, N, D, st, dq, &tail));  // + parked weight gradients
  // du = sum_m ds[m] X[m,:],  dv = sum partials,  dc = sum_m ds[m]: row-slice partials in one launch; the fold's
  // backward sums the slices itself (duvc stays unused)
  long part_off[3];
  int ns = 0;
  GC_TRY(colsum3(X, ds, duvc, M, D, D, dvpart, nullptr, duvc + D, M, D, D, ds, nullptr, duvc + 2 * D, M, 1, 1, scratch,
                 st, false, part_off, &ns));
  return gat_fold_bwd(flat, duvc, dflat, D, Dh, st, scratch, part_off, ns);
}

// ---- the output projection's backward in gcgcn_gcn_bwd (OutBwdQuery -> OutBwdPlan, gcn_plan.hpp) --------------------------------
// Pure.  q.fuse without q.scratch is not a query (chain_plan_bwd never fuses without workspace; the callers check).
static OutBwdPlan out_bwd_plan(const OutBwdQuery& q) {
  OutBwdPlan p = OutBwdPlan();
  const bool masked = q.ragged || q.odrop;   // gradients arriving on padding rows are ignored; back through the output dropout
  if (q.fuse) {  // the chain computes dHO = dout Wlin and dXres itself, masking / un-dropping dout while it stages it; only
                 // sum_h Wlin_h is left to this call, and dWlin and the column sums wait for the launch behind the chain
    p.mask = masked ? OutBwdPlan::MASK_CHAIN : OutBwdPlan::MASK_NONE;
    p.wsum = q.H == 1 ? OutBwdPlan::WSUM_NONE : q.wsum_fwd ? OutBwdPlan::WSUM_FORWARD : OutBwdPlan::WSUM_HERE;
    p.dwlin = OutBwdPlan::DWLIN_BACK;
    const bool in_chain = 2 * q.B <= COL_RIDE_SLICES;   // stage 1 inside the chain (it holds dout_b in LDS): two slices a document
    p.col1 = in_chain ? OutBwdPlan::COL1_CHAIN : OutBwdPlan::COL1_BACK;
    p.chain_slices = in_chain ? 2 * q.B : 0;
    return p;
  }
  p.mask = masked ? OutBwdPlan::MASK_LAUNCH : OutBwdPlan::MASK_NONE;
  // Small blocks (launch-bound: cfg 1, the reference's own model) fold the head-sum / dropout-backward kernel into the front
  // launch: dY = dropout_bwd(dHO) is the product's own epilogue (the forward mask: same site, same element offsets), and the
  // residual gradient dXres = sum_h dHO_h = dout (sum_h Wlin_h) is one more small product (one head: dHO itself, written
  // beside dY).  At cfg 3 the extra product and the second store cost more than the launch they save (round 2: +8 us).
  constexpr long fold_max = 2L << 20;   // elements of dHO up to which the fold pays
  const bool fold = q.scratch && (q.H == 1 || q.wsum_fwd) && (long)q.B * q.N * q.H * q.D <= fold_max && q.dxres_aligned;
  p.fold = !fold ? OutBwdPlan::FOLD_NONE : q.H == 1 ? OutBwdPlan::FOLD_ONE_HEAD : OutBwdPlan::FOLD_HEADS;
  p.fold_drop = fold && (q.H == 1 || q.drop);   // more heads: over C, the dropped value stays
  p.head_sum_launch = !fold;
  p.wsum = p.fold == OutBwdPlan::FOLD_HEADS ? OutBwdPlan::WSUM_FORWARD : OutBwdPlan::WSUM_NONE;
  p.dwlin = OutBwdPlan::DWLIN_FRONT;
  p.col1 = q.scratch ? OutBwdPlan::COL1_FRONT : OutBwdPlan::COL1_OWN_LAUNCH;
  return p;
}

// Where stage 2 of dblin's column sums runs, once gemm_group has said whether the front launch had a reduce pass to do it in
// (front_reduced; without a front launch it is not read).  Pure.
static OutBwdCol2 out_bwd_plan_col2(const OutBwdPlan& p, bool front_reduced) {
  switch (p.col1) {
    case OutBwdPlan::COL1_OWN_LAUNCH: return {OutBwdCol2::DONE, 0};
    case OutBwdPlan::COL1_CHAIN: return {OutBwdCol2::BACK_LAUNCH, p.chain_slices};
    case OutBwdPlan::COL1_BACK: return {OutBwdCol2::BACK_REDUCE, 0};
    default: break;  // FRONT
  }
  if (front_reduced) return {OutBwdCol2::FRONT_REDUCE, 0};
  if (p.head_sum_launch) return {OutBwdCol2::HEAD_SUM_KERNEL, 0};   // trailing workgroups of head_sum_drop_bwd
  return {OutBwdCol2::BACK_LAUNCH, COL_RIDE_SLICES};                // the fold left no kernel in between
}

}  // namespace gc

using namespace gc;

extern "C" {

int gcgcn_version(void) { return 7; }
const char* gcgcn_last_error(void) { return g_err; }

int gcgcn_set_option(const char* name, int value) {
  GC_REQUIRE(name, "set_option: null name");
  if (set_opt(name, value)) return 0;
  set_error("set_option: unknown option '%s'", name);
  return 1;
}

int64_t gcgcn_row_blocks_ints(int B, int N) { return (B > 0 && N > 0 && N % 16 == 0) ? row_blocks_ints(B, N) : 0; }
int gcgcn_row_blocks(int B, int N, const int32_t* n_valid, int32_t* out, void* stream) {
  return row_blocks(n_valid, B, N, out, (hipStream_t)stream);
}

int gcgcn_prof_start(const char* kernel_prefix, int capacity) {
  GC_REQUIRE(kernel_prefix && capacity > 0, "prof_start: bad arguments");
  for (hipEvent_t e : g_prof.ev) (void)hipEventDestroy(e);
  g_prof.ev.assign(2 * (size_t)capacity, nullptr);
  for (auto& e : g_prof.ev) {
    if (hipEventCreate(&e) != hipSuccess) {
      set_error("prof_start: hipEventCreate failed");
      return 2;
    }
  }
  strncpy(g_prof.filter, kernel_prefix, sizeof(g_prof.filter) - 1);
  g_prof.used = 0;
  g_prof.work = 0;
  g_prof.on = true;
  return 0;
}
int gcgcn_prof_enable(int on) {  // pause / resume recording without touching what was recorded
  g_prof.on = on != 0 && !g_prof.ev.empty();
  return 0;
}
int gcgcn_prof_stop(double* total_ms, int* launches, double* work) {
  GC_REQUIRE(total_ms && launches, "prof_stop: null pointer");
  if (work) *work = g_prof.work;
  g_prof.on = false;
  double tot = 0;
  for (int i = 0; i < g_prof.used; ++i) {
    float ms = 0.f;
    if (hipEventSynchronize(g_prof.ev[2 * i + 1]) != hipSuccess ||
        hipEventElapsedTime(&ms, g_prof.ev[2 * i], g_prof.ev[2 * i + 1]) != hipSuccess) {
      set_error("prof_stop: event query failed");
      return 2;
    }
    tot += ms;
  }
  *total_ms = tot;
  *launches = g_prof.used;
  for (hipEvent_t e : g_prof.ev) (void)hipEventDestroy(e);
  g_prof.ev.clear();
  g_prof.used = 0;
  return 0;
}

int gcgcn_rng_next(void* state, void* snaps, int count, void* stream) {
  GC_REQUIRE(state && snaps && count > 0, "rng_next: bad arguments");
  return rng_next(state, snaps, count, (hipStream_t)stream);
}
int gcgcn_dropout_keep(uint8_t* keep, int64_t n, const void* rng_snap, uint64_t salt, float p, void* stream) {
  GC_REQUIRE(keep && rng_snap, "dropout_keep: null pointer");
  Drop d = make_drop(rng_snap, salt, p);
  d.snap = (const uint64_t*)rng_snap;
  return dropout_keep(keep, n, d, (hipStream_t)stream);
}
int gcgcn_dropout(const float* x, float* y, int64_t n, const void* rng_snap, uint64_t salt, float p, void* stream) {
  GC_REQUIRE(x && y && rng_snap, "dropout: null pointer");
  GC_REQUIRE(p >= 0.f && p < 1.f, "dropout: p=%f out of [0,1)", p);
  Drop d = make_drop(rng_snap, salt, p);
  d.snap = (const uint64_t*)rng_snap;
  return dropout(x, y, n, d, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// GATAttention and the edge mean, on a dense E or on the producer's compact rows (compact.hip)
// ---------------------------------------------------------------------------------------------
int gcgcn_gat_layout(int D, int Dh, int64_t* o) {
  GC_REQUIRE(D > 0 && Dh > 0 && o, "gat_layout: bad arguments");
  const long DD = (long)Dh * D;
  o[0] = 0;              // W_h [Dh, D]
  o[1] = DD;             // b_h
  o[2] = o[1] + Dh;      // W_t
  o[3] = o[2] + DD;      // b_t
  o[4] = o[3] + Dh;      // W_r
  o[5] = o[4] + DD;      // b_r
  o[6] = o[5] + Dh;      // wt
  o[7] = o[6] + 3 * Dh;  // wt bias
  o[8] = o[7] + 1;
  return 0;
}

int gcgcn_gat_fwd(int B, int N, int D, int Dh, const float* X, const float* E, const int32_t* n_valid, const float* flat,
                  const void* rng_snap, float p, float* uvc, float* s, float* P, float* A, float* Ebar, void* rng_state,
                  void* rng_snaps, int rng_count, const uint8_t* mask, int uvc_valid, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  GC_TRY(check_dims("gat_fwd", B, N, D, 1, 1));
  GC_REQUIRE(Dh > 0, "gat_fwd: hidden_dim=%d", Dh);
  GC_REQUIRE(X && E && flat && uvc && s && P && Ebar, "gat_fwd: null pointer");
  const Drop drop = make_drop(rng_snap, GCGCN_SALT_GAT, p);
  GC_REQUIRE(!drop.snap || A, "gat_fwd: dropout on but A is NULL");
  GC_REQUIRE(!rng_state || (rng_snaps && rng_count > 0), "gat_fwd: rng_state given without snapshots to fill");
  GC_TRY(gat_node_fwd(X, flat, uvc, s, (long)B * N, D, Dh, uvc_valid, rng_state, rng_snaps, rng_count, st));
  return edge_fwd(E, uvc + D, n_valid, Ebar, s, P, A, drop, B, N, D, st, mask);  // + row softmax + dropout
}

int gcgcn_gat_fwd_compact(int B, int N, int D, int Dh, const float* X, const float* Ec, const int32_t* prow, const float* bias,
                          const int32_t* n_valid, const float* flat, const void* rng_snap, float p, float* uvc, float* s, float* P,
                          float* A, float* Ebar, void* rng_state, void* rng_snaps, int rng_count, int uvc_valid, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  GC_TRY(cmp_check("gat_fwd_compact", B, N, D, Ec, prow, bias));
  GC_REQUIRE(Dh > 0 && X && flat && uvc && s && P && Ebar, "gat_fwd_compact: null pointer");
  const Drop drop = make_drop(rng_snap, GCGCN_SALT_GAT, p);
  GC_REQUIRE(!drop.snap || A, "gat_fwd_compact: dropout on but A is NULL");
  GC_REQUIRE(!rng_state || (rng_snaps && rng_count > 0), "gat_fwd_compact: rng_state given without snapshots to fill");
  GC_TRY(gat_node_fwd(X, flat, uvc, s, (long)B * N, D, Dh, uvc_valid, rng_state, rng_snaps, rng_count, st));
  return cmp_fwd(CmpE{Ec, prow, bias}, uvc + D, n_valid, Ebar, s, P, A, drop, B, N, D, st);
}

int64_t gcgcn_gat_bwd_scratch(int B, int N, int D) { return edge_plan_bwd({B, N, D, false, true, false, false, 0}).scratch; }
int64_t gcgcn_gat_bwd_compact_scratch(int B, int N, int D) { return edge_plan_bwd({B, N, D, true, true, false, false, 0}).scratch; }

int gcgcn_gat_bwd(int B, int N, int D, int Dh, const float* X, const float* E, const int32_t* n_valid, const float* flat,
                  const void* rng_snap, float p, const float* uvc, const float* P, const float* dA, const float* dEbar,
                  const float* dX_in, float* dX, float* dE, float* dflat, float* dlogit, float* ds, float* dvpart,
                  float* duvc, float* scratch, void* defer_queue, void* stream) {
  GC_TRY(check_dims("gat_bwd", B, N, D, 1, 1));
  GC_REQUIRE(Dh > 0, "gat_bwd: hidden_dim=%d", Dh);
  GC_REQUIRE(X && E && flat && uvc && P && dA && dX && dflat && dlogit && ds && dvpart && duvc,
             "gat_bwd: null pointer");
  GC_REQUIRE(scratch, "gat_bwd: scratch is required");
  return gat_bwd(EdgeOperand{E, CmpE()}, B, N, D, Dh, X, n_valid, flat, make_drop(rng_snap, GCGCN_SALT_GAT, p), uvc, P, dA, dEbar, dX_in,
                 dX, dE, nullptr, dflat, dlogit, ds, dvpart, duvc, scratch, (DeferQueue*)defer_queue, (hipStream_t)stream);
}

int gcgcn_gat_bwd_compact(int B, int N, int D, int Dh, const float* X, const float* Ec, const int32_t* prow, const float* bias,
                          const int32_t* n_valid, const float* flat, const void* rng_snap, float p, const float* uvc, const float* P,
                          const float* dA, const float* dEbar, const float* dX_in, float* dX, float* dEc, float* dbias, float* dflat,
                          float* dlogit, float* ds, float* dvpart, float* duvc, float* scratch, void* stream) {
  GC_TRY(cmp_check("gat_bwd_compact", B, N, D, Ec, prow, bias));
  GC_REQUIRE(Dh > 0 && X && flat && uvc && P && dA && dX && dEc && dbias && dflat && dlogit && ds && dvpart && duvc && scratch,
             "gat_bwd_compact: null pointer");
  return gat_bwd(EdgeOperand{nullptr, CmpE{Ec, prow, bias}}, B, N, D, Dh, X, n_valid, flat, make_drop(rng_snap, GCGCN_SALT_GAT, p), uvc, P,
                 dA, dEbar, dX_in, dX, dEc, dbias, dflat, dlogit, ds, dvpart, duvc, scratch, nullptr, (hipStream_t)stream);
}

int gcgcn_edge_mean_fwd(int B, int N, int D, const float* E, const int32_t* n_valid, float* Ebar, void* stream) {
  return edge_fwd(E, nullptr, n_valid, Ebar, nullptr, nullptr, nullptr, make_drop(nullptr, 0, 0.f), B, N, D,
                  (hipStream_t)stream);
}
int gcgcn_edge_mean_bwd(int B, int N, int D, const float* dEbar, const int32_t* n_valid, float* dE, void* stream) {
  GC_REQUIRE(B > 0 && N > 0 && D > 0, "edge_mean_bwd: bad shape");
  return edge_bcast(dEbar, n_valid, dE, B, N, D, (hipStream_t)stream);
}

int gcgcn_edge_mean_fwd_compact(int B, int N, int D, const float* Ec, const int32_t* prow, const float* bias, const int32_t* n_valid,
                                float* Ebar, void* stream) {
  GC_TRY(cmp_check("edge_mean_fwd_compact", B, N, D, Ec, prow, bias));
  GC_REQUIRE(Ebar, "edge_mean_fwd_compact: null pointer");
  return cmp_fwd(CmpE{Ec, prow, bias}, nullptr, n_valid, Ebar, nullptr, nullptr, nullptr, make_drop(nullptr, 0, 0.f), B, N, D,
                 (hipStream_t)stream);
}

int gcgcn_edge_mean_bwd_compact(int B, int N, int D, const int32_t* prow, const int32_t* n_valid, const float* dEbar, float* dEc,
                                float* dbias, float* rowbuf, void* stream) {
  GC_REQUIRE(B > 0 && N > 0 && D > 0, "edge_mean_bwd_compact: bad shape B=%d N=%d D=%d", B, N, D);
  GC_REQUIRE(D <= 64 * CMAXK, "edge_mean_bwd_compact: hidden width %d (compact rows support up to %d)", D, 64 * CMAXK);
  GC_REQUIRE(prow && dEbar && dEc && dbias && rowbuf, "edge_mean_bwd_compact: null pointer");
  return cmp_bwd(CmpE{nullptr, prow, nullptr}, nullptr, n_valid, nullptr, dEbar, dEc, nullptr, rowbuf, dbias,
                 edge_plan_bcast({B, N, D, true, false, false, true, 0}), B, N, D, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// MultiHeadAttention
// ---------------------------------------------------------------------------------------------
int gcgcn_mha_layout(int D, int64_t* o) {
  GC_REQUIRE(D > 0 && o, "mha_layout: bad arguments");
  o[0] = 0;
  o[1] = (long)D * D;
  o[2] = o[1] + D;
  return 0;
}

int gcgcn_mha_fwd(int B, int N, int D, int H, const float* X, const int32_t* n_valid, const float* flat,
                  const void* rng_snap, float p, float* Q, float* P, float* A, float* scratch, const int32_t* rowblk, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  GC_TRY(check_dims("mha_fwd", B, N, D, 1, H));
  const long wse = scratch ? gemm_scratch_elems(B, N, D, 1) : 0;
  GC_REQUIRE(X && flat && Q && P, "mha_fwd: null pointer");
  const AttnPlan plan = attn_plan_fwd(make_attn_query(N, D, H, Q, nullptr, false, false, false));
  const GcnCtx::MhaFwd m = attn_core(GcnCtx::MhaFwd{Q, P, A}, D, H, plan, rng_snap, p);
  GC_REQUIRE(!m.drop.snap || A, "mha_fwd: dropout on but A is NULL");
  const long M = (long)B * N;
  {  // Q = X Wq^T + bq      (glove:136, all heads at once)
    GemmArgs g = gemm_nt(X, D, flat, D, Q, D, (int)M, D, D).split_ws(scratch, wse);
    g.bias = flat + (long)D * D;
    use_rows(g, live_rows(rowblk, N, n_valid != nullptr), 1, 1);
    GC_TRY(gemm(g, st));
  }
  switch (plan.route) {
    case AttnPlan::CORE: return mha_core_fwd(m, n_valid, B, N, D, H, st);
    default: {  // GEMM: S[b,h] = Q_h Q_h^T / sqrt(dh)   (glove:137-138: keys use the query projection), then the row softmax
      GemmArgs g = gemm_nt(Q, D, Q, D, P, N, N, N, m.dh).split_ws(scratch, wse);
      g.batch_z1(B, (long)N * D, (long)N * D, (long)H * N * N).batch_z2(H, m.dh, m.dh, (long)N * N);
      g.alpha = m.alpha;
      GC_TRY(gemm(g, st));
      return softmax_fwd(P, nullptr, n_valid, P, A, M * H, N, H, m.drop, st);
    }
  }
}

int64_t gcgcn_mha_scratch(int B, int N, int D) { return scratch_elems(B, N, D, 1); }

int gcgcn_mha_bwd(int B, int N, int D, int H, const float* X, const float* flat, const void* rng_snap, float p,
                  const float* Q, const float* P, const float* dA, const float* dX_in, float* dX, float* dflat, float* dS,
                  float* dQ, float* scratch, void* defer_queue, int core_done, const int32_t* rowblk, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  GC_TRY(check_dims("mha_bwd", B, N, D, 1, H));
  const long wse = scratch ? gemm_scratch_elems(B, N, D, 1) : 0;
  GC_REQUIRE(X && flat && Q && P && dA && dX && dflat && dS && dQ, "mha_bwd: null pointer");
  const AttnPlan plan = attn_plan_bwd(make_attn_query(N, D, H, Q, dQ, false, false, core_done != 0));
  const MhaPass mp = attn_core(mha_pass(Q, P, dA, dQ, B, N, D, H), D, H, plan, rng_snap, p);
  const long M = (long)B * N;
  switch (plan.route) {
    case AttnPlan::DONE: break;
    case AttnPlan::CORE: GC_TRY(mha_core_bwd(mp, st)); break;
    default:  // GEMM
      GC_TRY(softmax_bwd(P, dA, dS, M * H, N, mp.drop, st));
      for (int pass = 0; pass < 2; ++pass) {  // dQ_h = alpha (dS + dS^T) Q_h: dS Q_h, then += dS^T Q_h
        GemmArgs g = (pass == 0 ? gemm_nn : gemm_tn)(dS, N, Q, D, dQ, D, N, mp.dh, N).split_ws(scratch, wse);
        g.batch_z1(B, (long)H * N * N, (long)N * D, (long)N * D).batch_z2(H, (long)N * N, mp.dh, mp.dh);
        g.alpha = mp.alpha, g.accumulate = pass;
        GC_TRY(gemm(g, st));
      }
  }
  {  // one launch: dX = dQ Wq  and  dWq = dQ^T X
    GemmArgs gs[2] = {gemm_nn(dQ, D, flat, D, dX, D, (int)M, D, D).split_ws(scratch, wse),
                      gemm_tn(dQ, D, X, D, dflat, D, D, D, (int)M).split_ws(scratch, wse)};
    gs[0].add = dX_in, gs[0].ldadd = D;  // + the gradient X already collected downstream (NULL = none)
    const int* rows = live_rows(rowblk, N, true);   // (a list is only handed in for a ragged batch): the rows that exist
    use_rows(gs[0], rows, 1, 1), use_rows(gs[1], rows, 2);
    const int ng = gemm_defer((DeferQueue*)defer_queue, gs[1]) ? 1 : 2;  // dWq parked (see gcgcn_gcn_bwd)
    if (scratch) {  // dbq = column sums of dQ ride in the same two launches
      const ColRide cr = col_sum(dQ, M, D, D, dflat + (long)D * D, scratch + wse);
      // with dWq parked the launch has nothing to reduce: the sums' second stage (one workgroup) would be a launch of its own --
      // it is parked too (nobody reads dbq before the end of backward; `scratch` must then outlive the call like dQ and X)
      bool later = false;
      GC_TRY(gemm_group(gs, ng, st, &cr, (ng == 1 && defer_queue) ? &later : nullptr));
      if (later) {  // finish stage 2: park it or run it now
        const ColRide c2 = cr.stage2(COL_RIDE_SLICES);
        if (!gemm_defer_col2((DeferQueue*)defer_queue, c2)) GC_TRY(col_sum_stage2_launch(c2, st));
      }
    } else {
      GC_TRY(gemm_group(gs, ng, st));
      GC_TRY(colsum(dQ, nullptr, dflat + (long)D * D, M, D, D, 1, 0, 0, 0, 0, scratch, st));
    }
  }
  return 0;
}

void* gcgcn_defer_create(void) { return new (std::nothrow) DeferQueue(); }
void gcgcn_defer_destroy(void* queue) { delete (DeferQueue*)queue; }
int gcgcn_defer_count(const void* queue) { return queue ? ((const DeferQueue*)queue)->n + ((const DeferQueue*)queue)->ncol2 : 0; }
int gcgcn_defer_flush(void* queue, void* stream) { return gemm_flush_deferred((DeferQueue*)queue, (hipStream_t)stream); }

// ---------------------------------------------------------------------------------------------
// trainer loss
// ---------------------------------------------------------------------------------------------
int gcgcn_pair_bce_fwd(int B, int N, int R, const float* logits, const float* labels, const int32_t* n_valid, float* loss,
                       float* part, void* stream) {
  GC_REQUIRE(B > 0 && N > 0 && R > 0 && (long)B * N <= 0x7fffffffL && (long)N * R <= 0x7fffffffL,
             "pair_bce_fwd: bad shape B=%d N=%d R=%d", B, N, R);
  GC_REQUIRE(logits && labels && loss && part, "pair_bce_fwd: null pointer");
  return pair_bce_fwd(logits, labels, n_valid, loss, part, B, N, R, (hipStream_t)stream);
}

int gcgcn_pair_bce_bwd(int B, int N, int R, const float* logits, const float* labels, const int32_t* n_valid,
                       const float* dloss, float* dlogits, void* stream) {
  GC_REQUIRE(B > 0 && N > 0 && R > 0, "pair_bce_bwd: bad shape B=%d N=%d R=%d", B, N, R);
  GC_REQUIRE(logits && labels && dlogits, "pair_bce_bwd: null pointer");
  return pair_bce_bwd(logits, labels, n_valid, dloss, dlogits, B, N, R, (hipStream_t)stream);
}

int gcgcn_pair_stats(int B, int N, int R, const float* logits, const float* labels, const int32_t* n_valid, int64_t* counters,
                     void* stream) {
  GC_REQUIRE(B > 0 && N > 0 && R > 0 && (long)B * N <= 0x7fffffffL && (long)N * R <= 0x7fffffffL,
             "pair_stats: bad shape B=%d N=%d R=%d", B, N, R);
  GC_REQUIRE(logits && labels && counters, "pair_stats: null pointer");
  return pair_stats(logits, labels, n_valid, counters, B, N, R, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// GraphConvolution / MultiGraphConvolution
// ---------------------------------------------------------------------------------------------
int gcgcn_gcn_layout(int D, int L, int H, int64_t* o) {
  GC_TRY(check_dims("gcn_layout", 1, 1, D, L, H));
  GC_REQUIRE(o, "gcn_layout: null pointer");
  const GcnLayout y = gcn_layout(D, L, H);
  o[0] = y.oWnX, o[1] = y.oWe, o[2] = y.oWd, o[3] = y.oWlin, o[4] = y.oblin, o[5] = y.total, o[6] = y.wd_head;
  return 0;
}

int gcgcn_gcn_fwd(int B, int N, int D, int L, int H, const float* X, const float* Ebar, const float* A,
                  const int32_t* n_valid, const float* flat, const void* rng_snap, float p, const void* out_rng_snap,
                  float out_p, float* out, float* Pn, float* Y, float* HO, float* rinv, float* G, float* wsum, float* scratch,
                  const gcgcn_edge_ride* ride, const gcgcn_mha_hook* mha, const int32_t* rowblk, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  GC_TRY(check_dims("gcn_fwd", B, N, D, L, H));
  AttnQuery aq = make_attn_query(N, D, H, mha ? mha->Q : nullptr, nullptr, mha != nullptr, false, false);
  const int refusal = attn_hook_refusal(aq);   // (no hook: served)
  GC_REQUIRE(refusal != ATTN_REFUSED_SHAPE, "gcn_fwd: attention hook on a shape it does not serve");
  GC_REQUIRE(!mha || (mha->flat_q && mha->Q && mha->P), "gcn_fwd: attention hook on a shape it does not serve");
  GC_REQUIRE(refusal != ATTN_REFUSED_ALIGN, "gcn_fwd: attention hook: misaligned Q");
  if (mha) A = mha->A ? mha->A : mha->P;   // what the attention core below writes
  EdgeRide er;
  GC_TRY(make_ride("gcn_fwd", ride, 1, er));
  const long wse = scratch ? gemm_scratch_elems(B, N, D, H) : 0;
  GC_REQUIRE(X && Ebar && A && flat && out && Pn && Y && HO && rinv && G, "gcn_fwd: null pointer");
  const GcnLayout y = gcn_layout(D, L, H);
  const Drop drop = make_drop(rng_snap, GCGCN_SALT_GCN, p);
  const long M = (long)B * N;
  const long HD = (long)H * D;
  GC_REQUIRE(M <= 0x7fffffffL, "gcn_fwd: B*N too large");
  // The per-(doc, head) context, with the passenger that will actually ride attached.  Ragged batch with a row-block list:
  // the products around the chain run on the rows that exist; what they leave on the dead row blocks is ZERO (rb_zero), so the
  // chain kernels -- whichever serves the shape -- see exactly what the dense products would have left there.
  ChainQuery q = make_query(B, N, D, L, H, y, flat, n_valid != nullptr, scratch != nullptr, mha != nullptr, er, A, Pn, Y);
  q.G = G, q.HO = HO, q.X = X;
  const ChainPlan plan = chain_plan_fwd(q);
  aq.chain_attends = plan.attention;   // the hook's core runs where the chain plan lets it
  const AttnPlan ap = attn_plan_fwd(aq);
  GcnCtx c = make_ctx(B, N, D, L, H, y, X, A, flat, n_valid, drop);
  c.G = G, c.Pn = Pn, c.Y = Y, c.HO = HO, c.rinv = rinv;
  if (plan.ride) c.ride = er;
  const int* rows = live_rows(rowblk, N, n_valid != nullptr);

  {  // one launch: Pn = X WnX (node term of every (head, sub-layer), X part of the dense input)
     //             G  = Ebar We (edge term, mean commuted with the projection, glove:40-41)
    GemmArgs g3[3] = {gemm_nn(X, D, flat + y.oWnX, HD, Pn, HD, (int)M, (int)HD, D).split_ws(scratch, wse),
                      gemm_nn(Ebar, D, flat + y.oWe, HD, G, HD, (int)M, (int)HD, D).split_ws(scratch, wse), GemmArgs()};
    const int ng = mha ? 3 : 2;
    if (mha) {  // Q = X Wq^T + bq (glove:136, all heads at once): one more problem of this launch
      g3[2] = gemm_nt(X, D, mha->flat_q, D, mha->Q, D, (int)M, D, D).split_ws(scratch, wse);
      g3[2].bias = mha->flat_q + (long)D * D;
    }
    for (int q = 0; q < ng; ++q) use_rows(g3[q], rows, 1, 1);   // (the attention core stages all N rows of Q: zeros past the live blocks)
    // wsum = sum_h Wlin[:, h, :] (a by-product for gcgcn_gcn_bwd) in trailing workgroups of this launch
    const ColRide hs = head_sum(flat + y.oWlin, H, D, wsum);
    GC_TRY(gemm_group(g3, ng, st, (wsum && H > 1) ? &hs : nullptr));
  }
  {  // the dependent per-(doc, head) sequence: normaliser, then per sub-layer dense connection + aggregation
    if (er.kind && !plan.ride) {  // the riding pass as its own launch
      GC_TRY(edge_fwd(er.in, nullptr, er.n_valid, er.out, nullptr, nullptr, nullptr, Drop(), er.B, er.N, er.D, st));
      er.kind = 0;
    }
    if (mha) {  // the attention core: scores in LDS, P / A out (glove:137-140)
      const GcnCtx::MhaFwd m = attn_core(GcnCtx::MhaFwd{mha->Q, mha->P, mha->A}, D, H, ap, mha->rng_snap, mha->p);
      GC_REQUIRE(!m.drop.snap || mha->A, "gcn_fwd: attention dropout on but A is NULL");
      switch (ap.route) {
        case AttnPlan::CHAIN: c.mha = m; break;                              // the prologue of the chain launch below
        default: GC_TRY(mha_core_fwd(m, n_valid, B, N, D, H, st));           // CORE: a launch of its own
      }
    }
    if (plan.kind != ChainPlan::NONE) {
      GC_TRY(gcn_chain_fwd(c, plan, st));
    } else {
      GC_TRY(rowsum_inv(A, rinv, (long)B * H * N, N, st));  // glove:47-49
      for (int l = 0; l < L; ++l) {
        if (l > 0) GC_TRY(gemm(plan_fwd_dense(c, l), st, 0, 1));
        GC_TRY(gemm(plan_fwd_agg(c, l), st, 0, 1));
      }
    }
  }
  {  // out = HO Wlin^T + blin   (glove:78 / 118)
    GemmArgs g = gemm_nt(HO, HD, flat + y.oWlin, HD, out, D, (int)M, D, (int)HD).split_ws(scratch, wse);
    g.bias = flat + y.oblin;
    g.n_valid = n_valid, g.nv_rows = N, g.nv_zdoc = 0;
    use_rows(g, rows, 1, 1);   // the block's output: its padding rows are zero
    const Drop odrop = make_drop(out_rng_snap, GCGCN_SALT_GLUE, out_p);
    if (odrop.snap) {  // the hop's output dropout (glove:341) in the same epilogue: out = dropout(linear)
      g.C = G;         // the undropped values go to workspace that is free by now; nobody reads them
      g.C2 = out, g.ldc2 = D;
      g.drop = odrop;
    }
    GC_TRY(gemm(g, st));
  }
  return 0;
}

int64_t gcgcn_gcn_scratch(int B, int N, int D, int H) { return scratch_elems(B, N, D, H); }

int gcgcn_gcn_bwd(int B, int N, int D, int L, int H, const float* X, const float* Ebar, const float* A,
                  const int32_t* n_valid, const float* flat, const void* rng_snap, float p, const void* out_rng_snap,
                  float out_p, const float* Pn, const float* Y, const float* HO, const float* rinv, const float* wsum_fwd,
                  const float* dout, float* dX, float* dEbar,
                  float* dA, float* dflat, float* W1, float* W2, float* W3, float* drow, float* dXres, float* dout_m,
                  float* scratch, const gcgcn_edge_ride* ride, const gcgcn_mha_hook* mha, void* defer_queue, const int32_t* rowblk,
                  void* stream) {
  DeferQueue* dq = (DeferQueue*)defer_queue;
  MhaPass mp;
  AttnPlan ap;
  if (mha) {
    const AttnQuery aq = make_attn_query(N, D, H, mha->Q, mha->dQ, true, false, false);
    GC_REQUIRE(!attn_hook_refusal(aq) && mha->Q && mha->P && mha->dQ, "gcn_bwd: attention hook on a shape it does not serve");
    ap = attn_plan_bwd(aq);
    mp = attn_core(mha_pass(mha->Q, mha->P, dA, mha->dQ, B, N, D, H), D, H, ap, mha->rng_snap, mha->p);
  }
  const Drop odrop = make_drop(out_rng_snap, GCGCN_SALT_GLUE, out_p);
  hipStream_t st = (hipStream_t)stream;
  GC_TRY(check_dims("gcn_bwd", B, N, D, L, H));
  EdgeRide er;
  GC_TRY(make_ride("gcn_bwd", ride, 2, er));
  const long wse = scratch ? gemm_scratch_elems(B, N, D, H) : 0;
  GC_REQUIRE(X && Ebar && A && flat && Pn && Y && HO && rinv && dout && dX && dEbar && dA && dflat && W1 && W2 && W3 &&
                 drow && dXres,
             "gcn_bwd: null pointer");
  GC_REQUIRE(!(n_valid || odrop.snap) || dout_m, "gcn_bwd: n_valid / output dropout given without dout_m workspace");
  const GcnLayout y = gcn_layout(D, L, H);
  const Drop drop = make_drop(rng_snap, GCGCN_SALT_GCN, p);
  const long M = (long)B * N;
  const int gh = y.gh;
  const long HD = (long)H * D;
  float* dYa = W1;  // dHO, then the running gradient of the relu outputs Y (same layout)
  float* dM = W2;   // gradient of M_l = G_l + A_h Pn_l  (== dG)
  float* dP = W3;   // gradient of Pn_l

  // Where the plan says fuse, the chain kernel computes dHO = dout Wlin and dXres = sum_h dHO_h itself (chain.hip): no launch for
  // that product, no head-sum / dropout kernel, dHO never in HBM.
  ChainQuery q = make_query(B, N, D, L, H, y, flat, n_valid != nullptr, scratch != nullptr, false, er, A, Pn, Y);
  q.dYa = dYa, q.dM = dM, q.dP = dP, q.dA = dA, q.dout = dout, q.dXres = dXres, q.dout_m = dout_m;
  const ChainPlan plan = chain_plan_bwd(q);
  GC_REQUIRE(!plan.fuse || scratch, "gcn_bwd: the fused chain backward without scratch");   // (chain_plan_bwd: fuse needs q.scratch)
  const OutBwdPlan ob = out_bwd_plan({plan.fuse, B, N, D, H, scratch != nullptr, wsum_fwd != nullptr, n_valid != nullptr,
                                      odrop.snap != nullptr, drop.snap != nullptr, al16(dXres)});
  GcnCtx c = make_ctx(B, N, D, L, H, y, X, A, flat, n_valid, drop);
  c.Pn = const_cast<float*>(Pn), c.Y = const_cast<float*>(Y), c.rinv = const_cast<float*>(rinv);
  c.dYa = dYa, c.dM = dM, c.dP = dP, c.dA = dA, c.drow = drow, c.oWlin = y.oWlin;
  // ragged batch with a row-block list: the products around the chain run on the rows that exist (see gcgcn_gcn_fwd)
  if (plan.ride) c.ride = er;
  const int* rows = live_rows(rowblk, N, n_valid != nullptr);
  // sum_h Wlin_h: from the forward call if it left one, else summed here into dYa's buffer (free when the chain computes dHO)
  const float* wsum = ob.wsum == OutBwdPlan::WSUM_FORWARD ? wsum_fwd : ob.wsum == OutBwdPlan::WSUM_HERE ? dYa : nullptr;
  if (ob.wsum == OutBwdPlan::WSUM_HERE) GC_TRY(mask_rows(nullptr, nullptr, M, D, N, nullptr, odrop, st, flat + y.oWlin, dYa, H));
  const float* dout_raw = dout;
  if (ob.mask == OutBwdPlan::MASK_LAUNCH) GC_TRY(mask_rows(dout, dout_m, M, D, N, n_valid, odrop, st));
  if (ob.mask != OutBwdPlan::MASK_NONE) dout = dout_m;   // (MASK_CHAIN: the chain writes it back for dWlin)
  // dWlin = dout^T HO: a weight gradient nobody needs before the end of backward.  It is parked for a later launch with idle
  // matrix pipes, or runs in the launch in front of the chain -- where the chain computes dHO (fuse), in the one behind it
  GemmArgs dWlin = gemm_tn(dout, D, HO, HD, dflat + y.oWlin, HD, D, (int)HD, (int)M).split_ws(scratch, wse);
  use_rows(dWlin, rows, 2);
  // dblin = column sums of dout: they ride in launches of this call where it has workspace (every Col1 but OWN_LAUNCH)
  const ColRide cr = ob.col1 != OutBwdPlan::COL1_OWN_LAUNCH ? col_sum(dout, M, D, D, dflat + y.oblin, scratch + wse) : ColRide();
  bool front_reduced = false;
  if (plan.fuse) {
    c.dout = dout_raw, c.dXres = dXres, c.Wsum = wsum;
    if (dout != dout_raw) c.dout_m = dout_m, c.odrop = odrop;   // c.n_valid is set
    if (ob.col1 == OutBwdPlan::COL1_CHAIN) c.colpart = cr.part;
  } else {  // one launch: dHO = dout Wlin  and  dWlin = dout^T HO  (+ the fold: out_bwd_plan)
    GemmArgs run[3];
    int nr = 1;
    GemmArgs& dHO = run[0];
    dHO = gemm_nn(dout, D, flat + y.oWlin, HD, dYa, HD, (int)M, (int)HD, D).split_ws(scratch, wse);
    use_rows(dHO, rows, 1, 1);
    if (ob.fold == OutBwdPlan::FOLD_ONE_HEAD) dHO.C = dXres, dHO.ldc = D;   // HD == D: the head sum is dHO
    if (ob.fold_drop) dHO.C2 = dYa, dHO.ldc2 = HD, dHO.drop = drop, dHO.drop_base = 0;
    if (!gemm_defer(dq, dWlin)) run[nr++] = dWlin;
    if (ob.fold == OutBwdPlan::FOLD_HEADS) {  // dXres = dout (sum_h Wlin_h)
      run[nr] = gemm_nn(dout, D, wsum, D, dXres, D, (int)M, D, D).split_ws(scratch, wse);
      use_rows(run[nr++], rows, 1, 1);
    }
    if (ob.col1 == OutBwdPlan::COL1_FRONT) {  // stage 1 rides here; stage 2 in this launch's reduce, if it has one
      bool later = false;
      GC_TRY(gemm_group(run, nr, st, &cr, &later));
      front_reduced = !later;
    } else {
      GC_TRY(gemm_group(run, nr, st));
      GC_TRY(colsum(dout, nullptr, dflat + y.oblin, M, D, D, 1, 0, 0, 0, 0, scratch, st));
    }
  }
  const OutBwdCol2 col2 = out_bwd_plan_col2(ob, front_reduced);
  if (ob.head_sum_launch) {  // residual + dropout backward (+ stage 2 of the column sums in trailing workgroups)
    const ColRide fin = cr.stage2(COL_RIDE_SLICES);
    GC_TRY(head_sum_drop_bwd(dYa, dYa, dXres, M, H, D, drop, st, col2.where == OutBwdCol2::HEAD_SUM_KERNEL ? &fin : nullptr));
  }
  // what is left of the column sums rides in the launch behind the chain: their second stage, or both
  const ColRide back = col2.where == OutBwdCol2::BACK_LAUNCH ? cr.stage2(col2.back_ready_slices) : cr;
  const bool back_rides = col2.where == OutBwdCol2::BACK_LAUNCH || col2.where == OutBwdCol2::BACK_REDUCE;

  {  // the dependent per-(doc, head) sequence, last sub-layer first
    if (er.kind && !c.ride.kind) {
      GC_TRY(edge_bcast(er.in, er.n_valid, er.out, er.B, er.N, er.D, st));
      er.kind = 0;
    }
    if (plan.kind != ChainPlan::NONE) {
      GC_TRY(gcn_chain_bwd(c, plan, st, dq));  // + parked weight gradients of earlier blocks where the chain leaves room
    } else {
      for (int l = L - 1; l >= 0; --l) {
        GC_TRY(relu_norm_bwd(dYa, Y, rinv, dM, drow, M, N, H, L, gh, l, l == L - 1, st));
        GC_TRY(gemm(plan_bwd_dP(c, l), st, 0, 1));
        GC_TRY(gemm(plan_bwd_dA(c, l), st, 0, 1));
        if (l > 0) GC_TRY(gemm(plan_bwd_dY(c, l), st, 0, 1));
      }
    }
  }
  {  // one launch for every product that only needs the finished dPn / dM:
     //   dWnX = X^T dPn, dWe = Ebar^T dM, dX = dPn WnX^T + sum_h dHO_h, dEbar = dM We^T,
     //   dWd_{h,l} = [Y_0 .. Y_{l-1}]_h^T dPn_{h,l}  (l >= 1, batched over heads)
    constexpr int GMAX = 16;
    GemmArgs gs[GMAX];
    int n = 0;
    auto weight_grad = [&](GemmArgs g) {  // over the rows that exist; parked if asked to (and possible)
      use_rows(g.split_ws(scratch, wse), rows, 2);
      if (!gemm_defer(dq, g)) gs[n++] = g;
    };
    auto data_grad = [&](GemmArgs g) -> GemmArgs& {  // the gradients that leave the block: zero on padding rows
      use_rows(g.split_ws(scratch, wse), rows, 1, 1);
      return gs[n++] = g;
    };
    if (ob.dwlin == OutBwdPlan::DWLIN_BACK) weight_grad(dWlin);
    weight_grad(gemm_tn(X, D, dP, HD, dflat + y.oWnX, HD, D, (int)HD, (int)M));
    weight_grad(gemm_tn(Ebar, D, dM, HD, dflat + y.oWe, HD, D, (int)HD, (int)M));
    GemmArgs& gx = data_grad(gemm_nt(dP, HD, flat + y.oWnX, HD, dX, D, (int)M, D, (int)HD));
    gx.add = dXres, gx.ldadd = D;
    data_grad(gemm_nt(dM, HD, flat + y.oWe, HD, dEbar, D, (int)M, D, (int)HD));
    for (int l = 1; l < L; ++l) {
      if (n == GMAX) {  // many sub-layers and nothing parked: launch what has been described so far
        GC_TRY(gemm_group(gs, n, st));
        n = 0;
      }
      weight_grad(gemm_tn(Y, HD, dP + (long)l * gh, HD, dflat + y.wd_off(0, l), gh, l * gh, gh, (int)M)
                      .batch_z2(H, (long)L * gh, (long)L * gh, y.wd_head));
    }
    const MhaPass* riders = nullptr;   // + the attention core's backward, where attn_plan_bwd put it
    if (mha) switch (ap.route) {
        case AttnPlan::GROUP: riders = &mp; break;        // passenger workgroups of this launch
        default: GC_TRY(mha_core_bwd(mp, st));            // CORE: a launch of its own in front of it
      }
    GC_TRY(gemm_group(gs, n, st, back_rides ? &back : nullptr, nullptr, riders));
  }
  return 0;
}

int gcgcn_maggc_fusable(int N, int D, int H) { return attn_plan_fwd(make_attn_query(N, D, H, nullptr, nullptr, false, false, false)).fusable; }

// ---------------------------------------------------------------------------------------------
// GraphConv (the leaf layer, glove:18-50): out = (Ebar We + A X Wn (+ bias)) / rowsum(A)
// ---------------------------------------------------------------------------------------------
int gcgcn_graphconv_fwd(int B, int N, int Din, int De, int Dout, const float* X, const float* Ebar, const float* A,
                        const float* We, const float* Wn, const float* bias, float* out, float* T, float* rinv,
                        float* scratch, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  GC_REQUIRE(B > 0 && N > 0 && Din > 0 && De > 0 && Dout > 0, "graphconv_fwd: bad shape");
  GC_REQUIRE(X && Ebar && A && We && Wn && out && T && rinv, "graphconv_fwd: null pointer");
  const long M = (long)B * N;
  const long wse = scratch ? scratch_elems(B, N, Dout > Din ? Dout : Din, 1) : 0;
  GC_TRY(rowsum_inv(A, rinv, M, N, st));
  {  // one launch: out <- Ebar We (edge term),  T <- X Wn
    GemmArgs gs[2] = {gemm_nn(Ebar, De, We, Dout, out, Dout, (int)M, Dout, De).split_ws(scratch, wse),
                      gemm_nn(X, Din, Wn, Dout, T, Dout, (int)M, Dout, Din).split_ws(scratch, wse)};
    GC_TRY(gemm_group(gs, 2, st));
  }
  {  // out = (out + A T + bias) * rinv        (glove:42-50; the bias joins before the division, glove:45-46)
    GemmArgs g = gemm_nn(A, N, T, Dout, out, Dout, N, Dout, N).batch_z1(B, (long)N * N, (long)N * Dout, (long)N * Dout);
    g.add = out, g.ldadd = Dout, g.sAdd1 = (long)N * Dout;
    g.bias = bias;
    g.rowscale = rinv, g.sRs1 = N;
    GC_TRY(gemm(g, st, 0, 1));
  }
  return 0;
}

int gcgcn_graphconv_bwd(int B, int N, int Din, int De, int Dout, const float* X, const float* Ebar, const float* A,
                        const float* We, const float* Wn, const float* out, const float* T, const float* rinv,
                        const float* dout, float* dX, float* dEbar, float* dA, float* dWe, float* dWn, float* dbias,
                        float* dS, float* dT, float* drow, float* scratch, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  GC_REQUIRE(B > 0 && N > 0 && Din > 0 && De > 0 && Dout > 0, "graphconv_bwd: bad shape");
  GC_REQUIRE(X && Ebar && A && We && Wn && out && T && rinv && dout && dX && dEbar && dA && dWe && dWn && dS && dT &&
                 drow,
             "graphconv_bwd: null pointer");
  const long M = (long)B * N;
  const long wse = scratch ? scratch_elems(B, N, Dout > Din ? Dout : Din, 1) : 0;
  // dS = dout * rinv ;  drow = -rinv * sum_c dout * out      (no relu in the leaf)
  GC_TRY(relu_norm_bwd(dout, out, rinv, dS, drow, M, N, 1, 1, Dout, 0, 1, st, 0));
  if (dbias) GC_TRY(colsum(dS, nullptr, dbias, M, Dout, Dout, 1, 0, 0, 0, 0, scratch, st));
  {  // dT = A^T dS
    GemmArgs g = gemm_tn(A, N, dS, Dout, dT, Dout, N, Dout, N).batch_z1(B, (long)N * N, (long)N * Dout, (long)N * Dout);
    GC_TRY(gemm(g, st, 0, 1));
  }
  GemmArgs gs[5] = {
      gemm_nt(dS, Dout, T, Dout, dA, N, N, N, Dout).batch_z1(B, (long)N * Dout, (long)N * Dout, (long)N * N),  // dA = dS T^T + drow
      gemm_tn(Ebar, De, dS, Dout, dWe, Dout, De, Dout, (int)M),                                                // dWe = Ebar^T dS
      gemm_nt(dS, Dout, We, Dout, dEbar, De, (int)M, De, Dout),                                                // dEbar = dS We^T
      gemm_tn(X, Din, dT, Dout, dWn, Dout, Din, Dout, (int)M),                                                 // dWn = X^T dT
      gemm_nt(dT, Dout, Wn, Dout, dX, Din, (int)M, Din, Dout)};                                                // dX = dT Wn^T
  for (auto& g : gs) g.split_ws(scratch, wse);
  gs[0].rowadd = drow, gs[0].sRa1 = N;   // (broadcast along j)
  GC_TRY(gemm_group(gs, 5, st));
  return 0;
}

// The placement of tile passengers among the rows of a carrying launch (Spread, common.hpp), evaluated on the host with the
// very function the kernels call: for every workgroup index x of a launch of n_tiles + n_others workgroups, kind[x] = 1 and
// ordinal[x] = the tile's number, or kind[x] = 0 and ordinal[x] = the row's number.  Exposed for tests (no GPU needed).
int gcgcn_debug_spread(int64_t n_tiles, int64_t n_others, int64_t cohort, int64_t pct, int32_t* kind, int32_t* ordinal) {
  GC_REQUIRE(n_tiles >= 0 && n_others >= 0 && kind && ordinal, "debug_spread: bad arguments");
  const Spread sp = make_spread(n_tiles, n_others, cohort, pct);
  for (long x = 0; x < n_tiles + n_others; ++x) {
    int idx = -1;
    kind[x] = spread_pick((int)x, sp, idx) ? 1 : 0;
    ordinal[x] = idx;
  }
  return 0;
}

// The chain kernel a convolution call of this shape gets, by the very plan function gcgcn_gcn_fwd / _bwd call (chain.hip), on
// made-up operand addresses: misalign bit 0 puts the per-(document, head) tensors off a 16-byte boundary, bit 1 the output
// projection's dout / dXres / dout_m, bit 2 the ride's in / out, bit 3 the parameter block.  out[0..5] = kind (0 none, 1 generic,
// 2 s, 3 t), aligned, full, fuse, attention, ride.  Exposed for tests (no GPU needed).
int gcgcn_debug_chain_plan(int bwd, int B, int N, int D, int L, int H, int ragged, int ride, int hook, int scratch, int misalign,
                           int32_t* out) {
  GC_TRY(check_dims("debug_chain_plan", B, N, D, L, H));
  GC_REQUIRE(out, "debug_chain_plan: null pointer");
  int slot = 0;
  auto at = [&](int bit) { return (const float*)(uintptr_t)(0x100000ul * ++slot + ((misalign & bit) ? 4 : 0)); };
  EdgeRide er = EdgeRide();
  if (ride) er.kind = bwd ? 2 : 1, er.B = B, er.N = N, er.D = D, er.in = at(4), er.out = const_cast<float*>(at(4));
  ChainQuery q = make_query(B, N, D, L, H, gcn_layout(D, L, H), at(8), ragged != 0, scratch != 0, hook != 0, er, at(1), at(1), at(1));
  q.G = at(1), q.HO = at(1), q.X = at(1), q.dYa = at(1), q.dM = at(1), q.dP = at(1), q.dA = at(1);
  q.dout = at(2), q.dXres = at(2), q.dout_m = at(2);
  const ChainPlan p = bwd ? chain_plan_bwd(q) : chain_plan_fwd(q);
  out[0] = p.kind, out[1] = p.aligned, out[2] = p.full, out[3] = p.fuse, out[4] = p.attention, out[5] = p.ride;
  return 0;
}

// The output stage of a convolution backward call, by the very plan functions gcgcn_gcn_bwd calls (out_bwd_plan, then
// out_bwd_plan_col2 with what the front group launch would report).  out[0..9] = mask, wsum, fold, fold_drop, head_sum_launch, dwlin,
// col1, chain_slices (OutBwdPlan), then where stage 2 of dblin's sums runs and the slices the back launch's ride sums
// (OutBwdCol2).  fuse without scratch is refused, as gcgcn_gcn_bwd refuses it.  Exposed for tests (no GPU needed).
int gcgcn_debug_out_bwd_plan(int fuse, int B, int N, int D, int H, int scratch, int wsum_fwd, int ragged, int odrop, int drop,
                             int dxres_misaligned, int front_reduced, int32_t* out) {
  GC_REQUIRE(B > 0 && N > 0 && D > 0 && H > 0 && out, "debug_out_bwd_plan: bad arguments");
  GC_REQUIRE(!fuse || scratch, "debug_out_bwd_plan: the fused chain backward without scratch");
  const OutBwdPlan p = out_bwd_plan({fuse != 0, B, N, D, H, scratch != 0, wsum_fwd != 0, ragged != 0, odrop != 0, drop != 0, !dxres_misaligned});
  const OutBwdCol2 c2 = out_bwd_plan_col2(p, front_reduced != 0);
  out[0] = p.mask, out[1] = p.wsum, out[2] = p.fold, out[3] = p.fold_drop, out[4] = p.head_sum_launch, out[5] = p.dwlin, out[6] = p.col1;
  out[7] = p.chain_slices, out[8] = c2.where, out[9] = c2.back_ready_slices;
  return 0;
}

// Where the attention core of a call of this shape runs, by the very plan functions the four entry points call (mha_core.hip), on
// made-up operand addresses: misalign bit 0 puts Q off a 16-byte boundary, bit 1 dQ.  out[0..3] = AttnPlan's route, kchunk, fusable,
// then attn_hook_refusal (the hooked gcgcn_gcn_fwd / _bwd fail on it: route and kchunk -1).  Exposed for tests (no GPU needed).
int gcgcn_debug_attn_plan(int bwd, int N, int D, int H, int hook, int chain_attends, int core_done, int misalign, int32_t* out) {
  GC_REQUIRE(N > 0 && D > 0 && H > 0 && D % H == 0 && out, "debug_attn_plan: bad arguments");
  const void *Q = (const void*)(uintptr_t)(0x100000ul + ((misalign & 1) ? 4 : 0)), *dQ = (const void*)(uintptr_t)(0x200000ul + ((misalign & 2) ? 4 : 0));
  const AttnQuery q = make_attn_query(N, D, H, Q, bwd ? dQ : nullptr, hook != 0, chain_attends != 0, core_done != 0);
  const AttnPlan p = bwd ? attn_plan_bwd(q) : attn_plan_fwd(q);
  out[3] = attn_hook_refusal(q);
  out[0] = out[3] ? -1 : p.route, out[1] = out[3] ? -1 : p.kchunk, out[2] = p.fusable;
  return 0;
}

// The launch an edge pass of this shape gets, by the very plan functions the launchers call (edge.hip): pass 0 forward, 1 backward,
// 2 the mean's backward alone; compact 0 / 1; att: P wanted (forward), a logit gradient comes in (backward: the GATAttention call;
// a dense backward always has one).  misalign puts an operand off a 16-byte boundary: bit 0 E, 1 v, 2 dE, 3 dEbar, 4 Ebar.  The queue
// summary (dense backward): parked_tiles = the tile workgroups gemm_take_deferred would hand over (0: nothing parked), any_rb, col_C
// = the width of a parked column-sum second stage, or 0.  No decision depends on `ragged`.  out[0..16] = vec, att, dlogit route,
// slices, ngat, LDS bytes, lds_ok, carry_ok, RB, grid, col_base, ncolwg, the Spread's na / cohort / stride, scratch elements, rowbuf
// offset; -1 where a field does not apply.  Exposed for tests (no GPU needed).
int gcgcn_debug_edge_plan(int pass, int compact, int B, int N, int D, int ragged, int att, int has_dE, int has_dEbar, int misalign,
                          int parked_tiles, int any_rb, int col_C, int32_t* out) {
  (void)ragged;
  GC_REQUIRE(pass >= 0 && pass <= 2 && B > 0 && N > 0 && D > 0 && parked_tiles >= 0 && col_C >= 0 && out, "debug_edge_plan: bad arguments");
  GC_REQUIRE((long)B * N * 9 + parked_tiles < (1L << 31) && (long)B * N * D < (1L << 31), "debug_edge_plan: shape too large");
  GC_REQUIRE(!compact || D <= 64 * CMAXK, "debug_edge_plan: hidden width %d (compact rows support up to %d)", D, 64 * CMAXK);
  const bool dense_bwd = pass == 1 && !compact;
  GC_REQUIRE(!dense_bwd || att, "debug_edge_plan: a dense backward without a logit gradient is pass 2");
  const EdgeQuery q = {B, N, D, compact != 0, att != 0, has_dE != 0, has_dEbar != 0, (unsigned)misalign};
  EdgePlan p = pass == 0 ? edge_plan_fwd(q) : pass == 1 ? edge_plan_bwd(q) : edge_plan_bcast(q);
  if (dense_bwd && p.carry_ok) edge_plan_carry(p, parked_tiles, any_rb != 0, col_C);
  const int na = -1;
  out[0] = p.compact ? na : p.vec, out[1] = p.att, out[2] = p.route, out[3] = p.slices, out[4] = dense_bwd ? p.ngat : na;
  out[5] = (int)p.lds, out[6] = p.lds_limit ? (int)p.lds_ok() : na, out[7] = dense_bwd ? (int)p.carry_ok : na, out[8] = dense_bwd ? (int)p.RB : na;
  out[9] = (int)p.grid, out[10] = dense_bwd ? p.col_base : na, out[11] = dense_bwd ? p.ncolwg : na;
  out[12] = dense_bwd ? p.spread.na : na, out[13] = dense_bwd ? p.spread.cohort : na, out[14] = dense_bwd ? p.spread.stride : na;
  out[15] = (int)p.scratch, out[16] = (int)p.rowbuf_off;
  return 0;
}

// ---- trainer evaluation (eval.hip) ------------------------------------------------------------------------------------
static const int64_t kEvalMaxRecords = 0xffffffffLL;  // a record's ordinal has 32 bits

int64_t gcgcn_eval_ws_bytes(int64_t n_records, int64_t n_keep) {
  if (n_records < 0 || n_keep < 0 || n_records > kEvalMaxRecords) {
    set_error("eval: %lld records do not fit the 32-bit ordinal of a record (at most %lld)", (long long)n_records,
              (long long)kEvalMaxRecords);
    return -1;
  }
  return eval_ws_bytes(n_records, n_keep < n_records ? n_keep : n_records);
}

int gcgcn_eval_scan(int B, int N, int R, const float* logits, const float* labels, const uint8_t* in_train, const int32_t* n_valid,
                    const int64_t* doc_base, uint64_t* records, int64_t capacity, int64_t* counters, void* stream) {
  GC_REQUIRE(B > 0 && N > 0 && R > 1 && (long)B * N <= 0x7fffffffL && (long)N * R <= 0x7fffffffL,
             "eval_scan: bad shape B=%d N=%d R=%d", B, N, R);
  GC_REQUIRE(logits && labels && doc_base && records && counters, "eval_scan: null pointer");
  GC_REQUIRE(capacity > 0 && capacity <= kEvalMaxRecords, "eval_scan: capacity %lld outside (0, %lld]: a record's ordinal has 32 bits",
             (long long)capacity, (long long)kEvalMaxRecords);
  return eval_scan(logits, labels, in_train, n_valid, doc_base, records, capacity, counters, B, N, R, (hipStream_t)stream);
}

int gcgcn_eval_rank(const uint64_t* records, int64_t n, void* ws, int64_t ws_bytes, int64_t* sorted_off, void* stream) {
  GC_REQUIRE(n > 0 && n <= kEvalMaxRecords, "eval_rank: %lld records outside (0, %lld]", (long long)n, (long long)kEvalMaxRecords);
  GC_REQUIRE(records && ws && sorted_off, "eval_rank: null pointer");
  return eval_rank(records, n, ws, ws_bytes, sorted_off, (hipStream_t)stream);
}

int gcgcn_eval_curve(const uint64_t* ranked, int64_t m, int64_t n_records, const int64_t* counters, double input_theta,
                     float* pr_x, float* pr_y, float* ign_pr_y, double* result, void* ws, int64_t ws_bytes, void* stream) {
  GC_REQUIRE(m > 0 && m <= n_records && n_records <= kEvalMaxRecords, "eval_curve: bad sizes m=%lld n_records=%lld", (long long)m,
             (long long)n_records);
  GC_REQUIRE(ranked && counters && pr_x && pr_y && result && ws, "eval_curve: null pointer");
  return eval_curve(ranked, m, counters, input_theta, pr_x, pr_y, ign_pr_y, result, ws, ws_bytes, n_records, (hipStream_t)stream);
}

int gcgcn_gemm(int M, int N, int K, const float* A, int64_t lda, int a_kc, const float* B, int64_t ldb, int b_kc,
               float* C, int64_t ldc, int batch, int64_t sA, int64_t sB, int64_t sC, float alpha, const float* bias,
               int relu, int accumulate, int tile, int splits, float* ws, int64_t ws_elems, void* stream) {
  GemmArgs g = gemm_stored(a_kc, b_kc, A, lda, B, ldb, C, ldc, M, N, K).batch_z2(batch, sA, sB, sC).split_ws(ws, ws_elems);
  g.alpha = alpha, g.bias = bias, g.relu = relu, g.accumulate = accumulate;
  return gemm(g, (hipStream_t)stream, tile, splits);
}


int gcgcn_gemm_dyn(int M, int N, int K, const float* A, int64_t lda, int a_kc, const float* B, int64_t ldb, int b_kc, float* C,
                   int64_t ldc, const float* bias, int accumulate, const int32_t* count, int dyn, int64_t cap, float* ws,
                   int64_t ws_elems, void* stream) {
  GemmArgs g = gemm_stored(a_kc, b_kc, A, lda, B, ldb, C, ldc, M, N, K).split_ws(ws, ws_elems);
  g.bias = bias, g.accumulate = accumulate;
  return gemm_dyn(g, count, dyn, cap, (hipStream_t)stream);
}

// ---- the token encoder's LSTM layer (lstm.hip) ---------------------------------------------------------------------------------
static int lstm_shape_ok(const char* who, int B, int T, int I, int H, int nd) {
  GC_REQUIRE(H == LSTM_H, "%s: hidden width %d is not served (the recurrence kernels hold H = %d)", who, H, LSTM_H);
  GC_REQUIRE(nd == 1 || nd == 2, "%s: %d directions (1 or 2)", who, nd);
  GC_REQUIRE(B >= 1 && T >= 1 && I >= 1, "%s: bad shape B=%d T=%d I=%d", who, B, T, I);
  GC_REQUIRE((long)B * T * nd * 4 * H <= 0x7fffffffL && (long)B * T * I <= 0x7fffffffL, "%s: B=%d T=%d I=%d is too large", who, B, T, I);
  return 0;
}

int64_t gcgcn_lstm_ws_bytes(int B, int T, int I, int H, int nd) {
  if (lstm_shape_ok("lstm_ws_bytes", B, T, I, H, nd)) return -1;
  return (int64_t)sizeof(float) * lstm_ws_elems(B, T, I, nd);
}

int gcgcn_lstm_fwd(int B, int T, int I, int H, int nd, const float* x, const float* w_ih, const float* w_hh, const float* bias,
                   const float* h0, const float* c0, float* out, float* gates, float* csave, void* stream) {
  return gcgcn_lstm_fwd_len(B, T, I, H, nd, x, w_ih, w_hh, bias, h0, c0, out, gates, csave, nullptr, stream);
}

int gcgcn_lstm_fwd_len(int B, int T, int I, int H, int nd, const float* x, const float* w_ih, const float* w_hh, const float* bias,
                       const float* h0, const float* c0, float* out, float* gates, float* csave, const int* lens, void* stream) {
  const int recurrent = lstm_recurrent_take();   // first: whatever this call returns, the announcement was for it
  GC_TRY(lstm_shape_ok("lstm_fwd", B, T, I, H, nd));
  GC_REQUIRE(x && w_ih && w_hh && bias && h0 && c0 && out && gates, "lstm_fwd: null pointer");
  GC_REQUIRE((((uintptr_t)w_hh) & 15) == 0, "lstm_fwd: w_hh must be 16-byte aligned");
  return lstm_fwd(B, T, I, nd, x, w_ih, w_hh, bias, h0, c0, out, gates, csave, lens, recurrent, (hipStream_t)stream);
}

int gcgcn_lstm_bwd(int B, int T, int I, int H, int nd, const float* x, const float* w_ih, const float* w_hh, const float* h0,
                   const float* c0, const float* out, const float* gates, const float* csave, const float* dout, float* dgates,
                   float* dx, float* dw_ih, float* dw_hh, float* db, float* dh0, float* dc0, void* ws, int64_t ws_bytes, void* stream) {
  return gcgcn_lstm_bwd_len(B, T, I, H, nd, x, w_ih, w_hh, h0, c0, out, gates, csave, dout, dgates, dx, dw_ih, dw_hh, db, dh0, dc0, ws,
                            ws_bytes, nullptr, stream);
}

int gcgcn_lstm_bwd_len(int B, int T, int I, int H, int nd, const float* x, const float* w_ih, const float* w_hh, const float* h0,
                       const float* c0, const float* out, const float* gates, const float* csave, const float* dout, float* dgates,
                       float* dx, float* dw_ih, float* dw_hh, float* db, float* dh0, float* dc0, void* ws, int64_t ws_bytes,
                       const int* lens, void* stream) {
  const int recurrent = lstm_recurrent_take();   // first: whatever this call returns, the announcement was for it
  GC_TRY(lstm_shape_ok("lstm_bwd", B, T, I, H, nd));
  GC_REQUIRE(x && w_ih && w_hh && h0 && c0 && out && gates && csave && dout && dgates && dx && dw_ih && dw_hh && db && dh0 && dc0 && ws,
             "lstm_bwd: null pointer");
  GC_REQUIRE(dout != out, "lstm_bwd: dout aliases the output (H_prev is read from the output after dout has been consumed)");
  GC_REQUIRE(dgates != gates, "lstm_bwd: dgates aliases the saved gates");
  GC_REQUIRE((((uintptr_t)ws) & 15) == 0 && (((uintptr_t)out) & 15) == 0 && (((uintptr_t)h0) & 15) == 0,
             "lstm_bwd: ws, out and h0 must be 16-byte aligned");
  GC_REQUIRE(ws_bytes >= gcgcn_lstm_ws_bytes(B, T, I, H, nd), "lstm_bwd: workspace of %lld bytes needed (gcgcn_lstm_ws_bytes)",
             (long long)gcgcn_lstm_ws_bytes(B, T, I, H, nd));
  return lstm_bwd(B, T, I, nd, x, w_ih, w_hh, h0, c0, out, gates, csave, dout, dgates, dx, dw_ih, dw_hh, db, dh0, dc0, (float*)ws,
                  ws_bytes / (int64_t)sizeof(float), lens, recurrent, (hipStream_t)stream);
}

// ---- the token front end (frontend.hip) ------------------------------------------------------------------------------------------
static int embed_shape_ok(const char* who, int B, int T, int V, int P, int R, int Dw, int Dc, int Dn) {
  GC_REQUIRE(B >= 1 && T >= 1, "%s: bad shape B=%d T=%d", who, B, T);
  GC_REQUIRE(V >= 1 && P >= 1 && R >= 1, "%s: a table without rows (V=%d P=%d R=%d)", who, V, P, R);
  GC_REQUIRE(Dw >= 1 && Dc >= 1 && Dn >= 1, "%s: a width below 1 (Dw=%d Dc=%d Dn=%d)", who, Dw, Dc, Dn);
  GC_REQUIRE((long)B * T <= 0x7fffff00L && (long)Dw + Dc + Dn <= 0x7fffffffL, "%s: B=%d T=%d is too large", who, B, T);
  return 0;
}
static int context_shape_ok(const char* who, int B, int T, int N, int K, int Hd) {
  GC_REQUIRE(Hd == FE_HD, "%s: token-state width %d is not served (Hd = %d)", who, Hd, FE_HD);
  GC_REQUIRE(B >= 1 && T >= 1 && N >= 1 && K >= 1, "%s: bad shape B=%d T=%d N=%d K=%d", who, B, T, N, K);
  GC_REQUIRE((long)B * T * (K > Hd ? K : Hd) <= 0x7fffffffL && (long)B * N * T <= 0x7fffffffL && B <= 65535,
             "%s: B=%d T=%d N=%d K=%d is too large", who, B, T, N, K);
  return 0;
}
static EmbedTables embed_tables(int V, int P, int R, int Dw, int Dc, int Dn, const int64_t* document, const int64_t* document_pos,
                                const int64_t* document_ner) {
  EmbedTables tb;
  tb.t[0] = {document, nullptr, nullptr, V, Dw, -1};
  tb.t[1] = {document_pos, nullptr, nullptr, P, Dc, -1};
  tb.t[2] = {document_ner, nullptr, nullptr, R, Dn, -1};
  return tb;
}

int64_t gcgcn_frontend_ws_bytes(int B, int T, int V, int P, int R, int Dw, int Dc, int Dn, int K) {
  int64_t need = 0;
  if (V == 0 && K == 0) {
    set_error("frontend_ws_bytes: neither tables (V) nor a context width (K) given");
    return -1;
  }
  if (V != 0) {
    if (embed_shape_ok("frontend_ws_bytes", B, T, V, P, R, Dw, Dc, Dn)) return -1;
    need = embed_ws_bytes((long)B * T, embed_tables(V, P, R, Dw, Dc, Dn, nullptr, nullptr, nullptr));
  }
  if (K != 0) {
    if (context_shape_ok("frontend_ws_bytes", B, T, 1, K, FE_HD)) return -1;
    const int64_t c = (int64_t)sizeof(float) * context_ws_elems(K);
    need = c > need ? c : need;
  }
  return need;
}

int gcgcn_embed_fwd(int B, int T, int V, int P, int R, int Dw, int Dc, int Dn, const int64_t* document, const int64_t* document_pos,
                    const int64_t* document_ner, const float* word_w, const float* coref_w, const float* ner_w, const float* scale,
                    float* x, void* stream) {
  GC_TRY(embed_shape_ok("embed_fwd", B, T, V, P, R, Dw, Dc, Dn));
  GC_REQUIRE(document && document_pos && document_ner && word_w && coref_w && ner_w && x, "embed_fwd: null pointer");
  EmbedTables tb = embed_tables(V, P, R, Dw, Dc, Dn, document, document_pos, document_ner);
  tb.t[0].w = word_w, tb.t[1].w = coref_w, tb.t[2].w = ner_w;
  return embed_fwd(B, T, tb, scale, x, (hipStream_t)stream);
}

int gcgcn_embed_bwd(int B, int T, int V, int P, int R, int Dw, int Dc, int Dn, const int64_t* document, const int64_t* document_pos,
                    const int64_t* document_ner, const float* dx, const float* scale, int coref_padding_idx, int ner_padding_idx,
                    float* dword, float* dcoref, float* dner, void* ws, int64_t ws_bytes, void* stream) {
  GC_TRY(embed_shape_ok("embed_bwd", B, T, V, P, R, Dw, Dc, Dn));
  GC_REQUIRE(document && document_pos && document_ner && dx && dword && dcoref && dner && ws, "embed_bwd: null pointer");
  GC_REQUIRE((((uintptr_t)ws) & 15) == 0, "embed_bwd: ws must be 16-byte aligned");
  GC_REQUIRE(ws_bytes >= gcgcn_frontend_ws_bytes(B, T, V, P, R, Dw, Dc, Dn, 0), "embed_bwd: workspace of %lld bytes needed (gcgcn_frontend_ws_bytes)",
             (long long)gcgcn_frontend_ws_bytes(B, T, V, P, R, Dw, Dc, Dn, 0));
  EmbedTables tb = embed_tables(V, P, R, Dw, Dc, Dn, document, document_pos, document_ner);
  tb.t[0].dw = dword, tb.t[1].dw = dcoref, tb.t[2].dw = dner;
  tb.t[1].pad = coref_padding_idx, tb.t[2].pad = ner_padding_idx;
  return embed_bwd(B, T, tb, dx, scale, ws, ws_bytes, (hipStream_t)stream);
}

int gcgcn_context_fwd(int B, int T, int N, int K, int Hd, const float* h, const float* w, const float* bias, const float* node_pos,
                      float* pre, float* ctx, float* node_feat, void* stream) {
  GC_TRY(context_shape_ok("context_fwd", B, T, N, K, Hd));
  GC_REQUIRE(h && w && bias && node_pos && pre && ctx && node_feat, "context_fwd: null pointer");
  GC_REQUIRE((((uintptr_t)pre) & 15) == 0 && (((uintptr_t)ctx) & 15) == 0, "context_fwd: pre and ctx must be 16-byte aligned");
  GC_REQUIRE(pre != ctx, "context_fwd: ctx aliases pre (the pooling reads pre while ctx is being written)");
  return context_fwd(B, T, N, K, h, w, bias, node_pos, pre, ctx, node_feat, (hipStream_t)stream);
}

int gcgcn_context_bwd(int B, int T, int N, int K, int Hd, const float* h, const float* w, const float* node_pos, const float* ctx,
                      const float* dctx, const float* dnode_feat, float* dpre, float* dh, float* dw, float* db, void* ws,
                      int64_t ws_bytes, void* stream) {
  GC_TRY(context_shape_ok("context_bwd", B, T, N, K, Hd));
  GC_REQUIRE(h && w && node_pos && ctx && dctx && dnode_feat && dpre && dh && dw && db && ws, "context_bwd: null pointer");
  GC_REQUIRE((((uintptr_t)ws) & 15) == 0, "context_bwd: ws must be 16-byte aligned");
  GC_REQUIRE(ws_bytes >= gcgcn_frontend_ws_bytes(B, T, 0, 0, 0, 0, 0, 0, K), "context_bwd: workspace of %lld bytes needed (gcgcn_frontend_ws_bytes)",
             (long long)gcgcn_frontend_ws_bytes(B, T, 0, 0, 0, 0, 0, 0, K));
  return context_bwd(B, T, N, K, h, w, node_pos, ctx, dctx, dnode_feat, dpre, dh, dw, db, (float*)ws, ws_bytes / (int64_t)sizeof(float),
                     (hipStream_t)stream);
}

// ---- the BERT encoder layer (bert.hip) ---------------------------------------------------------------------------------------------
static int bert_attn_shape_ok(const char* who, int B, int T, int H, int dh) {
  GC_REQUIRE(dh == BERT_DH, "%s: head width %d is not served (the attention kernels hold dh = %d)", who, dh, BERT_DH);
  GC_REQUIRE(T >= 1 && T <= BERT_MAX_T, "%s: T = %d is outside [1, %d]", who, T, BERT_MAX_T);
  GC_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && H <= 65535, "%s: bad shape B=%d H=%d", who, B, H);
  GC_REQUIRE((long)B * T * 3 * H * dh <= 0x7fffffffL, "%s: B=%d T=%d H=%d is too large", who, B, T, H);
  return 0;
}
static int bert_drop_ok(const char* who, const void* snap, float p) {
  GC_REQUIRE(p >= 0.f && p < 1.f, "%s: p=%f out of [0,1)", who, p);
  GC_REQUIRE(!(p > 0.f) || snap, "%s: dropout without an rng snapshot", who);
  return 0;
}
static int bert_layer_shape_ok(const char* who, int B, int T, int D, int H, int Dff) {
  GC_REQUIRE(H >= 1 && D == H * BERT_DH, "%s: D = %d with %d heads is a head width other than %d", who, D, H, BERT_DH);
  GC_TRY(bert_attn_shape_ok(who, B, T, H, BERT_DH));
  GC_REQUIRE(D <= BERT_LN_MAX_D, "%s: D = %d exceeds %d", who, D, BERT_LN_MAX_D);
  GC_REQUIRE(Dff >= 4 && Dff % 4 == 0 && (long)B * T * Dff <= 0x7fffffffL, "%s: intermediate size %d (a multiple of 4; B T Dff < 2^31)", who, Dff);
  return 0;
}

// Token lengths: t_valid int32 [B] on the device, row (b, t) live iff t < t_valid[b] (gcgcn.h).  Each operation below has ONE body
// that checks, unpacks and calls into gc::.  It takes the most general argument list, the name of the symbol that was called (who)
// and need_len, whether that symbol requires t_valid.  The exported symbols only forward: the plain ones pass no lengths (and
// BERT_MM_FP32), the _len ones set need_len, _mm passes everything but the attention selector through, _mx everything.
static int bert_attn_sel_ok(const char* who, int attn) {
  GC_REQUIRE(attn == BERT_ATTN_FP32 || attn == BERT_ATTN_BF16, "%s: attn = %d (0: fp32, 1: bf16 operands)", who, attn);
  return 0;
}
static int bert_len_ok(const char* who, const int32_t* t_valid, int64_t rows, int T) {
  GC_REQUIRE(t_valid, "%s: t_valid is null (the entry point without _len takes no lengths)", who);
  GC_REQUIRE(T >= 1 && rows % T == 0, "%s: %lld rows are no whole documents of T = %d", who, (long long)rows, T);
  return 0;
}

static int attn_fwd(const char* who, bool need_len, int B, int T, int H, int dh, const float* qkv, const float* key_bias,
                    const int32_t* t_valid, float* ctx, float* lse, const void* rng_snap, uint64_t salt, float p, void* stream, int attn) {
  GC_TRY(bert_attn_shape_ok(who, B, T, H, dh));
  GC_TRY(bert_attn_sel_ok(who, attn));
  GC_TRY(bert_drop_ok(who, rng_snap, p));
  GC_REQUIRE(qkv && ctx && lse && (t_valid || !need_len), "%s: null pointer", who);
  GC_REQUIRE(al16(qkv), "%s: qkv must be 16-byte aligned", who);
  GC_REQUIRE(attn == BERT_ATTN_FP32 || al16(ctx), "%s: ctx must be 16-byte aligned with attn = 1", who);
  return bert_attn_fwd(B, T, H, qkv, key_bias, ctx, lse, make_drop(rng_snap, salt, p), (hipStream_t)stream, t_valid, attn);
}
static int attn_bwd(const char* who, bool need_len, int B, int T, int H, int dh, const float* qkv, const float* key_bias,
                    const int32_t* t_valid, const float* ctx, const float* lse, const float* dctx, float* dqkv, float* delta,
                    const void* rng_snap, uint64_t salt, float p, void* stream, int attn) {
  GC_TRY(bert_attn_shape_ok(who, B, T, H, dh));
  GC_TRY(bert_attn_sel_ok(who, attn));
  GC_TRY(bert_drop_ok(who, rng_snap, p));
  GC_REQUIRE(qkv && ctx && lse && dctx && dqkv && delta && (t_valid || !need_len), "%s: null pointer", who);
  GC_REQUIRE(al16(qkv) && al16(dctx), "%s: qkv and dctx must be 16-byte aligned", who);
  GC_REQUIRE(attn == BERT_ATTN_FP32 || al16(dqkv), "%s: dqkv must be 16-byte aligned with attn = 1", who);
  return bert_attn_bwd(B, T, H, qkv, key_bias, ctx, lse, dctx, dqkv, delta, make_drop(rng_snap, salt, p), (hipStream_t)stream, t_valid,
                       attn);
}
int gcgcn_bert_attn_fwd(int B, int T, int H, int dh, const float* qkv, const float* key_bias, float* ctx, float* lse, const void* rng_snap,
                        uint64_t salt, float p, void* stream) {
  return attn_fwd("bert_attn_fwd", false, B, T, H, dh, qkv, key_bias, nullptr, ctx, lse, rng_snap, salt, p, stream, BERT_ATTN_FP32);
}
int gcgcn_bert_attn_fwd_len(int B, int T, int H, int dh, const float* qkv, const float* key_bias, const int32_t* t_valid, float* ctx,
                            float* lse, const void* rng_snap, uint64_t salt, float p, void* stream) {
  return attn_fwd("bert_attn_fwd_len", true, B, T, H, dh, qkv, key_bias, t_valid, ctx, lse, rng_snap, salt, p, stream, BERT_ATTN_FP32);
}
int gcgcn_bert_attn_fwd_mx(int B, int T, int H, int dh, const float* qkv, const float* key_bias, const int32_t* t_valid, float* ctx,
                           float* lse, const void* rng_snap, uint64_t salt, float p, void* stream, int attn) {
  return attn_fwd("bert_attn_fwd_mx", false, B, T, H, dh, qkv, key_bias, t_valid, ctx, lse, rng_snap, salt, p, stream, attn);
}
int gcgcn_bert_attn_bwd(int B, int T, int H, int dh, const float* qkv, const float* key_bias, const float* ctx, const float* lse,
                        const float* dctx, float* dqkv, float* delta, const void* rng_snap, uint64_t salt, float p, void* stream) {
  return attn_bwd("bert_attn_bwd", false, B, T, H, dh, qkv, key_bias, nullptr, ctx, lse, dctx, dqkv, delta, rng_snap, salt, p, stream,
                  BERT_ATTN_FP32);
}
int gcgcn_bert_attn_bwd_len(int B, int T, int H, int dh, const float* qkv, const float* key_bias, const int32_t* t_valid, const float* ctx,
                            const float* lse, const float* dctx, float* dqkv, float* delta, const void* rng_snap, uint64_t salt, float p,
                            void* stream) {
  return attn_bwd("bert_attn_bwd_len", true, B, T, H, dh, qkv, key_bias, t_valid, ctx, lse, dctx, dqkv, delta, rng_snap, salt, p, stream,
                  BERT_ATTN_FP32);
}
int gcgcn_bert_attn_bwd_mx(int B, int T, int H, int dh, const float* qkv, const float* key_bias, const int32_t* t_valid, const float* ctx,
                           const float* lse, const float* dctx, float* dqkv, float* delta, const void* rng_snap, uint64_t salt, float p,
                           void* stream, int attn) {
  return attn_bwd("bert_attn_bwd_mx", false, B, T, H, dh, qkv, key_bias, t_valid, ctx, lse, dctx, dqkv, delta, rng_snap, salt, p, stream,
                  attn);
}

static int res_ln_shape_ok(const char* who, int64_t rows, int D) {
  GC_REQUIRE(D >= 64 && D % 64 == 0 && D <= BERT_LN_MAX_D, "%s: D = %d (a multiple of 64, at most %d)", who, D, BERT_LN_MAX_D);
  GC_REQUIRE(rows >= 1 && rows * D <= 0x7fffffffL, "%s: %lld rows", who, (long long)rows);
  return 0;
}
int64_t gcgcn_res_ln_ws_bytes(int D) {
  if (res_ln_shape_ok("res_ln_ws_bytes", 1, D)) return -1;
  return (int64_t)sizeof(float) * res_ln_ws_elems(D);
}
static int ln_fwd(const char* who, bool need_len, int64_t rows, int D, const float* x, const float* bias, const float* res,
                  const float* weight, const float* lnb, const int32_t* t_valid, int T, float* y, float* mean, float* rstd,
                  const void* rng_snap, uint64_t salt, float p, void* stream) {
  GC_TRY(res_ln_shape_ok(who, rows, D));
  if (need_len) GC_TRY(bert_len_ok(who, t_valid, rows, T));
  GC_TRY(bert_drop_ok(who, rng_snap, p));
  GC_REQUIRE(x && weight && lnb && y && (!mean == !rstd), "%s: null pointer", who);
  return res_ln_fwd(rows, D, x, bias, res, weight, lnb, y, mean, rstd, make_drop(rng_snap, salt, p), (hipStream_t)stream, t_valid, T);
}
static int ln_bwd(const char* who, bool need_len, int64_t rows, int D, const float* dy, const float* x, const float* bias, const float* res,
                  const float* weight, const float* mean, const float* rstd, const int32_t* t_valid, int T, float* dx, float* dres,
                  float* dweight, float* dlnb, void* ws, int64_t ws_bytes, const void* rng_snap, uint64_t salt, float p, void* stream) {
  GC_TRY(res_ln_shape_ok(who, rows, D));
  if (need_len) GC_TRY(bert_len_ok(who, t_valid, rows, T));
  GC_TRY(bert_drop_ok(who, rng_snap, p));
  GC_REQUIRE(dy && x && weight && mean && rstd && dx && dweight && dlnb && ws, "%s: null pointer", who);
  GC_REQUIRE(ws_bytes >= gcgcn_res_ln_ws_bytes(D), "%s: workspace of %lld bytes needed (gcgcn_res_ln_ws_bytes)", who,
             (long long)gcgcn_res_ln_ws_bytes(D));
  return res_ln_bwd(rows, D, dy, x, bias, res, weight, mean, rstd, dx, dres, dweight, dlnb, (float*)ws, make_drop(rng_snap, salt, p),
                    (hipStream_t)stream, t_valid, T);
}
int gcgcn_res_ln_fwd(int64_t rows, int D, const float* x, const float* bias, const float* res, const float* weight, const float* lnb,
                     float* y, float* mean, float* rstd, const void* rng_snap, uint64_t salt, float p, void* stream) {
  return ln_fwd("res_ln_fwd", false, rows, D, x, bias, res, weight, lnb, nullptr, 0, y, mean, rstd, rng_snap, salt, p, stream);
}
int gcgcn_res_ln_fwd_len(int64_t rows, int D, const float* x, const float* bias, const float* res, const float* weight, const float* lnb,
                         const int32_t* t_valid, int T, float* y, float* mean, float* rstd, const void* rng_snap, uint64_t salt, float p,
                         void* stream) {
  return ln_fwd("res_ln_fwd_len", true, rows, D, x, bias, res, weight, lnb, t_valid, T, y, mean, rstd, rng_snap, salt, p, stream);
}
int gcgcn_res_ln_bwd(int64_t rows, int D, const float* dy, const float* x, const float* bias, const float* res, const float* weight,
                     const float* mean, const float* rstd, float* dx, float* dres, float* dweight, float* dlnb, void* ws, int64_t ws_bytes,
                     const void* rng_snap, uint64_t salt, float p, void* stream) {
  return ln_bwd("res_ln_bwd", false, rows, D, dy, x, bias, res, weight, mean, rstd, nullptr, 0, dx, dres, dweight, dlnb, ws, ws_bytes,
                rng_snap, salt, p, stream);
}
int gcgcn_res_ln_bwd_len(int64_t rows, int D, const float* dy, const float* x, const float* bias, const float* res, const float* weight,
                         const float* mean, const float* rstd, const int32_t* t_valid, int T, float* dx, float* dres, float* dweight,
                         float* dlnb, void* ws, int64_t ws_bytes, const void* rng_snap, uint64_t salt, float p, void* stream) {
  return ln_bwd("res_ln_bwd_len", true, rows, D, dy, x, bias, res, weight, mean, rstd, t_valid, T, dx, dres, dweight, dlnb, ws, ws_bytes,
                rng_snap, salt, p, stream);
}

static int gelu_shape_ok(const char* who, int64_t rows, int C, const void* a, const void* b, const void* c) {
  GC_REQUIRE(rows >= 1 && C >= 4 && C % 4 == 0, "%s: rows = %lld, C = %d (a multiple of 4)", who, (long long)rows, C);
  GC_REQUIRE(al16(a) && al16(b) && al16(c), "%s: buffers must be 16-byte aligned", who);
  return 0;
}
static int gelu_fwd(const char* who, bool need_len, int64_t rows, int C, const float* x, const float* bias, const int32_t* t_valid, int T,
                    float* y, void* stream) {
  GC_REQUIRE(x && y, "%s: null pointer", who);
  GC_TRY(gelu_shape_ok(who, rows, C, x, bias, y));
  if (need_len) GC_TRY(bert_len_ok(who, t_valid, rows, T));
  return bias_gelu_fwd(rows, C, x, bias, y, (hipStream_t)stream, t_valid, T);
}
static int gelu_bwd(const char* who, bool need_len, int64_t rows, int C, const float* dy, const float* x, const float* bias,
                    const int32_t* t_valid, int T, float* dx, void* stream) {
  GC_REQUIRE(dy && x && dx, "%s: null pointer", who);
  GC_TRY(gelu_shape_ok(who, rows, C, x, bias, dx));
  GC_REQUIRE(al16(dy), "%s: buffers must be 16-byte aligned", who);
  if (need_len) GC_TRY(bert_len_ok(who, t_valid, rows, T));
  return bias_gelu_bwd(rows, C, dy, x, bias, dx, (hipStream_t)stream, t_valid, T);
}
int gcgcn_bias_gelu_fwd(int64_t rows, int C, const float* x, const float* bias, float* y, void* stream) {
  return gelu_fwd("bias_gelu_fwd", false, rows, C, x, bias, nullptr, 0, y, stream);
}
int gcgcn_bias_gelu_fwd_len(int64_t rows, int C, const float* x, const float* bias, const int32_t* t_valid, int T, float* y, void* stream) {
  return gelu_fwd("bias_gelu_fwd_len", true, rows, C, x, bias, t_valid, T, y, stream);
}
int gcgcn_bias_gelu_bwd(int64_t rows, int C, const float* dy, const float* x, const float* bias, float* dx, void* stream) {
  return gelu_bwd("bias_gelu_bwd", false, rows, C, dy, x, bias, nullptr, 0, dx, stream);
}
int gcgcn_bias_gelu_bwd_len(int64_t rows, int C, const float* dy, const float* x, const float* bias, const int32_t* t_valid, int T, float* dx,
                            void* stream) {
  return gelu_bwd("bias_gelu_bwd_len", true, rows, C, dy, x, bias, t_valid, T, dx, stream);
}

// The layer.  rowblk: gcgcn_row_blocks(B, T, t_valid) or null.  matmul: 0 = the fp32 GEMM layer, 1 = the twelve Linear products with
// bf16 operands (gemm_bf16.hip).  attn: 0 = the fp32 attention core, 1 = the bf16 one (bert_attn_bf16.hip).
int64_t gcgcn_bert_layer_ws_bytes(int B, int T, int D, int H, int Dff, int which) {
  if (bert_layer_shape_ok("bert_layer_ws_bytes", B, T, D, H, Dff)) return -1;
  if (which != 0 && which != 1) {
    set_error("bert_layer_ws_bytes: which = %d (0: what the forward saves, 1: the backward's workspace)", which);
    return -1;
  }
  return (int64_t)sizeof(float) * (which ? bert_layer_ws_elems(B, T, D, H, Dff) : bert_layer_saved_elems(B, T, D, H, Dff));
}
static int bert_params_ok(const char* who, const float* const* p) {
  GC_REQUIRE(p, "%s: null parameter list", who);
  for (int i = 0; i < GCGCN_BERT_LAYER_PARAMS; ++i) GC_REQUIRE(p[i] && al16(p[i]), "%s: parameter %d is null or not 16-byte aligned", who, i);
  return 0;
}
static_assert(GCGCN_BERT_LAYER_PARAMS == 12, "bert_unpack names every tensor of the layer");
extern "C++" template <class S, class P>   // BertLayerParams from the parameters' list, BertLayerGrads from the gradients'
static S bert_unpack(P* const* p) {
  return {p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11]};
}
// what the forward and the backward check alike, in front of their own buffers
static int bert_layer_ok(const char* who, bool need_len, int B, int T, int D, int H, int Dff, const int32_t* t_valid, const int32_t* rowblk,
                         const float* const* params, const void* rng_snap, float p_attn, float p_hidden, int matmul, int attn) {
  GC_TRY(bert_layer_shape_ok(who, B, T, D, H, Dff));
  GC_REQUIRE(matmul == BERT_MM_FP32 || matmul == BERT_MM_BF16, "%s: matmul = %d (0: fp32, 1: bf16 operands)", who, matmul);
  GC_TRY(bert_attn_sel_ok(who, attn));
  GC_TRY(bert_drop_ok(who, rng_snap, p_attn));
  GC_TRY(bert_drop_ok(who, rng_snap, p_hidden));
  GC_TRY(bert_params_ok(who, params));
  GC_REQUIRE(t_valid || !need_len, "%s: t_valid is null", who);
  GC_REQUIRE(t_valid || !rowblk, "%s: a row-block list without t_valid", who);
  GC_REQUIRE(!rowblk || T % 16 == 0, "%s: a row-block list needs T a multiple of 16 (T = %d)", who, T);
  return 0;
}
static int layer_fwd(const char* who, bool need_len, int B, int T, int D, int H, int Dff, const float* x, const float* key_bias,
                     const int32_t* t_valid, const int32_t* rowblk, const float* const* params, float* y, void* saved, int64_t saved_bytes,
                     const void* rng_snap, float p_attn, float p_hidden, void* stream, int matmul, int attn) {
  GC_TRY(bert_layer_ok(who, need_len, B, T, D, H, Dff, t_valid, rowblk, params, rng_snap, p_attn, p_hidden, matmul, attn));
  GC_REQUIRE(x && y && saved && al16(x) && al16(y) && al16(saved), "%s: x, y, saved must be given and 16-byte aligned", who);
  GC_REQUIRE(saved_bytes >= gcgcn_bert_layer_ws_bytes(B, T, D, H, Dff, 0), "%s: %lld bytes of saved activations needed "
             "(gcgcn_bert_layer_ws_bytes, which = 0)", who, (long long)gcgcn_bert_layer_ws_bytes(B, T, D, H, Dff, 0));
  return bert_layer_fwd(B, T, D, H, Dff, x, key_bias, bert_unpack<BertLayerParams>(params), y, (float*)saved, rng_snap, p_attn, p_hidden,
                        (hipStream_t)stream, t_valid, rowblk, matmul, attn);
}
static int layer_bwd(const char* who, bool need_len, int B, int T, int D, int H, int Dff, const float* x, const float* key_bias,
                     const int32_t* t_valid, const int32_t* rowblk, const float* const* params, const void* saved, int64_t saved_bytes,
                     const float* dy, float* dx, float* const* grads, void* ws, int64_t ws_bytes, const void* rng_snap, float p_attn,
                     float p_hidden, void* stream, int matmul, int attn) {
  GC_TRY(bert_layer_ok(who, need_len, B, T, D, H, Dff, t_valid, rowblk, params, rng_snap, p_attn, p_hidden, matmul, attn));
  GC_TRY(bert_params_ok(who, grads));
  GC_REQUIRE(x && saved && dy && dx && ws && al16(x) && al16(saved) && al16(dy) && al16(dx) && al16(ws),
             "%s: x, saved, dy, dx, ws must be given and 16-byte aligned", who);
  GC_REQUIRE(dx != dy, "%s: dx aliases dy", who);
  GC_REQUIRE(saved_bytes >= gcgcn_bert_layer_ws_bytes(B, T, D, H, Dff, 0), "%s: %lld bytes of saved activations needed "
             "(gcgcn_bert_layer_ws_bytes, which = 0)", who, (long long)gcgcn_bert_layer_ws_bytes(B, T, D, H, Dff, 0));
  GC_REQUIRE(ws_bytes >= gcgcn_bert_layer_ws_bytes(B, T, D, H, Dff, 1), "%s: workspace of %lld bytes needed "
             "(gcgcn_bert_layer_ws_bytes, which = 1)", who, (long long)gcgcn_bert_layer_ws_bytes(B, T, D, H, Dff, 1));
  return bert_layer_bwd(B, T, D, H, Dff, x, key_bias, bert_unpack<BertLayerParams>(params), (const float*)saved, dy, dx,
                        bert_unpack<BertLayerGrads>(grads), (float*)ws, ws_bytes / (int64_t)sizeof(float), rng_snap, p_attn, p_hidden,
                        (hipStream_t)stream, t_valid, rowblk, matmul, attn);
}
int gcgcn_bert_layer_fwd(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const float* const* params, float* y,
                         void* saved, int64_t saved_bytes, const void* rng_snap, float p_attn, float p_hidden, void* stream) {
  return layer_fwd("bert_layer_fwd", false, B, T, D, H, Dff, x, key_bias, nullptr, nullptr, params, y, saved, saved_bytes, rng_snap, p_attn,
                   p_hidden, stream, BERT_MM_FP32, BERT_ATTN_FP32);
}
int gcgcn_bert_layer_fwd_len(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const int32_t* t_valid,
                             const int32_t* rowblk, const float* const* params, float* y, void* saved, int64_t saved_bytes,
                             const void* rng_snap, float p_attn, float p_hidden, void* stream) {
  return layer_fwd("bert_layer_fwd_len", true, B, T, D, H, Dff, x, key_bias, t_valid, rowblk, params, y, saved, saved_bytes, rng_snap,
                   p_attn, p_hidden, stream, BERT_MM_FP32, BERT_ATTN_FP32);
}
int gcgcn_bert_layer_fwd_mm(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const int32_t* t_valid,
                            const int32_t* rowblk, const float* const* params, float* y, void* saved, int64_t saved_bytes,
                            const void* rng_snap, float p_attn, float p_hidden, void* stream, int matmul) {
  return layer_fwd("bert_layer_fwd_mm", false, B, T, D, H, Dff, x, key_bias, t_valid, rowblk, params, y, saved, saved_bytes, rng_snap,
                   p_attn, p_hidden, stream, matmul, BERT_ATTN_FP32);
}
int gcgcn_bert_layer_fwd_mx(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const int32_t* t_valid,
                            const int32_t* rowblk, const float* const* params, float* y, void* saved, int64_t saved_bytes,
                            const void* rng_snap, float p_attn, float p_hidden, void* stream, int matmul, int attn) {
  return layer_fwd("bert_layer_fwd_mx", false, B, T, D, H, Dff, x, key_bias, t_valid, rowblk, params, y, saved, saved_bytes, rng_snap,
                   p_attn, p_hidden, stream, matmul, attn);
}
int gcgcn_bert_layer_bwd(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const float* const* params,
                         const void* saved, int64_t saved_bytes, const float* dy, float* dx, float* const* grads, void* ws, int64_t ws_bytes,
                         const void* rng_snap, float p_attn, float p_hidden, void* stream) {
  return layer_bwd("bert_layer_bwd", false, B, T, D, H, Dff, x, key_bias, nullptr, nullptr, params, saved, saved_bytes, dy, dx, grads, ws,
                   ws_bytes, rng_snap, p_attn, p_hidden, stream, BERT_MM_FP32, BERT_ATTN_FP32);
}
int gcgcn_bert_layer_bwd_len(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const int32_t* t_valid,
                             const int32_t* rowblk, const float* const* params, const void* saved, int64_t saved_bytes, const float* dy,
                             float* dx, float* const* grads, void* ws, int64_t ws_bytes, const void* rng_snap, float p_attn, float p_hidden,
                             void* stream) {
  return layer_bwd("bert_layer_bwd_len", true, B, T, D, H, Dff, x, key_bias, t_valid, rowblk, params, saved, saved_bytes, dy, dx, grads, ws,
                   ws_bytes, rng_snap, p_attn, p_hidden, stream, BERT_MM_FP32, BERT_ATTN_FP32);
}
int gcgcn_bert_layer_bwd_mm(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const int32_t* t_valid,
                            const int32_t* rowblk, const float* const* params, const void* saved, int64_t saved_bytes, const float* dy,
                            float* dx, float* const* grads, void* ws, int64_t ws_bytes, const void* rng_snap, float p_attn, float p_hidden,
                            void* stream, int matmul) {
  return layer_bwd("bert_layer_bwd_mm", false, B, T, D, H, Dff, x, key_bias, t_valid, rowblk, params, saved, saved_bytes, dy, dx, grads, ws,
                   ws_bytes, rng_snap, p_attn, p_hidden, stream, matmul, BERT_ATTN_FP32);
}
int gcgcn_bert_layer_bwd_mx(int B, int T, int D, int H, int Dff, const float* x, const float* key_bias, const int32_t* t_valid,
                            const int32_t* rowblk, const float* const* params, const void* saved, int64_t saved_bytes, const float* dy,
                            float* dx, float* const* grads, void* ws, int64_t ws_bytes, const void* rng_snap, float p_attn, float p_hidden,
                            void* stream, int matmul, int attn) {
  return layer_bwd("bert_layer_bwd_mx", false, B, T, D, H, Dff, x, key_bias, t_valid, rowblk, params, saved, saved_bytes, dy, dx, grads, ws,
                   ws_bytes, rng_snap, p_attn, p_hidden, stream, matmul, attn);
}

// ---- opt-in bf16 matrix products (gemm_bf16.hip) -------------------------------------------------------------
int64_t gcgcn_gemm_bf16_ws_bytes(int M, int N, int K) {
  if (M < 1 || N < 1 || K < 1) {
    set_error("gemm_bf16_ws_bytes: M = %d, N = %d, K = %d (each at least 1)", M, N, K);
    return -1;
  }
  return (int64_t)sizeof(float) * gemm_bf16_ws_elems(M, N, K);
}
int gcgcn_gemm_bf16(int a_kc, int b_kc, const float* A, int64_t lda, const float* B, int64_t ldb, float* C, int64_t ldc, int M, int N, int K,
                    const float* bias, const float* add, int64_t ldadd, void* ws, int64_t ws_bytes, void* stream) {
  GC_REQUIRE(M >= 1 && N >= 1 && K >= 1, "gemm_bf16: M = %d, N = %d, K = %d (each at least 1)", M, N, K);
  const int64_t need = gcgcn_gemm_bf16_ws_bytes(M, N, K);
  GC_REQUIRE(need == 0 || (ws && al16(ws) && ws_bytes >= need), "gemm_bf16: a 16-byte aligned workspace of %lld bytes needed "
             "(gcgcn_gemm_bf16_ws_bytes)", (long long)need);
  GemmBf16Args g = gemm_bf16_stored(a_kc != 0, b_kc != 0, A, lda, B, ldb, C, ldc, M, N, K);
  g.bias = bias, g.add = add, g.ldadd = add ? ldadd : 0;
  g.ws = (float*)ws, g.ws_elems = ws ? ws_bytes / (int64_t)sizeof(float) : 0;
  return gemm_bf16(g, (hipStream_t)stream);
}
}  // extern "C"
