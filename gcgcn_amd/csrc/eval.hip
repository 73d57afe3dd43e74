// Relation evaluation of the reference's trainer (config/Config.py:432-561 `test`, config/Config_bert.py:488-656 for the
// ignore-train-facts curve), written there as a Python triple loop that appends one tuple per (head, tail, relation != NA),
// list.sort, a Python prefix loop and sklearn.metrics.auc.  Here, three stages on the device:
//   scan   one workgroup per (document, head entity) row of the padded [B,N,N,R] logits: sigmoid, per-pair first argmax over the
//          PROBABILITIES, the six integer counters, and one 64-bit record per (pair, k >= 1) written AT ITS ORDINAL (its
//          position in the reference's append order), so the record buffer is dense and already in append order;
//   rank   a stable least-significant-digit radix sort of the records over the 30 score bits only: the buffer starts in ordinal
//          order and every pass is stable, so the result is the strict total order (score descending, ordinal ascending) that
//          Python's stable sort produces, whatever the algorithm;
//   curve  prefix sums of label and label && flag over the kept prefix, the fp32 curves from fp64 quotients, F1 maxima with
//          first argmax, w, and the two trapezoids in fp64 -- every reduction in a fixed order.
// Record (uint64):  [63:34] 0x3fffffff - bits(p)   (p in [0,1] has its two top bits clear)
//                   [33:2]  ordinal                (32 bits; gcgcn_eval_ws_bytes refuses more records than that)
//                   [1]     label != 0             [0] sticky in-train flag of the pair (Config_bert.py:545-562)
// Ascending order of the record is the ranking.  wave = 64 throughout; integer atomics only.
#include "rowops.hpp"

namespace gc {

namespace {

constexpr int EV_SCORE_SHIFT = 34;
constexpr uint32_t EV_SCORE_MAX = 0x3fffffffu;
constexpr int EV_PASSES = 4;  // digits of 8 bits at 34, 42, 50 and (6 bits) 58

constexpr int RS_THREADS = 256, RS_ROUNDS = 16, RS_TILE = RS_THREADS * RS_ROUNDS, RS_BINS = 256;
constexpr int SC_THREADS = 256, SC_ITEMS = 8, SC_TILE = SC_THREADS * SC_ITEMS;

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    const uint64_t u = ((uint64_t)hi << 32) | lo;
    v = u > v ? u : v;
  }
  return v;
}

// ---- scan pass --------------------------------------------------------------------------------------------------------
// counters[0..5] = top1_acc, na_recall, na_correct, total_recall, total_correct, have_label (Config.py:487-505);
// counters[6] = NaN probabilities met, counters[7] = records that did not fit `capacity` (neither is ever written past it).
__global__ __launch_bounds__(256) void eval_scan_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                        const uint8_t* __restrict__ in_train, const int* __restrict__ n_valid,
                                                        const int64_t* __restrict__ doc_base, uint64_t* __restrict__ rec,
                                                        uint64_t capacity, unsigned long long* __restrict__ counters, int N,
                                                        int R) {
  __shared__ unsigned long long red[4][8];
  const int bh = blockIdx.x, b = bh / N, i = bh - b * N;
  const int nv = n_valid ? min(max(n_valid[b], 0), N) : N;
  if (i >= nv || nv < 2) return;  // the whole workgroup: no pair in this row
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t le_mask = (2ull << lane) - 1ull;  // lanes 0..lane
  const uint64_t base = (uint64_t)doc_base[b];
  unsigned long long c[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // wave-uniform
  for (int j = wave; j < nv; j += 4) {
    if (j == i) continue;
    const long off = ((long)bh * N + j) * R;
    // r* = first maximum of the probabilities: (bits(p), -k) packed so that one unsigned maximum does both
    uint64_t best = 0;
    bool nan = false;
    for (int k0 = 0; k0 < R; k0 += 64) {
      const int k = k0 + lane;
      if (k < R) {
        const float p = 1.f / (1.f + expf(-logits[off + k]));
        nan |= p != p;
        const uint64_t v = ((uint64_t)__float_as_uint(p) << 32) | (uint32_t)(0xffffffffu - (uint32_t)k);
        best = v > best ? v : best;
      }
    }
    best = wave_max_u64(best);
    const int rstar = (int)(0xffffffffu - (uint32_t)best);
    const int jp = j - (j > i ? 1 : 0);
    const uint64_t pbase = base + ((uint64_t)i * (uint64_t)(nv - 1) + (uint64_t)jp) * (uint64_t)(R - 1);
    bool carry = false, ovf = false;
    unsigned pos = 0, lab_r = 0, na = 0;
    for (int k0 = 0; k0 < R; k0 += 64) {
      const int k = k0 + lane;
      const bool valid = k < R;
      const float x = valid ? logits[off + k] : 0.f;
      const bool lab = valid && labels[off + k] != 0.f;
      const bool f = lab && k >= 1 && in_train != nullptr && in_train[off + k] != 0;
      const uint64_t fm = __ballot(f), lm = __ballot(lab);
      const bool flag = carry || (fm & le_mask) != 0;  // sticky: OR over 1 <= k' <= k, carried from chunk to chunk
      carry = carry || fm != 0;
      if (k0 == 0) na = (unsigned)(lm & 1ull);
      pos += (unsigned)__popcll(k0 == 0 ? (lm & ~1ull) : lm);
      if (rstar >= k0 && rstar < k0 + 64) lab_r = (unsigned)((lm >> (rstar - k0)) & 1ull);
      if (valid && k >= 1) {
        const float p = 1.f / (1.f + expf(-x));
        const uint32_t bits = min(__float_as_uint(p), EV_SCORE_MAX);
        const uint64_t ord = pbase + (uint64_t)(k - 1);
        if (ord < capacity)
          rec[ord] = ((uint64_t)(EV_SCORE_MAX - bits) << EV_SCORE_SHIFT) | (ord << 2) | ((uint64_t)lab << 1) | (uint64_t)flag;
        else
          ovf = true;
      }
    }
    c[0] += lab_r;
    c[1] += na;
    c[2] += (na && rstar == 0) ? 1u : 0u;
    c[3] += pos;
    c[4] += (lab_r && rstar >= 1) ? 1u : 0u;
    c[5] += pos > 0 ? 1u : 0u;
    c[6] += __ballot(nan) != 0 ? 1u : 0u;
    c[7] += __ballot(ovf) != 0 ? 1u : 0u;
  }
  if (lane == 0) {
#pragma unroll
    for (int q = 0; q < 8; ++q) red[wave][q] = c[q];
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    const unsigned long long s = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    if (s) atomicAdd(&counters[threadIdx.x], s);
  }
}

// ---- exclusive prefix sums (three launches: tile sums, one workgroup over the tile sums, tiles again) ---------------------
template <typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* lds, T& total) {  // 256 threads; lds[256]
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
  for (int o = 1; o < SC_THREADS; o <<= 1) {
    const T u = t >= o ? lds[t - o] : T(0);
    __syncthreads();
    lds[t] += u;
    __syncthreads();
  }
  const T incl = lds[t];
  total = lds[SC_THREADS - 1];
  __syncthreads();
  return incl - v;
}

template <typename T>
__global__ __launch_bounds__(256) void scan_tile_sums_kernel(const T* __restrict__ in, uint64_t n, T* __restrict__ sums) {
  __shared__ T lds[SC_THREADS];
  const uint64_t e0 = (uint64_t)blockIdx.x * SC_TILE + (uint64_t)threadIdx.x * SC_ITEMS;
  T s = 0;
#pragma unroll
  for (int u = 0; u < SC_ITEMS; ++u) s += (e0 + u < n) ? in[e0 + u] : T(0);
  T total;
  block_excl_scan(s, lds, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

template <typename T>
__global__ __launch_bounds__(256) void scan_sums_kernel(T* __restrict__ sums, uint64_t nblk) {  // one workgroup, in place
  __shared__ T lds[SC_THREADS];
  T carry = 0;
  for (uint64_t c0 = 0; c0 < nblk; c0 += SC_THREADS) {
    const uint64_t e = c0 + threadIdx.x;
    const T v = e < nblk ? sums[e] : T(0);
    T total;
    const T ex = block_excl_scan(v, lds, total);
    if (e < nblk) sums[e] = carry + ex;
    carry += total;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void scan_apply_kernel(T* __restrict__ data, uint64_t n, const T* __restrict__ sums) {
  __shared__ T lds[SC_THREADS];
  const uint64_t e0 = (uint64_t)blockIdx.x * SC_TILE + (uint64_t)threadIdx.x * SC_ITEMS;
  T v[SC_ITEMS], s = 0;
#pragma unroll
  for (int u = 0; u < SC_ITEMS; ++u) v[u] = (e0 + u < n) ? data[e0 + u] : T(0), s += v[u];
  T total;
  T run = sums[blockIdx.x] + block_excl_scan(s, lds, total);
#pragma unroll
  for (int u = 0; u < SC_ITEMS; ++u) {
    if (e0 + u < n) data[e0 + u] = run;
    run += v[u];
  }
}

// ---- radix sort ---------------------------------------------------------------------------------------------------------
// Occupancy of every digit, all passes at once: the host skips a pass whose keys share one digit value (probabilities
// occupy few exponent values).  Counts only, so the order of the integer atomics does not matter.
__global__ __launch_bounds__(256) void radix_digit_hist_kernel(const uint64_t* __restrict__ keys, uint64_t n,
                                                               unsigned* __restrict__ ghist) {
  __shared__ unsigned h[EV_PASSES * RS_BINS];
  for (int q = threadIdx.x; q < EV_PASSES * RS_BINS; q += RS_THREADS) h[q] = 0;
  __syncthreads();
  for (uint64_t e = (uint64_t)blockIdx.x * RS_THREADS + threadIdx.x; e < n; e += (uint64_t)gridDim.x * RS_THREADS) {
    const uint64_t k = keys[e];
#pragma unroll
    for (int p = 0; p < EV_PASSES; ++p) atomicAdd(&h[p * RS_BINS + (int)((k >> (EV_SCORE_SHIFT + 8 * p)) & 255)], 1u);
  }
  __syncthreads();
  for (int q = threadIdx.x; q < EV_PASSES * RS_BINS; q += RS_THREADS)
    if (h[q]) atomicAdd(&ghist[q], h[q]);
}

// hist[digit * nwg + workgroup] = keys of the workgroup's tile with that digit
__global__ __launch_bounds__(256) void radix_tile_hist_kernel(const uint64_t* __restrict__ keys, uint64_t n, int shift,
                                                              unsigned* __restrict__ hist, unsigned nwg) {
  __shared__ unsigned h[RS_BINS];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint64_t t0 = (uint64_t)blockIdx.x * RS_TILE;
#pragma unroll
  for (int r = 0; r < RS_ROUNDS; ++r) {
    const uint64_t e = t0 + (uint64_t)r * RS_THREADS + threadIdx.x;
    if (e < n) atomicAdd(&h[(int)((keys[e] >> shift) & 255)], 1u);
  }
  __syncthreads();
  hist[(uint64_t)threadIdx.x * nwg + blockIdx.x] = h[threadIdx.x];
}

// Stable scatter.  A wave owns 1024 consecutive keys of the tile and takes them 64 at a time in order; within a round the lanes
// that share a digit find each other by ballots (match-any) and are ranked by lane number, and the wave's running count of
// the digit (LDS, touched by this wave only, no atomics) places the round after the earlier ones.  Waves, then workgroups,
// follow in index order through the scanned (digit, workgroup) histogram.
__global__ __launch_bounds__(256) void radix_scatter_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, uint64_t n,
                                                            int shift, const unsigned* __restrict__ offs, unsigned nwg) {
  __shared__ unsigned cnt[4][RS_BINS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  volatile unsigned* wc = &cnt[wave][0];
#pragma unroll
  for (int q = 0; q < 4; ++q) cnt[q][threadIdx.x] = 0;
  __syncthreads();
  const uint64_t w0 = (uint64_t)blockIdx.x * RS_TILE + (uint64_t)wave * (RS_ROUNDS * 64);
  const uint64_t lt_mask = (1ull << lane) - 1ull;
  uint64_t key[RS_ROUNDS];
  unsigned rk[RS_ROUNDS];
#pragma unroll
  for (int r = 0; r < RS_ROUNDS; ++r) {
    const uint64_t e = w0 + (uint64_t)r * 64 + lane;
    const bool valid = e < n;
    key[r] = valid ? in[e] : 0ull;
    const unsigned d = (unsigned)((key[r] >> shift) & 255);
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
      const bool on = (d >> bit) & 1u;
      const uint64_t bb = __ballot(on);
      m &= on ? bb : ~bb;
    }
    const unsigned below = (unsigned)__popcll(m & lt_mask), same = (unsigned)__popcll(m);
    const unsigned old = wc[d];
    __builtin_amdgcn_wave_barrier();
    if (valid && below == 0) wc[d] = old + same;
    __builtin_amdgcn_wave_barrier();
    rk[r] = old + below;
  }
  __syncthreads();
  {
    const int d = threadIdx.x;
    const unsigned a0 = cnt[0][d], a1 = cnt[1][d], a2 = cnt[2][d], g = offs[(uint64_t)d * nwg + blockIdx.x];
    cnt[0][d] = g, cnt[1][d] = g + a0, cnt[2][d] = g + a0 + a1, cnt[3][d] = g + a0 + a1 + a2;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < RS_ROUNDS; ++r) {
    const uint64_t e = w0 + (uint64_t)r * 64 + lane;
    const uint64_t dst = (uint64_t)cnt[wave][(int)((key[r] >> shift) & 255)] + rk[r];
    if (e < n && dst < n) out[dst] = key[r];
  }
}

// ---- curve pass -----------------------------------------------------------------------------------------------------
struct CurvePart {
  double auc, ign_auc;
  unsigned long long f1_pos;
  long long w;  // last index with score > input_theta, -1: none
  float f1, ign_f1;
};

__device__ __forceinline__ uint64_t curve_item(uint64_t key) {  // label in the low word, label && flag in the high word
  const uint64_t l = (key >> 1) & 1ull;
  return l | ((l & key & 1ull) << 32);
}
__device__ __forceinline__ float curve_f1(float x, float y) {  // numpy: 2 * pr_x * pr_y / (pr_x + pr_y + 1e-20), all fp32
  return __fdiv_rn(__fmul_rn(__fmul_rn(2.f, x), y), __fadd_rn(__fadd_rn(x, y), 1e-20f));
}
__device__ __forceinline__ float key_score(uint64_t key) {
  return __uint_as_float(EV_SCORE_MAX - (uint32_t)(key >> EV_SCORE_SHIFT));
}
struct CurvePoint {
  float x, y, iy;
};
// the point after `cnt` records of which `correct` are positives and `cit` positives flagged in-train
__device__ __forceinline__ CurvePoint curve_point(uint64_t cnt, uint64_t correct, uint64_t cit, double recall) {
  CurvePoint p;
  p.x = (float)((double)correct / recall);
  p.y = (float)((double)correct / (double)cnt);
  p.iy = cit == correct ? 0.f : (float)((double)(correct - cit) / (double)(cnt - cit));
  return p;
}

__global__ __launch_bounds__(256) void curve_tile_sums_kernel(const uint64_t* __restrict__ keys, uint64_t m,
                                                              uint64_t* __restrict__ sums) {
  __shared__ uint64_t lds[SC_THREADS];
  const uint64_t e0 = (uint64_t)blockIdx.x * SC_TILE + (uint64_t)threadIdx.x * SC_ITEMS;
  uint64_t s = 0;
#pragma unroll
  for (int u = 0; u < SC_ITEMS; ++u) s += (e0 + u < m) ? curve_item(keys[e0 + u]) : 0ull;
  uint64_t total;
  block_excl_scan(s, lds, total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void curve_apply_kernel(const uint64_t* __restrict__ keys, uint64_t m,
                                                          const uint64_t* __restrict__ sums,
                                                          const unsigned long long* __restrict__ counters, double input_theta,
                                                          float* __restrict__ pr_x, float* __restrict__ pr_y,
                                                          float* __restrict__ ign_pr_y, CurvePart* __restrict__ parts) {
  __shared__ uint64_t lds[SC_THREADS];
  __shared__ CurvePart sp[SC_THREADS];
  const uint64_t e0 = (uint64_t)blockIdx.x * SC_TILE + (uint64_t)threadIdx.x * SC_ITEMS;
  uint64_t key[SC_ITEMS], s = 0;
#pragma unroll
  for (int u = 0; u < SC_ITEMS; ++u) key[u] = (e0 + u < m) ? keys[e0 + u] : 0ull, s += curve_item(key[u]);
  uint64_t total;
  uint64_t run = sums[blockIdx.x] + block_excl_scan(s, lds, total);  // exclusive: the counts before element e0
  const unsigned long long tr = counters[3];
  const double recall = tr ? (double)tr : 1.0;
  CurvePart me;
  me.auc = 0.0, me.ign_auc = 0.0, me.f1 = -1.f, me.ign_f1 = -1.f, me.f1_pos = 0, me.w = -1;
  CurvePoint prev = {0.f, 0.f, 0.f};
  if (e0 > 0 && e0 < m) prev = curve_point(e0, run & 0xffffffffull, run >> 32, recall);
#pragma unroll
  for (int u = 0; u < SC_ITEMS; ++u) {
    const uint64_t e = e0 + u;
    if (e < m) {
      run += curve_item(key[u]);
      const CurvePoint pt = curve_point(e + 1, run & 0xffffffffull, run >> 32, recall);
      pr_x[e] = pt.x, pr_y[e] = pt.y;
      if (ign_pr_y) ign_pr_y[e] = pt.iy;
      const float f1 = curve_f1(pt.x, pt.y), if1 = curve_f1(pt.x, pt.iy);
      if (f1 > me.f1) me.f1 = f1, me.f1_pos = e;  // strict: the first maximum stays
      if (if1 > me.ign_f1) me.ign_f1 = if1;
      if ((double)key_score(key[u]) > input_theta) me.w = (long long)e;
      if (e > 0) {
        const double dx = (double)pt.x - (double)prev.x;
        me.auc += dx * ((double)pt.y + (double)prev.y) / 2.0;
        me.ign_auc += dx * ((double)pt.iy + (double)prev.iy) / 2.0;
      }
      prev = pt;
    }
  }
  sp[threadIdx.x] = me;
  __syncthreads();
  if (threadIdx.x == 0) {  // threads in index order: one fixed order of the fp64 sums, first maximum kept
    CurvePart a = sp[0];
    for (int t = 1; t < SC_THREADS; ++t) {
      const CurvePart& q = sp[t];
      a.auc += q.auc, a.ign_auc += q.ign_auc;
      if (q.f1 > a.f1) a.f1 = q.f1, a.f1_pos = q.f1_pos;
      if (q.ign_f1 > a.ign_f1) a.ign_f1 = q.ign_f1;
      if (q.w > a.w) a.w = q.w;
    }
    parts[blockIdx.x] = a;
  }
}

// res[0..10] = f1, f1_pos, theta, p, r, w, f1_at_w, auc, ign_f1, ign_auc, total_recall as used (all exact in fp64)
__global__ __launch_bounds__(64) void curve_finish_kernel(const CurvePart* __restrict__ parts, uint64_t nblk,
                                                          const uint64_t* __restrict__ keys, const float* __restrict__ pr_x,
                                                          const float* __restrict__ pr_y,
                                                          const unsigned long long* __restrict__ counters, double input_theta,
                                                          double* __restrict__ res) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  CurvePart a = parts[0];
  for (uint64_t q = 1; q < nblk; ++q) {  // workgroups in index order
    const CurvePart p = parts[q];
    a.auc += p.auc, a.ign_auc += p.ign_auc;
    if (p.f1 > a.f1) a.f1 = p.f1, a.f1_pos = p.f1_pos;
    if (p.ign_f1 > a.ign_f1) a.ign_f1 = p.ign_f1;
    if (p.w > a.w) a.w = p.w;
  }
  const uint64_t w = input_theta == -1.0 ? a.f1_pos : (a.w < 0 ? 0ull : (uint64_t)a.w);
  res[0] = (double)a.f1, res[1] = (double)a.f1_pos, res[2] = (double)key_score(keys[a.f1_pos]);
  res[3] = (double)pr_x[a.f1_pos], res[4] = (double)pr_y[a.f1_pos];
  res[5] = (double)w, res[6] = (double)curve_f1(pr_x[w], pr_y[w]);
  res[7] = a.auc, res[8] = (double)a.ign_f1, res[9] = a.ign_auc;
  res[10] = counters[3] ? (double)counters[3] : 1.0;
}

inline int64_t align256(int64_t x) { return (x + 255) & ~(int64_t)255; }

struct EvalWs {
  int64_t a, b, ghist, hist, sums32, sums64, parts, total;
  unsigned nwg;
  uint64_t nhist, nsum32, ncurve;
};
EvalWs eval_ws(int64_t n, int64_t m) {
  EvalWs w;
  w.nwg = (unsigned)((n + RS_TILE - 1) / RS_TILE);
  w.nhist = (uint64_t)RS_BINS * w.nwg;
  w.nsum32 = (w.nhist + SC_TILE - 1) / SC_TILE;
  w.ncurve = (uint64_t)((m + SC_TILE - 1) / SC_TILE);
  int64_t o = 0;
  w.a = o, o += align256(n * 8);
  w.b = o, o += align256(n * 8);
  w.ghist = o, o += align256(EV_PASSES * RS_BINS * 4);
  w.hist = o, o += align256((int64_t)w.nhist * 4);
  w.sums32 = o, o += align256((int64_t)w.nsum32 * 4);
  w.sums64 = o, o += align256((int64_t)w.ncurve * 8);
  w.parts = o, o += align256((int64_t)w.ncurve * (int64_t)sizeof(CurvePart));
  w.total = o;
  return w;
}

}  // namespace

int64_t eval_ws_bytes(int64_t n_records, int64_t n_keep) { return eval_ws(n_records, n_keep).total; }

int eval_scan(const float* logits, const float* labels, const uint8_t* in_train, const int* n_valid, const int64_t* doc_base,
              uint64_t* rec, int64_t capacity, int64_t* counters, int B, int N, int R, hipStream_t st) {
  ProfScope ps("eval_scan", st, 8.0 * B * N * N * R);
  hipLaunchKernelGGL(eval_scan_kernel, dim3((unsigned)(B * N)), dim3(256), 0, st, logits, labels, in_train, n_valid, doc_base, rec,
                     (uint64_t)capacity, (unsigned long long*)counters, N, R);
  return check_launch("eval_scan");
}

int eval_rank(const uint64_t* rec, int64_t n, void* ws, int64_t ws_bytes, int64_t* sorted_off, hipStream_t st) {
  const EvalWs w = eval_ws(n, 0);
  GC_REQUIRE(ws_bytes >= w.total, "eval_rank: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)w.total);
  char* base = (char*)ws;
  uint64_t* bufs[2] = {(uint64_t*)(base + w.a), (uint64_t*)(base + w.b)};
  unsigned* ghist = (unsigned*)(base + w.ghist);
  unsigned* hist = (unsigned*)(base + w.hist);
  unsigned* sums = (unsigned*)(base + w.sums32);
  ProfScope ps("eval_rank", st, 16.0 * n);
  if (hipMemsetAsync(ghist, 0, EV_PASSES * RS_BINS * 4, st) != hipSuccess) {
    set_error("eval_rank: hipMemsetAsync failed");
    return 2;
  }
  hipLaunchKernelGGL(radix_digit_hist_kernel, dim3((unsigned)std::min<int64_t>(1024, (n + RS_THREADS - 1) / RS_THREADS)),
                     dim3(RS_THREADS), 0, st, rec, (uint64_t)n, ghist);
  GC_TRY(check_launch("radix_digit_hist"));
  unsigned host_hist[EV_PASSES * RS_BINS];
  hipError_t herr = hipMemcpyAsync(host_hist, ghist, sizeof(host_hist), hipMemcpyDeviceToHost, st);
  if (herr == hipSuccess) herr = hipStreamSynchronize(st);
  if (herr != hipSuccess) {
    set_error("eval_rank: reading the digit histogram failed: %s", hipGetErrorString(herr));
    return 2;
  }
  const uint64_t* src = rec;
  int next = 0;
  for (int p = 0; p < EV_PASSES; ++p) {
    bool single = false;
    for (int d = 0; d < RS_BINS; ++d) single |= host_hist[p * RS_BINS + d] == (uint64_t)n;
    if (single) continue;  // every key has the same digit here: the pass would move nothing
    const int shift = EV_SCORE_SHIFT + 8 * p;
    uint64_t* dst = bufs[next];
    hipLaunchKernelGGL(radix_tile_hist_kernel, dim3(w.nwg), dim3(RS_THREADS), 0, st, src, (uint64_t)n, shift, hist, w.nwg);
    GC_TRY(check_launch("radix_tile_hist"));
    hipLaunchKernelGGL(scan_tile_sums_kernel<unsigned>, dim3((unsigned)w.nsum32), dim3(SC_THREADS), 0, st, hist, w.nhist, sums);
    hipLaunchKernelGGL(scan_sums_kernel<unsigned>, dim3(1), dim3(SC_THREADS), 0, st, sums, w.nsum32);
    hipLaunchKernelGGL(scan_apply_kernel<unsigned>, dim3((unsigned)w.nsum32), dim3(SC_THREADS), 0, st, hist, w.nhist, sums);
    GC_TRY(check_launch("radix_scan"));
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(w.nwg), dim3(RS_THREADS), 0, st, src, dst, (uint64_t)n, shift, hist, w.nwg);
    GC_TRY(check_launch("radix_scatter"));
    src = dst, next ^= 1;
  }
  if (src == rec) {  // all scores equal: the append order is the ranking
    if (hipMemcpyAsync(bufs[0], rec, (size_t)n * 8, hipMemcpyDeviceToDevice, st) != hipSuccess) {
      set_error("eval_rank: device copy failed");
      return 2;
    }
    src = bufs[0];
  }
  *sorted_off = (int64_t)((const char*)src - base);
  return 0;
}

int eval_curve(const uint64_t* keys, int64_t m, const int64_t* counters, double input_theta, float* pr_x, float* pr_y,
               float* ign_pr_y, double* res, void* ws, int64_t ws_bytes, int64_t n_records, hipStream_t st) {
  const EvalWs w = eval_ws(n_records, m);
  GC_REQUIRE(ws_bytes >= w.total, "eval_curve: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)w.total);
  uint64_t* sums = (uint64_t*)((char*)ws + w.sums64);
  CurvePart* parts = (CurvePart*)((char*)ws + w.parts);
  const unsigned long long* cnt = (const unsigned long long*)counters;
  ProfScope ps("eval_curve", st, 20.0 * m);
  hipLaunchKernelGGL(curve_tile_sums_kernel, dim3((unsigned)w.ncurve), dim3(SC_THREADS), 0, st, keys, (uint64_t)m, sums);
  hipLaunchKernelGGL(scan_sums_kernel<uint64_t>, dim3(1), dim3(SC_THREADS), 0, st, sums, w.ncurve);
  GC_TRY(check_launch("curve_scan"));
  hipLaunchKernelGGL(curve_apply_kernel, dim3((unsigned)w.ncurve), dim3(SC_THREADS), 0, st, keys, (uint64_t)m, sums, cnt,
                     input_theta, pr_x, pr_y, ign_pr_y, parts);
  GC_TRY(check_launch("curve_apply"));
  hipLaunchKernelGGL(curve_finish_kernel, dim3(1), dim3(64), 0, st, parts, w.ncurve, keys, pr_x, pr_y, cnt, input_theta, res);
  return check_launch("curve_finish");
}

}  // namespace gc
