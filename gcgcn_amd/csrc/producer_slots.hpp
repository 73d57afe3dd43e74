// What csrc/producer.hip (dense [B,N,N,S,T] byte tensors) and csrc/producer_rec.hip (the packed slot records themselves) share:
// the compact index's layout, the distance-id arithmetic, and the per-row bodies of the kernels that look at a sentence slot's
// tokens -- the index scan, the word attention forward, its two backward passes and tmax.  Each body is written once and takes a
// SLOT SOURCE:
//   DenseSlots  today's loads: one mask byte and one position id per (slot, token), the slot found through ix.row_slot;
//   RecSlots    the row's record (doc, u, v, j, s0, s1, h0, h1, t0, t1), found through row_rec and fetched once per row: the token
//               range [max(s0, 0), min(s1, T)) and the four mention bounds then sit in registers, a token is unmasked iff it lies in
//               the range and its distance ids are pos_id(t, h0, h1) / pos_id(t, t0, t1) truncated to a byte -- exactly what
//               gcgcn_tensorise (csrc/tensorise.hip) would have written into the dense tensors from the same record.
// Both forms number the compact rows alike and run the same arithmetic in the same order per row, so their results are equal bit
// for bit (tests/test_producer_rec_gpu.py).
#pragma once
#include "common.hpp"
#include "rowops.hpp"

namespace gc {

constexpr int PW = 4;      // waves per workgroup of the row kernels
constexpr int PGRID = 2048;  // persistent grid of the row kernels (8 workgroups per CU)
constexpr int HCLIM = 8;   // Hd <= 64 * HCLIM

struct ProdIdx {           // compact index of the live slots / pairs (device memory, int32)
  int* doc_counts;         // [B][2] live slots, live pairs per document
  int* pair_bits;          // [B*N*N] bit s set: slot s of the pair is live
  int* pair_row0;          // [B*N*N] first compact row of the pair (its live slots are consecutive rows)
  int* pair_prow;          // [B*N*N] compact pair index, -1: no live slot
  float* pair_div;         // [B*N*N] padded slots + 1e-10 (glove:205, 212); 0 for padding entities
  int* row_slot;           // [cap_rows] flat slot index ((b*N + i)*N + j)*S + s of a compact row
  int* prow_pair;          // [cap_pairs] flat pair index of a compact pair
  int* counts;             // [4] rows, pairs, overflow flag, unused
  int* doc_off;            // [B + 1] first compact row of each document (its live rows are consecutive)
  int* row_rng;            // [cap_rows] token range of the row's slot, t0 | t1 << 16 (written by the forward's word kernel)
  int* tmax;               // [B] one past the last token any live slot of the document covers
};

__device__ __forceinline__ int pos_at(const void* pos, int pos_bytes, long idx) {
  return pos_bytes == 8 ? (int)((const long long*)pos)[idx] : (pos_bytes == 4 ? ((const int*)pos)[idx] : (int)((const unsigned char*)pos)[idx]);
}

// config/Config.py:106-116: 0, 1, 2, 2, 3 x4, 4 x8, ... , 10 from 512 on (the table has 1024 entries)
__device__ __forceinline__ int dis2idx(int d) {
  d = min(max(d, 0), 1023);
  return d == 0 ? 0 : min(10, 32 - __clz(d));
}
// Config.py:190-203: signed bucket of the token's distance to a mention span [a, b): left of it negative, right positive,
// inside 0; then + dis_plus
__device__ __forceinline__ int pos_id(int k, int a, int b, int dis_plus) {
  const int dl = k - a, dr = k - b;
  int v = 0;
  if (dl < 0) v = -dis2idx(-dl);
  else if (dr > 0) v = dis2idx(dr);
  return v + dis_plus;
}

// =====================================================================================================================
// slot sources
// =====================================================================================================================
constexpr int REC_W = 10;  // ints per record: doc, u, v, j, s0, s1, h0, h1, t0, t1

// The record's verdict on a slot, shared by every kernel that reads a record: dropped (u, v, j or doc outside the batch's shape, or an
// empty range) or kept with its clipped range.  Live iff token 0 lies in the range.
struct RecSlot {
  bool kept, live;
  int r0, r1;              // [max(s0, 0), min(s1, T))
  long pair;               // (b*N + u)*N + v
};
__device__ __forceinline__ RecSlot rec_slot(const int* __restrict__ rec, int B, int N, int S, int T) {
  RecSlot o;
  const int b = rec[0], u = rec[1], v = rec[2], j = rec[3];
  o.r0 = max(rec[4], 0), o.r1 = min(rec[5], T);
  o.kept = b >= 0 && b < B && u >= 0 && u < N && v >= 0 && v < N && j >= 0 && j < S && o.r0 < o.r1;
  o.live = o.kept && o.r0 == 0;
  o.pair = ((long)b * N + u) * N + v;
  return o;
}

struct DenseSlots {
  static constexpr bool kRange = false;   // the token range of a row is found by scanning its mask
  const unsigned char* __restrict__ sen;
  const void* __restrict__ pos_h;
  const void* __restrict__ pos_t;
  int pos_bytes;

  struct Row {
    const unsigned char* m;
    const void* pos;
    int pos_bytes;
    long slot_base, b;
    int r0, r1;            // (unused: kRange == false)
    __device__ __forceinline__ int lo() const { return 0; }
    __device__ __forceinline__ int hi(int T) const { return T; }
    // Gathered scores of one (slot, side) for the wave's tokens t = c0 + 64 u + lane, u < 8: the mask byte, the position id and
    // the table entry of all eight chunks are requested before the first one is used (clamped addresses, not guarded loads: a
    // load inside a branch is waited for at the branch's end).  sc[u] = -inf for masked / out-of-range tokens.
    __device__ __forceinline__ void scores8(const float* __restrict__ tab, int T, int ND, int c0, int lane, float (&sc)[8]) const {
      unsigned char mm[8];
      int kk[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int tc = min(c0 + 64 * u + lane, T - 1);
        mm[u] = m[tc];
        kk[u] = pos_at(pos, pos_bytes, slot_base + tc);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int tc = min(c0 + 64 * u + lane, T - 1);
        sc[u] = tab[(long)min(max(kk[u], 0), ND - 1) * T + tc];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (c0 + 64 * u + lane >= T || !mm[u]) sc[u] = -INFINITY;
    }
  };
  __device__ __forceinline__ Row open(const ProdIdx& ix, int row, int side, long slots_per_doc, int T) const {
    Row o;
    const long slot = ix.row_slot[row];
    o.b = slot / slots_per_doc;
    o.m = sen + slot * T;
    o.pos = side ? pos_t : pos_h;
    o.pos_bytes = pos_bytes;
    o.slot_base = slot * T;
    o.r0 = 0, o.r1 = T;
    return o;
  }
  // pass 2 of the backward: does live row `row`, whose range holds token t, have the token unmasked -- and its two clamped ids
  __device__ __forceinline__ bool token(const ProdIdx& ix, int row, int t, int T, int ND, int& kh, int& kt) const {
    const long slot = ix.row_slot[row];
    if (!sen[slot * T + t]) return false;
    kh = min(max(pos_at(pos_h, pos_bytes, slot * T + t), 0), ND - 1);
    kt = min(max(pos_at(pos_t, pos_bytes, slot * T + t), 0), ND - 1);
    return true;
  }
};

struct RecSlots {
  static constexpr bool kRange = true;    // the record states the row's token range
  const int* __restrict__ records;        // [n_records][REC_W]
  const int* __restrict__ row_rec;        // [rows] record of a compact row
  int dis_plus;

  // the id gcgcn_tensorise stores ((unsigned char)pos_id), clamped as the dense kernels clamp what they read
  static __device__ __forceinline__ int id_of(int t, int a, int b, int dis_plus, int ND) {
    return min((int)(unsigned char)pos_id(t, a, b, dis_plus), ND - 1);
  }

  struct Row {
    long b;
    int r0, r1, a0, a1, dis_plus;
    __device__ __forceinline__ int lo() const { return r0 & ~63; }
    __device__ __forceinline__ int hi(int) const { return r1; }
    // The same eight chunks; tokens outside [r0, r1) read the table at the nearest token inside (an address the range's own lanes
    // read anyway) and get -inf.
    __device__ __forceinline__ void scores8(const float* __restrict__ tab, int T, int ND, int c0, int lane, float (&sc)[8]) const {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int tc = min(max(c0 + 64 * u + lane, r0), r1 - 1);
        sc[u] = tab[(long)id_of(tc, a0, a1, dis_plus, ND) * T + tc];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int t = c0 + 64 * u + lane;
        if (t < r0 || t >= r1) sc[u] = -INFINITY;
      }
    }
  };
  __device__ __forceinline__ Row open(const ProdIdx&, int row, int side, long, int T) const {
    Row o;
    const int* rec = records + (long)row_rec[row] * REC_W;
    o.b = rec[0];
    o.r0 = max(rec[4], 0), o.r1 = min(rec[5], T);
    o.a0 = rec[side ? 8 : 6], o.a1 = rec[side ? 9 : 7];
    o.dis_plus = dis_plus;
    return o;
  }
  __device__ __forceinline__ bool token(const ProdIdx&, int row, int t, int, int ND, int& kh, int& kt) const {
    const int* rec = records + (long)row_rec[row] * REC_W;
    const int2 h = *reinterpret_cast<const int2*>(rec + 6), q = *reinterpret_cast<const int2*>(rec + 8);   // (8-byte aligned: 40-byte records)
    kh = id_of(t, h.x, h.y, dis_plus, ND);
    kt = id_of(t, q.x, q.y, dis_plus, ND);
    return true;                          // row_rng IS the mask: a record's range has no holes
  }
};

// =====================================================================================================================
// index, pass A: one workgroup per document.  bits_of(pp, p) -> the liveness bits of pair p of this document (flat index pp),
// asked only for pairs of real entities.
// =====================================================================================================================
// (Round 5: one workgroup per document is 32 workgroups of pure latency -- per 256 pairs it ran S dependent byte loads and a
// 16-barrier Hillis-Steele scan, 28 us per call and two calls per step of the model.  Now the liveness bytes of eight chunks of
// pairs are requested together, and the scan is a wave prefix (shuffles) plus one hand-over between the four waves: two
// barriers per chunk.  Same integers out.)
template <class BitsOf>
__device__ __forceinline__ void prod_index_a_body(BitsOf bits_of, const int* __restrict__ n_valid, const ProdIdx& ix, int N) {
  __shared__ int wsum[2][4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nv = n_valid ? min(max(n_valid[b], 0), N) : N;
  const int NN = N * N;
  auto wave_incl = [&](int v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(v, d, 64);
      if (lane >= d) v += t;
    }
    return v;
  };
  int run_s = 0, run_p = 0;
  constexpr int CH = 8;   // chunks of 256 pairs whose loads are in flight together
  for (int base0 = 0; base0 < NN; base0 += CH * 256) {
    int bitsv[CH];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
      const int p = base0 + ch * 256 + tid;
      int bits = 0;
      if (p < NN) {
        const int i = p / N, j = p - i * N;
        if (i < nv && j < nv) bits = bits_of((long)b * NN + p);
      }
      bitsv[ch] = bits;
    }
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
      const int base = base0 + ch * 256;
      if (base >= NN) break;                       // (uniform)
      const int p = base + tid, bits = bitsv[ch];
      const int c = __popc(bits), live = c > 0;
      const int ic = wave_incl(c), il = wave_incl(live);
      if (lane == 63) wsum[0][wave] = ic, wsum[1][wave] = il;
      __syncthreads();
      int offc = 0, offl = 0, totc = 0, totl = 0;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const int a_ = wsum[0][w], q_ = wsum[1][w];
        if (w < wave) offc += a_, offl += q_;
        totc += a_, totl += q_;
      }
      if (p < NN) {
        const long pp = (long)b * NN + p;
        ix.pair_bits[pp] = bits;
        ix.pair_row0[pp] = run_s + offc + ic - c;          // local to the document; pass B adds the document's offset
        ix.pair_prow[pp] = live ? run_p + offl + il - 1 : -1;
      }
      run_s += totc, run_p += totl;
      __syncthreads();
    }
  }
  if (tid == 0) ix.doc_counts[2 * b] = run_s, ix.doc_counts[2 * b + 1] = run_p;
}

// =====================================================================================================================
// word attention of the live slots (glove:184-187): CW[row, side*Hd + c] = sum_t softmax_t(score)[t] ctx[b, t, c]
// wsm: PW * T floats of LDS (the un-normalised weights of the wave's slot)
// =====================================================================================================================
template <int HC, class Src>
__device__ __forceinline__ void prod_word_fwd_body(const Src& src, float* wsm, const float* __restrict__ ctx,
                                                   const float* __restrict__ table, const ProdIdx& ix, float* __restrict__ CW,
                                                   float* __restrict__ stats, int N, int S, int T, int Hd, int ND) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* ev = wsm + (long)wave * T;
  const int nrows = ix.counts[0], total = 2 * nrows;
  const long slots_per_doc = (long)N * N * S;
  for (int r0 = blockIdx.x * PW; r0 < total; r0 += gridDim.x * PW) {
    const int r = r0 + wave;
    const bool on = r < total;
    int t0 = T, t1 = 0;
    float inv = 0.f;
    long b = 0;
    if (on) {
      const int row = r >> 1, side = r & 1;
      const typename Src::Row sr = src.open(ix, row, side, slots_per_doc, T);
      b = sr.b;
      const float* tab = table + b * ND * T;
      float mx = -INFINITY;
      for (int c0 = sr.lo(); c0 < sr.hi(T); c0 += 512) {
        float sc[8];
        sr.scores8(tab, T, ND, c0, lane, sc);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int t = c0 + 64 * u + lane;
          if (t < sr.hi(T)) {
            ev[t] = sc[u];
            if (!Src::kRange && sc[u] != -INFINITY) t0 = min(t0, t), t1 = max(t1, t + 1);
            mx = fmaxf(mx, sc[u]);
          }
        }
      }
      mx = wave_max(mx);
      if (Src::kRange) t0 = sr.r0, t1 = sr.r1;
      else t0 = -(int)wave_max((float)-t0), t1 = (int)wave_max((float)t1);   // exact for |t| < 2^24
      float sum = 0.f;
      for (int t = sr.lo() + lane; t < sr.hi(T); t += 64) {
        const float e = ev[t] == -INFINITY ? 0.f : expf(ev[t] - mx);   // masked tokens: exp(-100000 - max) == 0 in fp32
        ev[t] = e;
        sum += e;
      }
      sum = wave_sum(sum);
      inv = 1.f / sum;
      if (lane == 0) {
        stats[2 * (long)r] = mx, stats[2 * (long)r + 1] = inv;
        if (side == 0) ix.row_rng[row] = t0 | (t1 << 16);   // the slot's token range (T <= 2048): read again by the backward
      }
    }
    __syncthreads();  // ev[] written lane-wise, read by every lane below (uniform trip count: every wave gets here)
    if (on) {
      const int row = r >> 1, side = r & 1;
      const float* cb = ctx + b * T * Hd;
      float acc[HC];
#pragma unroll
      for (int cc = 0; cc < HC; ++cc) acc[cc] = 0.f;
      int t = t0;
      for (; t + 3 < t1; t += 4) {  // four token rows in flight
        float x[4][HC];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int cc = 0; cc < HC; ++cc) {
            const int c = lane + 64 * cc;
            x[u][cc] = c < Hd ? cb[(long)(t + u) * Hd + c] : 0.f;
          }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float e = ev[t + u];
#pragma unroll
          for (int cc = 0; cc < HC; ++cc) acc[cc] = fmaf(e, x[u][cc], acc[cc]);
        }
      }
      for (; t < t1; ++t) {
        const float e = ev[t];
#pragma unroll
        for (int cc = 0; cc < HC; ++cc) {
          const int c = lane + 64 * cc;
          if (c < Hd) acc[cc] = fmaf(e, cb[(long)t * Hd + c], acc[cc]);
        }
      }
#pragma unroll
      for (int cc = 0; cc < HC; ++cc) {
        const int c = lane + 64 * cc;
        if (c < Hd) CW[(long)row * 2 * Hd + side * Hd + c] = acc[cc] * inv;
      }
    }
    __syncthreads();  // before the next slot overwrites ev[]
  }
  // rows [nrows, roundup64(nrows)) feed the K-dynamic GEMMs as zeros
  if (blockIdx.x == 0) {
    const int hi = (nrows + 63) & ~63;
    for (long e = (long)nrows * 2 * Hd + threadIdx.x; e < (long)hi * 2 * Hd; e += 64 * PW) CW[e] = 0.f;
  }
}

// ---- tmax[b] = one past the last token any live slot of document b covers (bounds the backward's per-token work) -------
__device__ __forceinline__ void prod_tmax_body(const ProdIdx& ix) {
  __shared__ int red[4];
  const int b = blockIdx.x;
  int m = 0;
  for (int row = ix.doc_off[b] + threadIdx.x; row < ix.doc_off[b + 1]; row += 256) m = max(m, ix.row_rng[row] >> 16);
  m = (int)wave_max((float)m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) ix.tmax[b] = max(max(red[0], red[1]), max(red[2], red[3]));
}

// =====================================================================================================================
// backward of the word attention, two passes, no atomics
//   dcw = dCW[row, side]:  g[t] = dcw . ctx[t];  dscore[t] = att[t] (g[t] - sum_t att g)
//   dtable[b, pos[t], t] += dscore,  dctx[b, t, :] += att[t] dcw     -- sums over MANY (row, side) per (document, token)
// Pass 1 (one wave per (row, side), like the forward): the softmax-weighted sum  dots[r] = sum_t att[t] g[t], the slot's
// token range and the document's last covered token.  Pass 2 (one workgroup per (document, token), the OWNER of
// dctx[b, t, :] and dtable[b, :, t]): scans the document's live rows, and for those whose slot holds the token recomputes
// att and g (a 128-wide dot with the token state it keeps in registers) and accumulates in a fixed order -- deterministic,
// and ~20x faster than scatter-adding with fp32 atomics.
// =====================================================================================================================
// pass 1; wsm: PW * (T + Hd) floats of LDS
template <int HC, class Src>
__device__ __forceinline__ void prod_word_bwd_rows_body(const Src& src, float* wsm, const float* __restrict__ ctx,
                                                        const float* __restrict__ table, const float* __restrict__ stats,
                                                        const float* __restrict__ dCW, const ProdIdx& ix, float* __restrict__ dots,
                                                        int N, int S, int T, int Hd, int ND) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* av = wsm + (long)wave * T;  // att[t]
  const int nrows = ix.counts[0], total = 2 * nrows;
  const long slots_per_doc = (long)N * N * S;
  for (int r0 = blockIdx.x * PW; r0 < total; r0 += gridDim.x * PW) {
    const int r = r0 + wave;
    const bool on = r < total;
    int t0 = T, t1 = 0;
    long b = 0;
    if (on) {
      const int row = r >> 1, side = r & 1;
      const typename Src::Row sr = src.open(ix, row, side, slots_per_doc, T);
      b = sr.b;
      const float* tab = table + b * ND * T;
      const float mx = stats[2 * (long)r], inv = stats[2 * (long)r + 1];
      for (int c0 = sr.lo(); c0 < sr.hi(T); c0 += 512) {
        float sc[8];
        sr.scores8(tab, T, ND, c0, lane, sc);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int t = c0 + 64 * u + lane;
          if (t < sr.hi(T)) {
            av[t] = sc[u] == -INFINITY ? 0.f : expf(sc[u] - mx) * inv;
            if (!Src::kRange && sc[u] != -INFINITY) t0 = min(t0, t), t1 = max(t1, t + 1);
          }
        }
      }
      if (Src::kRange) t0 = sr.r0, t1 = sr.r1;
      else t0 = -(int)wave_max((float)-t0), t1 = (int)wave_max((float)t1);
    }
    float* dl = wsm + (long)PW * T + (long)wave * Hd;   // this (row, side)'s dCW row, broadcast to every lane below
    if (on)
      for (int c = lane; c < Hd; c += 64) dl[c] = dCW[(long)(r >> 1) * 2 * Hd + (r & 1) * Hd + c];
    __syncthreads();
    if (on && (Hd & 3) == 0) {
      // lanes over TOKENS: g[t] = dcw . ctx[t] is a private 128-wide dot per lane (16-byte loads of the lane's own token row,
      // dcw broadcast from LDS) -- one wave reduction per 64 tokens instead of one per token
      const float* cb = ctx + b * T * Hd;
      float dotsum = 0.f;
      for (int tb = t0; tb < t1; tb += 64) {
        const int t = tb + lane;
        const float4* cr = reinterpret_cast<const float4*>(cb + (long)min(t, t1 - 1) * Hd);
        float g0 = 0.f, g1 = 0.f;
        for (int q = 0; q < Hd / 4; q += 2) {
          const float4 x0 = cr[q], x1 = cr[q + 1 < Hd / 4 ? q + 1 : q];
          const float4 d0 = *reinterpret_cast<const float4*>(dl + 4 * q), d1 = *reinterpret_cast<const float4*>(dl + 4 * (q + 1 < Hd / 4 ? q + 1 : q));
          g0 = fmaf(x0.x, d0.x, fmaf(x0.y, d0.y, fmaf(x0.z, d0.z, fmaf(x0.w, d0.w, g0))));
          if (q + 1 < Hd / 4) g1 = fmaf(x1.x, d1.x, fmaf(x1.y, d1.y, fmaf(x1.z, d1.z, fmaf(x1.w, d1.w, g1))));
        }
        if (t < t1) dotsum = fmaf(av[t], g0 + g1, dotsum);
      }
      dotsum = wave_sum(dotsum);
      if (lane == 0) dots[r] = dotsum;
    } else if (on) {
      const int row = r >> 1, side = r & 1;
      const float* cb = ctx + b * T * Hd;
      float dcw[HC], dotsum = 0.f;
#pragma unroll
      for (int cc = 0; cc < HC; ++cc) dcw[cc] = (lane + 64 * cc) < Hd ? dCW[(long)row * 2 * Hd + side * Hd + lane + 64 * cc] : 0.f;
      for (int t = t0; t < t1; t += 4) {  // four tokens at a time: independent loads, interleaved reductions
        float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int tt = min(t + u, t1 - 1);
#pragma unroll
          for (int cc = 0; cc < HC; ++cc) {
            const int c = lane + 64 * cc;
            if (c < Hd) p[u] = fmaf(dcw[cc], cb[(long)tt * Hd + c], p[u]);
          }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const float g = wave_sum(p[u]);
          if (t + u < t1) dotsum = fmaf(av[t + u], g, dotsum);
        }
      }
      if (lane == 0) dots[r] = dotsum;
    }
    __syncthreads();
  }
}

// pass 2: one workgroup per (document, token); sm: PW * (Hd + ND) floats of LDS
template <int HC, class Src>
__device__ __forceinline__ void prod_word_bwd_tok_body(const Src& src, float* sm, const float* __restrict__ ctx,
                                                       const float* __restrict__ table, const float* __restrict__ stats,
                                                       const float* __restrict__ dCW, const float* __restrict__ dots, const ProdIdx& ix,
                                                       float* __restrict__ dtable, float* __restrict__ dctx, int T, int Hd, int ND) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long bt = blockIdx.x;
  const int b = (int)(bt / T), t = (int)(bt - (long)b * T);
  float* accs = sm;                    // [PW][Hd] partial dctx rows
  float* dts = sm + (long)PW * Hd;     // [PW][ND] partial dtable columns
  for (int e = threadIdx.x; e < PW * ND; e += 64 * PW) dts[e] = 0.f;
  float acc[HC], cx[HC];
#pragma unroll
  for (int cc = 0; cc < HC; ++cc) acc[cc] = 0.f, cx[cc] = (lane + 64 * cc) < Hd ? ctx[bt * Hd + lane + 64 * cc] : 0.f;
  __syncthreads();
  if (t < ix.tmax[b]) {
    const int r_lo = ix.doc_off[b], r_hi = ix.doc_off[b + 1];
    const float* tab = table + (long)b * ND * T;
    float* dtw = dts + wave * ND;
    for (int base = r_lo + wave * 64; base < r_hi; base += PW * 64) {
      // lane-parallel: everything a hit needs except the dCW rows -- one latency chain per 64 candidate rows, not per hit
      const int row = base + lane;
      bool hit = false;
      float ah = 0.f, at = 0.f, dh = 0.f, dt = 0.f;
      int kh = 0, kt = 0;
      if (row < r_hi) {
        const int rg = ix.row_rng[row];
        if (t >= (rg & 0xffff) && t < (rg >> 16)) {
          if (src.token(ix, row, t, T, ND, kh, kt)) {
            hit = true;
            const float4 st = *reinterpret_cast<const float4*>(stats + 4L * row);   // max / 1/sum of the head, of the tail side
            ah = expf(tab[(long)kh * T + t] - st.x) * st.y;
            at = expf(tab[(long)kt * T + t] - st.z) * st.w;
            dh = dots[2L * row], dt = dots[2L * row + 1];
          }
        }
      }
      unsigned long long todo = __ballot(hit);
      float nh[HC], nt[HC];   // dCW rows of the NEXT hit, requested one hit ahead
      int l = todo ? __ffsll((long long)todo) - 1 : 0;
#pragma unroll
      for (int cc = 0; cc < HC; ++cc) {
        const int c = lane + 64 * cc;
        nh[cc] = (todo && c < Hd) ? dCW[(long)(base + l) * 2 * Hd + c] : 0.f;
        nt[cc] = (todo && c < Hd) ? dCW[(long)(base + l) * 2 * Hd + Hd + c] : 0.f;
      }
      while (todo) {
        const int cur = l;
        todo &= todo - 1;
        float ch[HC], ct[HC], ph = 0.f, pt = 0.f;
#pragma unroll
        for (int cc = 0; cc < HC; ++cc) ch[cc] = nh[cc], ct[cc] = nt[cc];
        if (todo) {
          l = __ffsll((long long)todo) - 1;
#pragma unroll
          for (int cc = 0; cc < HC; ++cc) {
            const int c = lane + 64 * cc;
            nh[cc] = c < Hd ? dCW[(long)(base + l) * 2 * Hd + c] : 0.f;
            nt[cc] = c < Hd ? dCW[(long)(base + l) * 2 * Hd + Hd + c] : 0.f;
          }
        }
#pragma unroll
        for (int cc = 0; cc < HC; ++cc) ph = fmaf(ch[cc], cx[cc], ph), pt = fmaf(ct[cc], cx[cc], pt);
        const float gh = wave_sum(ph), gt = wave_sum(pt);
        const float a_h = lane_value(ah, cur), a_t = lane_value(at, cur);
        if (lane == 0) {   // one lane, program order: deterministic
          dtw[__builtin_amdgcn_readlane(kh, cur)] += a_h * (gh - lane_value(dh, cur));
          dtw[__builtin_amdgcn_readlane(kt, cur)] += a_t * (gt - lane_value(dt, cur));
        }
#pragma unroll
        for (int cc = 0; cc < HC; ++cc) acc[cc] = fmaf(a_h, ch[cc], fmaf(a_t, ct[cc], acc[cc]));
      }
    }
  }
#pragma unroll
  for (int cc = 0; cc < HC; ++cc)
    if ((lane + 64 * cc) < Hd) accs[wave * Hd + lane + 64 * cc] = acc[cc];
  __syncthreads();
  for (int c = threadIdx.x; c < Hd; c += 64 * PW) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < PW; ++w) v += accs[w * Hd + c];
    dctx[bt * Hd + c] = v;
  }
  for (int k = threadIdx.x; k < ND; k += 64 * PW) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < PW; ++w) v += dts[w * ND + k];
    dtable[((long)b * ND + k) * T + t] = v;
  }
}

// =====================================================================================================================
// host side: what the two files' entry points share (defined in csrc/producer.hip unless said otherwise)
// =====================================================================================================================
// kernels are instantiated for HC = ceil(Hd / 64) in {1, 2, 4, 8} column chunks per lane (the reference's Hd = 128: HC = 2)
#define PROD_LAUNCH(kernel, Hd, grid, block, lds, st, ...)                                            \
  do {                                                                                                \
    const int _hc = ((Hd) + 63) / 64;                                                                 \
    if (_hc <= 1) hipLaunchKernelGGL((kernel<1>), grid, block, lds, st, __VA_ARGS__);                 \
    else if (_hc <= 2) hipLaunchKernelGGL((kernel<2>), grid, block, lds, st, __VA_ARGS__);            \
    else if (_hc <= 4) hipLaunchKernelGGL((kernel<4>), grid, block, lds, st, __VA_ARGS__);            \
    else hipLaunchKernelGGL((kernel<8>), grid, block, lds, st, __VA_ARGS__);                          \
  } while (0)

// Where a call's sentence slots come from.  records == nullptr with rec == false: the dense tensors; rec == true: the record table
// (n_records may be 0, records then unused) and row_rec, the compact rows' records, inside the caller's int32 buffer.
struct ProdSrc {
  const unsigned char* sen = nullptr;
  const void* pos_h = nullptr;
  const void* pos_t = nullptr;
  int pos_bytes = 0;
  bool rec = false;
  int n_records = 0;
  const int* records = nullptr;
  int dis_plus = 0;
  int* row_rec = nullptr;
};

struct ProdBufs {  // caller-owned device memory (include/gcgcn.h lists the sizes)
  float *sentF, *disF, *table, *CW, *stats, *cwa, *sfeat, *nterm, *score, *CS, *Ec;
};
struct ProdGrads {  // caller-owned workspace of the backward pass
  float *dEc, *dCS, *dcwa, *dsfeat, *dnterm, *dCW, *dtable, *dsentF, *ddisF, *dwb, *part, *wpair, *dots, *tpart;
};
struct ProdBound { ProdIdx ix; ProdBufs w; ProdGrads g; float* scratch; int* row_rec; long n_int, n_fwd, n_bwd, counts_off, prow_off, ec_off; };

ProdBound prod_bind(int32_t* ibuf, float* fwd, float* bwd, bool want_bwd, int B, int N, int S, int T, int Hd, int P, int ND,
                    long cap_rows, long cap_pairs);
long prod_scratch_elems(int B, int N, int T, int Hd);
long prod_det_elems(int Hd, long cap_pairs);
int prod_wpair(const int* n_valid, float* wpair, int B, int N, hipStream_t st);
int prod_index_b(const int* n_valid, ProdIdx ix, int B, int N, int S, long cap_rows, long cap_pairs, hipStream_t st);   // pass B alone
int prod_fwd(int B, int N, int S, int T, int Hd, int P, int ND, const float* ctx, const ProdSrc& src, const float* node,
             const float* dis_table, const int* n_valid, const float* flat, ProdIdx ix, long cap_rows, long cap_pairs, ProdBufs w, float* E,
             float* ws, long wse, hipStream_t st);
int prod_bwd(int B, int N, int S, int T, int Hd, int P, int ND, const float* ctx, const ProdSrc& src, const float* node,
             const float* dis_table, const int* n_valid, const float* flat, ProdIdx ix, long cap_rows, long cap_pairs, ProdBufs w,
             const float* dE, ProdGrads g, float* dctx, float* dnode, float* ddis_table, float* dflat, float* ws, long wse, hipStream_t st,
             const float* dEc_in = nullptr, bool det = false, float* detbuf = nullptr);

// csrc/producer_rec.hip: the record route's launches, called by prod_fwd / prod_bwd where src.rec
int prod_rec_index(const ProdSrc& src, const int* n_valid, ProdIdx ix, int B, int N, int S, int T, long cap_rows, long cap_pairs,
                   hipStream_t st);
int prod_rec_word_fwd(const ProdSrc& src, const float* ctx, const float* table, ProdIdx ix, float* CW, float* stats, int N, int S, int T,
                      int Hd, int ND, hipStream_t st);
int prod_rec_word_bwd(const ProdSrc& src, const float* ctx, const float* table, const float* stats, const float* dCW, ProdIdx ix,
                      float* dots, float* dtable, float* dctx, int B, int N, int S, int T, int Hd, int ND, hipStream_t st);

}  // namespace gc
