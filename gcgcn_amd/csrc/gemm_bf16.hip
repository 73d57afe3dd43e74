// bf16-operand products for the BERT encoder's Linears (gemm_bf16.hpp has the contract).
//
// One workgroup of four waves computes a 64 x 64 tile of C over a run of 64-deep k-steps.  Per k-step the two operand tiles are
// fetched as fp32 into registers (coalesced float4 loads along whichever dimension is contiguous in memory), rounded to bf16 by the
// packed convert and written into ONE kind of LDS image for every storage form:
//     As [64 rows of op(A)][64 k + 8 pad] bf16,  Bs [64 columns of op(B)][64 k + 8 pad] bf16        (k contiguous, 144-byte rows)
// An operand stored [K][.] (the weight gradient's two, NN's B) is transposed while the image is written: a thread holds a 4 (k) x 4
// (row) patch and writes four 8-byte k-runs.  The loads of step s + 1 are issued before the matrix instructions of step s, so
// they fly under them; the image is single-buffered (two barriers per step, 18 KB of LDS).
// Wave w owns the 32 x 32 quarter (w & 1, w >> 1) as 2 x 2 tiles of v_mfma_f32_16x16x32_bf16.  Both operand fragments of that
// instruction are read the same way from a k-contiguous image (lane l: row l & 15, k = 8 (l >> 4) .. + 7: one 16-byte LDS read), so
// the product is issued TRANSPOSED (op(B)'s fragment as the instruction's A): a lane's four accumulator registers are then four
// consecutive COLUMNS of one row of C and the epilogue loads bias / add and stores C as float4.
// The 144-byte row pitch puts the 16 rows of a fragment read on 16 disjoint 4-bank groups.
#include "gemm_bf16.hpp"

namespace gc {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int TM = 64;          // tile rows and columns
constexpr int TK = 64;          // k-step
constexpr int LP = TK + 8;      // bf16 elements per image row
constexpr int MAX_SPLITS = 16;
constexpr int LIVE_WORDS = 32;  // rb_mode 2: the liveness bitmap of a split run's k-steps (1024 of them; longer runs drop the list)

struct Params {
  GemmBf16Args g;
  int tiles_m, tiles_n, splits, kchunk;   // kchunk: k per split, a multiple of TK
  int vec;                                // every pointer 16-byte aligned, every ld a multiple of 4 and K a multiple of TK
};

// What a tile knows of the row-block list (RB = the mode the launcher kept; 0: nothing, an empty argument).
//   mode 1: the tile's four 16-row blocks are memory rows base[j] .. + 15; the first `live` of them are live (the list has the live
//           blocks first, so a tile's live blocks are a prefix)
//   mode 2: bit s of steps[] = k-step s of this split run has a live block (LDS, written by the kernel in front of the tile)
struct Rows {
  int b0 = 0, b1 = 0, b2 = 0, b3 = 0;   // four scalars, not an array: an array behind a reference is a stack slot
  int live = 0;
  const uint32_t* steps = nullptr;
  __device__ __forceinline__ int base(const int j) const { return j == 0 ? b0 : j == 1 ? b1 : j == 2 ? b2 : b3; }
};

// two floats -> two bf16, round to nearest even (v_cvt_pk_bf16_f32)
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
}

// What a thread holds of one operand tile between its global loads and its LDS writes.
//   KC  (stored [rows][K]): element j = float4 at row (t + 256 j) >> 4, k = 4 ((t + 256 j) & 15) .. + 3
//   !KC (stored [K][rows]): element j = float4 at k = 4 (t >> 4) + j, rows 4 (t & 15) .. + 3
struct Patch {
  f32x4 v[4];
};

// G: guarded -- an element outside [r0, R) x [k0, kend) is a zero that is never loaded.
template <bool KC, bool G>
__device__ __forceinline__ void fetch(Patch& p, const float* __restrict__ P, const long ld, const int r0, const int R, const int k0,
                                      const int kend) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int r, k;   // of element .x; the other three follow along the contiguous dimension
    if constexpr (KC) r = r0 + ((t + 256 * j) >> 4), k = k0 + 4 * ((t + 256 * j) & 15);
    else r = r0 + 4 * (t & 15), k = k0 + 4 * (t >> 4) + j;
    const float* src = KC ? P + (long)r * ld + k : P + (long)k * ld + r;
    if constexpr (!G) {
      p.v[j] = *reinterpret_cast<const f32x4*>(src);
    } else {
      float e[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool in = KC ? (r < R && k + i < kend) : (r + i < R && k < kend);
        e[i] = in ? src[i] : 0.f;
      }
      p.v[j] = f32x4{e[0], e[1], e[2], e[3]};
    }
  }
}

// rb_mode 1, A stored [rows][K]: element j of the patch lies in block j of the tile (row (t >> 4) of it).  A dead block is zeros
// that are never loaded.
__device__ __forceinline__ void fetch_rows(Patch& p, const float* __restrict__ P, const long ld, const Rows& rw, const int k0) {
  const int t = threadIdx.x;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < rw.live) p.v[j] = *reinterpret_cast<const f32x4*>(P + (long)(rw.base(j) + (t >> 4)) * ld + k0 + 4 * (t & 15));
    else p.v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
}

// rb_mode 2: the first live k-step at or after step s of the run, or nsteps (uniform: the bitmap words are read into scalars)
__device__ __forceinline__ int next_live(const uint32_t* steps, int s, const int nsteps) {
  while (s < nsteps) {
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)steps[s >> 5]) >> (s & 31);
    if (w) return s + __builtin_ctz(w);
    s = (s | 31) + 1;
  }
  return nsteps;
}

template <bool KC>
__device__ __forceinline__ void stage(const Patch& p, __bf16* __restrict__ img) {
  const int t = threadIdx.x;
  if constexpr (KC) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = (t + 256 * j) >> 4, k = 4 * ((t + 256 * j) & 15);
      *reinterpret_cast<uint2*>(img + r * LP + k) = make_uint2(pack2(p.v[j][0], p.v[j][1]), pack2(p.v[j][2], p.v[j][3]));
    }
  } else {   // the transpose: row 4 (t & 15) + i takes component i of the four k
    const int r = 4 * (t & 15), k = 4 * (t >> 4);
    *reinterpret_cast<uint2*>(img + (r + 0) * LP + k) = make_uint2(pack2(p.v[0][0], p.v[1][0]), pack2(p.v[2][0], p.v[3][0]));
    *reinterpret_cast<uint2*>(img + (r + 1) * LP + k) = make_uint2(pack2(p.v[0][1], p.v[1][1]), pack2(p.v[2][1], p.v[3][1]));
    *reinterpret_cast<uint2*>(img + (r + 2) * LP + k) = make_uint2(pack2(p.v[0][2], p.v[1][2]), pack2(p.v[2][2], p.v[3][2]));
    *reinterpret_cast<uint2*>(img + (r + 3) * LP + k) = make_uint2(pack2(p.v[0][3], p.v[1][3]), pack2(p.v[2][3], p.v[3][3]));
  }
}

// One tile over k in [kb, ke).  out / ldo: C with the epilogue, or the split's slab of partial sums without it.
// RB (the row-block mode the launch kept, interior problems only: G is false then) changes three things.  Mode 1: A's rows, and the
// rows of add and of the output, are the list's (rw.base), dead blocks are fed as zeros and stored as zeros or not at all.  Mode 2:
// "the next step" is the next LIVE step of the run (rw.steps); a dead step is not fetched, staged or multiplied.
template <bool AKC, bool BKC, bool G, int RB = 0>
__device__ __forceinline__ void tile_body(const GemmBf16Args& g, __bf16* __restrict__ As, __bf16* __restrict__ Bs, const int m0, const int n0,
                                          const int kb, const int ke, float* __restrict__ out, const long ldo, const bool epilogue,
                                          const Rows& rw = Rows{}) {
  static_assert(RB == 0 || !G, "a launch that keeps the row-block list has interior tiles only");
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, c16 = l & 15, q = l >> 4;
  const int wm = 32 * (w & 1), wn = 32 * (w >> 1);
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  Patch pa, pb;
  if constexpr (RB != 2) {
    if (kb < ke) {
      if constexpr (RB == 1) fetch_rows(pa, g.A, g.lda, rw, kb);
      else fetch<AKC, G>(pa, g.A, g.lda, m0, g.M, kb, ke);
      fetch<BKC, G>(pb, g.B, g.ldb, n0, g.N, kb, ke);
    }
    for (int k0 = kb; k0 < ke; k0 += TK) {
      __syncthreads();   // the previous step's readers are done with the image
      stage<AKC>(pa, As);
      stage<BKC>(pb, Bs);
      __syncthreads();
      if (k0 + TK < ke) {   // uniform; the next step's loads fly under this step's matrix instructions
        if constexpr (RB == 1) fetch_rows(pa, g.A, g.lda, rw, k0 + TK);
        else fetch<AKC, G>(pa, g.A, g.lda, m0, g.M, k0 + TK, ke);
        fetch<BKC, G>(pb, g.B, g.ldb, n0, g.N, k0 + TK, ke);
      }
#pragma unroll
      for (int s = 0; s < TK / 32; ++s) {
        bf16x8 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          a[i] = *reinterpret_cast<const bf16x8*>(As + (wm + 16 * i + c16) * LP + 32 * s + 8 * q);
          b[i] = *reinterpret_cast<const bf16x8*>(Bs + (wn + 16 * i + c16) * LP + 32 * s + 8 * q);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
      }
    }
  } else {   // the same loop over the run's LIVE steps, each at its dense position: "the next step" is the next live one
    const int nsteps = (ke - kb) / TK;
    int st = next_live(rw.steps, 0, nsteps);
    if (st < nsteps) {
      fetch<AKC, G>(pa, g.A, g.lda, m0, g.M, kb + TK * st, ke);
      fetch<BKC, G>(pb, g.B, g.ldb, n0, g.N, kb + TK * st, ke);
    }
    while (st < nsteps) {
      __syncthreads();
      stage<AKC>(pa, As);
      stage<BKC>(pb, Bs);
      __syncthreads();
      st = next_live(rw.steps, st + 1, nsteps);
      if (st < nsteps) {
        fetch<AKC, G>(pa, g.A, g.lda, m0, g.M, kb + TK * st, ke);
        fetch<BKC, G>(pb, g.B, g.ldb, n0, g.N, kb + TK * st, ke);
      }
#pragma unroll
      for (int s = 0; s < TK / 32; ++s) {
        bf16x8 a[2], b[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          a[i] = *reinterpret_cast<const bf16x8*>(As + (wm + 16 * i + c16) * LP + 32 * s + 8 * q);
          b[i] = *reinterpret_cast<const bf16x8*>(Bs + (wn + 16 * i + c16) * LP + 32 * s + 8 * q);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
      }
    }
  }

  // The build's MFMA hazard check prices every low-precision matrix instruction as a 16-pass one (19 wait states before its result
  // is read); the compiler leaves what this shorter one needs.  Twenty wait states once per tile satisfy the stricter count.  The
  // accumulators are operands of the statement so that no read of them moves in front of it, and the kernel's launch bound (two
  // workgroups per SIMD: a budget of 256 registers) keeps them in VGPRs, so that no copy out of the accumulation file is one either.
  asm volatile("s_nop 15\n\ts_nop 3" : "+v"(acc[0][0]), "+v"(acc[0][1]), "+v"(acc[1][0]), "+v"(acc[1][1]));

  // lane l holds, of tile (i, j): row wm + 16 i + c16, columns wn + 16 j + 4 q .. + 3
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    int row = m0 + wm + 16 * i + c16;
    bool live = true;
    if constexpr (RB == 1) {   // block 2 (w & 1) + i of the tile; selects, not an indexed array
      row = ((w & 1) ? rw.base(2 + i) : rw.base(i)) + c16;
      live = 2 * (w & 1) + i < rw.live;
      if (!live && !(epilogue && g.rb_zero)) continue;   // a dead block of a workspace or of a slab: nobody reads it
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn + 16 * j + 4 * q;
      f32x4 v = acc[i][j];
      if constexpr (!G) {
        if (RB == 1 && !live) v = f32x4{0.f, 0.f, 0.f, 0.f};
        else if (epilogue) {
          if (g.bias) {
            const float4 bv = *reinterpret_cast<const float4*>(g.bias + col);
            v[0] += bv.x, v[1] += bv.y, v[2] += bv.z, v[3] += bv.w;
          }
          if (g.add) {
            const float4 av = *reinterpret_cast<const float4*>(g.add + (long)row * g.ldadd + col);
            v[0] += av.x, v[1] += av.y, v[2] += av.z, v[3] += av.w;
          }
        }
        *reinterpret_cast<float4*>(out + (long)row * ldo + col) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        if (row < g.M) {
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (col + r < g.N) {
              float x = v[r];
              if (epilogue) {
                if (g.bias) x += g.bias[col + r];
                if (g.add) x += g.add[(long)row * g.ldadd + col + r];
              }
              out[(long)row * ldo + col + r] = x;
            }
        }
      }
    }
  }
}

// RB: the row-block mode the launcher kept (0: none -- the kernel without a list).  Such a launch is interior in every tile.
template <bool AKC, bool BKC, int RB = 0>
__global__ __launch_bounds__(256, 2) void gemm_bf16_kernel(const Params p) {
  __shared__ __attribute__((aligned(16))) __bf16 As[TM * LP];
  __shared__ __attribute__((aligned(16))) __bf16 Bs[TM * LP];
  const GemmBf16Args& g = p.g;
  int b = blockIdx.x;
  const int tn = b % p.tiles_n;
  b /= p.tiles_n;
  const int tm = b % p.tiles_m, s = b / p.tiles_m;
  const int m0 = tm * TM, n0 = tn * TM;
  const int kb = s * p.kchunk, ke = min(g.K, kb + p.kchunk);
  const bool split = p.splits > 1;
  float* out = split ? g.ws + (long)s * g.M * g.N : g.C;
  const long ldo = split ? g.N : g.ldc;
  if constexpr (RB == 1) {
    // list entries 4 tm .. + 3, clamped to the problem's blocks (a list that is not this batch's must not reach outside the views)
    const int blocks = g.M / 16, nlive = min(max(*g.rb_n, 0), blocks);
    const auto rows_of = [&](const int j) { return 16 * min(max(g.rb[4 * tm + j], 0), blocks - 1); };
    Rows rw;
    rw.live = min(max(nlive - 4 * tm, 0), 4);
    rw.b0 = rows_of(0), rw.b1 = rows_of(1), rw.b2 = rows_of(2), rw.b3 = rows_of(3);
    // a tile past the live blocks runs no k-step: it stores zeros (rb_zero, unsplit) or nothing
    tile_body<AKC, BKC, false, 1>(g, As, Bs, m0, n0, kb, rw.live ? ke : kb, out, ldo, !split, rw);
    return;
  } else if constexpr (RB == 2) {
    // which k-steps of this run [kb, ke) hold a live block: every live block of the list sets the bit of its step
    __shared__ uint32_t steps[LIVE_WORDS];
    const int t = threadIdx.x, nsteps = (ke - kb) / TK, first = kb / TK;
    if (t < LIVE_WORDS) steps[t] = 0;
    __syncthreads();
    const int nlive = min(max(*g.rb_n, 0), g.K / 16);
    for (int i = t; i < nlive; i += 256) {
      const int st = (g.rb[i] >> 2) - first;
      if (st >= 0 && st < nsteps) atomicOr(&steps[st >> 5], 1u << (st & 31));
    }
    __syncthreads();
    Rows rw;
    rw.steps = steps;
    tile_body<AKC, BKC, false, 2>(g, As, Bs, m0, n0, kb, ke, out, ldo, !split, rw);
    return;
  }
  // uniform per workgroup.  A slab's rows are N floats apart: 16-byte aligned on an interior tile's problem only if N is a multiple of 4
  const bool interior = p.vec && m0 + TM <= g.M && n0 + TM <= g.N && (!split || (g.N & 3) == 0);
  if (interior) tile_body<AKC, BKC, false>(g, As, Bs, m0, n0, kb, ke, out, ldo, !split);
  else tile_body<AKC, BKC, true>(g, As, Bs, m0, n0, kb, ke, out, ldo, !split);
}

// C = the partial slabs in split order, then bias, then add: one thread per element.  RB1 (the launch kept a mode-1 list): element i
// is a VIRTUAL row's; a live row is summed and stored at its memory row, a dead one is stored as zero (rb_zero) or left alone, and its
// slab elements, which no tile wrote, are not read.
template <bool RB1 = false>
__global__ __launch_bounds__(256) void gemm_bf16_reduce_kernel(const GemmBf16Args g, const int splits) {
  const long mn = (long)g.M * g.N;
  long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= mn) return;
  int row = (int)(i / g.N);
  const int col = (int)(i % g.N);
  if constexpr (RB1) {
    const int blocks = g.M / 16, blk = row >> 4;
    row = 16 * min(max(g.rb[blk], 0), blocks - 1) + (row & 15);
    if (blk >= min(max(*g.rb_n, 0), blocks)) {
      if (g.rb_zero) g.C[(long)row * g.ldc + col] = 0.f;
      return;
    }
    i = (long)row * g.N + col;
  }
  float v = 0.f;
  for (int s = 0; s < splits; ++s) v += g.ws[(long)s * mn + i];
  if (g.bias) v += g.bias[col];
  if (g.add) v += g.add[(long)row * g.ldadd + col];
  g.C[(long)row * g.ldc + col] = v;
}

bool al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

}  // namespace

// Cut K while the tiles do not give every compute unit two workgroups and a run keeps at least four k-steps.
int gemm_bf16_splits(int M, int N, int K) {
  const long tiles = (long)cdiv(M, TM) * cdiv(N, TM);
  const int steps = cdiv(K, TK);
  int s = 1;
  while (s < MAX_SPLITS && tiles * s < 512 && steps / (2 * s) >= 4) s *= 2;
  return s;
}

namespace {
// the unguarded body's conditions on the whole problem but for the tile edges
bool vec_ok(const GemmBf16Args& g) {
  return al16(g.A) && al16(g.B) && al16(g.C) && al16(g.bias) && al16(g.add) && g.lda % 4 == 0 && g.ldb % 4 == 0 && g.ldc % 4 == 0 &&
         g.ldadd % 4 == 0 && g.K % TK == 0;
}
// the split factor the workspace allows, and the k of one run
int splits_taken(const GemmBf16Args& g) {
  int splits = gemm_bf16_splits(g.M, g.N, g.K);
  while (splits > 1 && (!g.ws || !al16(g.ws) || splits * (long)g.M * g.N > g.ws_elems)) splits /= 2;
  return splits;
}
int kchunk_of(const GemmBf16Args& g, int splits) { return cdiv(cdiv(g.K, TK), splits) * TK; }
}  // namespace

// gemm_bf16.hpp states the rule.  Nothing here depends on the list's contents: the grid and the cut are the dense launch's.
int gemm_bf16_keeps_rows(const GemmBf16Args& g) {
  if (!g.rb || !g.rb_n || (g.rb_mode != 1 && g.rb_mode != 2)) return 0;
  if (!vec_ok(g) || g.M % TM || g.N % TM) return 0;
  if (g.rb_mode == 1) return g.a_kc ? 1 : 0;
  if (g.a_kc || g.b_kc) return 0;
  return kchunk_of(g, splits_taken(g)) / TK <= 32 * LIVE_WORDS ? 2 : 0;
}

int gemm_bf16(const GemmBf16Args& g, hipStream_t st) {
  GC_REQUIRE(g.M >= 1 && g.N >= 1 && g.K >= 1, "gemm_bf16: M = %d, N = %d, K = %d (each at least 1)", g.M, g.N, g.K);
  GC_REQUIRE(g.A && g.B && g.C, "gemm_bf16: null operand");
  GC_REQUIRE(g.lda >= (g.a_kc ? g.K : g.M) && g.ldb >= (g.b_kc ? g.K : g.N) && g.ldc >= g.N && (!g.add || g.ldadd >= g.N),
             "gemm_bf16: a leading dimension is smaller than its row");
  GC_REQUIRE(g.a_kc || !g.b_kc, "gemm_bf16: the storage form A [K][M], B [N][K] is not served (NN, NT and TN are)");
  GC_REQUIRE(!g.rb || (g.rb_n && (g.rb_mode == 1 || g.rb_mode == 2)), "gemm_bf16: a row-block list needs its live count and rb_mode 1 or 2");
  Params p;
  p.g = g;
  const int rb = gemm_bf16_keeps_rows(g);
  if (!rb) p.g.rb = nullptr, p.g.rb_n = nullptr, p.g.rb_mode = 0, p.g.rb_zero = 0;
  p.tiles_m = cdiv(g.M, TM), p.tiles_n = cdiv(g.N, TM);
  const int splits = splits_taken(g);
  const long mn = (long)g.M * g.N;
  p.splits = splits;
  p.kchunk = kchunk_of(g, splits);
  p.vec = vec_ok(g);
  const long blocks = (long)p.tiles_m * p.tiles_n * splits;
  GC_REQUIRE(blocks < (1L << 31), "gemm_bf16: %ld workgroups", blocks);
  const double flops = 2.0 * g.M * g.N * g.K;
  const dim3 grid((unsigned)blocks), block(256);
  if (rb) {
    const auto kernel = rb == 2 ? gemm_bf16_kernel<false, false, 2> : g.b_kc ? gemm_bf16_kernel<true, true, 1> : gemm_bf16_kernel<true, false, 1>;
    GC_LAUNCH_TIMED("gemm_bf16_rb", flops, kernel, grid, block, 0, st, p);
  } else {
    const auto kernel = g.a_kc && g.b_kc ? gemm_bf16_kernel<true, true> : g.a_kc ? gemm_bf16_kernel<true, false> : gemm_bf16_kernel<false, false>;
    GC_LAUNCH_TIMED("gemm_bf16", flops, kernel, grid, block, 0, st, p);
  }
  GC_TRY(check_launch("gemm_bf16"));
  if (splits == 1) return 0;
  ProfScope ps("gemm_bf16_reduce", st);
  const auto reduce = rb == 1 ? gemm_bf16_reduce_kernel<true> : gemm_bf16_reduce_kernel<false>;
  hipLaunchKernelGGL(reduce, dim3(cdiv(mn, 256)), block, 0, st, p.g, splits);
  return check_launch("gemm_bf16_reduce");
}

}  // namespace gc
