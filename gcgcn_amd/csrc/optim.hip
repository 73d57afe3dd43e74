// One-launch Adam over many tensors: the optimiser step of the reference's trainer (config/Config.py:300 `optim.Adam(...,
// lr)` and :372-373 `optimizer.step()`), torch.optim.Adam's arithmetic (no weight decay, no amsgrad):
//   m <- m + (1 - b1) (g - m);  v <- b2 v + (1 - b2) g g;  p <- p - (lr / (1 - b1^t)) m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// with t counted per tensor (a parameter without a gradient in some step is skipped by torch and keeps its own t).
// The model's parameters are a few dozen tensors (one flat tensor per block); launching torch's per-tensor kernels costs
// ~5 launches each.  Here a table in device memory lists {p, g, m, v, numel, first block}; one workgroup handles 1024
// consecutive elements of one tensor (16 bytes per lane where the four pointers allow it).
//
// gcgcn_adam_step_dev is the same update for a step that is captured in a hipGraph: nothing of it is decided on the host.  Each
// tensor's step counter is an fp32 device scalar that a one-workgroup tick launch advances, computing the tensor's two
// bias-correction factors from it and from a device-side learning rate; with max_norm > 0 a launch in front of it writes one
// partial of sum g^2 per workgroup (the update's own decomposition), the tick launch adds them in a fixed order (no float atomics:
// the norm is bit-reproducible) and the update multiplies every gradient element by min(1, max_norm / (norm + 1e-6)).  Three
// launches with clipping, two without; no workgroup waits for another.
#include "../../include/gcgcn.h"
#include "../../include/gcgcn_optim.h"
#include "common.hpp"

namespace gc {

struct AdamEntry {
  float* p;
  const float* g;
  float* m;
  float* v;
  long numel;
  long block_begin;   // first workgroup of this tensor; entries are sorted by it
  float step_size;    // lr / (1 - b1^t)
  float inv_bc2_sqrt; // 1 / sqrt(1 - b2^t)
};
static_assert(sizeof(AdamEntry) == 56, "table layout is shared with gcgcn_amd/optim.py (7 x 8 bytes)");

// The same row as gcgcn_adam_step_dev reads it: the last 8 bytes point at the tensor's own step counter (an fp32 device scalar,
// torch.optim.Adam(capturable=True)'s state["step"]) and the two factors come from a side array that the tick launch fills.
struct AdamEntryDev {
  float* p;
  const float* g;
  float* m;
  float* v;
  long numel;
  long block_begin;
  float* step;
};
static_assert(sizeof(AdamEntryDev) == sizeof(AdamEntry), "one table layout for both entry points");

__device__ __forceinline__ void adam1(float& p, const float g, float& m, float& v, const float b1c, const float b2, const float b2c,
                                      const float eps, const float ss, const float ib) {
  m = m + b1c * (g - m);                 // exp_avg.lerp_(grad, 1 - beta1)
  v = v * b2 + b2c * (g * g);            // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
  const float denom = sqrtf(v) * ib + eps;
  p = p - ss * (m / denom);              // param.addcdiv_(exp_avg, denom, value = -step_size)
}

// b1c = 1 - beta1 and b2c = 1 - beta2 arrive rounded from double, as torch passes them to lerp_ / addcmul_ (1.f - 0.999f is
// 4.7e-5 away from 0.001f).  DEV (gcgcn_adam_step_dev): the two factors of tensor i are fac[i], written by the tick launch, and
// every gradient element is multiplied by *coefp first (rounded to fp32 on its own, as clip_grad_norm_'s g.mul_(coef) leaves it;
// 1.0f when nothing is clipped, which changes no bit).
// The kernel is a template over the arguments that only gcgcn_adam_step_dev passes (an inlined common body would do, but
// the compiler lays the blocks of an inlined body out differently: this way gcgcn_adam_step's instantiation is, instruction for
// instruction, the kernel it was before there were two).
__device__ __forceinline__ void dev_factors(AdamEntry&, int, float&) {}
__device__ __forceinline__ void dev_factors(AdamEntry& e, int i, float& coef, const float2* __restrict__ fac, const float* __restrict__ coefp) {
  e.step_size = fac[i].x, e.inv_bc2_sqrt = fac[i].y, coef = *coefp;   // (the row's last 8 bytes held the counter's address)
}
template <bool DEV>
__device__ __forceinline__ float adam_grad(const float g, const float coef) {
  return DEV ? __fmul_rn(g, coef) : g;
}

template <class... Dev>
__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamEntry* __restrict__ tab, int n, float b1c, float b2, float b2c,
                                                         float eps, Dev... dev) {
  constexpr bool DEV = sizeof...(Dev) > 0;
  int lo = 0, hi = n - 1;                // last entry whose block_begin <= blockIdx.x
  const long blk = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].block_begin <= blk) lo = mid;
    else hi = mid - 1;
  }
  AdamEntry e = tab[lo];
  const long base = (blk - e.block_begin) * 1024 + threadIdx.x * 4;
  if (base >= e.numel) return;
  float coef = 1.f;
  dev_factors(e, lo, coef, dev...);
  const bool vec = base + 4 <= e.numel && ((((uintptr_t)e.p) | ((uintptr_t)e.g) | ((uintptr_t)e.m) | ((uintptr_t)e.v)) & 15) == 0;
  if (vec) {
    float4 p = *reinterpret_cast<const float4*>(e.p + base), m = *reinterpret_cast<const float4*>(e.m + base);
    float4 v = *reinterpret_cast<const float4*>(e.v + base);
    const float4 g = *reinterpret_cast<const float4*>(e.g + base);
    adam1(p.x, adam_grad<DEV>(g.x, coef), m.x, v.x, b1c, b2, b2c, eps, e.step_size, e.inv_bc2_sqrt);
    adam1(p.y, adam_grad<DEV>(g.y, coef), m.y, v.y, b1c, b2, b2c, eps, e.step_size, e.inv_bc2_sqrt);
    adam1(p.z, adam_grad<DEV>(g.z, coef), m.z, v.z, b1c, b2, b2c, eps, e.step_size, e.inv_bc2_sqrt);
    adam1(p.w, adam_grad<DEV>(g.w, coef), m.w, v.w, b1c, b2, b2c, eps, e.step_size, e.inv_bc2_sqrt);
    *reinterpret_cast<float4*>(e.p + base) = p;
    *reinterpret_cast<float4*>(e.m + base) = m;
    *reinterpret_cast<float4*>(e.v + base) = v;
  } else {
    for (long i = base; i < base + 4 && i < e.numel; ++i) {
      float p = e.p[i], m = e.m[i], v = e.v[i];
      adam1(p, adam_grad<DEV>(e.g[i], coef), m, v, b1c, b2, b2c, eps, e.step_size, e.inv_bc2_sqrt);
      e.p[i] = p, e.m[i] = m, e.v[i] = v;
    }
  }
}

// ---- gcgcn_adam_step_dev: the gradient norm and the per-tensor tick --------------------------------------------------------------
// Workspace: float2 fac[n_tensors] | pad to 16 | float coef (16 bytes) | float part[total_blocks].
__host__ __device__ inline long adam_ws_coef_off(long n) { return (n * 8 + 15) & ~15L; }

// The four wave totals of a 256-lane workgroup, combined as (w0 + w1) + (w2 + w3) in lane 0: with wave_sum's fixed DPP tree the
// whole sum has one association, whatever order the workgroups run in.
__device__ __forceinline__ float block_sum_256(float s, float* lds4) {
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = s;
  __syncthreads();
  return (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
}

// Sum of g^2 over the 1024 elements that adam_multi_kernel's workgroup blockIdx.x updates, to part[blockIdx.x] (every slot of
// part[0, gridDim.x) is written in every call: nothing to clear, no atomics).
__global__ __launch_bounds__(256) void adam_gradnorm_kernel(const AdamEntry* __restrict__ tab, int n, float* __restrict__ part) {
  __shared__ float lds4[4];
  int lo = 0, hi = n - 1;
  const long blk = blockIdx.x;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].block_begin <= blk) lo = mid;
    else hi = mid - 1;
  }
  const float* g = tab[lo].g;
  const long numel = tab[lo].numel, base = (blk - tab[lo].block_begin) * 1024 + threadIdx.x * 4;
  float s = 0.f;
  if (base + 4 <= numel && (((uintptr_t)g) & 15) == 0) {
    const float4 q = *reinterpret_cast<const float4*>(g + base);
    s = (q.x * q.x + q.y * q.y) + (q.z * q.z + q.w * q.w);
  } else {
    for (long i = base; i < base + 4 && i < numel; ++i) s += g[i] * g[i];
  }
  s = block_sum_256(s, lds4);            // every lane arrives: no early return above
  if (threadIdx.x == 0) part[blk] = s;
}

// ONE workgroup.  With clipping: lane t adds part[t], part[t + 256], ... in increasing index, the lanes combine in the fixed
// tree; total = sqrt(sum) goes to *grad_norm and coef = min(1, max_norm / (total + 1e-6)) (fp32 throughout, torch's
// clip_grad_norm_; written as a comparison so that a NaN norm stays NaN) to *coefp.  Then one lane per tensor: t = *step + 1
// is written back and the two bias-correction factors are computed in double, as the host path computes them, and rounded to fp32.
__global__ __launch_bounds__(256) void adam_tick_kernel(const AdamEntryDev* __restrict__ tab, int n, double b1, double b2,
                                                        const float* __restrict__ lr, float max_norm, const float* __restrict__ part,
                                                        long nparts, float2* __restrict__ fac, float* __restrict__ coefp,
                                                        float* __restrict__ grad_norm) {
  __shared__ float lds4[4];
  if (max_norm > 0.f) {                  // uniform over the workgroup
    float s = 0.f;
    for (long i = threadIdx.x; i < nparts; i += 256) s += part[i];
    s = block_sum_256(s, lds4);
    if (threadIdx.x == 0) {
      const float total = sqrtf(s), c = max_norm / (total + 1e-6f);
      if (grad_norm) *grad_norm = total;
      *coefp = c > 1.f ? 1.f : c;
    }
  } else if (threadIdx.x == 0) {
    *coefp = 1.f;
  }
  const double lrd = (double)*lr;
  for (int i = threadIdx.x; i < n; i += 256) {
    float* sp = tab[i].step;
    const float t = *sp + 1.f;
    *sp = t;
    const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
    fac[i] = make_float2((float)(lrd / bc1), (float)(1.0 / sqrt(bc2)));
  }
}

// ---- gcopt_adamw_step / gcopt_adamw_step_dev: weight decay (L2 or decoupled), amsgrad, maximize, no bias correction -------------
// Sibling kernels of the three above, which stay as they are.  ONE table spans every parameter group of the step: a row is the
// 56-byte row with amsgrad's running maximum and the index of the tensor's group added, and the hyper-parameters that were launch
// arguments above come from a small array of per-group records.  What a group asks for is uniform over a workgroup (a workgroup
// serves one tensor): the update kernel reads its group's record once, through uniform addresses (scalar loads), and picks one of
// six bodies, <decay mode, amsgrad>, before it touches an element; the plain body is adam1 over the same loads and stores.
struct AdamwEntry {
  float* p;
  const float* g;
  float* m;
  float* v;
  float* vmax;        // amsgrad's max_exp_avg_sq; null in a group without amsgrad
  long numel;
  long block_begin;
  float step_size;    // gcopt_adamw_step_dev: these 8 bytes are `float* step`, as in AdamEntryDev
  float inv_bc2_sqrt;
  int group;          // index into the group records
  int pad;
};
static_assert(sizeof(AdamwEntry) == 72, "table layout is shared with gcgcn_amd/optim.py (9 x 8 bytes)");
static_assert(offsetof(AdamwEntry, step_size) == 56 && offsetof(AdamwEntry, group) == 64, "table layout is shared with gcgcn_amd/optim.py");

struct AdamwGroup {
  double beta1, beta2, eps, weight_decay;
  double lr;          // gcopt_adamw_step_dev: these 8 bytes are `const float* lr`, the group's device-side learning rate
  unsigned flags;     // ADAMW_* below
  unsigned pad;
};
static_assert(sizeof(AdamwGroup) == 48, "group record layout is shared with gcgcn_amd/optim.py (6 x 8 bytes)");

enum : unsigned { ADAMW_L2 = 1, ADAMW_DECOUPLED = 2, ADAMW_AMSGRAD = 4, ADAMW_MAXIMIZE = 8, ADAMW_NO_BIAS_CORRECTION = 16 };

template <class T>
__device__ __forceinline__ T load_as(const void* at) {   // the 8 bytes that hold an address in the _dev form
  T t;
  __builtin_memcpy(&t, at, sizeof(T));
  return t;
}

template <class E>
__device__ __forceinline__ int entry_of_block(const E* __restrict__ tab, int n, long blk) {
  int lo = 0, hi = n - 1;                // last entry whose block_begin <= blk
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (tab[mid].block_begin <= blk) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// The per-workgroup constants of the update: the group's record as fp32, rounded from double as the host rounds the launch
// arguments of adam_multi_kernel, the tensor's two factors and the gradient's multiplier.
struct AdamwConst {
  float b1c, b2, b2c, eps, ss, ib;
  float wd;           // L2: g <- g + wd p
  float dmul;         // decoupled: p <- p * dmul, dmul = 1 - lr wd (rounded from double)
  float coef;         // DEV: the clipping coefficient
  unsigned sign;      // maximize: 0x80000000, xor-ed into the gradient's bits first (g <- -g, exact)
};

// DECAY: 0 none, 1 L2, 2 decoupled.  torch.optim.Adam's single-tensor path, op for op (_single_tensor_adam).
template <int DECAY, bool AMS, bool DEV>
__device__ __forceinline__ void adamw1(float& p, float g, float& m, float& v, float& vm, const AdamwConst& c) {
  g = __uint_as_float(__float_as_uint(g) ^ c.sign);
  if (DEV) g = __fmul_rn(g, c.coef);
  if (DECAY == 1) g = g + c.wd * p;      // grad.add(param, alpha = weight_decay)
  if (DECAY == 2) p = p * c.dmul;        // param.mul_(1 - lr * weight_decay)
  m = m + c.b1c * (g - m);
  v = v * c.b2 + c.b2c * (g * g);
  float d = v;
  if (AMS) {
    vm = (v > vm || v != v) ? v : vm;    // torch.maximum: a NaN on either side stays
    d = vm;
  }
  const float denom = sqrtf(d) * c.ib + c.eps;
  p = p - c.ss * (m / denom);
}

template <int DECAY, bool AMS, bool DEV>
__device__ __forceinline__ void adamw_body(const AdamwEntry& e, const long base, const AdamwConst& c) {
  uintptr_t al = ((uintptr_t)e.p) | ((uintptr_t)e.g) | ((uintptr_t)e.m) | ((uintptr_t)e.v);
  if (AMS) al |= (uintptr_t)e.vmax;
  if (base + 4 <= e.numel && (al & 15) == 0) {
    float4 p = *reinterpret_cast<const float4*>(e.p + base), m = *reinterpret_cast<const float4*>(e.m + base);
    float4 v = *reinterpret_cast<const float4*>(e.v + base), vm = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 g = *reinterpret_cast<const float4*>(e.g + base);
    if (AMS) vm = *reinterpret_cast<const float4*>(e.vmax + base);
    adamw1<DECAY, AMS, DEV>(p.x, g.x, m.x, v.x, vm.x, c);
    adamw1<DECAY, AMS, DEV>(p.y, g.y, m.y, v.y, vm.y, c);
    adamw1<DECAY, AMS, DEV>(p.z, g.z, m.z, v.z, vm.z, c);
    adamw1<DECAY, AMS, DEV>(p.w, g.w, m.w, v.w, vm.w, c);
    *reinterpret_cast<float4*>(e.p + base) = p;
    *reinterpret_cast<float4*>(e.m + base) = m;
    *reinterpret_cast<float4*>(e.v + base) = v;
    if (AMS) *reinterpret_cast<float4*>(e.vmax + base) = vm;
  } else {
    for (long i = base; i < base + 4 && i < e.numel; ++i) {
      float p = e.p[i], m = e.m[i], v = e.v[i], vm = AMS ? e.vmax[i] : 0.f;
      adamw1<DECAY, AMS, DEV>(p, e.g[i], m, v, vm, c);
      e.p[i] = p, e.m[i] = m, e.v[i] = v;
      if (AMS) e.vmax[i] = vm;
    }
  }
}

// DEV: fac[i] are tensor i's factors, gmul[group] the group's 1 - lr wd and *coefp the clipping coefficient, all written by the
// tick launch (the row's step_size / inv_bc2_sqrt bytes and the record's lr bytes hold addresses then and are not read here).
template <bool DEV>
__global__ __launch_bounds__(256) void adamw_multi_kernel(const AdamwEntry* __restrict__ tab, int n, const AdamwGroup* __restrict__ groups,
                                                          int n_groups, const float2* __restrict__ fac, const float* __restrict__ gmul,
                                                          const float* __restrict__ coefp) {
  const long blk = blockIdx.x;
  const int ti = entry_of_block(tab, n, blk);
  const AdamwEntry e = tab[ti];
  const long base = (blk - e.block_begin) * 1024 + threadIdx.x * 4;
  if (base >= e.numel || (unsigned)e.group >= (unsigned)n_groups) return;
  const AdamwGroup gr = groups[e.group];
  const unsigned fl = gr.flags;
  AdamwConst c;
  c.b1c = (float)(1.0 - gr.beta1), c.b2 = (float)gr.beta2, c.b2c = (float)(1.0 - gr.beta2), c.eps = (float)gr.eps;
  c.wd = (float)gr.weight_decay;
  c.sign = (fl & ADAMW_MAXIMIZE) ? 0x80000000u : 0u;
  if (DEV) {
    c.ss = fac[ti].x, c.ib = fac[ti].y, c.dmul = gmul[e.group], c.coef = *coefp;
  } else {
    c.ss = e.step_size, c.ib = e.inv_bc2_sqrt, c.dmul = (float)(1.0 - gr.lr * gr.weight_decay), c.coef = 1.f;
  }
  const bool ams = (fl & ADAMW_AMSGRAD) && e.vmax != nullptr;
  const int decay = (fl & ADAMW_DECOUPLED) ? 2 : (fl & ADAMW_L2) ? 1 : 0;
  if (!ams) {                            // uniform over the workgroup: one body runs
    if (decay == 0) adamw_body<0, false, DEV>(e, base, c);
    else if (decay == 1) adamw_body<1, false, DEV>(e, base, c);
    else adamw_body<2, false, DEV>(e, base, c);
  } else {
    if (decay == 0) adamw_body<0, true, DEV>(e, base, c);
    else if (decay == 1) adamw_body<1, true, DEV>(e, base, c);
    else adamw_body<2, true, DEV>(e, base, c);
  }
}

// Workspace of gcopt_adamw_step_dev: float2 fac[n_tensors] | pad to 16 | float coef (16 bytes) | float gmul[n_groups] | pad to 16 |
// float part[total_blocks].
__host__ __device__ inline long adamw_ws_part_off(long n, long n_groups) { return adam_ws_coef_off(n) + 16 + ((n_groups * 4 + 15) & ~15L); }

// adam_gradnorm_kernel over the 72-byte rows: the same partial per workgroup, of the WHOLE table (all groups).
__global__ __launch_bounds__(256) void adamw_gradnorm_kernel(const AdamwEntry* __restrict__ tab, int n, float* __restrict__ part) {
  __shared__ float lds4[4];
  const long blk = blockIdx.x;
  const int ti = entry_of_block(tab, n, blk);
  const float* g = tab[ti].g;
  const long numel = tab[ti].numel, base = (blk - tab[ti].block_begin) * 1024 + threadIdx.x * 4;
  float s = 0.f;
  if (base + 4 <= numel && (((uintptr_t)g) & 15) == 0) {
    const float4 q = *reinterpret_cast<const float4*>(g + base);
    s = (q.x * q.x + q.y * q.y) + (q.z * q.z + q.w * q.w);
  } else {
    for (long i = base; i < base + 4 && i < numel; ++i) s += g[i] * g[i];
  }
  s = block_sum_256(s, lds4);            // every lane arrives: no early return above
  if (threadIdx.x == 0) part[blk] = s;
}

// adam_tick_kernel for a table that spans groups: ONE norm and ONE coef for all of them, then one lane per group writes its
// 1 - lr wd and one lane per tensor advances the counter and computes the factors from ITS group's device lr (double, as above;
// without bias correction step_size = lr and inv_bc2_sqrt = 1, and the counter still ticks).
__global__ __launch_bounds__(256) void adamw_tick_kernel(const AdamwEntry* __restrict__ tab, int n, const AdamwGroup* __restrict__ groups,
                                                         int n_groups, float max_norm, const float* __restrict__ part, long nparts,
                                                         float2* __restrict__ fac, float* __restrict__ gmul, float* __restrict__ coefp,
                                                         float* __restrict__ grad_norm) {
  __shared__ float lds4[4];
  if (max_norm > 0.f) {                  // uniform over the workgroup
    float s = 0.f;
    for (long i = threadIdx.x; i < nparts; i += 256) s += part[i];
    s = block_sum_256(s, lds4);
    if (threadIdx.x == 0) {
      const float total = sqrtf(s), c = max_norm / (total + 1e-6f);
      if (grad_norm) *grad_norm = total;
      *coefp = c > 1.f ? 1.f : c;
    }
  } else if (threadIdx.x == 0) {
    *coefp = 1.f;
  }
  for (int i = threadIdx.x; i < n_groups; i += 256) {
    gmul[i] = (float)(1.0 - (double)*load_as<const float*>(&groups[i].lr) * groups[i].weight_decay);
  }
  for (int i = threadIdx.x; i < n; i += 256) {
    float* sp = load_as<float*>(&tab[i].step_size);
    const float t = *sp + 1.f;
    *sp = t;
    const int gi = tab[i].group;
    if ((unsigned)gi >= (unsigned)n_groups) continue;
    const AdamwGroup gr = groups[gi];
    const double lrd = (double)*load_as<const float*>(&groups[gi].lr);
    if (gr.flags & ADAMW_NO_BIAS_CORRECTION) {
      fac[i] = make_float2((float)lrd, 1.f);
    } else {
      const double bc1 = 1.0 - pow(gr.beta1, (double)t), bc2 = 1.0 - pow(gr.beta2, (double)t);
      fac[i] = make_float2((float)(lrd / bc1), (float)(1.0 / sqrt(bc2)));
    }
  }
}

}  // namespace gc

using namespace gc;

extern "C" int gcgcn_adam_step(int n_tensors, const void* table, int64_t total_blocks, double beta1, double beta2, double eps,
                               void* stream) {
  GC_REQUIRE(n_tensors >= 0 && total_blocks >= 0, "adam_step: bad arguments");
  if (n_tensors == 0 || total_blocks == 0) return 0;
  GC_REQUIRE(table, "adam_step: null table");
  GC_REQUIRE(total_blocks <= 0x7fffffffL, "adam_step: too many elements for one launch");
  ProfScope ps("adam_step", (hipStream_t)stream);
  hipLaunchKernelGGL(adam_multi_kernel<>, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream, (const AdamEntry*)table,
                     n_tensors, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps);
  return check_launch("adam_step");
}

extern "C" int64_t gcgcn_adam_ws_bytes(int n_tensors, int64_t total_blocks) {
  if (n_tensors < 0 || total_blocks < 0) return -1;
  return adam_ws_coef_off(n_tensors) + 16 + total_blocks * 4;
}

extern "C" int gcgcn_adam_step_dev(int n_tensors, const void* table, int64_t total_blocks, double beta1, double beta2, double eps,
                                   const float* lr, double max_norm, void* ws, int64_t ws_bytes, float* grad_norm, void* stream) {
  GC_REQUIRE(n_tensors >= 0 && total_blocks >= 0, "adam_step_dev: bad arguments");
  if (n_tensors == 0) return 0;
  GC_REQUIRE(table && lr && ws, "adam_step_dev: null table, lr or workspace");
  GC_REQUIRE(total_blocks <= 0x7fffffffL, "adam_step_dev: too many elements for one launch");
  GC_REQUIRE((((uintptr_t)ws) & 15) == 0 && ws_bytes >= gcgcn_adam_ws_bytes(n_tensors, total_blocks),
             "adam_step_dev: workspace of %lld bytes, 16-byte aligned, needed (gcgcn_adam_ws_bytes)",
             (long long)gcgcn_adam_ws_bytes(n_tensors, total_blocks));
  const bool clip = max_norm > 0.0;
  GC_REQUIRE(!clip || (float)max_norm > 0.f, "adam_step_dev: max_norm underflows fp32");
  hipStream_t st = (hipStream_t)stream;
  float2* fac = (float2*)ws;
  float* coefp = (float*)((char*)ws + adam_ws_coef_off(n_tensors));
  float* part = coefp + 4;
  ProfScope ps("adam_step_dev", st);
  if (clip && total_blocks > 0) {
    hipLaunchKernelGGL(adam_gradnorm_kernel, dim3((unsigned)total_blocks), dim3(256), 0, st, (const AdamEntry*)table, n_tensors, part);
    GC_TRY(check_launch("adam_step_dev (norm)"));
  }
  hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(256), 0, st, (const AdamEntryDev*)table, n_tensors, beta1, beta2, lr,
                     clip ? (float)max_norm : 0.f, (const float*)part, (long)total_blocks, fac, coefp, grad_norm);
  GC_TRY(check_launch("adam_step_dev (tick)"));
  if (total_blocks == 0) return 0;       // only empty tensors: their counters have ticked, nothing to update
  hipLaunchKernelGGL((adam_multi_kernel<const float2*, const float*>), dim3((unsigned)total_blocks), dim3(256), 0, st, (const AdamEntry*)table, n_tensors,
                     (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (const float2*)fac, (const float*)coefp);
  return check_launch("adam_step_dev");
}

// ---- the same step with weight decay / amsgrad / maximize, one table over all parameter groups ---------------------------------
extern "C" int gcopt_adamw_step(int n_tensors, const void* table, int n_groups, const void* groups, int64_t total_blocks, void* stream) {
  GC_REQUIRE(n_tensors >= 0 && n_groups >= 0 && total_blocks >= 0, "adamw_step: bad arguments");
  if (n_tensors == 0 || total_blocks == 0) return 0;
  GC_REQUIRE(table && groups && n_groups > 0, "adamw_step: null table or no group records");
  GC_REQUIRE(total_blocks <= 0x7fffffffL, "adamw_step: too many elements for one launch");
  GC_LAUNCH_TIMED("adamw_update", 0.0, adamw_multi_kernel<false>, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                  (const AdamwEntry*)table, n_tensors, (const AdamwGroup*)groups, n_groups, (const float2*)nullptr, (const float*)nullptr,
                  (const float*)nullptr);
  return check_launch("adamw_step");
}

extern "C" int64_t gcopt_adamw_ws_bytes(int n_tensors, int n_groups, int64_t total_blocks) {
  if (n_tensors < 0 || n_groups < 0 || total_blocks < 0) return -1;
  return adamw_ws_part_off(n_tensors, n_groups) + total_blocks * 4;
}

extern "C" int gcopt_adamw_step_dev(int n_tensors, const void* table, int n_groups, const void* groups, int64_t total_blocks,
                                    double max_norm, void* ws, int64_t ws_bytes, float* grad_norm, void* stream) {
  GC_REQUIRE(n_tensors >= 0 && n_groups >= 0 && total_blocks >= 0, "adamw_step_dev: bad arguments");
  if (n_tensors == 0) return 0;
  GC_REQUIRE(table && groups && n_groups > 0 && ws, "adamw_step_dev: null table, group records or workspace");
  GC_REQUIRE(total_blocks <= 0x7fffffffL, "adamw_step_dev: too many elements for one launch");
  GC_REQUIRE((((uintptr_t)ws) & 15) == 0 && ws_bytes >= gcopt_adamw_ws_bytes(n_tensors, n_groups, total_blocks),
             "adamw_step_dev: workspace of %lld bytes, 16-byte aligned, needed (gcopt_adamw_ws_bytes)",
             (long long)gcopt_adamw_ws_bytes(n_tensors, n_groups, total_blocks));
  const bool clip = max_norm > 0.0;
  GC_REQUIRE(!clip || (float)max_norm > 0.f, "adamw_step_dev: max_norm underflows fp32");
  hipStream_t st = (hipStream_t)stream;
  float2* fac = (float2*)ws;
  float* coefp = (float*)((char*)ws + adam_ws_coef_off(n_tensors));
  float* gmul = coefp + 4;
  float* part = (float*)((char*)ws + adamw_ws_part_off(n_tensors, n_groups));
  if (clip && total_blocks > 0) {
    GC_LAUNCH_TIMED("adamw_norm", 0.0, adamw_gradnorm_kernel, dim3((unsigned)total_blocks), dim3(256), 0, st, (const AdamwEntry*)table,
                    n_tensors, part);
    GC_TRY(check_launch("adamw_step_dev (norm)"));
  }
  GC_LAUNCH_TIMED("adamw_tick", 0.0, adamw_tick_kernel, dim3(1), dim3(256), 0, st, (const AdamwEntry*)table, n_tensors,
                  (const AdamwGroup*)groups, n_groups, clip ? (float)max_norm : 0.f, (const float*)part, (long)total_blocks, fac, gmul,
                  coefp, grad_norm);
  GC_TRY(check_launch("adamw_step_dev (tick)"));
  if (total_blocks == 0) return 0;       // only empty tensors: their counters have ticked, nothing to update
  GC_LAUNCH_TIMED("adamw_update", 0.0, adamw_multi_kernel<true>, dim3((unsigned)total_blocks), dim3(256), 0, st, (const AdamwEntry*)table,
                  n_tensors, (const AdamwGroup*)groups, n_groups, (const float2*)fac, (const float*)gmul, (const float*)coefp);
  return check_launch("adamw_step_dev");
}
