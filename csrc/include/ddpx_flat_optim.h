// ddpx — helpers shared by the optimizers over the flat store (optim_elementwise.hip, grad_norm.hip, lars.hip,
// lamb.hip, adamw.hip, ema.hip): the chunk table's row, the sum of squares of a chunk in the one summation shape every
// partial has, the workgroup reduction, the gradient loaders, the streaming loop of every update kernel (stream2), the
// SGD element step and Adam's moment sequence; for the host side the capped grid, the alignment check and the
// runtime-flag dispatch.
//
// The .hip files that count roundings set `#pragma clang fp contract(off)` AFTER including this header, so code here
// is compiled under the default contraction mode: a function with a product that feeds an add carries the pragma
// itself (adam_moments) or spells every fma out (sgd_step); stream2 holds index arithmetic only.
//
// Summation shape of one partial (the tests derive their tolerances from it; documented in grad_norm.hip): a
// thread owns 4 accumulators, accumulator k takes the 16-B vectors tid + (4 j + k) * 256 of the chunk with one fma
// per element, + the scalar tail on accumulator 0; then (a0 + a1) + (a2 + a3), a 6-level butterfly over the wave
// and (w0 + w1) + (w2 + w3) through LDS.
#pragma once

#include <type_traits>
#include <utility>

#include "ddpx_common.h"

namespace ddpx {

// One row of a chunk table (ddpx.ops.clip.ChunkPlan): 16 bytes.
struct FlatChunk {
  int64_t start;  // first flat element (a multiple of 8: 16-B aligned for fp32 and bf16)
  int32_t len;    // 1 .. 32768 elements (grad_norm.hip kChunk), all inside one parameter
  int32_t pid;    // that parameter's index in the store (0 in a table that carries none)
};

// One row of a per-parameter hyper-parameter table (ddpx.optim.flat: parameter groups): 8 bytes, [P] rows in store
// order like LARS's trust and plain tables.  A chunk-driven update loads row table[blockIdx.x].pid once per
// workgroup (wave-uniform) and uses lr = (lr_ptr ? *lr_ptr : lr_host) * lr_mul (one fp32 product) and wd.
struct ParamHyper {
  float lr_mul;  // the group's base learning rate over group 0's, rounded once to fp32
  float wd;      // the group's weight decay
};

// Workgroups of 256 threads for a grid-stride kernel over n_vec 16-B vectors: one thread per vector, capped at 8 per
// CU of a 256-CU chip.
constexpr int kFlatBlock = 256;
constexpr int kFlatMaxBlocks = 256 * 8;

static inline int flat_grid_for(int64_t n_vec) {
  int64_t b = (n_vec + kFlatBlock - 1) / kFlatBlock;
  if (b > kFlatMaxBlocks) b = kFlatMaxBlocks;
  if (b < 1) b = 1;
  return (int)b;
}

// Whether any of the addresses has a bit of mask set (a null pointer has none).
template <typename... T>
static inline bool misaligned(uintptr_t mask, const T*... ptrs) {
  return ((reinterpret_cast<uintptr_t>(ptrs) | ... | uintptr_t(0)) & mask) != 0;
}

// f(std::bool_constant<flags>...): runtime flags (g_bf16, nt, hyper != null) as a kernel's template arguments.
template <bool... Known, typename F>
static inline void with_flags(F&& f) {
  f(std::bool_constant<Known>{}...);
}
template <bool... Known, typename F, typename... Rest>
static inline void with_flags(F&& f, bool flag, Rest... rest) {
  if (flag) with_flags<Known..., true>(std::forward<F>(f), rest...);
  else with_flags<Known..., false>(std::forward<F>(f), rest...);
}

// The streaming loop of the update kernels: a thread takes the 16-B vectors first, first + stride, ... below nv, two
// per iteration, with ALL loads of both vectors issued before either update (twice the bytes in flight per wave of
// the one-vector loop).  load(i) returns the kernel's operands of vector i (a small struct of f32x4); update(i, a)
// does the arithmetic and the stores.  Flat kernels: I = int64_t, first = blockIdx.x * blockDim.x + threadIdx.x,
// stride = gridDim.x * blockDim.x.  Chunk-driven kernels (blockIdx.x: chunk; blockIdx.y: which of gridDim.y
// interleaved shares of the chunk's vectors): I = int, first = blockIdx.y * 256 + threadIdx.x, stride = gridDim.y * 256.
template <typename I, typename Load, typename Update>
__device__ __forceinline__ void stream2(I first, I stride, I nv, Load load, Update update) {
  for (I i = first; i < nv; i += 2 * stride) {
    const I j = i + stride;
    const bool two = j < nv;
    const auto a = load(i);
    auto b = a;
    if (two) b = load(j);
    update(i, a);
    if (two) update(j, b);
  }
}

template <bool NT, typename V>
__device__ __forceinline__ V ld16(const V* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  return *p;
}

__device__ __forceinline__ float sq4(f32x4 v, float a) {
  a = fmaf(v[0], v[0], a);
  a = fmaf(v[1], v[1], a);
  a = fmaf(v[2], v[2], a);
  return fmaf(v[3], v[3], a);
}

__device__ __forceinline__ float sq8(u32x4 r, float a) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float lo = __uint_as_float(r[q] << 16), hi = __uint_as_float(r[q] & 0xffff0000u);
    a = fmaf(lo, lo, a);
    a = fmaf(hi, hi, a);
  }
  return a;
}

// Sum of squares of the len elements at x (fp32, or bf16 with BF16; 16-B aligned): this thread's share of a
// 256-thread workgroup's, folded over its 4 accumulators.  NT: non-temporal loads.
template <bool BF16, bool NT>
__device__ __forceinline__ float thread_sumsq(const void* __restrict__ x, int len, int tid) {
  using V = std::conditional_t<BF16, u32x4, f32x4>;
  constexpr int W = BF16 ? 8 : 4;  // elements per 16-B vector
  const int nv = len / W;
  const V* src = reinterpret_cast<const V*>(x);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  auto sq = [](V r, float a) {
    if constexpr (BF16) return sq8(r, a);
    else return sq4(r, a);
  };
  for (int v = tid; v < nv; v += 4 * 256) {
    // four independent 16-B loads issued before the first use (a zero vector adds +0 to its accumulator)
    const V z = {};
    const V r0 = ld16<NT>(src + v);
    const V r1 = v + 256 < nv ? ld16<NT>(src + v + 256) : z;
    const V r2 = v + 512 < nv ? ld16<NT>(src + v + 512) : z;
    const V r3 = v + 768 < nv ? ld16<NT>(src + v + 768) : z;
    a0 = sq(r0, a0);
    a1 = sq(r1, a1);
    a2 = sq(r2, a2);
    a3 = sq(r3, a3);
  }
  if (tid < len - nv * W) {  // scalar tail
    float t;
    if constexpr (BF16) t = bf2f(reinterpret_cast<const unsigned short*>(x)[nv * W + tid]);
    else t = reinterpret_cast<const float*>(x)[nv * W + tid];
    a0 = fmaf(t, t, a0);
  }
  return (a0 + a1) + (a2 + a3);
}

// out[n] = the sum of v[n] over a 256-thread workgroup, n < N: the wave butterfly, then (w0 + w1) + (w2 + w3)
// through red (LDS).  Plain stores by threads 0 .. N - 1.  (lamb_moments_kernel keeps the same sequence inline.)
template <int N>
__device__ __forceinline__ void block_store_sums(const float (&v)[N], float (&red)[N][4], int tid,
                                                 float* __restrict__ out) {
  float s[N];
#pragma unroll
  for (int n = 0; n < N; ++n) s[n] = wave_sum(v[n]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int n = 0; n < N; ++n) red[n][tid >> 6] = s[n];
  }
  __syncthreads();
  if (tid < N) out[tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// Four gradient elements as fp32: vector i (of 4 elements) of the gradient buffer g from flat element start on,
// fp32 or bf16 (GBF16), loaded non-temporally (a read-once stream).
template <bool GBF16, typename I>
__device__ __forceinline__ f32x4 load_g4(const void* __restrict__ g, int64_t start, I i) {
  f32x4 gv;
  if constexpr (GBF16) {
    const u32x2 raw =
        __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(reinterpret_cast<const unsigned short*>(g) + start) + i);
    gv[0] = __uint_as_float(raw[0] << 16);
    gv[1] = __uint_as_float(raw[0] & 0xffff0000u);
    gv[2] = __uint_as_float(raw[1] << 16);
    gv[3] = __uint_as_float(raw[1] & 0xffff0000u);
  } else {
    gv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(g) + start) + i);
  }
  return gv;
}

// Element j of the gradient buffer as fp32 (the scalar tails).
template <bool GBF16, typename I>
__device__ __forceinline__ float load_g1(const void* __restrict__ g, I j) {
  if constexpr (GBF16) return bf2f(reinterpret_cast<const unsigned short*>(g)[j]);
  else return reinterpret_cast<const float*>(g)[j];
}

// Vector i (of 4 elements) of the bf16 shadow from four fp32 values: a plain 8-B store (the shadow is the next
// forward's operand).
template <typename I>
__device__ __forceinline__ void store_bf4(unsigned short* __restrict__ shadow, I i, f32x4 v) {
  const u32x2 sh = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
  reinterpret_cast<u32x2*>(shadow)[i] = sh;
}

// One element of the flat SGD update (torch.optim.SGD, dampening 0):
//   d = wd * p + g * gscale  (TRUST: d = t * d);  buf = first ? d : mom * buf + d;  d = nesterov ? d + mom * buf : buf
//   p -= lr * d
// Returns the new p; bo takes the new momentum when mom != 0.  The fma sequence of sgd_apply() (the fused-backward
// epilogues): bitwise-identical updates; t == 1.0f changes no bit.
struct SgdScalars {
  float lr, mom, wd, gscale;
  float t;  // the parameter's trust ratio (TRUST only)
  int nesterov, first;
};

template <bool TRUST>
__device__ __forceinline__ float sgd_step(const SgdScalars& c, float pv, float gv, float b, float& bo) {
  float d = fmaf(c.wd, pv, gv * c.gscale);
  if constexpr (TRUST) d = c.t * d;
  if (c.mom != 0.f) {
    const float bb = c.first ? d : fmaf(c.mom, b, d);
    bo = bb;
    d = c.nesterov ? fmaf(c.mom, bb, d) : bb;
  }
  return fmaf(-c.lr, d, pv);
}

// Adam's moments of one element (torch's sequence), g scaled first and returned scaled:
//   m = m + (g - m) * w1,  v = beta2 * v + (g * g) * w2      with w1 = 1 - beta1, w2 = 1 - beta2
// 2 and 3 roundings (+1 and +2 with a gradient scale): no product may be contracted into the add it feeds.
__device__ __forceinline__ void adam_moments(float w1, float beta2, float w2, float gscale, float& m, float& v,
                                             float& g) {
#pragma clang fp contract(off)
  g = g * gscale;
  m = fmaf(g - m, w1, m);
  v = fmaf(beta2, v, (g * g) * w2);
}

}  // namespace ddpx
