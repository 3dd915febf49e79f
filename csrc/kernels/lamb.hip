// ddpx — LAMB (You et al., 2020): Adam moments with a layer-wise trust ratio, over the flat store.
//
// Per element, with gscale the host gradient scale times the optional device clip factor and
// bc = {1 - beta1^t, sqrt(1 - beta2^t)} the two device scalars of ddpx_adamw_advance (adamw.hip):
//   g  = g * gscale
//   m  = m + (g - m) * (1 - beta1)
//   v  = beta2 * v + (1 - beta2) * g * g
//   r  = (m / bc1) / (sqrt(v) / bc2s + eps)
//   u  = r + wd * w
// and per parameter tensor i:  t_i = |w_i| / |u_i| (1 for the excluded and the zero- or NaN-norm ones),
//   w  = w - (lr * t_i) * u.
// The ratio needs the norm of the update itself, so the step is two streaming passes over LARS's chunk table
// (FlatChunk {start, len, pid}, ddpx_flat_optim.h: at most 32768 elements inside ONE parameter, starts 16-B aligned), with
// no buffer for u: the second pass recomputes it from the m and v the first one wrote.
//
//   lamb_moments_kernel  one 256-thread workgroup per chunk: reads w, g, m, v, writes m, v, forms u in registers
//                        and stores two fp32 partials per chunk (sum w^2, sum u^2).
//                        24 B per weight, 16 read and 8 written (22 B with bf16 gradients).
//   (totals, table)      ddpx_lars_segment_reduce on the partials, then ddpx_lars_trust with trust_coef = 1,
//                        weight_decay = 0, eps = 0, max_norm = 0: (1 * wn) / (fma(0, wn, un) + 0) = wn / un under
//                        LARS's adapt rule.  Both unchanged (lars.hip).
//   lamb_apply_kernel    grid (n_chunks, split): reads w, m, v, recomputes u with the moments kernel's own
//                        lamb_u(), w = fma(-(lr * t), u, w), stores w and the bf16 shadow.
//                        18 B per weight (12 read, 6 written).
// 42 B per weight in all (40 B with bf16 gradients).
//
// No float atomics: every value depends only on the tables and the inputs, never on the grid or on arrival
// order.  Summation shape of one partial: exactly lars_sumsq_kernel's — a thread owns 4 accumulators,
// accumulator k takes the 16-B vectors tid + (4 j + k) * 256 of the chunk with one fma per element, the scalar
// tail goes on accumulator 0, then (a0 + a1) + (a2 + a3), the 6-level wave butterfly and (w0 + w1) + (w2 + w3)
// through LDS.
//
// Roundings per element (the tests count them; every product that feeds an add is an explicit fma, nothing is
// left to contraction):
//   m, v: adam_moments (ddpx_flat_optim.h), as in adamw.hip: 2 and 3 (+1 and +2 with a gradient scale)
//   u: m / bc1, sqrt, / bc2s, + eps, the division, fma(wd, w, r)                                 6
//   w: lr * t, the fma                                                                           2
// sqrtf and the divisions are the compiler's correctly rounded ones (no fast-math flag on this unit).
//
// m and v written by the moments pass are read again by the apply pass: the moments pass stores them with plain
// stores (they may still sit in the L2 / Infinity Cache), the apply pass reads them non-temporally.
// ddpx_lamb_set_nt switches the moments stores to non-temporal ones for measurements.
#include "ddpx_flat_optim.h"

#pragma clang fp contract(off)

namespace ddpx {
namespace lamb {

static int g_apply_split = 4;  // workgroups per chunk in the apply pass (ddpx_lamb_set_split; benchmarks)
static int g_moments_nt = 0;   // non-temporal m / v stores in the moments pass (ddpx_lamb_set_nt; benchmarks)

struct LambScalars {
  float bc1;   // 1 - beta1^t
  float bc2s;  // sqrt(1 - beta2^t)
  float w1;    // 1 - beta1
  float beta2;
  float w2;    // 1 - beta2
  float eps;
  float wd;
  float gscale;
};

// the update direction of one element from the NEW moments and the OLD weight: both kernels call this
__device__ __forceinline__ float lamb_u(const LambScalars& c, float w, float m, float v) {
  const float r = (m / c.bc1) / (sqrtf(v) / c.bc2s + c.eps);
  return fmaf(c.wd, w, r);
}

// partials[2 b] = sum w^2, partials[2 b + 1] = sum u^2 over chunk b of the table; m and v of the chunk updated.
// HYP: wd is the chunk's parameter's row of the hyper table (one wave-uniform load per workgroup).
template <bool GBF16, bool NT, bool HYP>
__global__ void __launch_bounds__(256)
lamb_moments_kernel(const float* __restrict__ w, float* __restrict__ m, float* __restrict__ v,
                    const void* __restrict__ g, const FlatChunk* __restrict__ table,
                    const ParamHyper* __restrict__ hyper, float* __restrict__ partials,
                    const float* __restrict__ bc, float w1, float beta2, float w2, float eps, float wd,
                    float gscale_host, const float* __restrict__ gscale_ptr) {
  __shared__ float red[2][4];
  const FlatChunk c = table[blockIdx.x];
  const int tid = threadIdx.x;
  LambScalars k;
  k.bc1 = bc[0];
  k.bc2s = bc[1];
  k.w1 = w1;
  k.beta2 = beta2;
  k.w2 = w2;
  k.eps = eps;
  if constexpr (HYP) k.wd = hyper[c.pid].wd;  // uniform over the workgroup
  else k.wd = wd;
  // a product of exactly 1.0 changes no bit of g
  k.gscale = gscale_ptr ? gscale_host * *gscale_ptr : gscale_host;
  const float* __restrict__ wc = w + c.start;
  float* __restrict__ mc = m + c.start;
  float* __restrict__ vc = v + c.start;
  const int nv = c.len >> 2;
  float aw[4] = {0.f, 0.f, 0.f, 0.f}, au[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i0 = tid; i0 < nv; i0 += 4 * 256) {
    // the loads of all four vectors issued before the first use
    f32x4 wv[4], gv[4], mv[4], vv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + q * 256;
      if (i < nv) {
        wv[q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(wc) + i);
        gv[q] = load_g4<GBF16>(g, c.start, i);
        mv[q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(mc) + i);
        vv[q] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(vc) + i);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int i = i0 + q * 256;
      if (i < nv) {
        f32x4 mo, vo;
        float a = aw[q], b = au[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float me = mv[q][e], ve = vv[q][e];
          float ge = gv[q][e];
          adam_moments(k.w1, k.beta2, k.w2, k.gscale, me, ve, ge);
          const float u = lamb_u(k, wv[q][e], me, ve);
          a = fmaf(wv[q][e], wv[q][e], a);
          b = fmaf(u, u, b);
          mo[e] = me;
          vo[e] = ve;
        }
        aw[q] = a;
        au[q] = b;
        if constexpr (NT) {
          __builtin_nontemporal_store(mo, reinterpret_cast<f32x4*>(mc) + i);
          __builtin_nontemporal_store(vo, reinterpret_cast<f32x4*>(vc) + i);
        } else {
          reinterpret_cast<f32x4*>(mc)[i] = mo;
          reinterpret_cast<f32x4*>(vc)[i] = vo;
        }
      }
    }
  }
  if (tid < (c.len & 3)) {  // scalar tail: only a parameter's last chunk has one
    const int j = (nv << 2) + tid;
    const float gj = GBF16 ? bf2f(reinterpret_cast<const unsigned short*>(g)[c.start + j])
                           : reinterpret_cast<const float*>(g)[c.start + j];
    const float wj = wc[j];
    float me = mc[j], ve = vc[j];
    float ge = gj;
    adam_moments(k.w1, k.beta2, k.w2, k.gscale, me, ve, ge);
    const float u = lamb_u(k, wj, me, ve);
    aw[0] = fmaf(wj, wj, aw[0]);
    au[0] = fmaf(u, u, au[0]);
    mc[j] = me;
    vc[j] = ve;
  }
  // block_store_sums' reduction written out: through the helper this kernel's wide bf16 step measured 1 % slower
  // (profiles/r12_optim)
  const float tw = (aw[0] + aw[1]) + (aw[2] + aw[3]);
  const float tu = (au[0] + au[1]) + (au[2] + au[3]);
  const float sw = wave_sum(tw), su = wave_sum(tu);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = sw;
    red[1][tid >> 6] = su;
  }
  __syncthreads();
  if (tid < 2) partials[2 * (size_t)blockIdx.x + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// w = fma(-(lr * trust[pid]), u, w) over the chunks of a table.  blockIdx.x: chunk; blockIdx.y: which of
// gridDim.y interleaved shares of the chunk's vectors.  Non-temporal 16-B accesses, two vectors in flight per
// thread; the bf16 shadow is the next forward's operand and takes a plain store.
// HYP: the parameter's row of the hyper table gives wd (the moments pass's, so that u is the same) and scales lr
// (one more rounding: lr * lr_mul, then * t).
template <bool HYP>
__global__ void __launch_bounds__(256)
lamb_apply_kernel(float* __restrict__ w, const float* __restrict__ m, const float* __restrict__ v,
                  unsigned short* __restrict__ shadow, const FlatChunk* __restrict__ table,
                  const float* __restrict__ trust, const ParamHyper* __restrict__ hyper,
                  const float* __restrict__ lr_ptr, float lr_host, const float* __restrict__ bc, float eps,
                  float wd) {
  const FlatChunk c = table[blockIdx.x];
  const float t = trust[c.pid];  // uniform over the workgroup
  float lr = lr_ptr ? *lr_ptr : lr_host;
  if constexpr (HYP) {
    const ParamHyper h = hyper[c.pid];
    lr = lr * h.lr_mul;
    wd = h.wd;
  }
  const float nstep = -(lr * t);
  LambScalars k;
  k.bc1 = bc[0];
  k.bc2s = bc[1];
  k.w1 = k.beta2 = k.w2 = 0.f;
  k.gscale = 1.f;
  k.eps = eps;
  k.wd = wd;
  float* __restrict__ wc = w + c.start;
  const float* __restrict__ mc = m + c.start;
  const float* __restrict__ vc = v + c.start;
  unsigned short* __restrict__ sc = shadow ? shadow + c.start : nullptr;
  const int nv = c.len >> 2;
  const int stride = gridDim.y * 256;
  auto update = [&](int i, f32x4 wv, f32x4 mv, f32x4 vv) {
    f32x4 wo;
#pragma unroll
    for (int e = 0; e < 4; ++e) wo[e] = fmaf(nstep, lamb_u(k, wv[e], mv[e], vv[e]), wv[e]);
    __builtin_nontemporal_store(wo, reinterpret_cast<f32x4*>(wc) + i);
    if (sc) {
      u32x2 sh = {pack_bf2(wo[0], wo[1]), pack_bf2(wo[2], wo[3])};
      reinterpret_cast<u32x2*>(sc)[i] = sh;
    }
  };
  for (int i = blockIdx.y * 256 + threadIdx.x; i < nv; i += 2 * stride) {
    const int j = i + stride;
    const bool two = j < nv;
    const f32x4 w0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(wc) + i);
    const f32x4 m0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(mc) + i);
    const f32x4 v0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(vc) + i);
    f32x4 w1 = w0, m1 = m0, v1 = v0;
    if (two) {
      w1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(wc) + j);
      m1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(mc) + j);
      v1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(vc) + j);
    }
    update(i, w0, m0, v0);
    if (two) update(j, w1, m1, v1);
  }
  if (blockIdx.y == 0 && (int)threadIdx.x < (c.len & 3)) {  // scalar tail
    const int j = (nv << 2) + threadIdx.x;
    const float wj = wc[j];
    const float wo = fmaf(nstep, lamb_u(k, wj, mc[j], vc[j]), wj);
    wc[j] = wo;
    if (sc) sc[j] = f2bf(wo);
  }
}

}  // namespace lamb
}  // namespace ddpx

using namespace ddpx::lamb;

// Workgroups per chunk in ddpx_lamb_apply (1, 2, 4 or 8); returns the value in force.
DDPX_API int ddpx_lamb_set_split(int split) {
  if (split == 1 || split == 2 || split == 4 || split == 8) g_apply_split = split;
  return g_apply_split;
}

// 1: the moments pass stores m and v non-temporally; 0: plain stores; anything else: no change.  Returns the
// value in force.
DDPX_API int ddpx_lamb_set_nt(int nt) {
  if (nt == 0 || nt == 1) g_moments_nt = nt;
  return g_moments_nt;
}

// Both entry points of a pass share its checks and its launch; hyper == null: the launch's own weight_decay.
static int lamb_moments_launch(const float* w, float* m, float* v, const void* g, int g_bf16, const void* table,
                               int n_chunks, const void* hyper, bool with_hyper, float* partials_out,
                               const float* bc_dev, double beta1, double beta2, float eps, float weight_decay,
                               float grad_scale, const float* clip_dev, hipStream_t s) {
  if (n_chunks <= 0) return 0;
  if (!w || !m || !v || !g || !table || !partials_out || !bc_dev || (with_hyper && !hyper)) return -1;
  if ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
       reinterpret_cast<uintptr_t>(table)) & 15)
    return -1;
  if (reinterpret_cast<uintptr_t>(g) & (g_bf16 ? 7 : 15)) return -1;
  if (reinterpret_cast<uintptr_t>(hyper) & 7) return -1;
  if ((reinterpret_cast<uintptr_t>(partials_out) | reinterpret_cast<uintptr_t>(bc_dev) |
       reinterpret_cast<uintptr_t>(clip_dev)) & 3)
    return -1;
  const ddpx::FlatChunk* t = reinterpret_cast<const ddpx::FlatChunk*>(table);
  const ddpx::ParamHyper* h = reinterpret_cast<const ddpx::ParamHyper*>(hyper);
  const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2);
  const dim3 grid(n_chunks), block(256);
#define DDPX_LAMB_MOMENTS(GB, NT)                                                                                \
  do {                                                                                                           \
    if (with_hyper)                                                                                              \
      hipLaunchKernelGGL((lamb_moments_kernel<GB, NT, true>), grid, block, 0, s, w, m, v, g, t, h, partials_out, \
                         bc_dev, w1, b2, w2, eps, 0.f, grad_scale, clip_dev);                                    \
    else                                                                                                         \
      hipLaunchKernelGGL((lamb_moments_kernel<GB, NT, false>), grid, block, 0, s, w, m, v, g, t, h, partials_out, \
                         bc_dev, w1, b2, w2, eps, weight_decay, grad_scale, clip_dev);                           \
  } while (0)
  if (g_bf16) {
    if (g_moments_nt) DDPX_LAMB_MOMENTS(true, true); else DDPX_LAMB_MOMENTS(true, false);
  } else {
    if (g_moments_nt) DDPX_LAMB_MOMENTS(false, true); else DDPX_LAMB_MOMENTS(false, false);
  }
#undef DDPX_LAMB_MOMENTS
  return (int)hipGetLastError();
}

static int lamb_apply_launch(float* w, const float* m, const float* v, void* shadow, const void* table, int n_chunks,
                             const float* trust, const void* hyper, bool with_hyper, const float* lr_dev,
                             float lr_host, const float* bc_dev, float eps, float weight_decay, hipStream_t s) {
  if (n_chunks <= 0) return 0;
  if (!w || !m || !v || !table || !trust || !bc_dev || (with_hyper && !hyper)) return -1;
  if ((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
       reinterpret_cast<uintptr_t>(table)) & 15)
    return -1;
  if ((reinterpret_cast<uintptr_t>(shadow) | reinterpret_cast<uintptr_t>(hyper)) & 7) return -1;
  if ((reinterpret_cast<uintptr_t>(trust) | reinterpret_cast<uintptr_t>(lr_dev) |
       reinterpret_cast<uintptr_t>(bc_dev)) & 3)
    return -1;
  const ddpx::FlatChunk* t = reinterpret_cast<const ddpx::FlatChunk*>(table);
  const ddpx::ParamHyper* h = reinterpret_cast<const ddpx::ParamHyper*>(hyper);
  const dim3 grid(n_chunks, g_apply_split), block(256);
  if (with_hyper)
    hipLaunchKernelGGL(lamb_apply_kernel<true>, grid, block, 0, s, w, m, v, (unsigned short*)shadow, t, trust, h,
                       lr_dev, lr_host, bc_dev, eps, 0.f);
  else
    hipLaunchKernelGGL(lamb_apply_kernel<false>, grid, block, 0, s, w, m, v, (unsigned short*)shadow, t, trust, h,
                       lr_dev, lr_host, bc_dev, eps, weight_decay);
  return (int)hipGetLastError();
}

// The moments pass over ``n_chunks`` chunks of ``table`` (FlatChunk[n_chunks], device).  w, m, v, g are the
// WHOLE store's buffers (chunk starts are flat indices; the caller guarantees that every chunk lies inside
// them).  partials_out[2 * n_chunks]: sum w^2 and sum u^2 per chunk.  bc_dev: the two fp32 device scalars of
// ddpx_adamw_advance.  The betas arrive as doubles so that 1 - beta is formed exactly before its one rounding to
// fp32.  clip_dev: optional device factor on the gradient, on top of grad_scale.
DDPX_API int ddpx_lamb_moments(const float* w, float* m, float* v, const void* g, int g_bf16, const void* table,
                               int n_chunks, float* partials_out, const float* bc_dev, double beta1, double beta2,
                               float eps, float weight_decay, float grad_scale, const float* clip_dev,
                               hipStream_t s) {
  return lamb_moments_launch(w, m, v, g, g_bf16, table, n_chunks, nullptr, false, partials_out, bc_dev, beta1, beta2,
                             eps, weight_decay, grad_scale, clip_dev, s);
}

// ddpx_lamb_moments with a per-parameter weight decay: hyper is ParamHyper[P] (device, 8-B aligned), the chunk's
// parameter forms u with wd = hyper[pid].wd.
DDPX_API int ddpx_lamb_moments_hyper(const float* w, float* m, float* v, const void* g, int g_bf16,
                                     const void* table, int n_chunks, const void* hyper, float* partials_out,
                                     const float* bc_dev, double beta1, double beta2, float eps, float grad_scale,
                                     const float* clip_dev, hipStream_t s) {
  return lamb_moments_launch(w, m, v, g, g_bf16, table, n_chunks, hyper, true, partials_out, bc_dev, beta1, beta2,
                             eps, 0.f, grad_scale, clip_dev, s);
}

// The apply pass over ``n_chunks`` chunks of ``table``: w and the bf16 shadow (may be null) from w, m, v and
// trust[pid].  lr_dev (device scalar) wins over lr_host.
DDPX_API int ddpx_lamb_apply(float* w, const float* m, const float* v, void* shadow, const void* table,
                             int n_chunks, const float* trust, const float* lr_dev, float lr_host,
                             const float* bc_dev, float eps, float weight_decay, hipStream_t s) {
  return lamb_apply_launch(w, m, v, shadow, table, n_chunks, trust, nullptr, false, lr_dev, lr_host, bc_dev, eps,
                           weight_decay, s);
}

// ddpx_lamb_apply with the hyper table: the chunk's parameter recomputes u with wd = hyper[pid].wd (as its moments
// pass formed it) and steps with lr * hyper[pid].lr_mul.
DDPX_API int ddpx_lamb_apply_hyper(float* w, const float* m, const float* v, void* shadow, const void* table,
                                   int n_chunks, const float* trust, const void* hyper, const float* lr_dev,
                                   float lr_host, const float* bc_dev, float eps, hipStream_t s) {
  return lamb_apply_launch(w, m, v, shadow, table, n_chunks, trust, hyper, true, lr_dev, lr_host, bc_dev, eps, 0.f,
                           s);
}
