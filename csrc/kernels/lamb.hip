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
//   lamb_apply_kernel    grid (n_chunks, split), stream2's chunk-driven form (ddpx_flat_optim.h): reads w, m, v,
//                        recomputes u with the moments kernel's own lamb_u(), w = fma(-(lr * t), u, w), stores w
//                        and the bf16 shadow.
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
    const float wj = wc[j];
    float me = mc[j], ve = vc[j];
    float ge = load_g1<GBF16>(g, c.start + j);
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

// w = fma(-(lr * trust[pid]), u, w) over the chunks of a table.  Non-temporal 16-B accesses; the bf16 shadow is the
// next forward's operand and takes a plain store.
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
  struct Vecs {
    f32x4 w, m, v;
  };
  auto step = [&](float wq, float mq, float vq) { return fmaf(nstep, lamb_u(k, wq, mq, vq), wq); };
  auto load = [&](int i) -> Vecs {
    return {__builtin_nontemporal_load(reinterpret_cast<const f32x4*>(wc) + i),
            __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(mc) + i),
            __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(vc) + i)};
  };
  auto update = [&](int i, const Vecs& x) {
    f32x4 wo;
#pragma unroll
    for (int e = 0; e < 4; ++e) wo[e] = step(x.w[e], x.m[e], x.v[e]);
    __builtin_nontemporal_store(wo, reinterpret_cast<f32x4*>(wc) + i);
    if (sc) store_bf4(sc, i, wo);
  };
  stream2<int>(blockIdx.y * 256 + threadIdx.x, gridDim.y * 256, nv, load, update);
  if (blockIdx.y == 0 && (int)threadIdx.x < (c.len & 3)) {  // scalar tail
    const int j = (nv << 2) + threadIdx.x;
    const float wo = step(wc[j], mc[j], vc[j]);
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

// The moments pass over ``n_chunks`` chunks of ``table`` (FlatChunk[n_chunks], device).  w, m, v, g are the
// WHOLE store's buffers (chunk starts are flat indices; the caller guarantees that every chunk lies inside
// them).  partials_out[2 * n_chunks]: sum w^2 and sum u^2 per chunk.  bc_dev: the two fp32 device scalars of
// ddpx_adamw_advance.  The betas arrive as doubles so that 1 - beta is formed exactly before its one rounding to
// fp32.  clip_dev: optional device factor on the gradient, on top of grad_scale.  hyper (may be null):
// ParamHyper[P] (device, 8-B aligned); the chunk's parameter forms u with wd = hyper[pid].wd and weight_decay is
// ignored.
DDPX_API int ddpx_lamb_moments(const float* w, float* m, float* v, const void* g, int g_bf16, const void* table,
                               int n_chunks, const void* hyper, float* partials_out, const float* bc_dev,
                               double beta1, double beta2, float eps, float weight_decay, float grad_scale,
                               const float* clip_dev, hipStream_t s) {
  if (n_chunks <= 0) return 0;
  if (!w || !m || !v || !g || !table || !partials_out || !bc_dev) return -1;
  if (ddpx::misaligned(15, w, m, v, table) || ddpx::misaligned(g_bf16 ? 7 : 15, g) || ddpx::misaligned(7, hyper) ||
      ddpx::misaligned(3, partials_out, bc_dev, clip_dev))
    return -1;
  const ddpx::FlatChunk* t = reinterpret_cast<const ddpx::FlatChunk*>(table);
  const ddpx::ParamHyper* h = reinterpret_cast<const ddpx::ParamHyper*>(hyper);
  const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2);
  ddpx::with_flags([&](auto gb, auto nt, auto hyp) {
    hipLaunchKernelGGL((lamb_moments_kernel<gb(), nt(), hyp()>), dim3(n_chunks), dim3(256), 0, s, w, m, v, g, t, h,
                       partials_out, bc_dev, w1, b2, w2, eps, hyp() ? 0.f : weight_decay, grad_scale, clip_dev);
  }, g_bf16 != 0, g_moments_nt != 0, hyper != nullptr);
  return (int)hipGetLastError();
}

// The apply pass over ``n_chunks`` chunks of ``table``: w and the bf16 shadow (may be null) from w, m, v and
// trust[pid].  lr_dev (device scalar) wins over lr_host.  hyper (may be null): the chunk's parameter recomputes u
// with wd = hyper[pid].wd (as its moments pass formed it; weight_decay is ignored) and steps with
// lr * hyper[pid].lr_mul.
DDPX_API int ddpx_lamb_apply(float* w, const float* m, const float* v, void* shadow, const void* table,
                             int n_chunks, const float* trust, const void* hyper, const float* lr_dev,
                             float lr_host, const float* bc_dev, float eps, float weight_decay, hipStream_t s) {
  if (n_chunks <= 0) return 0;
  if (!w || !m || !v || !table || !trust || !bc_dev) return -1;
  if (ddpx::misaligned(15, w, m, v, table) || ddpx::misaligned(7, shadow, hyper) ||
      ddpx::misaligned(3, trust, lr_dev, bc_dev))
    return -1;
  const ddpx::FlatChunk* t = reinterpret_cast<const ddpx::FlatChunk*>(table);
  const ddpx::ParamHyper* h = reinterpret_cast<const ddpx::ParamHyper*>(hyper);
  const dim3 grid(n_chunks, g_apply_split), block(256);
  ddpx::with_flags([&](auto hyp) {
    hipLaunchKernelGGL(lamb_apply_kernel<hyp()>, grid, block, 0, s, w, m, v, (unsigned short*)shadow, t, trust, h,
                       lr_dev, lr_host, bc_dev, eps, hyp() ? 0.f : weight_decay);
  }, hyper != nullptr);
  return (int)hipGetLastError();
}
