// ddpx — fused flat-buffer AdamW (decoupled weight decay; no amsgrad, no maximize).
//
// The sibling of sgd_flat_kernel (optim_elementwise.hip) over the same flat store: one streaming pass reads
// p, exp_avg, exp_avg_sq and the gradient once and writes p, both states and the bf16 compute shadow once:
// 30 B per weight with fp32 gradients (16 read, 14 written), 28 B with bf16 ones.  torch.optim.AdamW's
// per-element sequence (torch/optim/adam.py `_single_tensor_adam`):
//   g  = g * gscale
//   m  = m + (g - m) * (1 - beta1)                    (lerp form)
//   v  = beta2 * v + (1 - beta2) * g * g
//   p  = p * (1 - lr * wd) - (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
// bc = {1 - beta1^t, sqrt(1 - beta2^t)} are two device scalars that adamw_advance_kernel produces once per
// optimizer step from a device step counter, so every per-bucket / per-shard launch of a step reads the same t
// and a replayed HIP graph needs no host write.  With parameter groups that differ (per-parameter lr multiplier and
// weight decay, ParamHyper) the same update runs chunk by chunk: adamw_flat_hyper_kernel.
//
// Roundings per element (the GPU test's tolerances count them; every product that feeds an add is an explicit
// fma, nothing is left to contraction):
//   m: g - m, fma                                           2   (+1: g * gscale)
//   v: g * g, * (1 - beta2), fma                            3   (+2: the scaled g enters squared)
//   p: 1 - lr*wd (fma), sqrt, / bc2s, + eps, lr / bc1, * m, / denom, fma(p, decay, -update)      8
// sqrtf and the divisions are the compiler's correctly rounded ones (no fast-math flag on this unit): the
// kernel is bandwidth-bound.
#include "ddpx_flat_optim.h"

#pragma clang fp contract(off)

namespace ddpx {

static inline int adamw_grid_for(int64_t n_vec, int block = 256, int max_blocks = 256 * 8) {
  int64_t b = (n_vec + block - 1) / block;
  if (b > max_blocks) b = max_blocks;
  if (b < 1) b = 1;
  return (int)b;
}

struct AdamwScalars {
  float decay;  // 1 - lr * wd
  float step;   // lr / bc1
  float bc2s;   // sqrt(1 - beta2^t)
  float w1;     // 1 - beta1
  float beta2;
  float w2;     // 1 - beta2
  float eps;
  float gscale;
};

__device__ __forceinline__ void adamw_apply(const AdamwScalars& c, float& p, float& m, float& v, float g) {
  adam_moments(c.w1, c.beta2, c.w2, c.gscale, m, v, g);
  const float denom = sqrtf(v) / c.bc2s + c.eps;
  const float upd = (c.step * m) / denom;
  p = fmaf(p, c.decay, -upd);
}

template <bool GBF16>
__global__ void __launch_bounds__(256)
adamw_flat_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, const void* __restrict__ g,
                  unsigned short* __restrict__ shadow, int64_t n, const float* __restrict__ lr_ptr, float lr_host,
                  const float* __restrict__ bc, float w1, float beta2, float w2, float eps, float wd,
                  float gscale_host, const float* __restrict__ gscale_ptr) {
  const float lr = lr_ptr ? *lr_ptr : lr_host;
  AdamwScalars c;
  c.decay = fmaf(-lr, wd, 1.f);
  c.step = lr / bc[0];
  c.bc2s = bc[1];
  c.w1 = w1;
  c.beta2 = beta2;
  c.w2 = w2;
  c.eps = eps;
  // gscale_ptr: a device factor on top of the host one (the gradient-clipping coefficient, grad_norm.hip);
  // a product of exactly 1.0 changes no bit of g
  c.gscale = gscale_ptr ? gscale_host * *gscale_ptr : gscale_host;
  const int64_t nv = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  // read-once / write-once streams (master, both states, gradient): non-temporal, as in sgd_flat_kernel; the
  // bf16 shadow is the next forward's operand and takes a plain store
  auto load_g = [&](int64_t i) -> f32x4 { return load_g4<GBF16>(g, 0, i); };
  auto update = [&](int64_t i, f32x4 pv, f32x4 mv, f32x4 vv, f32x4 gv) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float pq = pv[q], mq = mv[q], vq = vv[q];
      adamw_apply(c, pq, mq, vq, gv[q]);
      pv[q] = pq;
      mv[q] = mq;
      vv[q] = vq;
    }
    __builtin_nontemporal_store(mv, reinterpret_cast<f32x4*>(m) + i);
    __builtin_nontemporal_store(vv, reinterpret_cast<f32x4*>(v) + i);
    __builtin_nontemporal_store(pv, reinterpret_cast<f32x4*>(p) + i);
    if (shadow) {
      u32x2 sh = {pack_bf2(pv[0], pv[1]), pack_bf2(pv[2], pv[3])};
      reinterpret_cast<u32x2*>(shadow)[i] = sh;
    }
  };
  // two vectors per thread per iteration, all eight loads issued before either update
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += 2 * stride) {
    const int64_t j = i + stride;
    const bool two = j < nv;
    const f32x4 p0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + i);
    const f32x4 g0 = load_g(i);
    const f32x4 m0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(m) + i);
    const f32x4 v0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(v) + i);
    f32x4 p1 = p0, g1 = g0, m1 = m0, v1 = v0;
    if (two) {
      p1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + j);
      g1 = load_g(j);
      m1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(m) + j);
      v1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(v) + j);
    }
    update(i, p0, m0, v0, g0);
    if (two) update(j, p1, m1, v1, g1);
  }
  // scalar tail (n not a multiple of 4)
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t j = (nv << 2) + threadIdx.x;
    const float gv = GBF16 ? bf2f(reinterpret_cast<const unsigned short*>(g)[j])
                           : reinterpret_cast<const float*>(g)[j];
    float pq = p[j], mq = m[j], vq = v[j];
    adamw_apply(c, pq, mq, vq, gv);
    p[j] = pq;
    m[j] = mq;
    v[j] = vq;
    if (shadow) shadow[j] = f2bf(pq);
  }
}

static int g_hyper_split = 4;  // workgroups per chunk in adamw_flat_hyper_kernel (ddpx_adamw_set_split; benchmarks)

// adamw_flat_kernel's update over the chunks of a table (FlatChunk, each inside ONE parameter), with the
// parameter's row of the hyper table: lr = lr * lr_mul (one product), wd = its wd.  The streaming shape is
// sgd_flat_lars_kernel's (lars.hip): blockIdx.x: chunk; blockIdx.y: which of gridDim.y interleaved shares of the
// chunk's vectors; two vectors in flight per thread, non-temporal streams, plain store of the bf16 shadow, scalar
// tail on a parameter's last chunk.  The same adamw_apply under the same fp contract(off): element by element the
// bits of adamw_flat_kernel launched with that lr and wd.
template <bool GBF16>
__global__ void __launch_bounds__(256)
adamw_flat_hyper_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                        const void* __restrict__ g, unsigned short* __restrict__ shadow,
                        const FlatChunk* __restrict__ table, const ParamHyper* __restrict__ hyper,
                        const float* __restrict__ lr_ptr, float lr_host, const float* __restrict__ bc, float w1,
                        float beta2, float w2, float eps, float gscale_host, const float* __restrict__ gscale_ptr) {
  const FlatChunk ch = table[blockIdx.x];
  const ParamHyper h = hyper[ch.pid];  // uniform over the workgroup
  const float lr = (lr_ptr ? *lr_ptr : lr_host) * h.lr_mul;
  AdamwScalars c;
  c.decay = fmaf(-lr, h.wd, 1.f);
  c.step = lr / bc[0];
  c.bc2s = bc[1];
  c.w1 = w1;
  c.beta2 = beta2;
  c.w2 = w2;
  c.eps = eps;
  c.gscale = gscale_ptr ? gscale_host * *gscale_ptr : gscale_host;
  float* __restrict__ pc = p + ch.start;
  float* __restrict__ mc = m + ch.start;
  float* __restrict__ vc = v + ch.start;
  unsigned short* __restrict__ sc = shadow ? shadow + ch.start : nullptr;
  const int nv = ch.len >> 2;
  const int stride = gridDim.y * 256;
  auto update = [&](int i, f32x4 pv, f32x4 mv, f32x4 vv, f32x4 gv) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float pq = pv[q], mq = mv[q], vq = vv[q];
      adamw_apply(c, pq, mq, vq, gv[q]);
      pv[q] = pq;
      mv[q] = mq;
      vv[q] = vq;
    }
    __builtin_nontemporal_store(mv, reinterpret_cast<f32x4*>(mc) + i);
    __builtin_nontemporal_store(vv, reinterpret_cast<f32x4*>(vc) + i);
    __builtin_nontemporal_store(pv, reinterpret_cast<f32x4*>(pc) + i);
    if (sc) {
      u32x2 sh = {pack_bf2(pv[0], pv[1]), pack_bf2(pv[2], pv[3])};
      reinterpret_cast<u32x2*>(sc)[i] = sh;
    }
  };
  for (int i = blockIdx.y * 256 + threadIdx.x; i < nv; i += 2 * stride) {
    const int j = i + stride;
    const bool two = j < nv;
    const f32x4 p0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(pc) + i);
    const f32x4 g0 = load_g4<GBF16>(g, ch.start, i);
    const f32x4 m0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(mc) + i);
    const f32x4 v0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(vc) + i);
    f32x4 p1 = p0, g1 = g0, m1 = m0, v1 = v0;
    if (two) {
      p1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(pc) + j);
      g1 = load_g4<GBF16>(g, ch.start, j);
      m1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(mc) + j);
      v1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(vc) + j);
    }
    update(i, p0, m0, v0, g0);
    if (two) update(j, p1, m1, v1, g1);
  }
  // scalar tail (chunk length not a multiple of 4): only a parameter's last chunk has one
  if (blockIdx.y == 0 && (int)threadIdx.x < (ch.len & 3)) {
    const int j = (nv << 2) + threadIdx.x;
    const float gv = GBF16 ? bf2f(reinterpret_cast<const unsigned short*>(g)[ch.start + j])
                           : reinterpret_cast<const float*>(g)[ch.start + j];
    float pq = pc[j], mq = mc[j], vq = vc[j];
    adamw_apply(c, pq, mq, vq, gv);
    pc[j] = pq;
    mc[j] = mq;
    vc[j] = vq;
    if (sc) sc[j] = f2bf(pq);
  }
}

// Device step counter and bias corrections: t = ++counter, bc = {1 - beta1^t, sqrt(1 - beta2^t)} in fp64,
// each rounded once to fp32 — one thread, once per optimizer step before its first update launch, captured
// inside the training-step HIP graph (the twin of lr_advance_kernel).
__global__ void adamw_advance_kernel(int* __restrict__ counter, double beta1, double beta2,
                                     float* __restrict__ bc) {
  const int t = *counter + 1;
  *counter = t;
  bc[0] = (float)(1.0 - pow(beta1, (double)t));
  bc[1] = (float)sqrt(1.0 - pow(beta2, (double)t));
}

}  // namespace ddpx

using namespace ddpx;

// One AdamW step over n elements.  bc_dev: the two fp32 device scalars of ddpx_adamw_advance.  lr_dev (device
// scalar) wins over lr_host.  clip_dev: optional device factor on the gradient, on top of grad_scale.  The
// betas arrive as doubles so that 1 - beta is formed exactly before its one rounding to fp32.
DDPX_API int ddpx_adamw_flat(float* p, float* m, float* v, const void* g, int g_bf16, void* shadow, int64_t n,
                             const float* lr_dev, float lr_host, const float* bc_dev, double beta1, double beta2,
                             float eps, float weight_decay, float grad_scale, const float* clip_dev,
                             hipStream_t s) {
  if (n <= 0) return 0;
  if (!p || !m || !v || !g || !bc_dev) return -1;
  if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v)) & 15)
    return -1;
  if (reinterpret_cast<uintptr_t>(g) & (g_bf16 ? 7 : 15)) return -1;
  if (reinterpret_cast<uintptr_t>(shadow) & 7) return -1;
  if ((reinterpret_cast<uintptr_t>(bc_dev) | reinterpret_cast<uintptr_t>(lr_dev) |
       reinterpret_cast<uintptr_t>(clip_dev)) & 3)
    return -1;
  const int grid = adamw_grid_for((n >> 2) + 1);
  const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2);
  if (g_bf16)
    hipLaunchKernelGGL(adamw_flat_kernel<true>, dim3(grid), dim3(256), 0, s, p, m, v, g, (unsigned short*)shadow,
                       n, lr_dev, lr_host, bc_dev, w1, b2, w2, eps, weight_decay, grad_scale, clip_dev);
  else
    hipLaunchKernelGGL(adamw_flat_kernel<false>, dim3(grid), dim3(256), 0, s, p, m, v, g, (unsigned short*)shadow,
                       n, lr_dev, lr_host, bc_dev, w1, b2, w2, eps, weight_decay, grad_scale, clip_dev);
  return (int)hipGetLastError();
}

// Workgroups per chunk in ddpx_adamw_flat_hyper (1, 2, 4 or 8); returns the value in force.
DDPX_API int ddpx_adamw_set_split(int split) {
  if (split == 1 || split == 2 || split == 4 || split == 8) g_hyper_split = split;
  return g_hyper_split;
}

// One AdamW step over ``n_chunks`` chunks of ``table`` (FlatChunk[n_chunks], device) with a per-parameter hyper
// table: hyper is ParamHyper[P] (device, 8-B aligned); the chunk's parameter takes wd = hyper[pid].wd and
// lr = lr * hyper[pid].lr_mul.  p, m, v, g, shadow are the WHOLE store's buffers (chunk starts are flat indices;
// the caller guarantees that every chunk lies inside them); shadow may be null.  The rest as ddpx_adamw_flat.
DDPX_API int ddpx_adamw_flat_hyper(float* p, float* m, float* v, const void* g, int g_bf16, void* shadow,
                                   const void* table, int n_chunks, const void* hyper, const float* lr_dev,
                                   float lr_host, const float* bc_dev, double beta1, double beta2, float eps,
                                   float grad_scale, const float* clip_dev, hipStream_t s) {
  if (n_chunks <= 0) return 0;
  if (!p || !m || !v || !g || !table || !hyper || !bc_dev) return -1;
  if ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(m) | reinterpret_cast<uintptr_t>(v) |
       reinterpret_cast<uintptr_t>(table)) & 15)
    return -1;
  if (reinterpret_cast<uintptr_t>(g) & (g_bf16 ? 7 : 15)) return -1;
  if ((reinterpret_cast<uintptr_t>(shadow) | reinterpret_cast<uintptr_t>(hyper)) & 7) return -1;
  if ((reinterpret_cast<uintptr_t>(bc_dev) | reinterpret_cast<uintptr_t>(lr_dev) |
       reinterpret_cast<uintptr_t>(clip_dev)) & 3)
    return -1;
  const FlatChunk* t = reinterpret_cast<const FlatChunk*>(table);
  const ParamHyper* h = reinterpret_cast<const ParamHyper*>(hyper);
  const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2);
  const dim3 grid(n_chunks, g_hyper_split), block(256);
  if (g_bf16)
    hipLaunchKernelGGL(adamw_flat_hyper_kernel<true>, grid, block, 0, s, p, m, v, g, (unsigned short*)shadow, t, h,
                       lr_dev, lr_host, bc_dev, w1, b2, w2, eps, grad_scale, clip_dev);
  else
    hipLaunchKernelGGL(adamw_flat_hyper_kernel<false>, grid, block, 0, s, p, m, v, g, (unsigned short*)shadow, t, h,
                       lr_dev, lr_host, bc_dev, w1, b2, w2, eps, grad_scale, clip_dev);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_adamw_advance(int* counter, double beta1, double beta2, float* bc_out, hipStream_t s) {
  if (!counter || !bc_out) return -1;
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return -1;
  hipLaunchKernelGGL(adamw_advance_kernel, dim3(1), dim3(1), 0, s, counter, beta1, beta2, bc_out);
  return (int)hipGetLastError();
}
