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
// weight decay, ParamHyper) the same update runs chunk by chunk: adamw_flat_hyper_kernel.  Both kernels are
// stream2 (ddpx_flat_optim.h) over the same load, update and tail: its flat form and its chunk-driven form.
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

// gscale_ptr: a device factor on top of the host one (the gradient-clipping coefficient, grad_norm.hip); a product
// of exactly 1.0 changes no bit of g
__device__ __forceinline__ AdamwScalars adamw_scalars(float lr, float wd, const float* __restrict__ bc, float w1,
                                                      float beta2, float w2, float eps, float gscale_host,
                                                      const float* __restrict__ gscale_ptr) {
  AdamwScalars c;
  c.decay = fmaf(-lr, wd, 1.f);
  c.step = lr / bc[0];
  c.bc2s = bc[1];
  c.w1 = w1;
  c.beta2 = beta2;
  c.w2 = w2;
  c.eps = eps;
  c.gscale = gscale_ptr ? gscale_host * *gscale_ptr : gscale_host;
  return c;
}

__device__ __forceinline__ void adamw_apply(const AdamwScalars& c, float& p, float& m, float& v, float g) {
  adam_moments(c.w1, c.beta2, c.w2, c.gscale, m, v, g);
  const float denom = sqrtf(v) / c.bc2s + c.eps;
  const float upd = (c.step * m) / denom;
  p = fmaf(p, c.decay, -upd);
}

// The buffers of one launch from flat element start on (0 in the flat kernel, the chunk's start in the chunk-driven
// one), with stream2's load and update and the scalar tail.  Read-once / write-once streams (master, both states,
// gradient): non-temporal, as in sgd_flat_kernel; the bf16 shadow is the next forward's operand and takes a plain
// store.
template <bool GBF16>
struct AdamwStreams {
  float* __restrict__ p;
  float* __restrict__ m;
  float* __restrict__ v;
  const void* __restrict__ g;  // the whole buffer: indexed from start
  unsigned short* __restrict__ shadow;
  int64_t start;
  struct Vecs {
    f32x4 p, g, m, v;
  };

  __device__ __forceinline__ AdamwStreams(float* p_, float* m_, float* v_, const void* g_, unsigned short* shadow_,
                                          int64_t start_)
      : p(p_ + start_), m(m_ + start_), v(v_ + start_), g(g_), shadow(shadow_ ? shadow_ + start_ : nullptr),
        start(start_) {}

  template <typename I>
  __device__ __forceinline__ Vecs load(I i) const {
    return {__builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + i), load_g4<GBF16>(g, start, i),
            __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(m) + i),
            __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(v) + i)};
  }

  template <typename I>
  __device__ __forceinline__ void update(const AdamwScalars& c, I i, Vecs x) const {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float pq = x.p[q], mq = x.m[q], vq = x.v[q];
      adamw_apply(c, pq, mq, vq, x.g[q]);
      x.p[q] = pq;
      x.m[q] = mq;
      x.v[q] = vq;
    }
    __builtin_nontemporal_store(x.m, reinterpret_cast<f32x4*>(m) + i);
    __builtin_nontemporal_store(x.v, reinterpret_cast<f32x4*>(v) + i);
    __builtin_nontemporal_store(x.p, reinterpret_cast<f32x4*>(p) + i);
    if (shadow) store_bf4(shadow, i, x.p);
  }

  template <typename I>
  __device__ __forceinline__ void tail(const AdamwScalars& c, I j) const {
    float pq = p[j], mq = m[j], vq = v[j];
    adamw_apply(c, pq, mq, vq, load_g1<GBF16>(g, start + j));
    p[j] = pq;
    m[j] = mq;
    v[j] = vq;
    if (shadow) shadow[j] = f2bf(pq);
  }
};

template <bool GBF16>
__global__ void __launch_bounds__(256)
adamw_flat_kernel(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, const void* __restrict__ g,
                  unsigned short* __restrict__ shadow, int64_t n, const float* __restrict__ lr_ptr, float lr_host,
                  const float* __restrict__ bc, float w1, float beta2, float w2, float eps, float wd,
                  float gscale_host, const float* __restrict__ gscale_ptr) {
  const float lr = lr_ptr ? *lr_ptr : lr_host;
  const AdamwScalars c = adamw_scalars(lr, wd, bc, w1, beta2, w2, eps, gscale_host, gscale_ptr);
  const AdamwStreams<GBF16> st(p, m, v, g, shadow, 0);
  const int64_t nv = n >> 2;
  stream2<int64_t>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, nv,
                   [&](int64_t i) { return st.load(i); }, [&](int64_t i, const auto& x) { st.update(c, i, x); });
  // scalar tail (n not a multiple of 4)
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) st.tail(c, (nv << 2) + threadIdx.x);
}

static int g_hyper_split = 4;  // workgroups per chunk in adamw_flat_hyper_kernel (ddpx_adamw_set_split; benchmarks)

// adamw_flat_kernel's update over the chunks of a table (FlatChunk, each inside ONE parameter), with the
// parameter's row of the hyper table: lr = lr * lr_mul (one product), wd = its wd.  stream2's chunk-driven form;
// scalar tail on a parameter's last chunk.  The same adamw_apply under the same fp contract(off): element by
// element the bits of adamw_flat_kernel launched with that lr and wd.
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
  const AdamwScalars c = adamw_scalars(lr, h.wd, bc, w1, beta2, w2, eps, gscale_host, gscale_ptr);
  const AdamwStreams<GBF16> st(p, m, v, g, shadow, ch.start);
  const int nv = ch.len >> 2;
  stream2<int>(blockIdx.y * 256 + threadIdx.x, gridDim.y * 256, nv, [&](int i) { return st.load(i); },
               [&](int i, const auto& x) { st.update(c, i, x); });
  // scalar tail (chunk length not a multiple of 4): only a parameter's last chunk has one
  if (blockIdx.y == 0 && (int)threadIdx.x < (ch.len & 3)) st.tail(c, (nv << 2) + (int)threadIdx.x);
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
  if (misaligned(15, p, m, v) || misaligned(g_bf16 ? 7 : 15, g) || misaligned(7, shadow) ||
      misaligned(3, bc_dev, lr_dev, clip_dev))
    return -1;
  const int grid = flat_grid_for((n >> 2) + 1);
  const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2);
  with_flags([&](auto gb) {
    hipLaunchKernelGGL(adamw_flat_kernel<gb()>, dim3(grid), dim3(256), 0, s, p, m, v, g, (unsigned short*)shadow, n,
                       lr_dev, lr_host, bc_dev, w1, b2, w2, eps, weight_decay, grad_scale, clip_dev);
  }, g_bf16 != 0);
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
  if (misaligned(15, p, m, v, table) || misaligned(g_bf16 ? 7 : 15, g) || misaligned(7, shadow, hyper) ||
      misaligned(3, bc_dev, lr_dev, clip_dev))
    return -1;
  const FlatChunk* t = reinterpret_cast<const FlatChunk*>(table);
  const ParamHyper* h = reinterpret_cast<const ParamHyper*>(hyper);
  const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2);
  const dim3 grid(n_chunks, g_hyper_split), block(256);
  with_flags([&](auto gb) {
    hipLaunchKernelGGL(adamw_flat_hyper_kernel<gb()>, grid, block, 0, s, p, m, v, g, (unsigned short*)shadow, t, h,
                       lr_dev, lr_host, bc_dev, w1, b2, w2, eps, grad_scale, clip_dev);
  }, g_bf16 != 0);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_adamw_advance(int* counter, double beta1, double beta2, float* bc_out, hipStream_t s) {
  if (!counter || !bc_out) return -1;
  if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) return -1;
  hipLaunchKernelGGL(adamw_advance_kernel, dim3(1), dim3(1), 0, s, counter, beta1, beta2, bc_out);
  return (int)hipGetLastError();
}
