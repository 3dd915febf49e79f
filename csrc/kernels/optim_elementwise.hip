// ddpx — memory-bound kernels: fused flat-buffer SGD, casts, column sums.
//
// All parameters of a model live in ONE flat fp32 buffer (ddpx.optim.flat),
// with a parallel momentum buffer, a parallel gradient buffer (the DDP bucket
// storage) and a parallel bf16 "compute shadow" that the MFMA GEMMs read.
// One SGD launch therefore replaces torch's foreach SGD (4 multi-tensor
// passes over 26 tensors, /root/reference/singlegpu.py:136-141 →
// torch/optim/sgd.py `_multi_tensor_sgd`): every element is read once and
// p, momentum and the bf16 shadow are written once.  16-B vector accesses,
// grid-stride, sized for 256 CUs.
#include "ddpx_flat_optim.h"
#include "ddpx_mx.h"

namespace ddpx {

// torch.optim.SGD semantics (dampening=0), sgd_step (ddpx_flat_optim.h) without a trust ratio:
//   d = g*gscale + wd*p ; buf = first ? d : mom*buf + d ; d = nesterov ? d + mom*buf : buf
//   p -= lr * d
// The streaming loop is stream2's flat form.
template <bool GBF16>
__global__ void __launch_bounds__(256)
sgd_flat_kernel(float* __restrict__ p, float* __restrict__ buf, const void* __restrict__ g,
                unsigned short* __restrict__ shadow, int64_t n, const float* __restrict__ lr_ptr,
                float lr_host, float mom, float wd, float gscale_host, const float* __restrict__ gscale_ptr,
                int nesterov, int first, unsigned char* __restrict__ q8, unsigned char* __restrict__ s8) {
  SgdScalars c;
  c.lr = lr_ptr ? *lr_ptr : lr_host;
  c.mom = mom;
  c.wd = wd;
  // gscale_ptr: a device factor on top of the host one (the gradient-clipping coefficient, grad_norm.hip)
  c.gscale = gscale_ptr ? gscale_host * *gscale_ptr : gscale_host;
  c.t = 1.f;
  c.nesterov = nesterov;
  c.first = first;
  const int64_t nv = n >> 2;
  struct Vecs {
    f32x4 p, g, b;
  };
  // read-once / write-once streams (master, momentum, gradient): non-temporal, so the optimizer does
  // not leave hundreds of MB of dirty lines in L2 / MALL for the next forward's GEMMs to write back
  auto load = [&](int64_t i) -> Vecs {
    return {__builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p) + i), load_g4<GBF16>(g, 0, i),
            __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(buf) + i)};
  };
  auto update = [&](int64_t i, const Vecs& x) {
    f32x4 po, bo;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float bq = 0.f;
      po[q] = sgd_step<false>(c, x.p[q], x.g[q], x.b[q], bq);
      bo[q] = bq;
    }
    if (mom != 0.f) __builtin_nontemporal_store(bo, reinterpret_cast<f32x4*>(buf) + i);
    __builtin_nontemporal_store(po, reinterpret_cast<f32x4*>(p) + i);
    if (shadow) store_bf4(shadow, i, po);
    if (q8) {  // MX-FP8 copy: vectors 8k..8k+7 (8 neighbouring lanes, all active: n % 32 == 0) = block k
      unsigned e8;
      const unsigned q = mx::e4m3_group8(po, &e8);
      reinterpret_cast<unsigned*>(q8)[i] = q;
      if ((i & 7) == 0) s8[i >> 3] = (unsigned char)e8;
    }
  };
  stream2<int64_t>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, nv, load, update);
  // scalar tail (n not a multiple of 4)
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t j = (nv << 2) + threadIdx.x;
    float bo = 0.f;
    const float po = sgd_step<false>(c, p[j], load_g1<GBF16>(g, j), mom != 0.f && !first ? buf[j] : 0.f, bo);
    if (mom != 0.f) buf[j] = bo;
    p[j] = po;
    if (shadow) shadow[j] = f2bf(po);
  }
}

__global__ void cast_f32_bf16_kernel(const float* __restrict__ x, unsigned short* __restrict__ y,
                                     int64_t n) {
  const int64_t nv = n >> 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
    u32x2 s = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
    reinterpret_cast<u32x2*>(y)[i] = s;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t j = (nv << 2) + threadIdx.x;
    y[j] = f2bf(x[j]);
  }
}

// out[n] (=|+=) scale * sum_m X[m][n] for a bf16 [M][N] matrix (bias gradient).
// One workgroup per 128 columns; each lane owns two adjacent columns (4-B
// loads, 256 B per wave-row); the 4 waves split the rows and meet in LDS.
__global__ void __launch_bounds__(256)
colsum_bf16_kernel(const unsigned short* __restrict__ X, float* __restrict__ out, int M, int N,
                   int ldx, float scale, int accumulate) {
  __shared__ float red[4][128];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n = blockIdx.x * 128 + lane * 2;
  float s0 = 0.f, s1 = 0.f;
  if (n + 1 < N) {
    for (int m = w; m < M; m += 4) {
      const unsigned v = *reinterpret_cast<const unsigned*>(X + (size_t)m * ldx + n);
      s0 += __uint_as_float(v << 16);
      s1 += __uint_as_float(v & 0xffff0000u);
    }
  } else if (n < N) {
    for (int m = w; m < M; m += 4) s0 += bf2f(X[(size_t)m * ldx + n]);
  }
  red[w][lane * 2] = s0;
  red[w][lane * 2 + 1] = s1;
  __syncthreads();
  if (threadIdx.x < 128) {
    const int c = blockIdx.x * 128 + threadIdx.x;
    if (c < N) {
      float t = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
      t *= scale;
      out[c] = accumulate ? out[c] + t : t;
    }
  }
}

// Elementwise scale (used for gradient averaging when the collective sums).
__global__ void scale_f32_kernel(float* __restrict__ x, int64_t n, float s) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] *= s;
}

}  // namespace ddpx

using namespace ddpx;

static int sgd_flat_launch(float* p, float* buf, const void* g, int g_bf16, void* shadow, int64_t n,
                           const float* lr_dev, float lr_host, float momentum, float weight_decay,
                           float grad_scale, const float* grad_scale_dev, int nesterov, int first, void* q8,
                           void* s8, hipStream_t s) {
  if (n <= 0) return 0;
  if (q8 && (n % 32 || !s8 || misaligned(3, q8))) return -1;
  if (misaligned(15, p, buf) || misaligned(g_bf16 ? 7 : 15, g) || misaligned(7, shadow)) return -1;
  const int grid = flat_grid_for((n >> 2) + 1);
  with_flags([&](auto gb) {
    hipLaunchKernelGGL(sgd_flat_kernel<gb()>, dim3(grid), dim3(256), 0, s, p, buf, g, (unsigned short*)shadow, n,
                       lr_dev, lr_host, momentum, weight_decay, grad_scale, grad_scale_dev, nesterov, first,
                       (unsigned char*)q8, (unsigned char*)s8);
  }, g_bf16 != 0);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_sgd_flat(float* p, float* buf, const void* g, int g_bf16, void* shadow, int64_t n,
                           const float* lr_dev, float lr_host, float momentum, float weight_decay,
                           float grad_scale, int nesterov, int first, void* q8, void* s8, hipStream_t s) {
  return sgd_flat_launch(p, buf, g, g_bf16, shadow, n, lr_dev, lr_host, momentum, weight_decay, grad_scale,
                         nullptr, nesterov, first, q8, s8, s);
}

// ddpx_sgd_flat with the gradient also scaled by the device scalar *clip_dev (the clip factor of
// ddpx_clip_coef): a factor of exactly 1.0 gives ddpx_sgd_flat's bits.
DDPX_API int ddpx_sgd_flat_clip(float* p, float* buf, const void* g, int g_bf16, void* shadow, int64_t n,
                                const float* lr_dev, float lr_host, float momentum, float weight_decay,
                                float grad_scale, const float* clip_dev, int nesterov, int first, void* q8,
                                void* s8, hipStream_t s) {
  if (!clip_dev) return -1;
  return sgd_flat_launch(p, buf, g, g_bf16, shadow, n, lr_dev, lr_host, momentum, weight_decay, grad_scale,
                         clip_dev, nesterov, first, q8, s8, s);
}

DDPX_API int ddpx_cast_f32_bf16(const float* x, void* y, int64_t n, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(flat_grid_for((n >> 2) + 1)), dim3(256), 0, s, x,
                     (unsigned short*)y, n);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_colsum_bf16(const void* X, float* out, int M, int N, int ldx, float scale,
                              int accumulate, hipStream_t s) {
  if (M <= 0 || N <= 0) return 0;
  if ((ldx & 1) || (reinterpret_cast<uintptr_t>(X) & 3)) return -1;
  hipLaunchKernelGGL(colsum_bf16_kernel, dim3((N + 127) / 128), dim3(256), 0, s,
                     (const unsigned short*)X, out, M, N, ldx, scale, accumulate);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_scale_f32(float* x, int64_t n, float scale, hipStream_t s) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(scale_f32_kernel, dim3(flat_grid_for(n)), dim3(256), 0, s, x, n, scale);
  return (int)hipGetLastError();
}

// Mirror image of a batch (flip test-time augmentation): x [R][W][E bytes] -> out, W reversed, E even.  Every loader
// layout is one of these: NCHW / flat R = N*C*H, E = the element size; NHWC R = N*H, E = C * the element size (16 B for
// the padded nhwc8_bf16 / nhwc4_f32).  V = the bytes a thread moves with one access: 16 where the rows allow it (a
// 16-B pixel; 4 fp32 or 8 bf16 neighbouring pixels, reversed in registers), else one 16-bit unit at a time.
template <int E>
__global__ void __launch_bounds__(256) hflip16_kernel(const u32x4* __restrict__ x, int64_t R, int W,
                                                      u32x4* __restrict__ out) {
  constexpr int P = 16 / E;  // pixels per 16-B vector: 1 (E = 16), 4 (fp32), 8 (bf16)
  const int G = W / P;       // vectors per row
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= R * G) return;
  const int64_t r = t / G;
  const int g = (int)(t - r * G);
  const u32x4 v = x[r * G + (G - 1 - g)];
  u32x4 o;
  if (E == 16) o = v;
  else if (E == 4) o = (u32x4){v[3], v[2], v[1], v[0]};
  else o = (u32x4){(v[3] >> 16) | (v[3] << 16), (v[2] >> 16) | (v[2] << 16), (v[1] >> 16) | (v[1] << 16),
                   (v[0] >> 16) | (v[0] << 16)};
  out[t] = o;
}

__global__ void __launch_bounds__(256) hflip2_kernel(const unsigned short* __restrict__ x, int64_t R, int W, int U,
                                                     unsigned short* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;  // 16-bit unit k of pixel w of row r; U = E / 2
  if (t >= R * W * U) return;
  const int k = (int)(t % U);
  const int64_t p = t / U;
  const int w = (int)(p % W);
  out[t] = x[((p - w) + (W - 1 - w)) * U + k];
}

DDPX_API int ddpx_hflip(const void* x, int64_t R, int W, int E, void* out, hipStream_t s) {
  if (R < 0 || W < 1 || E < 2 || (E & 1) || x == out) return -1;
  if (R == 0) return 0;
  const bool al = !(((uintptr_t)x | (uintptr_t)out) & 15);
  int64_t n;
  if (al && E == 16) {
    n = R * W;
    if ((n + 255) / 256 > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(hflip16_kernel<16>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const u32x4*)x, R, W,
                       (u32x4*)out);
  } else if (al && E == 4 && W % 4 == 0) {
    n = R * (W / 4);
    if ((n + 255) / 256 > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(hflip16_kernel<4>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const u32x4*)x, R, W,
                       (u32x4*)out);
  } else if (al && E == 2 && W % 8 == 0) {
    n = R * (W / 8);
    if ((n + 255) / 256 > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(hflip16_kernel<2>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const u32x4*)x, R, W,
                       (u32x4*)out);
  } else {
    n = R * W * (E / 2);
    if ((n + 255) / 256 > 0x7fffffffLL) return -1;
    hipLaunchKernelGGL(hflip2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const unsigned short*)x, R,
                       W, E / 2, (unsigned short*)out);
  }
  return (int)hipGetLastError();
}

// Device-side LR schedule: lr = table[min(step, n-1)], step += 1 — one thread, captured inside the
// training-step HIP graph, so a replayed step needs no host write of the learning rate.
__global__ void lr_advance_kernel(const float* __restrict__ table, int n, int* __restrict__ counter,
                                  float* __restrict__ lr) {
  const int k = *counter;
  *lr = table[k < n ? k : n - 1];
  *counter = k + 1;
}

DDPX_API int ddpx_lr_advance(const float* table, int n, int* counter, float* lr, hipStream_t s) {
  if (n <= 0) return -1;
  hipLaunchKernelGGL(lr_advance_kernel, dim3(1), dim3(1), 0, s, table, n, counter, lr);
  return (int)hipGetLastError();
}

