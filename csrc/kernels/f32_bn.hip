// ddpx — BatchNorm2d of the fp32 recipe (NHWC, fp32; the GEMM core is in f32_gemm.hip): training statistics as
// per-chunk (mean, M2) merged by Chan's formula (running stats: momentum, unbiased variance; num_batches_tracked
// on device), apply + ReLU + MaxPool2d(2) in one pass, and the backward with the pool routing (first maximum of
// each window, as torch) and the ReLU mask recomputed from the saved pre-BN activation.  Every merge over chunks
// runs in fp64 in a fixed order, as one kernel or split over chunk ranges — both from the same helpers below, so
// the two forms cannot drift apart.
#include <cstdlib>

#include "ddpx_common.h"
#include "ddpx_f32.h"

namespace ddpx {
namespace f32k {

// ------------------------------------------------------------------ BatchNorm (NHWC [P][C], fp32)
// Threads: channel c = tid % C, row group g = tid / C (G = blockDim / C groups).  blockDim = max(256, C).
__device__ __forceinline__ float block_group_sum(float v, float* red, int C, int G, int tid) {
  red[tid] = v;
  __syncthreads();
  float s = 0.f;
  if (tid < C)
    for (int g = 0; g < G; ++g) s += red[g * C + tid];
  __syncthreads();
  return s;  // valid on tid < C
}

// part[t][0][c] = mean of chunk t, part[t][1][c] = M2 of chunk t (two passes over the L2-resident chunk)
__global__ void __launch_bounds__(512) bn_stats_kernel(const float* __restrict__ y, int P, int C, int R,
                                                        float* __restrict__ part) {
  __shared__ float red[512];
  __shared__ float bc[512];
  const int tid = threadIdx.x, c = tid % C, G = blockDim.x / C, g = tid / C;
  const int r0 = blockIdx.x * R, r1 = min(P, r0 + R);
  float s = 0.f;
  for (int r = r0 + g; r < r1; r += G) s += y[(size_t)r * C + c];
  s = block_group_sum(s, red, C, G, tid);
  if (tid < C) bc[tid] = s / (float)(r1 - r0);
  __syncthreads();
  const float mu = bc[c];
  float q = 0.f;
  for (int r = r0 + g; r < r1; r += G) {
    const float d = y[(size_t)r * C + c] - mu;
    q = fmaf(d, d, q);
  }
  q = block_group_sum(q, red, C, G, tid);
  if (tid < C) {
    part[(size_t)blockIdx.x * 2 * C + c] = mu;
    part[(size_t)blockIdx.x * 2 * C + C + c] = q;
  }
}

// ---- the merges over the chunks: 1024 threads = 64 channels (cl) x 16 chunk groups (g); group g takes the chunks
// t0 + g, t0 + g + 16, ... below t1 in that order, then the 16 groups are added in group order.  All in fp64.

// sum of n_t * mean_t over group g's chunks (n_t = rows of chunk t): 8 chunks' loads in flight, summed in the same
// chunk order as one at a time
__device__ __forceinline__ double chunk_mean_sum(const float* __restrict__ part, int t0, int t1, int g, int R, int P,
                                                 int C, int c) {
  double sm = 0.0;
  int t = t0 + g;
  for (; t + 7 * 16 < t1; t += 8 * 16) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(t + 16 * u) * 2 * C + c];
#pragma unroll
    for (int u = 0; u < 8; ++u) sm += (double)min(R, P - (t + 16 * u) * R) * v[u];
  }
  for (; t < t1; t += 16) sm += (double)min(R, P - t * R) * part[(size_t)t * 2 * C + c];
  return sm;
}

// sum of M2_t + n_t * (mean_t - m)^2 over group g's chunks (Chan), m = the mean over all chunks
__device__ __forceinline__ double chunk_m2_sum(const float* __restrict__ part, int t0, int t1, int g, int R, int P,
                                               int C, int c, double m) {
  double m2 = 0.0;
  int t = t0 + g;
  for (; t + 7 * 16 < t1; t += 8 * 16) {
    float mv[8], qv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      mv[u] = part[(size_t)(t + 16 * u) * 2 * C + c];
      qv[u] = part[(size_t)(t + 16 * u) * 2 * C + C + c];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const double d = mv[u] - m;
      m2 += qv[u] + (double)min(R, P - (t + 16 * u) * R) * d * d;
    }
  }
  for (; t < t1; t += 16) {
    const double d = part[(size_t)t * 2 * C + c] - m;
    m2 += part[(size_t)t * 2 * C + C + c] + (double)min(R, P - t * R) * d * d;
  }
  return m2;
}

// (s1, s2) += the two columns of group g's chunks as they are (the backward's sums)
__device__ __forceinline__ void chunk_pair_sum(const float* __restrict__ part, int t0, int t1, int g, int C, int c,
                                               double& s1, double& s2) {
  int t = t0 + g;
  for (; t + 7 * 16 < t1; t += 8 * 16) {
    float v1[8], v2[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      v1[u] = part[(size_t)(t + 16 * u) * 2 * C + c];
      v2[u] = part[(size_t)(t + 16 * u) * 2 * C + C + c];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      s1 += v1[u];
      s2 += v2[u];
    }
  }
  for (; t < t1; t += 16) {
    s1 += part[(size_t)t * 2 * C + c];
    s2 += part[(size_t)t * 2 * C + C + c];
  }
}

// the 16 groups' sums of channel cl, added in group order (after the barrier that follows red[g][cl] = ...)
__device__ __forceinline__ double group_tree(const double (*red)[64], int cl) {
  double r = 0.0;
  for (int k = 0; k < 16; ++k) r += red[k][cl];
  return r;
}

// Forward outputs of channel c from the merged sums (m = mean, m2 = M2 over P rows; training), or from the running
// statistics (eval): the running-stat update with the unbiased variance, then a = gamma * rstd, b = beta, mean, rstd
__device__ __forceinline__ void bn_outputs(int training, double m, double m2, int P, int c,
                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                           float* __restrict__ rmean, float* __restrict__ rvar, float momentum,
                                           float eps, float* __restrict__ a, float* __restrict__ b,
                                           float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  float mu, var;
  if (training) {
    mu = (float)m;
    var = (float)(m2 / P);
    const float unb = P > 1 ? (float)(m2 / (P - 1)) : var;
    rmean[c] = (1.f - momentum) * rmean[c] + momentum * mu;
    rvar[c] = (1.f - momentum) * rvar[c] + momentum * unb;
  } else {
    mu = rmean[c];
    var = rvar[c];
  }
  const float rs = 1.f / sqrtf(var + eps);
  a[c] = gamma[c] * rs;
  b[c] = beta[c];
  mean_out[c] = mu;
  rstd_out[c] = rs;
}

// Backward outputs of channel c from s1 = sum gz, s2 = sum gz * xhat over P rows
__device__ __forceinline__ void bn_bwd_outputs(double s1, double s2, int P, int c, float* __restrict__ c1,
                                               float* __restrict__ c2, float* __restrict__ dgamma,
                                               float* __restrict__ dbeta, int accumulate) {
  c1[c] = (float)(s1 / P);
  c2[c] = (float)(s2 / P);
  if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)s2 : (float)s2;
  if (dbeta) dbeta[c] = accumulate ? dbeta[c] + (float)s1 : (float)s1;
}

// Chan merge of the chunk statistics + running-stat update + affine coefficients a = gamma*rstd, b = beta.
// The normalisation is applied as a*(y - mean) + beta, not a*y + (beta - a*mean): the folded form cancels
// two terms of size |mean|/std and loses that many bits per layer.  Eval: running statistics.
// 1024 threads = 64 channels x 16 chunk groups per workgroup; fp64 merge, fixed order (deterministic).
__global__ void __launch_bounds__(1024) bn_finalize_kernel(const float* __restrict__ part, int T, int R, int P, int C,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            float* __restrict__ rmean, float* __restrict__ rvar,
                                                            int64_t* __restrict__ nbt, float momentum, float eps,
                                                            int training, float* __restrict__ a,
                                                            float* __restrict__ b, float* __restrict__ mean_out,
                                                            float* __restrict__ rstd_out) {
  __shared__ double red[16][64];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  const bool ok = c < C;
  if (blockIdx.x == 0 && threadIdx.x == 0 && training && nbt) *nbt += 1;
  double m = 0.0, m2 = 0.0;
  if (training) {
    const double sm = ok ? chunk_mean_sum(part, 0, T, g, R, P, C, c) : 0.0;
    red[g][cl] = sm;
    __syncthreads();
    m = group_tree(red, cl) / P;
    __syncthreads();
    m2 = ok ? chunk_m2_sum(part, 0, T, g, R, P, C, c, m) : 0.0;
    red[g][cl] = m2;
    __syncthreads();
    m2 = group_tree(red, cl);
  }
  if (g != 0 || !ok) return;
  bn_outputs(training, m, m2, P, c, gamma, beta, rmean, rvar, momentum, eps, a, b, mean_out, rstd_out);
}

// The same merge split over chunk ranges, for few channels and many chunks (VGG conv0 / conv1: C = 64 / 128,
// T = 2048 / 4096, one or two workgroups of the kernel above: 78 / 52 us).  Three launches: (1) per split the
// fp64 sum of n * mean; (2) the mean from all splits' sums (split order), then per split the fp64 M2 sum;
// (3) the M2 of all splits (split order) and the outputs.  Deterministic; within a split the same 16-group
// interleave as bn_finalize_kernel.  The per-split partials live in a caller-allocated fp64 workspace
// ws[2][kFinSplitMax][C] (stream-ordered by the caller's allocator: two merges in flight on different streams
// cannot overwrite each other's partials).
constexpr int kFinSplitMax = 32, kFinSplitMaxC = 1024;

// sum_{k < S} v[k * C + c] in k order, 8 loads in flight (the fp64 adds stay in order: deterministic)
__device__ __forceinline__ double fin_split_sum(const double* v, int S, int C, int c) {
  double r = 0.0;
  int k = 0;
  for (; k + 8 <= S; k += 8) {
    double t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = v[(size_t)(k + u) * C + c];
#pragma unroll
    for (int u = 0; u < 8; ++u) r += t[u];
  }
  for (; k < S; ++k) r += v[(size_t)k * C + c];
  return r;
}

__global__ void __launch_bounds__(1024) bn_fin_sum_kernel(const float* __restrict__ part, int T, int Ts, int R,
                                                           int P, int C, double* __restrict__ fin_s1) {
  __shared__ double red[16][64];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl, sp = blockIdx.y;
  const int t0 = sp * Ts, t1 = min(T, t0 + Ts);
  red[g][cl] = c < C ? chunk_mean_sum(part, t0, t1, g, R, P, C, c) : 0.0;
  __syncthreads();
  if (g == 0 && c < C) fin_s1[(size_t)sp * C + c] = group_tree(red, cl);
}

__global__ void __launch_bounds__(1024) bn_fin_m2_kernel(const float* __restrict__ part, int T, int Ts, int S, int R,
                                                          int P, int C, const double* __restrict__ fin_s1,
                                                          double* __restrict__ fin_s2) {
  __shared__ double red[16][64];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl, sp = blockIdx.y;
  const int t0 = sp * Ts, t1 = min(T, t0 + Ts);
  double m2 = 0.0;
  if (c < C) {
    const double m = fin_split_sum(fin_s1, S, C, c) / P;
    m2 = chunk_m2_sum(part, t0, t1, g, R, P, C, c, m);
  }
  red[g][cl] = m2;
  __syncthreads();
  if (g == 0 && c < C) fin_s2[(size_t)sp * C + c] = group_tree(red, cl);
}

__global__ void __launch_bounds__(64) bn_fin_out_kernel(int S, int P, int C, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float* __restrict__ rmean,
                                                         float* __restrict__ rvar, int64_t* __restrict__ nbt,
                                                         float momentum, float eps, float* __restrict__ a,
                                                         float* __restrict__ b, float* __restrict__ mean_out,
                                                         float* __restrict__ rstd_out,
                                                         const double* __restrict__ fin_s1,
                                                         const double* __restrict__ fin_s2) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (blockIdx.x == 0 && threadIdx.x == 0 && nbt) *nbt += 1;
  if (c >= C) return;
  const double m = fin_split_sum(fin_s1, S, C, c) / P;
  const double m2 = fin_split_sum(fin_s2, S, C, c);
  bn_outputs(1, m, m2, P, c, gamma, beta, rmean, rvar, momentum, eps, a, b, mean_out, rstd_out);
}

// out = [maxpool2](relu(a*(y - mean) + b)), 4 channels per thread.  res (nullable, non-pooled only, [N][H][W][C]):
// out = res + relu(...), the skip connection of a residual block.
__global__ void __launch_bounds__(256) bn_apply_kernel(const float* __restrict__ y, const float* __restrict__ a,
                                                        const float* __restrict__ b, const float* __restrict__ mean,
                                                        const float* __restrict__ res, int N, int H, int W, int C,
                                                        int relu, int pool, float* __restrict__ out) {
  const int Ho = pool ? H / 2 : H, Wo = pool ? W / 2 : W, C4 = C / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)N * Ho * Wo * C4) return;
  const int c = (int)(i % C4) * 4;
  const long pix = i / C4;
  const int wo = (int)(pix % Wo), ho = (int)((pix / Wo) % Ho), n = (int)(pix / ((long)Wo * Ho));
  const f32x4 av = *reinterpret_cast<const f32x4*>(a + c), bv = *reinterpret_cast<const f32x4*>(b + c);
  const f32x4 mv = *reinterpret_cast<const f32x4*>(mean + c);
  f32x4 r;
  if (!pool) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(y + (size_t)pix * C + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float z = fmaf(av[e], v[e] - mv[e], bv[e]);
      r[e] = relu ? fmaxf(z, 0.f) : z;
    }
    if (res) r += *reinterpret_cast<const f32x4*>(res + (size_t)pix * C + c);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = -INFINITY;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy)
#pragma unroll
      for (int dx = 0; dx < 2; ++dx) {
        const size_t p = ((size_t)n * H + 2 * ho + dy) * W + 2 * wo + dx;
        const f32x4 v = *reinterpret_cast<const f32x4*>(y + p * C + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float z = fmaf(av[e], v[e] - mv[e], bv[e]);
          if (relu) z = fmaxf(z, 0.f);
          r[e] = fmaxf(r[e], z);
        }
      }
  }
  *reinterpret_cast<f32x4*>(out + (size_t)i * 4) = r;
}

// Gradient at pre-BN pixel (n,h,w,c) of the block output's gradient g: ReLU mask and the 2x2 max-pool routing
// (the FIRST maximum of the window in row-major order gets the gradient, as torch's max_pool2d backward).
// g2 (nullable, g's shape): a second gradient of the block's output (the skip connection of the residual block
// above); the gradient is g + g2, never stored.
__device__ __forceinline__ float grad_at(const float* __restrict__ g, const float* __restrict__ g2, size_t i) {
  return g2 ? g[i] + g2[i] : g[i];
}

__device__ __forceinline__ float routed_grad(const float* __restrict__ g, const float* __restrict__ g2,
                                             const float* __restrict__ y, float av,
                                             float bv, float mu, int n, int h, int w, int H, int W, int C, int c,
                                             int pool, float z) {
  if (!(z > 0.f)) return 0.f;  // ReLU(z) == 0: no gradient (torch threshold_backward)
  if (!pool) return grad_at(g, g2, (((size_t)n * H + h) * W + w) * C + c);
  const int h0 = h & ~1, w0 = w & ~1;
  int first = -1;
  float best = -INFINITY;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const size_t p = ((size_t)n * H + h0 + (q >> 1)) * W + w0 + (q & 1);
    const float zz = fmaxf(fmaf(av, y[p * C + c] - mu, bv), 0.f);
    if (zz > best) { best = zz; first = q; }
  }
  if (first != ((h - h0) << 1 | (w - w0))) return 0.f;
  return grad_at(g, g2, (((size_t)n * (H / 2) + (h >> 1)) * (W / 2) + (w >> 1)) * C + c);
}

// part[t][0][c] = sum gz, part[t][1][c] = sum gz * xhat over pixel chunk t
__global__ void __launch_bounds__(512) bn_bwd_sums_kernel(const float* __restrict__ g, const float* __restrict__ g2,
                                                           const float* __restrict__ y,
                                                           const float* __restrict__ a, const float* __restrict__ b,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, int N, int H, int W, int C,
                                                           int pool, int R, float* __restrict__ part) {
  __shared__ float red[512];
  const int tid = threadIdx.x, c = tid % C, G = blockDim.x / C, gi = tid / C;
  const int P = N * H * W;
  const int r0 = blockIdx.x * R, r1 = min(P, r0 + R);
  const float av = a[c], bv = b[c], mu = mean[c], rs = rstd[c];
  float s1 = 0.f, s2 = 0.f;
  for (int r = r0 + gi; r < r1; r += G) {
    const int w = r % W, h = (r / W) % H, n = r / (W * H);
    const float yv = y[(size_t)r * C + c];
    const float gz = routed_grad(g, g2, y, av, bv, mu, n, h, w, H, W, C, c, pool, fmaf(av, yv - mu, bv));
    s1 += gz;
    s2 = fmaf(gz, (yv - mu) * rs, s2);
  }
  s1 = block_group_sum(s1, red, C, G, tid);
  s2 = block_group_sum(s2, red, C, G, tid);
  if (tid < C) {
    part[(size_t)blockIdx.x * 2 * C + c] = s1;
    part[(size_t)blockIdx.x * 2 * C + C + c] = s2;
  }
}

// c1 = sum gz / P, c2 = sum gz*xhat / P;  dgamma (+)= sum gz*xhat, dbeta (+)= sum gz
// (64 channels x 16 chunk groups per workgroup, fp64, fixed order)
__global__ void __launch_bounds__(1024) bn_bwd_finalize_kernel(const float* __restrict__ part, int T, int P, int C,
                                                                float* __restrict__ c1, float* __restrict__ c2,
                                                                float* __restrict__ dgamma,
                                                                float* __restrict__ dbeta, int accumulate) {
  __shared__ double red[2][16][64];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl;
  double s1 = 0.0, s2 = 0.0;
  if (c < C) chunk_pair_sum(part, 0, T, g, C, c, s1, s2);
  red[0][g][cl] = s1;
  red[1][g][cl] = s2;
  __syncthreads();
  if (g != 0 || c >= C) return;
  bn_bwd_outputs(group_tree(red[0], cl), group_tree(red[1], cl), P, c, c1, c2, dgamma, dbeta, accumulate);
}

// The same sums split over chunk ranges for few channel groups and many chunks (BN0's 64 channels x 2048 chunks
// took 29 us in one workgroup): per split, the 16-group interleave and tree of bn_bwd_finalize_kernel into the
// split scratch; then the splits in order (bn_bwd_fin_out_kernel).  Deterministic.
__global__ void __launch_bounds__(1024) bn_bwd_fin_sum_kernel(const float* __restrict__ part, int T, int Ts, int C,
                                                               double* __restrict__ fin_s1,
                                                               double* __restrict__ fin_s2) {
  __shared__ double red[2][16][64];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + cl, sp = blockIdx.y;
  const int t0 = sp * Ts, t1 = min(T, t0 + Ts);
  double s1 = 0.0, s2 = 0.0;
  if (c < C) chunk_pair_sum(part, t0, t1, g, C, c, s1, s2);
  red[0][g][cl] = s1;
  red[1][g][cl] = s2;
  __syncthreads();
  if (g != 0 || c >= C) return;
  fin_s1[(size_t)sp * C + c] = group_tree(red[0], cl);
  fin_s2[(size_t)sp * C + c] = group_tree(red[1], cl);
}

__global__ void __launch_bounds__(64) bn_bwd_fin_out_kernel(int S, int P, int C, float* __restrict__ c1,
                                                             float* __restrict__ c2, float* __restrict__ dgamma,
                                                             float* __restrict__ dbeta, int accumulate,
                                                             const double* __restrict__ fin_s1,
                                                             const double* __restrict__ fin_s2) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= C) return;
  const double s1 = fin_split_sum(fin_s1, S, C, c), s2 = fin_split_sum(fin_s2, S, C, c);
  bn_bwd_outputs(s1, s2, P, c, c1, c2, dgamma, dbeta, accumulate);
}

// dy = a * (gz - c1 - xhat * c2)
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const float* __restrict__ g, const float* __restrict__ g2,
                                                            const float* __restrict__ y,
                                                            const float* __restrict__ a, const float* __restrict__ b,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ rstd,
                                                            const float* __restrict__ c1, const float* __restrict__ c2,
                                                            int N, int H, int W, int C, int pool,
                                                            float* __restrict__ dy) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)N * H * W * C) return;
  const int c = (int)(i % C);
  const long r = i / C;
  const int w = (int)(r % W), h = (int)((r / W) % H), n = (int)(r / ((long)W * H));
  const float av = a[c], bv = b[c], mu = mean[c], yv = y[i];
  const float gz = routed_grad(g, g2, y, av, bv, mu, n, h, w, H, W, C, c, pool, fmaf(av, yv - mu, bv));
  const float xh = (yv - mu) * rstd[c];
  dy[i] = av * (gz - c1[c] - xh * c2[c]);
}

// Vectorised BatchNorm(+ReLU+MaxPool) backward: a thread owns 4 channels of one "unit" — a 2x2 pool window (its 4
// pre-pool pixels and its pooled gradient are read once, 16-B accesses) or, without a pool, one pixel.  The
// per-element kernels above re-read the whole window for every pixel (4x the loads) and moved 4 B per access.
// Same routing (first maximum in row-major window order) and ReLU mask as routed_grad.
struct Win4 {
  f32x4 gz[4], xh[4];
};

__device__ __forceinline__ Win4 window_grads(const float* __restrict__ g, const float* __restrict__ g2,
                                             const float* __restrict__ y, f32x4 av,
                                             f32x4 bv, f32x4 mu, f32x4 rs, size_t pix0, int W, size_t gpix, int C,
                                             int c, int pool) {
  Win4 o;
  const int nq = pool ? 4 : 1;
  f32x4 yv[4], pre[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q < nq) {
      const size_t pp = pix0 + (size_t)(q >> 1) * W + (q & 1);
      yv[q] = *reinterpret_cast<const f32x4*>(y + pp * C + c);
    } else {
      yv[q] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  }
  f32x4 gv = *reinterpret_cast<const f32x4*>(g + gpix * C + c);
  if (g2) gv += *reinterpret_cast<const f32x4*>(g2 + gpix * C + c);
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      pre[q][e] = fmaf(av[e], yv[q][e] - mu[e], bv[e]);
      o.xh[q][e] = (yv[q][e] - mu[e]) * rs[e];
    }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    int first = 0;
    if (pool) {
      float best = -INFINITY;
      first = -1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float zz = fmaxf(pre[q][e], 0.f);
        if (zz > best) { best = zz; first = q; }
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) o.gz[q][e] = (q < nq && q == first && pre[q][e] > 0.f) ? gv[e] : 0.f;
  }
  return o;
}

// unit u of the tensor -> its first pre-pool pixel and its gradient pixel
__device__ __forceinline__ void unit_pixels(long u, int H, int W, int pool, size_t& pix0, size_t& gpix) {
  if (!pool) {
    pix0 = gpix = (size_t)u;
    return;
  }
  const int Wo = W / 2, Ho = H / 2;
  const int wo = (int)(u % Wo);
  const long r = u / Wo;
  const int ho = (int)(r % Ho);
  const long n = r / Ho;
  pix0 = ((size_t)n * H + 2 * ho) * W + 2 * wo;
  gpix = (size_t)u;
}

// part[t][0][c] = sum gz, part[t][1][c] = sum gz * xhat over the units of chunk t (R pre-pool pixels, a multiple
// of 2W when pooled: whole window rows).  256 threads = (C/4 channel quads) x G unit groups, fixed order.
__global__ void __launch_bounds__(256) bn_bwd_sums4_kernel(const float* __restrict__ g, const float* __restrict__ g2,
                                                            const float* __restrict__ y,
                                                            const float* __restrict__ a, const float* __restrict__ b,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, int N, int H, int W, int C,
                                                            int pool, int R, float* __restrict__ part,
                                                            float* __restrict__ dyw) {
  // dyw (bias + activation only: a = 1, mean = 0, rstd = 1, c1 = c2 = 0): dy = gz needs no sums, so this pass writes
  // it too and bn_bwd_apply4_kernel's second read of g and y goes away (DeepNN fp32's pooled blocks)
  __shared__ f32x4 red[2][256];
  const int tid = threadIdx.x, C4 = C / 4, cq = tid % C4, gi = tid / C4, G = 256 / C4;
  const int c = 4 * cq;
  const long P = (long)N * H * W;
  const long r0 = (long)blockIdx.x * R, r1 = min(P, r0 + (long)R);
  const long u0 = pool ? r0 / 4 : r0, u1 = pool ? r1 / 4 : r1;  // windows: 4 pixels each, chunks window-aligned
  const f32x4 av = *reinterpret_cast<const f32x4*>(a + c), bv = *reinterpret_cast<const f32x4*>(b + c);
  const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c), rs = *reinterpret_cast<const f32x4*>(rstd + c);
  f32x4 s1 = {0.f, 0.f, 0.f, 0.f}, s2 = {0.f, 0.f, 0.f, 0.f};
  for (long u = u0 + gi; u < u1; u += G) {
    size_t pix0, gpix;
    unit_pixels(u, H, W, pool, pix0, gpix);
    const Win4 w = window_grads(g, g2, y, av, bv, mu, rs, pix0, W, gpix, C, c, pool);
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s1[e] += w.gz[q][e];
        s2[e] = fmaf(w.gz[q][e], w.xh[q][e], s2[e]);
      }
    if (dyw) {
      const int nq = pool ? 4 : 1;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (q >= nq) break;
        const size_t pp = pix0 + (size_t)(q >> 1) * W + (q & 1);
        *reinterpret_cast<f32x4*>(dyw + pp * C + c) = (f32x4){w.gz[q][0], w.gz[q][1], w.gz[q][2], w.gz[q][3]};
      }
    }
  }
  red[0][tid] = s1;
  red[1][tid] = s2;
  __syncthreads();
  if (gi == 0) {
    f32x4 t1 = {0.f, 0.f, 0.f, 0.f}, t2 = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < G; ++k) {
      t1 += red[0][k * C4 + cq];
      t2 += red[1][k * C4 + cq];
    }
    *reinterpret_cast<f32x4*>(part + (size_t)blockIdx.x * 2 * C + c) = t1;
    *reinterpret_cast<f32x4*>(part + (size_t)blockIdx.x * 2 * C + C + c) = t2;
  }
}

// dy = a * (gz - c1 - xhat * c2) for every pixel of one unit (window or pixel), 4 channels, 16-B stores.
__global__ void __launch_bounds__(256) bn_bwd_apply4_kernel(const float* __restrict__ g, const float* __restrict__ g2,
                                                             const float* __restrict__ y,
                                                             const float* __restrict__ a, const float* __restrict__ b,
                                                             const float* __restrict__ mean,
                                                             const float* __restrict__ rstd,
                                                             const float* __restrict__ c1, const float* __restrict__ c2,
                                                             int N, int H, int W, int C, int pool,
                                                             float* __restrict__ dy) {
  const int C4 = C / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  const long units = pool ? (long)N * (H / 2) * (W / 2) : (long)N * H * W;
  if (i >= units * C4) return;
  const int c = (int)(i % C4) * 4;
  const long u = i / C4;
  size_t pix0, gpix;
  unit_pixels(u, H, W, pool, pix0, gpix);
  const f32x4 av = *reinterpret_cast<const f32x4*>(a + c), bv = *reinterpret_cast<const f32x4*>(b + c);
  const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c), rs = *reinterpret_cast<const f32x4*>(rstd + c);
  const f32x4 k1 = *reinterpret_cast<const f32x4*>(c1 + c), k2 = *reinterpret_cast<const f32x4*>(c2 + c);
  const Win4 w = window_grads(g, g2, y, av, bv, mu, rs, pix0, W, gpix, C, c, pool);
  const int nq = pool ? 4 : 1;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q >= nq) break;
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = av[e] * (w.gz[q][e] - k1[e] - w.xh[q][e] * k2[e]);
    const size_t pp = pix0 + (size_t)(q >> 1) * W + (q & 1);
    *reinterpret_cast<f32x4*>(dy + pp * C + c) = o;
  }
}

}  // namespace f32k
}  // namespace ddpx

using namespace ddpx;
using namespace ddpx::f32k;

static int bn_threads(int C) { return C >= 256 ? C : 256; }

// How a merge over T chunks of C channels splits over chunk ranges: Sr splits of Ts chunks each, their partial sums
// in the two halves of the caller's workspace ws[2][kFinSplitMax][C].  Sr = 0: no split, the one-kernel merge —
// without a workspace, in eval, and unless the channel groups are few and the chunks many (DDPX_F32_BN_SPLIT=0
// keeps the one-kernel merge everywhere).
struct FinSplit {
  int Sr = 0, Ts = 0;
  double *s1 = nullptr, *s2 = nullptr;
};

static FinSplit fin_split_plan(int T, int C, double* ws, int training) {
  static const bool split_ok = [] {
    const char* e = getenv("DDPX_F32_BN_SPLIT");
    return !(e && e[0] == '0');
  }();
  FinSplit sp;
  if (!(split_ok && ws && training && C <= kFinSplitMaxC && T >= 1024 && nblk(C, 64) < 8)) return sp;
  const int S = min(kFinSplitMax, (T + 127) / 128);
  sp.Ts = (T + S - 1) / S;
  sp.Sr = (T + sp.Ts - 1) / sp.Ts;  // splits with a chunk range
  sp.s1 = ws;
  sp.s2 = ws + (size_t)kFinSplitMax * C;
  return sp;
}

DDPX_API int ddpx_f32_bn_stats(const float* y, int P, int C, int R, float* part, hipStream_t s) {
  if (C > 512 || (256 % C && C % 256)) return -1;
  hipLaunchKernelGGL(bn_stats_kernel, dim3(nblk(P, R)), dim3(bn_threads(C)), 0, s, y, P, C, R, part);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_f32_bn_finalize(const float* part, int T, int R, int P, int C, const float* gamma, const float* beta,
                                  float* rmean, float* rvar, int64_t* nbt, float momentum, float eps, int training,
                                  float* a, float* b, float* mean, float* rstd, double* ws, hipStream_t s) {
  const FinSplit sp = fin_split_plan(T, C, ws, training);
  if (sp.Sr) {
    const dim3 grid(nblk(C, 64), sp.Sr);
    hipLaunchKernelGGL(bn_fin_sum_kernel, grid, dim3(1024), 0, s, part, T, sp.Ts, R, P, C, sp.s1);
    hipLaunchKernelGGL(bn_fin_m2_kernel, grid, dim3(1024), 0, s, part, T, sp.Ts, sp.Sr, R, P, C, sp.s1, sp.s2);
    hipLaunchKernelGGL(bn_fin_out_kernel, dim3(nblk(C, 64)), dim3(64), 0, s, sp.Sr, P, C, gamma, beta, rmean, rvar,
                       nbt, momentum, eps, a, b, mean, rstd, sp.s1, sp.s2);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(bn_finalize_kernel, dim3(nblk(C, 64)), dim3(1024), 0, s, part, T, R, P, C, gamma, beta, rmean, rvar,
                     nbt, momentum, eps, training, a, b, mean, rstd);
  return (int)hipGetLastError();
}

// res (nullable): the skip operand of a residual block, out = res + relu(...); not with a pool (-2)
DDPX_API int ddpx_f32_bn_apply_res(const float* y, const float* a, const float* b, const float* mean, const float* res,
                                   int N, int H, int W, int C, int relu, int pool, float* out, hipStream_t s) {
  if (C % 4 || (pool && (H % 2 || W % 2))) return -1;
  if (res && pool) return -2;
  const long n = (long)N * (pool ? H / 2 : H) * (pool ? W / 2 : W) * (C / 4);
  hipLaunchKernelGGL(bn_apply_kernel, dim3(nblk(n)), dim3(256), 0, s, y, a, b, mean, res, N, H, W, C, relu, pool, out);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_f32_bn_apply(const float* y, const float* a, const float* b, const float* mean, int N, int H, int W,
                               int C, int relu, int pool, float* out, hipStream_t s) {
  return ddpx_f32_bn_apply_res(y, a, b, mean, nullptr, N, H, W, C, relu, pool, out, s);
}

// The vectorised backward kernels need 4-channel quads that split a 256-thread block evenly and (pooled) chunks
// of whole window rows; DDPX_F32_BN_VEC=0 keeps the per-element kernels (A/B checks).
static bool bn_vec_ok(int C, int W, int pool, int R) {
  static const bool on = [] {
    const char* e = getenv("DDPX_F32_BN_VEC");
    return !(e && e[0] == '0');
  }();
  return on && C % 4 == 0 && C / 4 <= 256 && 256 % (C / 4) == 0 && (!pool || R % (2 * W) == 0);
}

// The _2g entry points take a second gradient g2 (nullable, g's shape) of the block's output, the skip connection of
// the residual block above: the kernels use g + g2.  The one-gradient entry points are the same launches with
// g2 = null.
DDPX_API int ddpx_f32_bn_bwd_sums_2g(const float* g, const float* g2, const float* y, const float* a, const float* b,
                                     const float* mean, const float* rstd, int N, int H, int W, int C, int pool, int R,
                                     float* part, hipStream_t s) {
  if (pool && (H % 2 || W % 2)) return -1;
  if (bn_vec_ok(C, W, pool, R)) {
    hipLaunchKernelGGL(bn_bwd_sums4_kernel, dim3(nblk((long)N * H * W, R)), dim3(256), 0, s, g, g2, y, a, b, mean,
                       rstd, N, H, W, C, pool, R, part, (float*)nullptr);
    return (int)hipGetLastError();
  }
  // any C <= 512: the threads past the last whole row group (256 % C of them) repeat rows of group 0 and their
  // sums are left out by block_group_sum, which adds the G = blockDim / C whole groups only
  if (C > 512) return -1;
  hipLaunchKernelGGL(bn_bwd_sums_kernel, dim3(nblk((long)N * H * W, R)), dim3(bn_threads(C)), 0, s, g, g2, y, a, b,
                     mean, rstd, N, H, W, C, pool, R, part);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_f32_bn_bwd_sums(const float* g, const float* y, const float* a, const float* b, const float* mean,
                                  const float* rstd, int N, int H, int W, int C, int pool, int R, float* part,
                                  hipStream_t s) {
  return ddpx_f32_bn_bwd_sums_2g(g, nullptr, y, a, b, mean, rstd, N, H, W, C, pool, R, part, s);
}

// Bias + activation backward (a = 1, b = 0, mean = 0, rstd = 1): the sums pass also writes dy = gz.  Returns 1
// when it did (the caller skips ddpx_f32_bn_bwd_apply), 0 when only the sums were written (no 4-channel path).
DDPX_API int ddpx_f32_bias_act_bwd_sums(const float* g, const float* y, const float* one, const float* zero, int N,
                                        int H, int W, int C, int pool, int R, float* part, float* dy, hipStream_t s) {
  if (pool && (H % 2 || W % 2)) return -1;
  if (bn_vec_ok(C, W, pool, R)) {
    hipLaunchKernelGGL(bn_bwd_sums4_kernel, dim3(nblk((long)N * H * W, R)), dim3(256), 0, s, g, (const float*)nullptr,
                       y, one, zero, zero, one, N, H, W, C, pool, R, part, dy);
    const int e = (int)hipGetLastError();
    return e ? -e : 1;
  }
  const int e = ddpx_f32_bn_bwd_sums(g, y, one, zero, zero, one, N, H, W, C, pool, R, part, s);
  return e ? (e < 0 ? e : -e) : 0;
}

DDPX_API int ddpx_f32_bn_bwd_finalize(const float* part, int T, int P, int C, float* c1, float* c2, float* dgamma,
                                      float* dbeta, int accumulate, double* ws, hipStream_t s) {
  const FinSplit sp = fin_split_plan(T, C, ws, 1);
  if (sp.Sr) {
    hipLaunchKernelGGL(bn_bwd_fin_sum_kernel, dim3(nblk(C, 64), sp.Sr), dim3(1024), 0, s, part, T, sp.Ts, C, sp.s1,
                       sp.s2);
    hipLaunchKernelGGL(bn_bwd_fin_out_kernel, dim3(nblk(C, 64)), dim3(64), 0, s, sp.Sr, P, C, c1, c2, dgamma, dbeta,
                       accumulate, sp.s1, sp.s2);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(nblk(C, 64)), dim3(1024), 0, s, part, T, P, C, c1, c2, dgamma, dbeta,
                     accumulate);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_f32_bn_bwd_apply_2g(const float* g, const float* g2, const float* y, const float* a, const float* b,
                                      const float* mean, const float* rstd, const float* c1, const float* c2, int N,
                                      int H, int W, int C, int pool, float* dy, hipStream_t s) {
  if (bn_vec_ok(C, W, pool, pool ? 2 * W : 1)) {
    const long units = pool ? (long)N * (H / 2) * (W / 2) : (long)N * H * W;
    hipLaunchKernelGGL(bn_bwd_apply4_kernel, dim3(nblk(units * (C / 4))), dim3(256), 0, s, g, g2, y, a, b, mean, rstd,
                       c1, c2, N, H, W, C, pool, dy);
    return (int)hipGetLastError();
  }
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(nblk((long)N * H * W * C)), dim3(256), 0, s, g, g2, y, a, b, mean, rstd,
                     c1, c2, N, H, W, C, pool, dy);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_f32_bn_bwd_apply(const float* g, const float* y, const float* a, const float* b, const float* mean,
                                   const float* rstd, const float* c1, const float* c2, int N, int H, int W, int C,
                                   int pool, float* dy, hipStream_t s) {
  return ddpx_f32_bn_bwd_apply_2g(g, nullptr, y, a, b, mean, rstd, c1, c2, N, H, W, C, pool, dy, s);
}
