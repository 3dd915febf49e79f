// ddpx — what the fp32 recipe runs between the convolution blocks and the loss (the GEMM core is in f32_gemm.hip,
// BatchNorm in f32_bn.hip): global average pool, the classifier head for up to 128 classes (logits + softmax
// cross-entropy + dlogits, and dW / db / dfeature with the ReLU / dropout mask in the backward), fixed-order column
// sums for the bias gradients, and the NCHW flatten between DeepNN's features and its classifier.
#include "ddpx_common.h"
#include "ddpx_f32.h"

namespace ddpx {
namespace f32k {

// ------------------------------------------------------------------ pooling / head
__global__ void __launch_bounds__(256) avgpool_kernel(const float* __restrict__ x, int N, int S, int C,
                                                       float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * C) return;
  const int n = i / C, c = i % C;
  float s = 0.f;
  for (int k = 0; k < S; ++k) s += x[((size_t)n * S + k) * C + c];
  out[i] = s / (float)S;
}

__global__ void __launch_bounds__(256) avgpool_bwd_kernel(const float* __restrict__ g, int N, int S, int C,
                                                           float* __restrict__ dx) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)N * S * C) return;
  const int c = (int)(i % C);
  const long n = i / ((long)S * C);
  dx[i] = g[n * C + c] / (float)S;
}

// Global max pool with a feature scale (the bf16 pair is in bn_pool.hip): out [N][C] = scale * max_s x[n][s][c], and
// the backward, which recomputes the argmax from x (lowest s among equal maxima, torch's tie rule) and writes
// scale * g there and +0 elsewhere.  One thread owns 4 consecutive channels of one sample, 16-B accesses; a NaN in the
// window stays in the forward.
__global__ void __launch_bounds__(256) gmaxpool_kernel(const float* __restrict__ x, int N, int S, int C, float scale,
                                                        float* __restrict__ out) {
  const int G = C >> 2;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= N * G) return;
  const int g = t % G, n = t / G;
  const float* xp = x + (size_t)n * S * C + g * 4;
  f32x4 m = *reinterpret_cast<const f32x4*>(xp);
  for (int i = 1; i < S; ++i) {
    const f32x4 f = *reinterpret_cast<const f32x4*>(xp + (size_t)i * C);
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = (f[j] > m[j] || f[j] != f[j]) ? f[j] : m[j];
  }
  *reinterpret_cast<f32x4*>(out + (size_t)n * C + g * 4) = m * scale;
}

__global__ void __launch_bounds__(256) gmaxpool_bwd_kernel(const float* __restrict__ go, const float* __restrict__ x,
                                                            int N, int S, int C, float scale, float* __restrict__ dx) {
  const int G = C >> 2;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= N * G) return;
  const int g = t % G, n = t / G;
  const size_t base = (size_t)n * S * C + g * 4;
  f32x4 m = *reinterpret_cast<const f32x4*>(x + base);
  int arg[4] = {0, 0, 0, 0};
  for (int i = 1; i < S; ++i) {
    const f32x4 f = *reinterpret_cast<const f32x4*>(x + base + (size_t)i * C);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (f[j] > m[j]) { m[j] = f[j]; arg[j] = i; }
  }
  const f32x4 gv = *reinterpret_cast<const f32x4*>(go + (size_t)n * C + g * 4) * scale;
  for (int i = 0; i < S; ++i) {
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = arg[j] == i ? gv[j] : 0.f;
    *reinterpret_cast<f32x4*>(dx + base + (size_t)i * C) = o;
  }
}

// logits[m][j] = h[m] . w[j] + bias[j] for a block of 16 classes (blockIdx.y = the class block, classes j0 ..
// j0 + 15 < NC): one wave per row, lanes stride K with 16-B loads and keep the block's class sums, then one wave
// reduction per class (the head is far below MFMA size; h is read once per class block).
constexpr int kMaxNC = 16;   // classes per block
constexpr int kWideNC = 128;
__global__ void __launch_bounds__(256) head_logits_blk_kernel(const float* __restrict__ h, const float* __restrict__ w,
                                                               const float* __restrict__ bias, int M, int K, int NC,
                                                               float* __restrict__ logits) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int j0 = blockIdx.y * kMaxNC;
  const int nj = min(kMaxNC, NC - j0);
  if (m >= M) return;
  float acc[kMaxNC];
#pragma unroll
  for (int j = 0; j < kMaxNC; ++j) acc[j] = 0.f;
  const f32x4* hp = reinterpret_cast<const f32x4*>(h + (size_t)m * K);
  for (int k4 = lane; k4 < K / 4; k4 += 64) {
    const f32x4 x = hp[k4];
#pragma unroll
    for (int j = 0; j < kMaxNC; ++j) {
      if (j >= nj) break;
      const f32x4 y = reinterpret_cast<const f32x4*>(w + (size_t)(j0 + j) * K)[k4];
      acc[j] = fmaf(x[0], y[0], fmaf(x[1], y[1], fmaf(x[2], y[2], fmaf(x[3], y[3], acc[j]))));
    }
  }
#pragma unroll
  for (int j = 0; j < kMaxNC; ++j) {
    if (j >= nj) break;
    const float v = wave_sum(acc[j]);
    if (lane == 0) logits[(size_t)m * NC + j0 + j] = v + bias[j0 + j];
  }
}

// The reference's 10-class head: one workgroup per row, the row's K / 4 vectors split over 256 threads with
// every load issued before the FMAs, then a wave + workgroup reduction in fixed order.  (One wave per row
// walking 16 dependent K-steps ran 63 us at M = 512, K = 4096: profiles/r3_models.)
template <int NC>
__global__ void __launch_bounds__(256) head_logits_row_kernel(const float* __restrict__ h, const float* __restrict__ w,
                                                              const float* __restrict__ bias, int K,
                                                              float* __restrict__ logits) {
  __shared__ float red[4][NC];
  const int m = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int K4 = K / 4;
  float acc[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) acc[j] = 0.f;
  const f32x4* hp = reinterpret_cast<const f32x4*>(h + (size_t)m * K);
  for (int k0 = tid; k0 < K4; k0 += 4 * 256) {
    f32x4 x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = k0 + u * 256 < K4 ? hp[k0 + u * 256] : (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const f32x4* wp = reinterpret_cast<const f32x4*>(w + (size_t)j * K);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const f32x4 y = k0 + u * 256 < K4 ? wp[k0 + u * 256] : (f32x4){0.f, 0.f, 0.f, 0.f};
        acc[j] = fmaf(x[u][0], y[0], fmaf(x[u][1], y[1], fmaf(x[u][2], y[2], fmaf(x[u][3], y[3], acc[j]))));
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const float v = wave_sum(acc[j]);
    if (lane == 0) red[wv][j] = v;
  }
  __syncthreads();
  if (tid < NC) logits[(size_t)m * NC + tid] = ((red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid])) + bias[tid];
}

// One workgroup: per-row log-softmax, loss = mean_m (lse - logit[target]), dl = (softmax - onehot) / M.
// SOFT: against q_j = (1 - smoothing) * (lam_m [j == tgt_m] + (1 - lam_m) [j == tgt_b_m]) + smoothing / NC
// (tgt_b null: no second label; lam null: 1): loss_m = lse - sum_j q_j l_j summed in class order (exactly
// l[t], the hard path's bits, when smoothing = 0 and lam = 1), dl = (softmax - q) / M.
template <bool SOFT>
__global__ void __launch_bounds__(1024) xent_kernel(const float* __restrict__ logits, const int64_t* __restrict__ tgt,
                                                     int M, int NC, float* __restrict__ loss,
                                                     float* __restrict__ dl, const int64_t* __restrict__ tgt_b,
                                                     const float* __restrict__ lam, float smoothing) {
  __shared__ float red[1024];
  const int tid = threadIdx.x;
  float acc = 0.f;
  for (int m = tid; m < M; m += 1024) {
    const float* l = logits + (size_t)m * NC;
    float mx = -INFINITY;
    for (int j = 0; j < NC; ++j) mx = fmaxf(mx, l[j]);
    float se = 0.f;
    for (int j = 0; j < NC; ++j) se += expf(l[j] - mx);
    const float lse = mx + logf(se);
    const int t = (int)tgt[m];
    if constexpr (SOFT) {
      const int tb = tgt_b ? (int)tgt_b[m] : t;
      const float la = (tgt_b && lam) ? lam[m] : 1.f;
      const float keep = 1.f - smoothing, oml = 1.f - la, uni = smoothing / (float)NC;
      float zt = 0.f;
      for (int j = 0; j < NC; ++j) {
        const float q = keep * ((j == t ? la : 0.f) + (j == tb ? oml : 0.f)) + uni;
        zt += q * l[j];
        if (dl) dl[(size_t)m * NC + j] = (expf(l[j] - lse) - q) / (float)M;
      }
      acc += lse - zt;
    } else {
      acc += lse - l[t];
      if (dl)
        for (int j = 0; j < NC; ++j) dl[(size_t)m * NC + j] = (expf(l[j] - lse) - (j == t ? 1.f : 0.f)) / (float)M;
    }
  }
  red[tid] = acc;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0 && loss) *loss = red[0] / (float)M;
}

// dW[j][k] (+)= go * sum_m dl[m][j] h[m][k];  db[j] (+)= go * sum_m dl[m][j]
// Workgroups of 64 columns k x 16 row groups (h read once, coalesced; all NC classes per thread), fixed-order
// LDS reduction over the row groups; the workgroups x = gridDim.x - 1 sum db instead (one wave per class).
// blockIdx.y = the block of 16 classes j0 .. j0 + 15 < NC, as in head_logits_blk_kernel.
// STAGE (NC <= 16, one class block): dlogits staged in LDS once per workgroup when they fit (every wave reads every
// row of it: broadcast LDS reads instead of 10 global loads per row per lane).  Without it (17..128 classes: M * NC
// is past the stage, the 16 values of a row and class block are one 64-B line) the kernel holds 32 KB less LDS:
// a compile-time flag, so that those launches keep their occupancy.
constexpr int kHeadDlLds = 8192;  // floats of dlogits staged in LDS (M * NC; 512 x 10 at the reference's batch)
template <bool STAGE>
__global__ void __launch_bounds__(1024) head_wgrad_kernel(const float* __restrict__ dl, const float* __restrict__ go,
                                                           const float* __restrict__ h, int M, int K, int NC,
                                                           float* __restrict__ dW, float* __restrict__ db,
                                                           int accumulate) {
  __shared__ float red[16][kMaxNC][64];
  const float s = go ? *go : 1.f;
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int j0 = STAGE ? 0 : blockIdx.y * kMaxNC;
  const int nj = STAGE ? NC : min(kMaxNC, NC - j0);
  if (blockIdx.x == gridDim.x - 1) {  // bias gradient
    if (g < nj && db) {
      float acc = 0.f;
      for (int m = cl; m < M; m += 64) acc += dl[(size_t)m * NC + j0 + g];
      acc = wave_sum(acc) * s;
      if (cl == 0) db[j0 + g] = accumulate ? db[j0 + g] + acc : acc;
    }
    return;
  }
  const int k = blockIdx.x * 64 + cl;
  float acc[kMaxNC];
#pragma unroll
  for (int j = 0; j < kMaxNC; ++j) acc[j] = 0.f;
  auto rows = [&](const auto* dsrc) {  // dsrc[m * NC + j]: class j0 + j of row m
    // 8 rows' loads in flight per thread (a dependent load per row was latency bound: 35 us at M = 512)
    int m = g;
    for (; m + 7 * 16 < M; m += 8 * 16) {
      float hv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) hv[u] = h[(size_t)(m + u * 16) * K + k];
#pragma unroll
      for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int j = 0; j < kMaxNC; ++j) {
          if (j >= nj) break;
          acc[j] = fmaf(dsrc[(size_t)(m + u * 16) * NC + j], hv[u], acc[j]);
        }
    }
    for (; m < M; m += 16) {
      const float hv = h[(size_t)m * K + k];
#pragma unroll
      for (int j = 0; j < kMaxNC; ++j) {
        if (j >= nj) break;
        acc[j] = fmaf(dsrc[(size_t)m * NC + j], hv, acc[j]);
      }
    }
  };
  if constexpr (STAGE) {
    __shared__ float dls[kHeadDlLds];
    if (M * NC <= kHeadDlLds) {
      for (int i = threadIdx.x; i < M * NC; i += 1024) dls[i] = dl[i];
      __syncthreads();
      if (k < K) rows(dls);
    } else if (k < K) {
      rows(dl);
    }
  } else if (k < K) {
    rows(dl + j0);
  }
#pragma unroll
  for (int j = 0; j < kMaxNC; ++j) red[g][j][cl] = acc[j];
  __syncthreads();
  if (g < nj && k < K) {
    float t = 0.f;
    for (int q = 0; q < 16; ++q) t += red[q][g][cl];
    t *= s;
    const size_t o = (size_t)(j0 + g) * K + k;
    dW[o] = accumulate ? dW[o] + t : t;
  }
}

// ------------------------------------------------------------------ 17..128 classes: cross-entropy
// One wave per row (4 rows per workgroup): lane l holds the classes l and l + 64, the maximum, the sum of
// exponentials and sum_j q_j l_j go through the fixed xor butterfly (every lane gets the same bits).  The row's
// loss goes to rows[m]; xent_rows_sum_kernel adds them in row order.  SOFT as xent_kernel: with smoothing = 0 and
// lam = 1 every q_j is exactly 0 or 1, the lane sums are l[t] and zeros, and the result is the hard path's bits.
template <bool SOFT>
__global__ void __launch_bounds__(256) xent_wave_kernel(const float* __restrict__ logits,
                                                         const int64_t* __restrict__ tgt, int M, int NC,
                                                         float* __restrict__ rows, float* __restrict__ dl,
                                                         const int64_t* __restrict__ tgt_b,
                                                         const float* __restrict__ lam, float smoothing) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const float* l = logits + (size_t)m * NC;
  float z[2];
  float mx = -INFINITY;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int j = lane + 64 * u;
    z[u] = j < NC ? l[j] : -INFINITY;
    mx = fmaxf(mx, z[u]);
  }
  mx = wave_max(mx);
  float se = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u)
    if (lane + 64 * u < NC) se += expf(z[u] - mx);
  se = wave_sum(se);
  const float lse = mx + logf(se);
  const int t = (int)tgt[m];
  int tb = t;
  float la = 1.f, keep = 1.f, oml = 0.f, uni = 0.f;
  if constexpr (SOFT) {
    if (tgt_b) tb = (int)tgt_b[m];
    if (tgt_b && lam) la = lam[m];
    keep = 1.f - smoothing;
    oml = 1.f - la;
    uni = smoothing / (float)NC;
  }
  float zt = 0.f;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int j = lane + 64 * u;
    if (j < NC) {
      float q;
      if constexpr (SOFT) {
        q = keep * ((j == t ? la : 0.f) + (j == tb ? oml : 0.f)) + uni;
        zt += q * z[u];
      } else {
        q = j == t ? 1.f : 0.f;
        zt += j == t ? z[u] : 0.f;
      }
      if (dl) dl[(size_t)m * NC + j] = (expf(z[u] - lse) - q) / (float)M;
    }
  }
  zt = wave_sum(zt);
  if (lane == 0) rows[m] = lse - zt;
}

__global__ void __launch_bounds__(64) xent_rows_sum_kernel(const float* __restrict__ rows, int M,
                                                            float* __restrict__ loss) {
  const int lane = threadIdx.x;
  float s = 0.f;
  for (int i0 = 0; i0 < M; i0 += 64 * 8) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = i0 + q * 64 + lane < M ? rows[i0 + q * 64 + lane] : 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) s += v[q];
  }
  s = wave_sum(s);
  if (lane == 0) *loss = s / (float)M;
}

// dh[m][k] = go * dh_scale * sum_j dl[m][j] w[j][k]   [* (h[m][k] > 0)]
// (dh_scale = 1/(1-p) when h is the output of an inverted Dropout(p) after a ReLU: h > 0 is then exactly "kept
// and positive", so the dropout + ReLU backward costs nothing extra; 1 otherwise)
__global__ void __launch_bounds__(256) head_dgrad_kernel(const float* __restrict__ dl, const float* __restrict__ go,
                                                          const float* __restrict__ w, const float* __restrict__ h,
                                                          int M, int K, int NC, int relu_mask, float dh_scale,
                                                          float* __restrict__ dh) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)M * K) return;
  const int m = (int)(i / K), k = (int)(i % K);
  float acc = 0.f;
  for (int j = 0; j < NC; ++j) acc = fmaf(dl[(size_t)m * NC + j], w[(size_t)j * K + k], acc);
  acc *= (go ? *go : 1.f) * dh_scale;
  if (relu_mask && !(h[i] > 0.f)) acc = 0.f;
  dh[i] = acc;
}

// Same as head_dgrad_kernel with 4 consecutive columns per thread (16-B loads / stores of w, h, dh); the sum over
// the classes runs in the same order, so the result is bitwise that of the scalar kernel.
__global__ void __launch_bounds__(256) head_dgrad4_kernel(const float* __restrict__ dl, const float* __restrict__ go,
                                                           const float* __restrict__ w, const float* __restrict__ h,
                                                           int M, int K, int NC, int relu_mask, float dh_scale,
                                                           float* __restrict__ dh) {
  const long i4 = (long)blockIdx.x * 256 + threadIdx.x;
  const int K4 = K / 4;
  if (i4 >= (long)M * K4) return;
  const int m = (int)(i4 / K4), k4 = (int)(i4 % K4);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < NC; ++j) {
    const float d = dl[(size_t)m * NC + j];
    const f32x4 wv = reinterpret_cast<const f32x4*>(w + (size_t)j * K)[k4];
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = fmaf(d, wv[q], acc[q]);
  }
  const float g = (go ? *go : 1.f) * dh_scale;
  const f32x4 hv = reinterpret_cast<const f32x4*>(h + (size_t)m * K)[k4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    acc[q] *= g;
    if (relu_mask && !(hv[q] > 0.f)) acc[q] = 0.f;
  }
  reinterpret_cast<f32x4*>(dh + (size_t)m * K)[k4] = acc;
}

// out[n] (+)= sum_m x[m][n]: workgroups of 64 columns x 16 row groups, fixed-order LDS reduction
// part[t][0][c] = sum of x[r][c] over chunk t's R rows, part[t][1][c] = 0 (the [T][2][C] layout
// ddpx_f32_bn_bwd_finalize merges in fixed order): the bias gradient of a conv + ReLU block whose data gradient
// was masked by the producing GEMM.  C / 4 lanes per row (16-B loads), 256 / (C / 4) rows in parallel, their
// partial sums combined in row-lane order (deterministic).
__global__ void __launch_bounds__(256) colsum_part_kernel(const float* __restrict__ x, int P, int C, int R,
                                                          float* __restrict__ part) {
  __shared__ f32x4 red[256];
  const int Q = C / 4, RP = 256 / Q;
  const int q = threadIdx.x % Q, rl = threadIdx.x / Q;
  const int r0 = blockIdx.x * R, r1 = min(P, r0 + R);
  f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
  if (rl < RP) {
    int r = r0 + rl;
    for (; r + 3 * RP < r1; r += 4 * RP) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const f32x4*>(x + (size_t)(r + u * RP) * C + 4 * q);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc += v[u];
    }
    for (; r < r1; r += RP) acc += *reinterpret_cast<const f32x4*>(x + (size_t)r * C + 4 * q);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < Q) {
    f32x4 t = red[threadIdx.x];
    for (int j = 1; j < RP; ++j) t += red[j * Q + threadIdx.x];
    *reinterpret_cast<f32x4*>(part + (size_t)blockIdx.x * 2 * C + 4 * threadIdx.x) = t;
    *reinterpret_cast<f32x4*>(part + (size_t)blockIdx.x * 2 * C + C + 4 * threadIdx.x) = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
}

__global__ void __launch_bounds__(1024) colsum_kernel(const float* __restrict__ x, int M, int N,
                                                       float* __restrict__ out, int accumulate) {
  __shared__ float red[16][64];
  const int cl = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + cl;
  float acc = 0.f;
  if (n < N) {
    // 8 rows' loads in flight, summed in the same row order as one at a time (bitwise unchanged)
    int m = g;
    for (; m + 7 * 16 < M; m += 8 * 16) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = x[(size_t)(m + u * 16) * N + n];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; m < M; m += 16) acc += x[(size_t)m * N + n];
  }
  red[g][cl] = acc;
  __syncthreads();
  if (g == 0 && n < N) {
    float t = 0.f;
    for (int q = 0; q < 16; ++q) t += red[q][cl];
    out[n] = accumulate ? out[n] + t : t;
  }
}

// torch.flatten(x, 1) of an NCHW activation held as NHWC: out[n][c * S + s] = x[n][s][c] (backward = 0), or the
// inverse for its gradient: out[n][s][c] = x[n][c * S + s] (backward = 1).  One thread per element, the NHWC
// side read / written contiguously.
__global__ void __launch_bounds__(256) nchw_flatten_kernel(const float* __restrict__ x, int N, int S, int C,
                                                            int backward, float* __restrict__ out) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;  // NHWC index
  if (i >= (long)N * S * C) return;
  const int c = (int)(i % C);
  const long r = i / C;
  const int sp = (int)(r % S);
  const long n = r / S;
  const size_t f = (size_t)n * S * C + (size_t)c * S + sp;
  if (backward) out[i] = x[f];
  else out[f] = x[i];
}

// bf16 version for the native DeepNN's classifier input (2048 = 32 channels x 8 x 8 features per image): one
// workgroup per image stages the image's S x C values in LDS, so both the NHWC side and the (C, H, W) side are
// read / written contiguously (2-byte elements).  S * C <= kFlatLds.
constexpr int kFlatLds = 16384;
__global__ void __launch_bounds__(256) nchw_flatten_bf16_kernel(const unsigned short* __restrict__ x, int S, int C,
                                                                 int backward, unsigned short* __restrict__ out) {
  __shared__ unsigned short img[kFlatLds];
  const int SC = S * C;
  const size_t base = (size_t)blockIdx.x * SC;
  for (int i = threadIdx.x; i < SC; i += 256) img[i] = x[base + i];
  __syncthreads();
  for (int j = threadIdx.x; j < SC; j += 256) {
    if (backward) {  // out NHWC j = s * C + c  <-  x (C, S) order c * S + s
      const int sp = j / C, c = j - sp * C;
      out[base + j] = img[c * S + sp];
    } else {         // out (C, S) order j = c * S + s  <-  x NHWC s * C + c
      const int c = j / S, sp = j - c * S;
      out[base + j] = img[sp * C + c];
    }
  }
}

}  // namespace f32k
}  // namespace ddpx

using namespace ddpx;
using namespace ddpx::f32k;

DDPX_API int ddpx_f32_avgpool(const float* x, int N, int S, int C, float* out, int backward, hipStream_t s) {
  if (backward)
    hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(nblk((long)N * S * C)), dim3(256), 0, s, x, N, S, C, out);
  else
    hipLaunchKernelGGL(avgpool_kernel, dim3(nblk((long)N * C)), dim3(256), 0, s, x, N, S, C, out);
  return (int)hipGetLastError();
}

// C % 4 == 0, S >= 1, 16-B aligned pointers; -1 otherwise.
DDPX_API int ddpx_f32_gmaxpool(const float* x, int N, int S, int C, float scale, float* out, hipStream_t s) {
  if (N < 0 || S < 1 || C < 4 || C % 4 || (((uintptr_t)x | (uintptr_t)out) & 15)) return -1;
  const long n = (long)N * (C / 4);
  if (n == 0) return 0;
  if (n > 0x7fffffffL) return -1;
  hipLaunchKernelGGL(gmaxpool_kernel, dim3(nblk(n)), dim3(256), 0, s, x, N, S, C, scale, out);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_f32_gmaxpool_bwd(const float* g, const float* x, int N, int S, int C, float scale, float* dx,
                                   hipStream_t s) {
  if (N < 0 || S < 1 || C < 4 || C % 4 || (((uintptr_t)g | (uintptr_t)x | (uintptr_t)dx) & 15)) return -1;
  const long n = (long)N * (C / 4);
  if (n == 0) return 0;
  if (n > 0x7fffffffL) return -1;
  hipLaunchKernelGGL(gmaxpool_bwd_kernel, dim3(nblk(n)), dim3(256), 0, s, g, x, N, S, C, scale, dx);
  return (int)hipGetLastError();
}

// Logits (the reference's 10 classes: one workgroup per row; otherwise by class blocks), then, with tgt, the
// cross-entropy: NC <= 16 in one workgroup (xent_kernel); above, one wave per row and the row losses [M] (rows:
// scratch, required there) summed in row order by a last one-wave step.
template <bool SOFT>
static int f32_head_fwd(const float* h, const float* w, const float* bias, const int64_t* tgt, const int64_t* tgt_b,
                        const float* lam, float smoothing, int M, int K, int NC, float* logits, float* loss, float* dl,
                        float* rows, hipStream_t s) {
  if (K % 4) return -1;
  if (NC < 1 || NC > kWideNC) return -2;
  if (tgt && NC > kMaxNC && (!rows || !loss)) return -5;
  if (M <= 0) return 0;
  if (NC == 10)
    hipLaunchKernelGGL(head_logits_row_kernel<10>, dim3(M), dim3(256), 0, s, h, w, bias, K, logits);
  else
    hipLaunchKernelGGL(head_logits_blk_kernel, dim3(nblk(M, 4), nblk(NC, kMaxNC)), dim3(256), 0, s, h, w, bias, M, K,
                       NC, logits);
  if (tgt && NC <= kMaxNC) {
    hipLaunchKernelGGL(xent_kernel<SOFT>, dim3(1), dim3(1024), 0, s, logits, tgt, M, NC, loss, dl, tgt_b, lam,
                       smoothing);
  } else if (tgt) {
    hipLaunchKernelGGL(xent_wave_kernel<SOFT>, dim3(nblk(M, 4)), dim3(256), 0, s, logits, tgt, M, NC, rows, dl, tgt_b,
                       lam, smoothing);
    hipLaunchKernelGGL(xent_rows_sum_kernel, dim3(1), dim3(64), 0, s, rows, M, loss);
  }
  return (int)hipGetLastError();
}

DDPX_API int ddpx_f32_head_fwd(const float* h, const float* w, const float* bias, const int64_t* tgt, int M, int K,
                               int NC, float* logits, float* loss, float* dl, float* rows, hipStream_t s) {
  return f32_head_fwd<false>(h, w, bias, tgt, nullptr, nullptr, 0.f, M, K, NC, logits, loss, dl, rows, s);
}

// Soft targets: tgt_b [M] int64 and lam [M] fp32 nullable, smoothing in [0, 1] (xent_kernel above).
DDPX_API int ddpx_f32_head_fwd_soft(const float* h, const float* w, const float* bias, const int64_t* tgt,
                                    const int64_t* tgt_b, const float* lam, float smoothing, int M, int K, int NC,
                                    float* logits, float* loss, float* dl, float* rows, hipStream_t s) {
  if (!tgt) return -3;
  if (!(smoothing >= 0.f && smoothing <= 1.f)) return -4;
  return f32_head_fwd<true>(h, w, bias, tgt, tgt_b, lam, smoothing, M, K, NC, logits, loss, dl, rows, s);
}

DDPX_API int ddpx_f32_head_bwd(const float* dl, const float* go, const float* h, const float* w, int M, int K, int NC,
                               float* dW, float* db, int accumulate, float* dh, int relu_mask, float dh_scale,
                               hipStream_t s) {
  if (NC > kWideNC) return -2;
  if (dW && NC > kMaxNC)
    hipLaunchKernelGGL(head_wgrad_kernel<false>, dim3(nblk(K, 64) + 1, nblk(NC, kMaxNC)), dim3(1024), 0, s, dl, go, h,
                       M, K, NC, dW, db, accumulate);
  else if (dW)
    hipLaunchKernelGGL(head_wgrad_kernel<true>, dim3(nblk(K, 64) + 1), dim3(1024), 0, s, dl, go, h, M, K, NC, dW, db,
                       accumulate);
  if (dh && K % 4 == 0 && !(((uintptr_t)w | (uintptr_t)h | (uintptr_t)dh) & 15))
    hipLaunchKernelGGL(head_dgrad4_kernel, dim3(nblk((long)M * (K / 4))), dim3(256), 0, s, dl, go, w, h, M, K, NC,
                       relu_mask, dh_scale, dh);
  else if (dh)
    hipLaunchKernelGGL(head_dgrad_kernel, dim3(nblk((long)M * K)), dim3(256), 0, s, dl, go, w, h, M, K, NC,
                       relu_mask, dh_scale, dh);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_f32_colsum_part(const float* x, int P, int C, int R, float* part, hipStream_t s) {
  if (C % 4 || C > 1024 || R < 1 || ((uintptr_t)x & 15) || ((uintptr_t)part & 15)) return -1;
  hipLaunchKernelGGL(colsum_part_kernel, dim3((P + R - 1) / R), dim3(256), 0, s, x, P, C, R, part);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_f32_colsum(const float* x, int M, int N, float* out, int accumulate, hipStream_t s) {
  hipLaunchKernelGGL(colsum_kernel, dim3(nblk(N, 64)), dim3(1024), 0, s, x, M, N, out, accumulate);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_f32_nchw_flatten(const float* x, int N, int S, int C, int backward, float* out, hipStream_t s) {
  hipLaunchKernelGGL(nchw_flatten_kernel, dim3(nblk((long)N * S * C)), dim3(256), 0, s, x, N, S, C, backward, out);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_bf16_nchw_flatten(const void* x, int N, int S, int C, int backward, void* out, hipStream_t s) {
  if (S * C > kFlatLds || N <= 0) return -1;
  hipLaunchKernelGGL(nchw_flatten_bf16_kernel, dim3(N), dim3(256), 0, s, (const unsigned short*)x, S, C, backward,
                     (unsigned short*)out);
  return (int)hipGetLastError();
}
