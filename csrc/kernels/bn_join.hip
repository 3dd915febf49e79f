// ddpx — the join of a basic residual block (ResNet-18/34 style) on NHWC bf16, fused into the BatchNorm passes.
//
//   out = relu(a*y + b + s)          y: raw output of the branch's second 3x3 convolution, (a, b) from bn_finalize
//   identity   mode: s = res         the block's input, bf16 [N][H][W][C]
//   projection mode: s = a2*y2 + b2  y2: raw output of the 1x1 / stride-2 shortcut convolution, (a2, b2) the
//                                    shortcut BatchNorm's coefficients
//
// The ReLU comes AFTER the add (bn_pool.hip's apply_kernel with res computes res + relu(a*y + b), ResNet-9's
// form), and in projection mode the second operand is itself a BatchNorm.  Composed from the existing kernels the
// join would cost three more activation-sized passes forward (shortcut apply, add, ReLU) and more backward; here
// it is one pass forward and two backward, as a plain BatchNorm block.
//
// Everything is fp32 arithmetic on bf16 storage, rounded once.  z = fmaf(a, y, b) + s lives in ONE device function
// (join_z) that the forward and both backward passes call: the backward recomputes the ReLU mask [z > 0] from the
// operands (nothing is stored for it) and so agrees with the forward bit for bit.
//
// Backward, with m = (g + g2) * [z > 0] (g2 nullable; the sum is formed in fp32 and never stored):
//   pass 1  per channel: S0 = sum m, S1 = sum m*xhat, and in projection mode S2 = sum m*xhat2 (xhat2 with the
//           shortcut BatchNorm's mean / rstd).  S0 serves both BatchNorms (dbeta2 = dbeta).  A block is
//           (C/8 channel groups) x (pixel lanes), grid-strided over pixels; per-thread fp32 accumulators, combined
//           over the pixel lanes through LDS in lane order, one partial row per block, no atomics: reproducible.
//           Layout part[V][B][2][C], V = 1 | 2: view 0 holds (S0, S1), view 1 (S0, S2), so each view is the
//           [B][2][C] array bn_pool.hip's merge kernels read: one merge call per BatchNorm, no third merge kernel.
//   merge   bn::launch_bwd_finalize per view: c1 = S0/M, c2 = S1/M (c2b = S2/M), dgamma / dbeta stored fp32, stored
//           bf16, accumulated or applied as the fused SGD update.
//   pass 2  re-reads g, [g2], y and (res | y2):  dy = a*(m - c1 - xhat*c2) for the branch; projection mode also
//           dy2 = a2*(m - c1 - xhat2*c2b) for the shortcut BatchNorm; identity mode also gm = bf16(m), the skip
//           gradient, which the block below takes as its second gradient (one write and two later reads, against
//           four or more reads and a mask recomputation in every consumer if (g, g2, operands) were handed down).
//
// Work split: one thread per (pixel, 8-channel group), 16-B loads and stores, per-channel coefficients in registers
// (the elementwise passes are bandwidth bound: identity forward moves 3 activation-sized arrays, pass 1 reads 3-4,
// pass 2 reads 3-4 and writes 2).  The sums pass-1/pass-2 entry points are separate so that a later SyncBatchNorm
// join can put its all-reduce between them.
#include <climits>
#include <cstdint>
#include <initializer_list>

#include "ddpx_bn.h"

namespace ddpx {
namespace bnjoin {

using bn::add_grad2;
using bn::pack8;
using bn::unpack8;

// Per-thread coefficients of one 8-channel group.
struct Coef {
  float a[8], b[8], mu[8], rs[8];
};

__device__ __forceinline__ void load_coef(Coef& k, const float* __restrict__ a, const float* __restrict__ b,
                                          const float* __restrict__ mean, const float* __restrict__ rstd, int g) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    k.a[j] = a[g * 8 + j];
    k.b[j] = b[g * 8 + j];
    k.mu[j] = mean ? mean[g * 8 + j] : 0.f;
    k.rs[j] = rstd ? rstd[g * 8 + j] : 1.f;
  }
}

// THE join expression.  f: y; so: res (identity) or y2 (projection), both as fp32.  z = fmaf(a, y, b) + s with
// s = so or fmaf(a2, so, b2).
template <bool PROJ>
__device__ __forceinline__ void join_z(const float (&f)[8], const float (&so)[8], const Coef& k, const Coef& k2,
                                       float (&z)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float s = PROJ ? fmaf(k2.a[j], so[j], k2.b[j]) : so[j];
    z[j] = fmaf(k.a[j], f[j], k.b[j]) + s;
  }
}

// m = (g + g2) * [z > 0] for the 8 channels at element offset off; f / so: the unpacked operands (kept for xhat).
template <bool PROJ>
__device__ __forceinline__ void join_m(const unsigned short* __restrict__ g, const unsigned short* __restrict__ g2,
                                       const unsigned short* __restrict__ y, const unsigned short* __restrict__ sop,
                                       size_t off, const Coef& k, const Coef& k2, float (&f)[8], float (&so)[8],
                                       float (&m)[8]) {
  float z[8], gg[8];
  unpack8(*reinterpret_cast<const u32x4*>(y + off), f);
  unpack8(*reinterpret_cast<const u32x4*>(sop + off), so);
  unpack8(*reinterpret_cast<const u32x4*>(g + off), gg);
  add_grad2(g2, off, gg);
  join_z<PROJ>(f, so, k, k2, z);
#pragma unroll
  for (int j = 0; j < 8; ++j) m[j] = z[j] > 0.f ? gg[j] : 0.f;
}

// ---------------------------------------------------------------- forward
template <bool PROJ>
__global__ void __launch_bounds__(256)
join_kernel(const unsigned short* __restrict__ y, const float* __restrict__ a, const float* __restrict__ b,
            const unsigned short* __restrict__ sop, const float* __restrict__ a2, const float* __restrict__ b2, int n,
            int C, unsigned short* __restrict__ out) {
  const int G = C / 8;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;  // n = pixels * G
  const int g = t % G;
  const size_t off = (size_t)(t / G) * C + g * 8;
  Coef k, k2;
  load_coef(k, a, b, nullptr, nullptr, g);
  if (PROJ) load_coef(k2, a2, b2, nullptr, nullptr, g);
  float f[8], so[8], z[8];
  unpack8(*reinterpret_cast<const u32x4*>(y + off), f);
  unpack8(*reinterpret_cast<const u32x4*>(sop + off), so);
  join_z<PROJ>(f, so, k, k2, z);
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = fmaxf(z[j], 0.f);
  *reinterpret_cast<u32x4*>(out + off) = pack8(z);
}

// ---------------------------------------------------------------- backward, pass 1
// part0[blk][0][c] = sum m, part0[blk][1][c] = sum m*xhat; PROJ: part1[blk][0][c] = sum m, part1[blk][1][c] =
// sum m*xhat2.  Block = (G = C/8 channel groups) x (lanes = 256/G pixel lanes); threads past lanes*G idle.
template <bool PROJ>
__global__ void __launch_bounds__(256)
join_reduce_kernel(const unsigned short* __restrict__ gout, const unsigned short* __restrict__ gout2,
                   const unsigned short* __restrict__ y, const unsigned short* __restrict__ sop,
                   const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ mean,
                   const float* __restrict__ rstd, const float* __restrict__ a2, const float* __restrict__ b2,
                   const float* __restrict__ mean2, const float* __restrict__ rstd2, int P, int C,
                   float* __restrict__ part0, float* __restrict__ part1) {
  constexpr int NS = PROJ ? 3 : 2;
  __shared__ float red[NS][256 * 8];
  const int G = C / 8;
  const int lanes = 256 / G;  // G <= 64 => >= 4
  const int g = threadIdx.x % G, pl = threadIdx.x / G;
  float s0[8], s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s0[j] = s1[j] = s2[j] = 0.f;
  if (pl < lanes) {
    Coef k, k2;
    load_coef(k, a, b, mean, rstd, g);
    if (PROJ) load_coef(k2, a2, b2, mean2, rstd2, g);
    for (int pix = blockIdx.x * lanes + pl; pix < P; pix += gridDim.x * lanes) {
      float f[8], so[8], m[8];
      join_m<PROJ>(gout, gout2, y, sop, (size_t)pix * C + g * 8, k, k2, f, so, m);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s0[j] += m[j];
        s1[j] = fmaf(m[j], (f[j] - k.mu[j]) * k.rs[j], s1[j]);
        if (PROJ) s2[j] = fmaf(m[j], (so[j] - k2.mu[j]) * k2.rs[j], s2[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[0][threadIdx.x * 8 + j] = s0[j];
    red[1][threadIdx.x * 8 + j] = s1[j];
    if (PROJ) red[2][threadIdx.x * 8 + j] = s2[j];
  }
  __syncthreads();
  // channel c = gg*8 + j: the pixel lanes q = 0 .. lanes-1 in order (threads q*G + gg)
  for (int i = threadIdx.x; i < NS * C; i += 256) {
    const int which = i / C, c = i % C, gg = c / 8, j = c % 8;
    float s = 0.f;
    for (int q = 0; q < lanes; ++q) s += red[which][(q * G + gg) * 8 + j];
    const size_t row = (size_t)blockIdx.x * 2;
    if (which == 0) {
      part0[row * C + c] = s;
      if (PROJ) part1[row * C + c] = s;
    } else if (which == 1) {
      part0[(row + 1) * C + c] = s;
    } else {
      part1[(row + 1) * C + c] = s;
    }
  }
}

// ---------------------------------------------------------------- backward, pass 2
// dy = a*(m - c1 - xhat*c2); PROJ: aux = dy2 = a2*(m - c1 - xhat2*c2b); identity: aux = gm = bf16(m).
template <bool PROJ>
__global__ void __launch_bounds__(256)
join_apply_kernel(const unsigned short* __restrict__ gout, const unsigned short* __restrict__ gout2,
                  const unsigned short* __restrict__ y, const unsigned short* __restrict__ sop,
                  const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ mean,
                  const float* __restrict__ rstd, const float* __restrict__ a2, const float* __restrict__ b2,
                  const float* __restrict__ mean2, const float* __restrict__ rstd2, const float* __restrict__ c1,
                  const float* __restrict__ c2, const float* __restrict__ c2b, int n, int C,
                  unsigned short* __restrict__ dy, unsigned short* __restrict__ aux) {
  const int G = C / 8;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int g = t % G;
  const size_t off = (size_t)(t / G) * C + g * 8;
  Coef k, k2;
  load_coef(k, a, b, mean, rstd, g);
  if (PROJ) load_coef(k2, a2, b2, mean2, rstd2, g);
  float f[8], so[8], m[8], o[8], o2[8];
  join_m<PROJ>(gout, gout2, y, sop, off, k, k2, f, so, m);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = g * 8 + j;
    const float k1 = c1[c];
    const float xh = (f[j] - k.mu[j]) * k.rs[j];
    o[j] = k.a[j] * (m[j] - k1 - xh * c2[c]);
    if (PROJ) {
      const float xh2 = (so[j] - k2.mu[j]) * k2.rs[j];
      o2[j] = k2.a[j] * (m[j] - k1 - xh2 * c2b[c]);
    } else {
      o2[j] = m[j];
    }
  }
  *reinterpret_cast<u32x4*>(dy + off) = pack8(o);
  *reinterpret_cast<u32x4*>(aux + off) = pack8(o2);
}

// ---------------------------------------------------------------- option-A shortcut and strided second gradient
// The parameter-free shortcut of the CIFAR ResNet-20/32/44/56 (He et al., option A) and the gradient it sends down.
//
//   PAD  the join's second operand is read straight from the block input x [N][Hx][Wx][C/2], H = (Hx+1)/2, W =
//        (Wx+1)/2:  s[n,h,w,c] = x[n,2h,2w,c - C/4] for C/4 <= c < 3C/4, else 0.  C % 32 == 0, so C/4 is a multiple
//        of 8 and no 16-B channel group straddles the pad boundary: a group in the pad region loads nothing for s.
//        The backward's skip gradient comes back compact, gs [N][H][W][C/2] = bf16(m[..., C/4 : 3C/4]), written by
//        the middle groups only; the zero-inserted array at x's resolution is never formed.
//   SUB  the second gradient exists at even (h, w) only and is read there from the compact gs of the block above,
//        gs[n][h/2][w/2][:] ([N][(H+1)/2][(W+1)/2][C]); elsewhere it is 0 (still added, so -0 becomes +0 as with a
//        dense zero-inserted array).
// Instantiated: PAD, PAD+SUB (a downsampling block directly below another, depth 8) and identity+SUB (the block
// below a downsampling block).  identity without SUB is the kernels above, which stay as they are.  All of them form
// z in join_z<false>, so mask and forward agree bit for bit, and dy is the expression of join_apply_kernel.
//
// Work split.  These joins run at 16 / 32 / 64 channels, 2 / 4 / 8 channel groups: with one thread per (pixel,
// group) every thread would fetch its 8-channel slice of up to six coefficient vectors for 16 B of each activation.
// Here a workgroup stages the channel vectors (a, b, mean, rstd and the merged c1, c2) in LDS once; a thread owns
// one channel group, takes its slice LDS -> registers once and keeps it across PPT pixels.  Block = (G groups) x
// (lanes = 256/G pixel lanes); pixel i of lane q in block B is B*lanes*PPT + i*lanes + q, so each of the PPT steps
// of a workgroup reads one contiguous 4 KB piece of every dense operand.  The sums pass is the reduce kernel's
// shape (grid-strided lanes, per-thread accumulators, LDS combine in lane order, one partial row per block, no
// atomics: reproducible) and leaves part[1][B][2][C] for the same merge call.
constexpr int PPT = 4;
constexpr int CMAX = 512;

// the NV channel vectors src[v][0..C) -> lds[v*C + c]; ends in a barrier
template <int NV>
__device__ __forceinline__ void stage_vectors(float* __restrict__ lds, const float* const (&src)[NV], int C) {
#pragma unroll
  for (int v = 0; v < NV; ++v)
    for (int c = threadIdx.x; c < C; c += 256) lds[v * C + c] = src[v][c];
  __syncthreads();
}

__device__ __forceinline__ void lds_vec8(const float* __restrict__ lds, int g, float (&v)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = lds[g * 8 + j];
}

// pixel geometry of the pad / sub operands
struct PadGeo {
  int H, W, Hx, Wx;  // the join's rows / columns; x's (PAD only)
};

// the shortcut operand of group g at pixel p = (n, h, w)
template <bool PAD>
__device__ __forceinline__ void load_shortcut(const unsigned short* __restrict__ sop, int p, int n, int h, int w,
                                              int C, int g, const PadGeo& q, float (&so)[8]) {
  if (!PAD) {
    unpack8(*reinterpret_cast<const u32x4*>(sop + (size_t)p * C + g * 8), so);
    return;
  }
  const int G4 = C / 32;  // groups in C/4 channels
  if (g >= G4 && g < 3 * G4) {
    const size_t off = (((size_t)n * q.Hx + 2 * h) * q.Wx + 2 * w) * (C / 2) + (g - G4) * 8;
    unpack8(*reinterpret_cast<const u32x4*>(sop + off), so);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) so[j] = 0.f;
  }
}

// m = (g + g2) * [z > 0] of group g at pixel p; f: the unpacked y (kept for xhat)
template <bool PAD, bool SUB>
__device__ __forceinline__ void pad_m(const unsigned short* __restrict__ gout, const unsigned short* __restrict__ g2,
                                      const unsigned short* __restrict__ y, const unsigned short* __restrict__ sop,
                                      int p, int C, int g, const PadGeo& q, const Coef& k, float (&f)[8],
                                      float (&m)[8]) {
  const int w = p % q.W, t = p / q.W, h = t % q.H, n = t / q.H;
  const size_t off = (size_t)p * C + g * 8;
  float so[8], gg[8], z[8];
  unpack8(*reinterpret_cast<const u32x4*>(y + off), f);
  load_shortcut<PAD>(sop, p, n, h, w, C, g, q, so);
  unpack8(*reinterpret_cast<const u32x4*>(gout + off), gg);
  if (SUB) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    if (!((h | w) & 1)) {
      const size_t o2 = (((size_t)n * ((q.H + 1) / 2) + h / 2) * ((q.W + 1) / 2) + w / 2) * C + g * 8;
      unpack8(*reinterpret_cast<const u32x4*>(g2 + o2), v);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) gg[j] += v[j];
  } else {
    add_grad2(g2, off, gg);
  }
  join_z<false>(f, so, k, k, z);
#pragma unroll
  for (int j = 0; j < 8; ++j) m[j] = z[j] > 0.f ? gg[j] : 0.f;
}

// forward: out = relu(fmaf(a, y, b) + s), s gathered from x
__global__ void __launch_bounds__(256)
pad_join_kernel(const unsigned short* __restrict__ y, const float* __restrict__ a, const float* __restrict__ b,
                const unsigned short* __restrict__ x, int P, int C, PadGeo q, unsigned short* __restrict__ out) {
  __shared__ float co[2 * CMAX];
  const float* const src[2] = {a, b};
  stage_vectors<2>(co, src, C);
  const int G = C / 8, lanes = 256 / G;
  const int g = threadIdx.x % G, pl = threadIdx.x / G;
  if (pl >= lanes) return;
  Coef k;
  lds_vec8(co, g, k.a);
  lds_vec8(co + C, g, k.b);
  const int p0 = blockIdx.x * (lanes * PPT) + pl;
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int p = p0 + i * lanes;
    if (p < P) {
      const int w = p % q.W, t = p / q.W, h = t % q.H, n = t / q.H;
      const size_t off = (size_t)p * C + g * 8;
      float f[8], so[8], z[8];
      unpack8(*reinterpret_cast<const u32x4*>(y + off), f);
      load_shortcut<true>(x, p, n, h, w, C, g, q, so);
      join_z<false>(f, so, k, k, z);
#pragma unroll
      for (int j = 0; j < 8; ++j) z[j] = fmaxf(z[j], 0.f);
      *reinterpret_cast<u32x4*>(out + off) = pack8(z);
    }
  }
}

// backward, pass 1: part[blk][0][c] = sum m, part[blk][1][c] = sum m*xhat
template <bool PAD, bool SUB>
__global__ void __launch_bounds__(256)
pad_reduce_kernel(const unsigned short* __restrict__ gout, const unsigned short* __restrict__ g2,
                  const unsigned short* __restrict__ y, const unsigned short* __restrict__ sop,
                  const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ mean,
                  const float* __restrict__ rstd, int P, int C, PadGeo q, float* __restrict__ part) {
  __shared__ float red[2][256 * 8];
  __shared__ float co[4 * CMAX];
  const float* const src[4] = {a, b, mean, rstd};
  stage_vectors<4>(co, src, C);
  const int G = C / 8, lanes = 256 / G;
  const int g = threadIdx.x % G, pl = threadIdx.x / G;
  float s0[8], s1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s0[j] = s1[j] = 0.f;
  if (pl < lanes) {
    Coef k;
    lds_vec8(co, g, k.a);
    lds_vec8(co + C, g, k.b);
    lds_vec8(co + 2 * C, g, k.mu);
    lds_vec8(co + 3 * C, g, k.rs);
#pragma unroll 2
    for (int p = blockIdx.x * lanes + pl; p < P; p += gridDim.x * lanes) {
      float f[8], m[8];
      pad_m<PAD, SUB>(gout, g2, y, sop, p, C, g, q, k, f, m);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s0[j] += m[j];
        s1[j] = fmaf(m[j], (f[j] - k.mu[j]) * k.rs[j], s1[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    red[0][threadIdx.x * 8 + j] = s0[j];
    red[1][threadIdx.x * 8 + j] = s1[j];
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * C; i += 256) {
    const int which = i / C, c = i % C, gg = c / 8, j = c % 8;
    float s = 0.f;
    for (int l = 0; l < lanes; ++l) s += red[which][(l * G + gg) * 8 + j];
    part[((size_t)blockIdx.x * 2 + which) * C + c] = s;
  }
}

// backward, pass 2: dy = a*(m - c1 - xhat*c2); aux = gs (PAD: the middle groups, compact) or gm = bf16(m)
template <bool PAD, bool SUB>
__global__ void __launch_bounds__(256)
pad_apply_kernel(const unsigned short* __restrict__ gout, const unsigned short* __restrict__ g2,
                 const unsigned short* __restrict__ y, const unsigned short* __restrict__ sop,
                 const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ mean,
                 const float* __restrict__ rstd, const float* __restrict__ c1, const float* __restrict__ c2, int P,
                 int C, PadGeo q, unsigned short* __restrict__ dy, unsigned short* __restrict__ aux) {
  __shared__ float co[6 * CMAX];
  const float* const src[6] = {a, b, mean, rstd, c1, c2};
  stage_vectors<6>(co, src, C);
  const int G = C / 8, lanes = 256 / G;
  const int g = threadIdx.x % G, pl = threadIdx.x / G;
  if (pl >= lanes) return;
  Coef k;
  float k1[8], k2[8];
  lds_vec8(co, g, k.a);
  lds_vec8(co + C, g, k.b);
  lds_vec8(co + 2 * C, g, k.mu);
  lds_vec8(co + 3 * C, g, k.rs);
  lds_vec8(co + 4 * C, g, k1);
  lds_vec8(co + 5 * C, g, k2);
  const int G4 = C / 32;
  const int p0 = blockIdx.x * (lanes * PPT) + pl;
#pragma unroll
  for (int i = 0; i < PPT; ++i) {
    const int p = p0 + i * lanes;
    if (p < P) {
      float f[8], m[8], o[8];
      pad_m<PAD, SUB>(gout, g2, y, sop, p, C, g, q, k, f, m);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xh = (f[j] - k.mu[j]) * k.rs[j];
        o[j] = k.a[j] * (m[j] - k1[j] - xh * k2[j]);
      }
      *reinterpret_cast<u32x4*>(dy + (size_t)p * C + g * 8) = pack8(o);
      if (!PAD)
        *reinterpret_cast<u32x4*>(aux + (size_t)p * C + g * 8) = pack8(m);
      else if (g >= G4 && g < 3 * G4)
        *reinterpret_cast<u32x4*>(aux + (size_t)p * (C / 2) + (g - G4) * 8) = pack8(m);
    }
  }
}

// C % 8 == 0, C <= 512 (at least 4 pixel lanes per reduce block), P * C/8 threads in an int, 16-B pointers
static inline bool shape_ok(int N, int H, int W, int C) {
  if (N < 1 || H < 1 || W < 1 || C < 8 || C % 8 || C > 512) return false;
  return (long)N * H * W * (C / 8) <= (long)INT_MAX - 256;
}
static inline bool aligned(std::initializer_list<const void*> ps) {
  uintptr_t v = 0;
  for (const void* p : ps) v |= (uintptr_t)p;
  return (v & 15) == 0;
}

}  // namespace bnjoin
}  // namespace ddpx

using namespace ddpx;
typedef const unsigned short* cus;

// out = relu(a*y + b + s): exactly one of res (identity) and y2 (projection, with a2 / b2).  -1: refused shape,
// operand combination or alignment.
DDPX_API int ddpx_bn_join(const void* y, const float* a, const float* b, const void* res, const void* y2,
                          const float* a2, const float* b2, int N, int H, int W, int C, void* out, hipStream_t s) {
  if (!bnjoin::shape_ok(N, H, W, C) || !y || !a || !b || !out || (res != nullptr) == (y2 != nullptr)) return -1;
  if (y2 && (!a2 || !b2)) return -1;
  if (!bnjoin::aligned({y, res, y2, out})) return -1;
  const int n = N * H * W * (C / 8);
  const dim3 grid((n + 255) / 256), blk(256);
  if (y2)
    hipLaunchKernelGGL(bnjoin::join_kernel<true>, grid, blk, 0, s, (cus)y, a, b, (cus)y2, a2, b2, n, C,
                       (unsigned short*)out);
  else
    hipLaunchKernelGGL(bnjoin::join_kernel<false>, grid, blk, 0, s, (cus)y, a, b, (cus)res, a2, b2, n, C,
                       (unsigned short*)out);
  return (int)hipGetLastError();
}

// Pass-1 blocks B: at least 4 pixels per lane, at most 1024 blocks (ResNet-18's 4x4 stage at batch 512 still gets
// 512 blocks; unmeasured choice).
DDPX_API int ddpx_bn_join_blocks(int N, int H, int W, int C) {
  if (!bnjoin::shape_ok(N, H, W, C)) return -1;
  const int lanes = 256 / (C / 8);
  const long P = (long)N * H * W;
  long blocks = (P + lanes * 4 - 1) / (lanes * 4);
  return (int)(blocks > 1024 ? 1024 : blocks);
}

// Pass 1: part[V][B][2][C] fp32, V = 2 in projection mode (y2 given), B = ddpx_bn_join_blocks.
DDPX_API int ddpx_bn_join_bwd_sums(const void* g, const void* g2, const void* y, const float* a, const float* b,
                                   const float* mean, const float* rstd, const void* res, const void* y2,
                                   const float* a2, const float* b2, const float* mean2, const float* rstd2, int N,
                                   int H, int W, int C, float* part, hipStream_t s) {
  if (!bnjoin::shape_ok(N, H, W, C) || !g || !y || !a || !b || !mean || !rstd || !part) return -1;
  if ((res != nullptr) == (y2 != nullptr) || (y2 && (!a2 || !b2 || !mean2 || !rstd2))) return -1;
  if (!bnjoin::aligned({g, g2, y, res, y2})) return -1;
  const int B = ddpx_bn_join_blocks(N, H, W, C);
  const int P = N * H * W;
  float* part1 = part + (size_t)B * 2 * C;
  if (y2)
    hipLaunchKernelGGL(bnjoin::join_reduce_kernel<true>, dim3(B), dim3(256), 0, s, (cus)g, (cus)g2, (cus)y, (cus)y2,
                       a, b, mean, rstd, a2, b2, mean2, rstd2, P, C, part, part1);
  else
    hipLaunchKernelGGL(bnjoin::join_reduce_kernel<false>, dim3(B), dim3(256), 0, s, (cus)g, (cus)g2, (cus)y, (cus)res,
                       a, b, mean, rstd, a2, b2, mean2, rstd2, P, C, part, (float*)nullptr);
  return (int)hipGetLastError();
}

// Merge of one view part[B][2][C] of the pass-1 partials by bn_pool.hip's merge kernels: c1 = S0/M, c2 = S1/M, dbeta
// = S0 and dgamma = S1 stored (fp32 / bf16, = / +=) or applied as the fused SGD update (sg_p / sb_p with lr).
DDPX_API int ddpx_bn_join_bwd_merge(const float* part, int B, int C, int M, float* c1, float* c2, void* dgamma,
                                    void* dbeta, int out_bf16, int accumulate, float* sg_p, float* sg_buf, float* sb_p,
                                    float* sb_buf, const float* lr, float mom, float wd, hipStream_t s) {
  if (C < 8 || C % 8 || C > 512 || B < 1 || M < 1 || !part || !c1 || !c2 || ((sg_p || sb_p) && !lr)) return -1;
  return (int)bn::launch_bwd_finalize(part, B, C, M, c1, c2, dgamma, dbeta, out_bf16, accumulate,
                                      SgdArgs{sg_p, sg_buf, nullptr, lr, mom, wd},
                                      SgdArgs{sb_p, sb_buf, nullptr, lr, mom, wd}, s);
}

// Pass 2: dy, and aux = gm (identity) or dy2 (projection, with c2b = S2/M of the shortcut BatchNorm).
DDPX_API int ddpx_bn_join_bwd_apply(const void* g, const void* g2, const void* y, const float* a, const float* b,
                                    const float* mean, const float* rstd, const void* res, const void* y2,
                                    const float* a2, const float* b2, const float* mean2, const float* rstd2,
                                    const float* c1, const float* c2, const float* c2b, int N, int H, int W, int C,
                                    void* dy, void* aux, hipStream_t s) {
  if (!bnjoin::shape_ok(N, H, W, C) || !g || !y || !a || !b || !mean || !rstd || !c1 || !c2 || !dy || !aux) return -1;
  if ((res != nullptr) == (y2 != nullptr) || (y2 && (!a2 || !b2 || !mean2 || !rstd2 || !c2b))) return -1;
  if (!bnjoin::aligned({g, g2, y, res, y2, dy, aux})) return -1;
  const int n = N * H * W * (C / 8);
  const dim3 grid((n + 255) / 256), blk(256);
  if (y2)
    hipLaunchKernelGGL(bnjoin::join_apply_kernel<true>, grid, blk, 0, s, (cus)g, (cus)g2, (cus)y, (cus)y2, a, b, mean,
                       rstd, a2, b2, mean2, rstd2, c1, c2, c2b, n, C, (unsigned short*)dy, (unsigned short*)aux);
  else
    hipLaunchKernelGGL(bnjoin::join_apply_kernel<false>, grid, blk, 0, s, (cus)g, (cus)g2, (cus)y, (cus)res, a, b,
                       mean, rstd, a2, b2, mean2, rstd2, c1, c2, c2b, n, C, (unsigned short*)dy,
                       (unsigned short*)aux);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------------- option-A shortcut / strided second gradient
// Common rules of the ddpx_bn_join_pad* entry points.  x (nullable) [N][Hx][Wx][C/2]: the pad shortcut, with C % 32
// == 0, H == (Hx+1)/2 and W == (Wx+1)/2.  -1: refused shape or operand combination; -2: a pointer that is not 16-B
// aligned; -3: an operand of 2 GiB or more.
static int pad_refusal(int N, int H, int W, int C, const void* x, int Hx, int Wx,
                       std::initializer_list<const void*> ps) {
  if (!bnjoin::shape_ok(N, H, W, C)) return -1;
  if (x && (C % 32 || Hx < 1 || Wx < 1 || (Hx + 1) / 2 != H || (Wx + 1) / 2 != W)) return -1;
  if (!bnjoin::aligned(ps)) return -2;
  const long lim = 1L << 31;
  if ((long)N * H * W * C * 2 >= lim || (x && (long)N * Hx * Wx * (C / 2) * 2 >= lim)) return -3;
  return 0;
}

// Elementwise grid: PPT pixels per thread, 256 / (C/8) pixel lanes per block.
static inline dim3 pad_grid(int P, int C) {
  const int per = 256 / (C / 8) * bnjoin::PPT;
  return dim3((P + per - 1) / per);
}

// out = relu(a*y + b + s), s the option-A shortcut of x.
DDPX_API int ddpx_bn_join_pad(const void* y, const float* a, const float* b, const void* x, int N, int H, int W, int C,
                              int Hx, int Wx, void* out, hipStream_t s) {
  if (!y || !a || !b || !x || !out) return -1;
  if (const int rc = pad_refusal(N, H, W, C, x, Hx, Wx, {y, x, out})) return rc;
  const int P = N * H * W;
  hipLaunchKernelGGL(bnjoin::pad_join_kernel, pad_grid(P, C), dim3(256), 0, s, (cus)y, a, b, (cus)x, P, C,
                     bnjoin::PadGeo{H, W, Hx, Wx}, (unsigned short*)out);
  return (int)hipGetLastError();
}

// Pass-1 blocks of the pad / sub sums: at least 4 pixels per lane, at most 1024 blocks (ddpx_bn_join_blocks' rule).
DDPX_API int ddpx_bn_join_pad_blocks(int N, int H, int W, int C) { return ddpx_bn_join_blocks(N, H, W, C); }

// Pass 1 of the pad join (x) or of the identity join (res) with a strided second gradient: part[B][2][C], B =
// ddpx_bn_join_pad_blocks.  Exactly one of res and x; at most one of g2 (dense) and g2_sub ([N][(H+1)/2][(W+1)/2][C]);
// res needs g2_sub (the identity join without it is ddpx_bn_join_bwd_sums).
DDPX_API int ddpx_bn_join_pad_bwd_sums(const void* g, const void* g2, const void* g2_sub, const void* y, const float* a,
                                       const float* b, const float* mean, const float* rstd, const void* res,
                                       const void* x, int N, int H, int W, int C, int Hx, int Wx, float* part,
                                       hipStream_t s) {
  if (!g || !y || !a || !b || !mean || !rstd || !part) return -1;
  if ((res != nullptr) == (x != nullptr) || (g2 && g2_sub) || (res && !g2_sub)) return -1;
  if (const int rc = pad_refusal(N, H, W, C, x, Hx, Wx, {g, g2, g2_sub, y, res, x})) return rc;
  const int B = ddpx_bn_join_pad_blocks(N, H, W, C);
  const int P = N * H * W;
  const bnjoin::PadGeo q{H, W, Hx, Wx};
  const dim3 grid(B), blk(256);
  if (res)
    hipLaunchKernelGGL((bnjoin::pad_reduce_kernel<false, true>), grid, blk, 0, s, (cus)g, (cus)g2_sub, (cus)y,
                       (cus)res, a, b, mean, rstd, P, C, q, part);
  else if (g2_sub)
    hipLaunchKernelGGL((bnjoin::pad_reduce_kernel<true, true>), grid, blk, 0, s, (cus)g, (cus)g2_sub, (cus)y, (cus)x,
                       a, b, mean, rstd, P, C, q, part);
  else
    hipLaunchKernelGGL((bnjoin::pad_reduce_kernel<true, false>), grid, blk, 0, s, (cus)g, (cus)g2, (cus)y, (cus)x, a,
                       b, mean, rstd, P, C, q, part);
  return (int)hipGetLastError();
}

// Pass 2, operands as pass 1: dy [N][H][W][C], and aux = gs [N][H][W][C/2] (x) or gm [N][H][W][C] (res).
DDPX_API int ddpx_bn_join_pad_bwd_apply(const void* g, const void* g2, const void* g2_sub, const void* y,
                                        const float* a, const float* b, const float* mean, const float* rstd,
                                        const void* res, const void* x, const float* c1, const float* c2, int N, int H,
                                        int W, int C, int Hx, int Wx, void* dy, void* aux, hipStream_t s) {
  if (!g || !y || !a || !b || !mean || !rstd || !c1 || !c2 || !dy || !aux) return -1;
  if ((res != nullptr) == (x != nullptr) || (g2 && g2_sub) || (res && !g2_sub)) return -1;
  if (const int rc = pad_refusal(N, H, W, C, x, Hx, Wx, {g, g2, g2_sub, y, res, x, dy, aux})) return rc;
  const int P = N * H * W;
  const bnjoin::PadGeo q{H, W, Hx, Wx};
  const dim3 grid = pad_grid(P, C), blk(256);
  if (res)
    hipLaunchKernelGGL((bnjoin::pad_apply_kernel<false, true>), grid, blk, 0, s, (cus)g, (cus)g2_sub, (cus)y, (cus)res,
                       a, b, mean, rstd, c1, c2, P, C, q, (unsigned short*)dy, (unsigned short*)aux);
  else if (g2_sub)
    hipLaunchKernelGGL((bnjoin::pad_apply_kernel<true, true>), grid, blk, 0, s, (cus)g, (cus)g2_sub, (cus)y, (cus)x, a,
                       b, mean, rstd, c1, c2, P, C, q, (unsigned short*)dy, (unsigned short*)aux);
  else
    hipLaunchKernelGGL((bnjoin::pad_apply_kernel<true, false>), grid, blk, 0, s, (cus)g, (cus)g2, (cus)y, (cus)x, a, b,
                       mean, rstd, c1, c2, P, C, q, (unsigned short*)dy, (unsigned short*)aux);
  return (int)hipGetLastError();
}
