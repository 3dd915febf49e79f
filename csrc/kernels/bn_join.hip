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
