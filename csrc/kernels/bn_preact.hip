// ddpx — the shortcut add of a pre-activation residual block (He et al. 2016, "Identity Mappings in Deep Residual
// Networks") on NHWC bf16, with the BatchNorm statistics of the sum.
//
//   z = bf16(float(y) + float(s))      y: raw output of the block's second 3x3 convolution, s: the shortcut (the
//                                      previous block's z, or the raw output of the 1x1 / stride-2 projection)
//
// A pre-activation block normalises the SUM: the next BatchNorm reads z, so the (mean, M2) that the convolution
// epilogue could produce are those of the wrong tensor.  Composed, the block would cost an add pass, a statistics
// pass over z and (evaluation) an apply pass.  Here one launch does the add and
//   training  writes per-row-tile (mean, M2) of the STORED, rounded z in the layout [T][2][C] of the convolution's
//             EPI_BNSTAT_BF16 epilogue, tile t = rows [t*BM, min(M, (t+1)*BM)): ddpx_bn_finalize / ddpx_bn_local_stats
//             merge them as they merge the epilogue's, no new merge kernel;
//   eval      (a, b are known before the pass) also writes act = bf16(relu(fmaf(a, z, b))) from the rounded z, the
//             expression of bn_pool.hip's apply_kernel on the stored z: one pass instead of two.
// z may alias y (every thread reads its 16 bytes of y before it writes them).
//
// Work split.  A workgroup owns one tile of BM rows over all C channels; a thread owns one 8-channel group (16-B loads
// and stores) of one pixel lane: 256 threads = (G = C/8 groups) x (lanes = 256/G pixel lanes), threads past lanes*G
// idle.  Row i*lanes + q of the tile belongs to lane q, so every step of a workgroup reads one contiguous piece of
// lanes*C*2 bytes (4 KB when G divides 256) of each operand.  A thread issues the loads of up to UNR steps before it
// touches the first value: the smallest layer of the network ([512,4,4,512]: 256 tiles, one per CU) has no second
// workgroup on its CU to hide the latency.
//
// Statistics.  Each thread keeps a running Welford (n, mean[8], M2[8]) in registers over its rows (n is the same for
// the 8 channels: one reciprocal per step); the lanes' states meet in LDS ([lanes][C], channel-contiguous: conflict
// free) and are merged with Chan's formula in lane order by up to 8 threads per channel (contiguous lane ranges,
// then the ranges in order).  The lane counts follow from the tile's row count, so only mean and M2 travel.  Fixed
// order, no atomics: two runs give the same bits.
//
// Tile rows: BM = 32 up to 65536 rows (ResNet-18's 8x8 and 4x4 stages at batch 512: [512,4,4,512] = 8192 rows gives
// 256 tiles, one per CU), else 128 (at most 4096 tiles at [512,32,32,64], VGG's largest merge).  Unmeasured choice.
//
// Build figures (gfx950, -O3, kernel-resource-usage): README "Pre-activation ResNet-18/34".
#include <climits>
#include <cstdint>

#include "ddpx_bn.h"

namespace ddpx {
namespace preact {

using bn::chan_merge;
using bn::pack8;
using bn::unpack8;

constexpr int UNR = 4;   // steps whose loads are in flight together
constexpr int SMAX = 8;  // merge threads per channel

template <bool EVAL>
__global__ void __launch_bounds__(256)
add_kernel(const unsigned short* y, const unsigned short* __restrict__ s, unsigned short* z,
           float* __restrict__ stats, const float* __restrict__ a, const float* __restrict__ b,
           unsigned short* __restrict__ act, int M, int C, int BM) {
  __shared__ float red[2][256 * 8];   // [mean | M2][lane * C + c]
  __shared__ float rng[3][256];       // [n | mean | M2][range * C + c], C <= 128
  const int G = C / 8, lanes = 256 / G;
  const int g = threadIdx.x % G, pl = threadIdx.x / G;
  const int row0 = blockIdx.x * BM;
  const int rows = min(BM, M - row0);
  float mu[8], m2[8], av[8], bv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = m2[j] = 0.f;
    av[j] = EVAL ? a[g * 8 + j] : 0.f;
    bv[j] = EVAL ? b[g * 8 + j] : 0.f;
  }
  if (pl < lanes) {
    int n = 0;
    for (int r0 = pl; r0 < rows; r0 += UNR * lanes) {
      u32x4 vy[UNR], vs[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int r = r0 + u * lanes;
        if (r < rows) {
          const size_t off = (size_t)(row0 + r) * C + g * 8;
          vy[u] = *reinterpret_cast<const u32x4*>(y + off);
          vs[u] = *reinterpret_cast<const u32x4*>(s + off);
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int r = r0 + u * lanes;
        if (r < rows) {
          const size_t off = (size_t)(row0 + r) * C + g * 8;
          float f[8], so[8];
          unpack8(vy[u], f);
          unpack8(vs[u], so);
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] += so[j];
          const u32x4 zv = pack8(f);
          *reinterpret_cast<u32x4*>(z + off) = zv;
          unpack8(zv, f);  // the stored values: what the next BatchNorm reads
          if (EVAL) {
#pragma unroll
            for (int j = 0; j < 8; ++j) f[j] = fmaxf(fmaf(av[j], f[j], bv[j]), 0.f);
            *reinterpret_cast<u32x4*>(act + off) = pack8(f);
          } else {
            const float inv = 1.f / (float)(++n);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const float d = f[j] - mu[j];
              mu[j] = fmaf(d, inv, mu[j]);
              m2[j] = fmaf(d, f[j] - mu[j], m2[j]);
            }
          }
        }
      }
    }
  }
  if (EVAL) return;
#pragma unroll
  for (int j = 0; j < 8; ++j) {  // thread (pl, g) -> [pl * C + g * 8 + j]
    red[0][threadIdx.x * 8 + j] = mu[j];
    red[1][threadIdx.x * 8 + j] = m2[j];
  }
  __syncthreads();
  // lane q holds rows q, q + lanes, ... of the tile
  const int S = max(1, min(SMAX, 256 / C));  // lane ranges per channel (1 when C > 128: S * C <= 256)
  const int chunk = (lanes + S - 1) / S;
  float* const st = stats + (size_t)blockIdx.x * 2 * C;
  for (int i = threadIdx.x; i < S * C; i += 256) {  // more than one trip only with S == 1 (C > 256)
    const int c = i % C, sp = i / C;
    float n = 0.f, m = 0.f, q2 = 0.f;
    const int qe = min(lanes, (sp + 1) * chunk);
    for (int q = sp * chunk; q < qe; ++q) {
      const int nq = q < rows ? (rows - q + lanes - 1) / lanes : 0;
      chan_merge(n, m, q2, (float)nq, red[0][q * C + c], red[1][q * C + c]);
    }
    if (S == 1) {
      st[c] = m;
      st[C + c] = q2;
    } else {
      rng[0][i] = n;
      rng[1][i] = m;
      rng[2][i] = q2;
    }
  }
  if (S == 1) return;
  __syncthreads();
  if (threadIdx.x < C) {
    const int c = threadIdx.x;
    float n = 0.f, m = 0.f, q2 = 0.f;
    for (int sp = 0; sp < S; ++sp) chan_merge(n, m, q2, rng[0][sp * C + c], rng[1][sp * C + c], rng[2][sp * C + c]);
    st[c] = m;
    st[C + c] = q2;
  }
}

// C % 8 == 0, 8 <= C <= 512; rows in an int
static inline bool shape_ok(int N, int H, int W, int C) {
  if (N < 1 || H < 1 || W < 1 || C < 8 || C % 8 || C > 512) return false;
  return (long)N * H * W <= (long)INT_MAX - 256;
}

}  // namespace preact
}  // namespace ddpx

using namespace ddpx;

// Rows per statistics tile (BM) and the tile count T = ceil(N*H*W / BM); -1: refused shape.
DDPX_API int ddpx_preact_add_tile_rows(int N, int H, int W, int C) {
  if (!preact::shape_ok(N, H, W, C)) return -1;
  return (long)N * H * W <= 65536 ? 32 : 128;
}

DDPX_API int ddpx_preact_add_tiles(int N, int H, int W, int C) {
  const int BM = ddpx_preact_add_tile_rows(N, H, W, C);
  if (BM < 0) return -1;
  return (int)(((long)N * H * W + BM - 1) / BM);
}

// z = bf16(y + s) over [N*H*W][C] (z may be y).  Training (stats [T][2][C] given; a, b, act null): the tiles' (mean,
// M2) of the stored z.  Eval (stats null; a, b, act given): act = bf16(relu(a*z + b)) in the same pass.
// -1: refused shape or operand combination; -2: a pointer that is not 16-B aligned; -3: an operand of 2 GiB or more.
DDPX_API int ddpx_preact_add(const void* y, const void* s, void* z, float* stats, const float* a, const float* b,
                             void* act, int N, int H, int W, int C, hipStream_t stream) {
  if (!preact::shape_ok(N, H, W, C) || !y || !s || !z) return -1;
  const bool eval = stats == nullptr;
  if (eval ? (!a || !b || !act) : (a || b || act)) return -1;
  if (((uintptr_t)y | (uintptr_t)s | (uintptr_t)z | (uintptr_t)act) & 15) return -2;
  if ((long)N * H * W * C * 2 >= (1L << 31)) return -3;
  const int M = N * H * W;
  const int BM = ddpx_preact_add_tile_rows(N, H, W, C);
  const dim3 grid((M + BM - 1) / BM), blk(256);
  typedef const unsigned short* cus;
  if (eval)
    hipLaunchKernelGGL(preact::add_kernel<true>, grid, blk, 0, stream, (cus)y, (cus)s, (unsigned short*)z, stats, a, b,
                       (unsigned short*)act, M, C, BM);
  else
    hipLaunchKernelGGL(preact::add_kernel<false>, grid, blk, 0, stream, (cus)y, (cus)s, (unsigned short*)z, stats, a,
                       b, (unsigned short*)act, M, C, BM);
  return (int)hipGetLastError();
}
