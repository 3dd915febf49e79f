// ddpx — what the fp32 path's translation units (f32_gemm.hip, f32_conv_s2.hip, f32_bn.hip, f32_head.hip) share.
#pragma once

#include "ddpx_common.h"

namespace ddpx {
namespace f32k {

// workgroups of b threads (or chunks of b rows) that cover n
static inline unsigned nblk(long n, int b = 256) { return (unsigned)((n + b - 1) / b); }

// ------------------------------------------------------------------ the LDS-DMA cores' operand images
// (f32_gemm.hip's gemm_f32_dma_kernel and f32_conv_s2.hip's conv_s2_kernel stage and read the same images)
enum Mode { DENSE_KC = 0, DENSE_OC = 1, IM2COL_KC = 2, IM2COL_OC = 3 };

constexpr int BK = 16, NT = 256;  // a K-step is 16 k: a KC image row is 4 float4

// LDS images (16-B chunks = 4 floats, lane-linear DMA writes, bank swizzles applied to the SOURCE chunk):
//   KC operand  [rows][16 k]   row = 64 B, chunk c at c ^ ((row >> 2) & 3)        (conflict-free b32 fragment reads)
//   OC operand  [16 k][rows]   row = 4*rows B, chunk c at c ^ (4 * (k & 3))        (rows >= 64)
constexpr unsigned kOOB32 = 0x80000000u;

// LDS chunk position pc of a tile's image -> the source chunk it holds: (row, chunk kc of the row's 16 k) of a KC
// image, (k-row, chunk oc of its ROWS outer elements) of an OC image
__device__ __forceinline__ void f32_kc_chunk(int pc, int& row, int& kc) {
  row = pc >> 2;
  const int cpos = pc & 3;
  kc = cpos ^ ((row >> 2) & 3);
}
template <int ROWS>
__device__ __forceinline__ void f32_oc_chunk(int pc, int& krow, int& oc) {
  constexpr int CPR = ROWS / 4;  // chunks per k-row
  krow = pc / CPR;
  const int cpos = pc % CPR;
  oc = cpos ^ (4 * (krow & 3));
}

template <int MODE, int ROWS>
__device__ __forceinline__ float f32_frag(const char* img, int r, int k) {
  constexpr bool KC = (MODE == DENSE_KC || MODE == IM2COL_KC);
  int byte;
  if constexpr (KC) byte = r * 64 + ((((k >> 2) ^ ((r >> 2) & 3)) << 4) | ((k & 3) << 2));
  else byte = k * (ROWS * 4) + ((((r >> 2) ^ (4 * (k & 3)))) << 4) + ((r & 3) << 2);
  return *reinterpret_cast<const float*>(img + byte);
}

// The accumulator tile staged through the idle LDS ring (RING bytes) as T[r * TLD + col], in EH row parts of BMH
// rows (two where the whole tile does not fit: each part is then the rows of the waves wm == part), so that the
// epilogue can walk it in rows: Q 16-B column quads x RSTEP rows per pass of the 256 threads, NV passes per part.
template <int BM, int BN, int RING>
struct TileStage {
  static constexpr int TLD = BN + 4;
  static constexpr int EH = (BM * TLD * 4 <= RING) ? 1 : 2;
  static constexpr int BMH = BM / EH;
  static_assert(BMH * TLD * 4 <= RING, "epilogue staging does not fit the ring");
  static constexpr int Q = BN / 4, RSTEP = NT / Q, NV = BMH / RSTEP;

  // part h of acc -> T, between two barriers: whoever read the ring (h = 0: the K loop, the statistics scratch) or
  // the previous part is done before the stores, and the part is complete after them
  static __device__ __forceinline__ void put(float* T, const f32x4 (&acc)[BM / 32][BN / 32], int h, int wm, int wn,
                                             int lr, int lc) {
    __syncthreads();
    if (wm == h || EH == 1) {
#pragma unroll
      for (int i = 0; i < BM / 32; ++i)
#pragma unroll
        for (int j = 0; j < BN / 32; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = (EH == 1 ? wm * (BM / 2) : 0) + i * 16 + lr * 4 + e;
            T[r * TLD + wn * (BN / 2) + j * 16 + lc] = acc[i][j][e];
          }
    }
    __syncthreads();
  }
};

}  // namespace f32k
}  // namespace ddpx
