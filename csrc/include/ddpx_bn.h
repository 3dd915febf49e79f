// ddpx — what the BatchNorm kernel files share (bn_pool.hip, bn_join.hip, bn_preact.hip): the 8-channel bf16 <-> fp32
// vector helpers, the second-gradient add, Chan's statistics merge, and the host launch of the backward-sums merge.
#pragma once

#include "ddpx_common.h"

namespace ddpx {
namespace bn {

__device__ __forceinline__ void unpack8(const u32x4 v, float (&f)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = __uint_as_float(v[j] << 16);
    f[2 * j + 1] = __uint_as_float(v[j] & 0xffff0000u);
  }
}

__device__ __forceinline__ u32x4 pack8(const float (&f)[8]) {
  return (u32x4){pack_bf2(f[0], f[1]), pack_bf2(f[2], f[3]), pack_bf2(f[4], f[5]), pack_bf2(f[6], f[7])};
}

// gout2 (nullable, same shape as gout): a second gradient of the block's output (the skip connection of the residual
// block above); the gradient is gout + gout2, summed in fp32 and never stored.
__device__ __forceinline__ void add_grad2(const unsigned short* __restrict__ gout2, size_t off, float (&gg)[8]) {
  if (!gout2) return;
  float g2[8];
  unpack8(*reinterpret_cast<const u32x4*>(gout2 + off), g2);
#pragma unroll
  for (int j = 0; j < 8; ++j) gg[j] += g2[j];
}

// Chan et al.'s merge of two (count, mean, M2) states: (n, mean, m2) <- (n, mean, m2) + (nb, meanb, m2b).
__device__ __forceinline__ void chan_merge(float& n, float& mean, float& m2, float nb, float meanb, float m2b) {
  if (nb <= 0.f) return;  // (a trailing epilogue part wholly past M: min(BM, M - t*BM) < 0)
  if (n == 0.f) { n = nb; mean = meanb; m2 = m2b; return; }
  const float nn = n + nb;
  const float d = meanb - mean;
  mean += d * (nb / nn);
  m2 += m2b + d * d * (n * nb / nn);
  n = nn;
}

// Merge of pass-1 partials part[B][2][C] (bn_pool.hip): c1 = sum0 / M, c2 = sum1 / M, dbeta = sum0 and dgamma = sum1
// stored (fp32 / bf16, = or +=) or applied as their fused SGD update.  Fixed order: deterministic.
hipError_t launch_bwd_finalize(const float* part, int B, int C, int M, float* c1, float* c2, void* dgamma, void* dbeta,
                               int out_bf16, int accumulate, SgdArgs sg, SgdArgs sb, hipStream_t s);

}  // namespace bn
}  // namespace ddpx
