// ddpx — what the fp32 path's translation units (f32_gemm.hip, f32_bn.hip, f32_head.hip) share.
#pragma once

namespace ddpx {
namespace f32k {

// workgroups of b threads (or chunks of b rows) that cover n
static inline unsigned nblk(long n, int b = 256) { return (unsigned)((n + b - 1) / b); }

}  // namespace f32k
}  // namespace ddpx
