// ddpx — MI355X (gfx950 / CDNA4): validation metrics of a batch of fp32 logits in one launch.
//
// ddpx_eval_metrics: per row m < m_valid, in fp32 (z = the logits, or with a second operand 0.5 * (z1 + z2)),
//   lse  = max + log(sum_c exp(z_c - max)),  loss = lse - z_t
//   rank = #{c : z_c > z_t} + #{c < t : z_c == z_t}      (0: the lowest-class argmax is the target, as ddpx_accuracy)
// and into the caller's accumulators (the caller zeroes them; a launch adds):
//   counts[0] += #{rank == 0}, counts[1] += #{rank < k}, counts[2] += m_valid     (integer atomics)
//   *loss_sum += sum_m loss_m                                                      (fp64, fixed order)
// A row whose target lies outside [0, C) reads no logit, is a miss and adds no loss.  Rows m >= m_valid (the
// padding of a sharded last batch) are read by nobody.
//
// Work layout: G lanes per row, striding the classes: G = 16 at C <= 16 (four rows per wave), G = 64 above (one wave
// per row); 256 threads = 256 / G rows per workgroup.  Group reductions are xor butterflies inside aligned G-lane
// groups (DPP / swizzle moves, no LDS).  The row losses go out write-through (agent-scope stores), every storing
// wave drains them, and the workgroup takes the launch's agent-scope ticket: the hand-off of head_xent.hip's batch
// loss.  The last workgroup to arrive sums the m_valid row losses in fp64, thread t rows t, t + 256, ... in
// ascending order, then a fixed butterfly and the four wave sums in wave order: the same bits whichever workgroup
// is last.  It resets the ticket.  No floating-point atomics.
#include "ddpx_common.h"

namespace ddpx {

template <int G>
__device__ __forceinline__ float group_max(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
template <int G>
__device__ __forceinline__ int group_sum(int v) {
#pragma unroll
  for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// TWO: every logit is the mean of two operands (flip test-time augmentation: the logits of a batch and of its mirror
// image), 0.5f * (z1 + z2) in fp32: one rounded add and an exact halving.  Loss, rank and counts follow as for one.
template <int G, bool TWO>
__global__ void __launch_bounds__(256)
eval_metrics_kernel(const float* __restrict__ logits, const float* __restrict__ logits2, int ld,
                    const int64_t* __restrict__ tgt, int m_valid, int C, int k, int* __restrict__ counts,
                    double* __restrict__ loss_sum, float* loss_rows, int* ticket) {
  constexpr int R = 256 / G;  // rows per workgroup
  __shared__ int cnt[2];
  __shared__ int flag;
  __shared__ double wsum[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int j = t % G;
  const int m = blockIdx.x * R + t / G;
  if (t < 2) cnt[t] = 0;
  __syncthreads();

  const bool ok = m < m_valid;
  const int64_t t64 = ok ? tgt[m] : (int64_t)-1;
  const bool in = t64 >= 0 && t64 < (int64_t)C;  // (false for rows past m_valid)
  const int tg = in ? (int)t64 : 0;
  const float* z = logits + (size_t)(ok ? m : 0) * ld;
  const float* z2 = TWO ? logits2 + (size_t)(ok ? m : 0) * ld : nullptr;
  auto zat = [&](int c) { return TWO ? 0.5f * (z[c] + z2[c]) : z[c]; };
  const float zt = in ? zat(tg) : 0.f;
  float mx = -INFINITY;
  if (in)
    for (int c = j; c < C; c += G) mx = fmaxf(mx, zat(c));
  mx = group_max<G>(mx);
  float se = 0.f;
  int rank = 0;
  if (in)
    for (int c = j; c < C; c += G) {
      const float v = zat(c);
      se += __expf(v - mx);
      rank += (v > zt || (v == zt && c < tg)) ? 1 : 0;
    }
  se = group_sum<G>(se);
  rank = group_sum<G>(rank);
  const bool lead = ok && j == 0;
  if (lead)  // (0 for a row with an out-of-range target: it adds no loss)
    __hip_atomic_store(loss_rows + m, in ? mx + __logf(se) - zt : 0.f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long b1 = __ballot(lead && in && rank == 0);
  const unsigned long long bk = __ballot(lead && in && rank < k);
  if (lane == 0) {
    if (b1) atomicAdd(&cnt[0], __popcll(b1));
    if (bk) atomicAdd(&cnt[1], __popcll(bk));
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its write-through stores
  __syncthreads();
  if (t < 2 && cnt[t]) atomicAdd(counts + t, cnt[t]);  // integer: deterministic
  if (t == 2) atomicAdd(counts + 2, min(R, m_valid - (int)blockIdx.x * R));
  if (t == 0)
    flag = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
  __syncthreads();
  if (!flag) return;

  // out-of-range lanes read zeros (buffer bounds check); sc1 loads, as the stores
  const __amdgpu_buffer_rsrc_t rl =
      __builtin_amdgcn_make_buffer_rsrc((void*)loss_rows, 0, (unsigned)m_valid * 4u, 0x00020000);
  double s = 0.0;
  for (int i0 = 0; i0 < m_valid; i0 += 256 * 4) {
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      v[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rl, (i0 + q * 256 + t) * 4, 0, 16));
#pragma unroll
    for (int q = 0; q < 4; ++q) s += (double)v[q];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) wsum[wave] = s;
  __syncthreads();
  if (t == 0) {
    *loss_sum += ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

}  // namespace ddpx

using namespace ddpx;

// Scratch (floats): the launch's row losses [M]; tickets (ints): one, zero between launches.
DDPX_API int64_t ddpx_eval_metrics_scratch(int M) { return M > 0 ? M : 1; }
DDPX_API int64_t ddpx_eval_metrics_tickets(int M) { (void)M; return 1; }

template <int G>
static void launch_eval_metrics(int blocks, const float* logits, const float* logits2, int ld, const int64_t* tgt,
                                int m_valid, int C, int k, int* counts, double* loss_sum, float* scratch, int* tickets,
                                hipStream_t s) {
  if (logits2)
    hipLaunchKernelGGL((eval_metrics_kernel<G, true>), dim3(blocks), dim3(256), 0, s, logits, logits2, ld, tgt, m_valid,
                       C, k, counts, loss_sum, scratch, tickets);
  else
    hipLaunchKernelGGL((eval_metrics_kernel<G, false>), dim3(blocks), dim3(256), 0, s, logits, logits2, ld, tgt,
                       m_valid, C, k, counts, loss_sum, scratch, tickets);
}

// logits2 (nullable; [M][ld] as logits): the second operand of the mean, see the kernel.  With a null pointer the
// launch is ddpx_eval_metrics's.
DDPX_API int ddpx_eval_metrics2(const float* logits, const float* logits2, int ld, const int64_t* tgt, int M,
                                int m_valid, int C, int k, int* counts, double* loss_sum, float* scratch, int* tickets,
                                hipStream_t s) {
  if (M < 0 || C < 1 || ld < C) return -1;
  if (k < 1 || k > C || m_valid < 0 || m_valid > M) return -2;
  if (!counts || !loss_sum || !scratch || !tickets) return -3;
  if (m_valid == 0) return 0;
  if (!logits || !tgt) return -3;
  if (m_valid > 0x1fffffff) return -1;  // the row losses' buffer offsets are 32-bit byte counts
  if (C <= 16)
    launch_eval_metrics<16>((m_valid + 15) / 16, logits, logits2, ld, tgt, m_valid, C, k, counts, loss_sum, scratch,
                            tickets, s);
  else
    launch_eval_metrics<64>((m_valid + 3) / 4, logits, logits2, ld, tgt, m_valid, C, k, counts, loss_sum, scratch,
                            tickets, s);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_eval_metrics(const float* logits, int ld, const int64_t* tgt, int M, int m_valid, int C, int k,
                               int* counts, double* loss_sum, float* scratch, int* tickets, hipStream_t s) {
  return ddpx_eval_metrics2(logits, nullptr, ld, tgt, M, m_valid, C, k, counts, loss_sum, scratch, tickets, s);
}
