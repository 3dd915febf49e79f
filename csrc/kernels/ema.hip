// ddpx — exponential moving average of the weights over the flat store (ddpx.optim.WeightEMA).
//
// The average is one more fp32 buffer laid out like the master.  After a step's updates one streaming pass moves
// it towards the new weights:
//   e = e + (p - e) * w                               (lerp form; w = 1 - decay)
// 12 B per weight (8 read, 4 written).  w is a device scalar that ema_advance_kernel produces once per optimizer
// step from two device counters {steps, updates}, so every launch of a step (one per shard under ZeRO-1) reads the
// same w and a replayed HIP graph needs no host write.
//
// Roundings per element (the GPU test's bound counts them): p - e, then one fma: 2.  The product is never left to
// contraction.
//
// w == 0 means "no update in this step" (WeightEMA(every=K) on K - 1 steps of K): the kernel returns after the one
// scalar load and touches nothing, so the average also stays bit-exact where p holds inf or NaN.
//
// Cache policy: plain loads and stores on both streams.  What is documented for gfx950 leaves little to choose: a
// non-temporal load bypasses the L1 only and is served by the L2 like a plain one (and was measured 0-3 % slower
// at 16 B), and plain and non-temporal stores both keep the line in the L2.  Neither stream has reuse to protect:
// e is read once and written once per step, p was written by the update just before and is read by nothing else
// before the next forward reads its bf16 shadow.  The first guess here was "non-temporal e as the state streams of
// sgd_flat_kernel / adamw_flat_kernel, plain p"; benchmarks/ema_bw.py (profiles/r14_ema), windows interleaved
// in one job, did not confirm it: over the toy MLP's 29.4 M weights all-plain took 52.7 us, that guess 54.6 us and
// all-non-temporal 57.4 us (each kernel's own window spread about 1 %; a second job: 51.9, 53.4, 59.3 us); over the
// wide MLP's 319 M they took 758, 761 and 747 us (second job: 810, 809, 801 us).  All-plain wins on the store the
// flagship runs on and is within 1.5 % of the best on the wide one.  ddpx_ema_set_nt switches either stream so
// that the benchmark keeps comparing them.
#include "ddpx_flat_optim.h"

#pragma clang fp contract(off)

namespace ddpx {

__device__ __forceinline__ float ema_apply(float e, float p, float w) { return fmaf(p - e, w, e); }

// stream2's flat form (ddpx_flat_optim.h).
template <bool NT_E, bool NT_P>
__global__ void __launch_bounds__(256)
ema_flat_kernel(float* __restrict__ e, const float* __restrict__ p, int64_t n, const float* __restrict__ w_ptr,
                float w_host) {
  const float w = w_ptr ? *w_ptr : w_host;
  if (w == 0.f) return;  // no update in this step: nothing is read or written
  const int64_t nv = n >> 2;
  struct Vecs {
    f32x4 e, p;
  };
  auto load = [&](int64_t i) -> Vecs {
    return {ld16<NT_E>(reinterpret_cast<const f32x4*>(e) + i), ld16<NT_P>(reinterpret_cast<const f32x4*>(p) + i)};
  };
  auto update = [&](int64_t i, Vecs x) {
#pragma unroll
    for (int q = 0; q < 4; ++q) x.e[q] = ema_apply(x.e[q], x.p[q], w);
    if constexpr (NT_E) __builtin_nontemporal_store(x.e, reinterpret_cast<f32x4*>(e) + i);
    else reinterpret_cast<f32x4*>(e)[i] = x.e;
  };
  stream2<int64_t>((int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x, nv, load, update);
  // scalar tail (n not a multiple of 4)
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const int64_t j = (nv << 2) + threadIdx.x;
    e[j] = ema_apply(e[j], p[j], w);
  }
}

// bit 0: non-temporal load / store of the average; bit 1: non-temporal load of the weights (ddpx_ema_set_nt)
static int g_ema_nt = 0;

// Device counters and the step's weight, one thread in fp64 (the twin of adamw_advance_kernel):
//   s = ++steps;  s % every != 0: w = 0 (no update in this step)
//   else u = ++updates, d = warmup ? min(decay, (1 + u) / (10 + u)) : decay, every > 1: d = d^every,
//   w = (float)(1 - d), rounded once.
__global__ void ema_advance_kernel(int* __restrict__ counters, double decay, int warmup, int every,
                                   float* __restrict__ w_out) {
  const int s = counters[0] + 1;
  counters[0] = s;
  if (s % every != 0) {
    *w_out = 0.f;
    return;
  }
  const int u = counters[1] + 1;
  counters[1] = u;
  double d = decay;
  if (warmup) {
    const double r = (1.0 + (double)u) / (10.0 + (double)u);
    d = r < d ? r : d;
  }
  if (every > 1) d = pow(d, (double)every);
  *w_out = (float)(1.0 - d);
}

}  // namespace ddpx

using namespace ddpx;

// ema[i] += (p[i] - ema[i]) * w over n elements; w_dev (device scalar) wins over w_host.  w == 0: nothing is touched.
DDPX_API int ddpx_ema_flat(float* ema, const float* p, int64_t n, const float* w_dev, float w_host, hipStream_t s) {
  if (n <= 0) return 0;
  if (!ema || !p) return -1;
  if (misaligned(15, ema, p) || misaligned(3, w_dev)) return -1;
  const dim3 grid(flat_grid_for((n >> 2) + 1)), block(kFlatBlock);
  with_flags([&](auto nt_e, auto nt_p) {
    hipLaunchKernelGGL((ema_flat_kernel<nt_e(), nt_p()>), grid, block, 0, s, ema, p, n, w_dev, w_host);
  }, (g_ema_nt & 1) != 0, (g_ema_nt & 2) != 0);
  return (int)hipGetLastError();
}

// Cache policy of ddpx_ema_flat's streams (0 .. 3, see g_ema_nt; benchmarks); returns the value in force.
DDPX_API int ddpx_ema_set_nt(int mask) {
  if (mask >= 0 && mask <= 3) g_ema_nt = mask;
  return g_ema_nt;
}

// Threads of a full grid: a thread's loop runs a second time from 2 * this many 16-B vectors on (tests).
DDPX_API int ddpx_ema_max_threads(void) { return kFlatMaxBlocks * kFlatBlock; }

DDPX_API int ddpx_ema_advance(int* counters, double decay, int warmup, int every, float* w_out, hipStream_t s) {
  if (!counters || !w_out) return -1;
  if (!(decay >= 0.0 && decay < 1.0) || every < 1) return -1;
  hipLaunchKernelGGL(ema_advance_kernel, dim3(1), dim3(1), 0, s, counters, decay, warmup, every, w_out);
  return (int)hipGetLastError();
}
