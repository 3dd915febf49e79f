// ddpx — LARS (You et al., 2017): layer-wise trust ratios fused into the flat SGD update.
//
// Each parameter tensor i gets t_i = trust_coef * |w_i| / (c |g_i| + wd |w_i| + eps) (1 for the excluded and the
// zero-norm ones), c the global clip factor, and its SGD update is scaled by it.  The flat store is cut by the
// host into chunks of at most 32768 elements (grad_norm.hip kChunk), each inside ONE parameter and tagged with its index
// (FlatChunk, ddpx_flat_optim.h):
//
//   lars_sumsq_kernel           one 256-thread workgroup per chunk -> two fp32 partials (w^2, g^2), plain stores
//   lars_segment_reduce_kernel  one wave per parameter: its chunks' partials summed in fp64 in a fixed order
//   lars_trust_kernel           one workgroup: the global gradient norm and clip factor from sq_g[.] (so the
//                               gradient is read once: no separate clip pass), then trust[P]
//   sgd_flat_chunks_kernel      the update, chunk by chunk (stream2's chunk-driven form, ddpx_flat_optim.h);
//                               trust[pid] is one wave-uniform load per workgroup
//
// No float atomics anywhere: every value depends only on the tables, never on the grid or on arrival order.
//
// Summation shape of one partial: exactly grad_sumsq_kernel's (grad_norm.hip) — a thread owns 4 accumulators,
// accumulator k takes the 16-B vectors tid + (4 j + k) * 256 of the chunk with one fma per element (32 elements
// per accumulator for fp32 and bf16, + 1 for the scalar tail on accumulator 0), then (a0 + a1) + (a2 + a3), a
// 6-level butterfly over the wave and (w0 + w1) + (w2 + w3) through LDS.
#include "ddpx_flat_optim.h"

namespace ddpx {
namespace lars {

struct LarsSegment {
  int32_t first;  // into the chunk-order array
  int32_t count;  // chunks of this parameter (0: the parameter has none in this reduction)
};

static int g_update_split = 4;  // workgroups per chunk in the update (ddpx_lars_set_split; benchmarks)

// partials[2 b] = sum w^2, partials[2 b + 1] = sum g^2 over chunk b of the table
template <bool GBF16>
__global__ void __launch_bounds__(256)
lars_sumsq_kernel(const float* __restrict__ w, const void* __restrict__ g, const FlatChunk* __restrict__ table,
                  float* __restrict__ partials) {
  __shared__ float red[2][4];
  const FlatChunk c = table[blockIdx.x];
  const int tid = threadIdx.x;
  const char* gc = reinterpret_cast<const char*>(g) + c.start * (GBF16 ? 2 : 4);
  const float t[2] = {thread_sumsq<false, false>(w + c.start, c.len, tid), thread_sumsq<GBF16, false>(gc, c.len, tid)};
  block_store_sums(t, red, tid, partials + 2 * (size_t)blockIdx.x);
}

// One wave per parameter.  Lane l sums the partials of chunks order[first + l], order[first + l + 64], ... in
// fp64, then a fixed LDS tree: the same bits for the same tables.  sq[pid] = w^2 total, sq[P + pid] = g^2 total.
__global__ void __launch_bounds__(64)
lars_segment_reduce_kernel(const float* __restrict__ partials, const int* __restrict__ order,
                           const LarsSegment* __restrict__ segments, int P, float* __restrict__ sq,
                           int accumulate) {
  __shared__ double red[2][64];
  const int pid = blockIdx.x, lane = threadIdx.x;
  const LarsSegment s = segments[pid];
  double aw = 0.0, ag = 0.0;
  for (int i = lane; i < s.count; i += 64) {
    const size_t b = (size_t)order[s.first + i];
    aw += (double)partials[2 * b];
    ag += (double)partials[2 * b + 1];
  }
  red[0][lane] = aw;
  red[1][lane] = ag;
  __syncthreads();
  for (int o = 32; o > 0; o >>= 1) {
    if (lane < o) {
      red[0][lane] += red[0][lane + o];
      red[1][lane] += red[1][lane + o];
    }
    __syncthreads();
  }
  if (lane < 2) {
    float* dst = sq + (size_t)lane * P + pid;
    *dst = (float)(accumulate ? (double)*dst + red[lane][0] : red[lane][0]);
  }
}

// trust[i] = adapt_i ? trust_coef * wn / (fma(wd, wn, gn) + eps) : 1 with wn = sqrt(sq_w[i]),
// gn = c * sqrt(sq_g[i]), adapt_i = !plain[i] && wn > 0 && gn > 0 (false for a NaN norm).  With clipping
// (max_norm > 0) c is clip_coef_kernel's formula on the fixed-order fp64 sum of sq_g and res3 takes
// {sum of squares, norm, c}; without it c = 1 and res3 may be null.  hyper (may be null): parameter i's wd is
// hyper[i].wd instead of the launch's.
__global__ void __launch_bounds__(256)
lars_trust_kernel(const float* __restrict__ sq, const int* __restrict__ plain, const ParamHyper* __restrict__ hyper,
                  int P, float trust_coef, float wd, float eps, float max_norm, float* __restrict__ res3,
                  float* __restrict__ trust) {
  __shared__ double red[256];
  __shared__ float coef_s;
  const int tid = threadIdx.x;
  float c = 1.f;
  if (max_norm > 0.f) {
    double s = 0.0;
    for (int i = tid; i < P; i += 256) s += (double)sq[P + i];
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) {
      const float total = (float)red[0];
      const float norm = sqrtf(total);
      const float q = max_norm / (norm + 1e-6f);
      const float cc = q > 1.f ? 1.f : q;  // a NaN factor stays NaN, as in torch
      res3[0] = total;
      res3[1] = norm;
      res3[2] = cc;
      coef_s = cc;
    }
    __syncthreads();
    c = coef_s;
  }
  for (int i = tid; i < P; i += 256) {
    const float wn = sqrtf(sq[i]);
    float gn = sqrtf(sq[P + i]);
    if (max_norm > 0.f) gn = c * gn;
    const bool adapt = !plain[i] && wn > 0.f && gn > 0.f;
    const float wdi = hyper ? hyper[i].wd : wd;
    trust[i] = adapt ? (trust_coef * wn) / (fmaf(wdi, wn, gn) + eps) : 1.f;
  }
}

// ddpx_sgd_flat's update (optim_elementwise.hip) over the chunks of a table, with d = t * fma(wd, p, g * gscale)
// (sgd_step<true>, ddpx_flat_optim.h): t == 1.0f gives that kernel's bits.  Streams are non-temporal 16-B accesses.
// HYP: the parameter's row of the hyper table gives wd and scales lr (one more wave-uniform load per workgroup), and
// a null trust table reads as all ones.
template <bool GBF16, bool HYP>
__global__ void __launch_bounds__(256)
sgd_flat_chunks_kernel(float* __restrict__ p, float* __restrict__ buf, const void* __restrict__ g,
                       unsigned short* __restrict__ shadow, const FlatChunk* __restrict__ table,
                       const float* __restrict__ trust, const ParamHyper* __restrict__ hyper,
                       const float* __restrict__ lr_ptr, float lr_host, float mom, float wd, float gscale_host,
                       const float* __restrict__ gscale_ptr, int nesterov, int first) {
  const FlatChunk c = table[blockIdx.x];
  SgdScalars k;
  k.lr = lr_ptr ? *lr_ptr : lr_host;
  k.wd = wd;
  if constexpr (HYP) {
    const ParamHyper h = hyper[c.pid];  // uniform over the workgroup
    k.t = trust ? trust[c.pid] : 1.f;
    k.lr = k.lr * h.lr_mul;
    k.wd = h.wd;
  } else {
    k.t = trust[c.pid];  // uniform over the workgroup
  }
  k.mom = mom;
  k.gscale = gscale_ptr ? gscale_host * *gscale_ptr : gscale_host;
  k.nesterov = nesterov;
  k.first = first;
  float* __restrict__ pc = p + c.start;
  float* __restrict__ bc = buf ? buf + c.start : nullptr;
  unsigned short* __restrict__ sc = shadow ? shadow + c.start : nullptr;
  const int nv = c.len >> 2;
  struct Vecs {
    f32x4 p, g, b;
  };
  auto load = [&](int i) -> Vecs {
    Vecs x;
    x.p = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(pc) + i);
    x.g = load_g4<GBF16>(g, c.start, i);
    x.b = x.p;
    if (mom != 0.f) x.b = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(bc) + i);
    return x;
  };
  auto update = [&](int i, const Vecs& x) {
    f32x4 po, bo;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      float bq = 0.f;
      po[q] = sgd_step<true>(k, x.p[q], x.g[q], x.b[q], bq);
      bo[q] = bq;
    }
    if (mom != 0.f) __builtin_nontemporal_store(bo, reinterpret_cast<f32x4*>(bc) + i);
    __builtin_nontemporal_store(po, reinterpret_cast<f32x4*>(pc) + i);
    if (sc) store_bf4(sc, i, po);
  };
  stream2<int>(blockIdx.y * 256 + threadIdx.x, gridDim.y * 256, nv, load, update);
  // scalar tail (chunk length not a multiple of 4): only a parameter's last chunk has one
  if (blockIdx.y == 0 && (int)threadIdx.x < (c.len & 3)) {
    const int j = (nv << 2) + threadIdx.x;
    float bo = 0.f;
    const float po = sgd_step<true>(k, pc[j], load_g1<GBF16>(g, c.start + j), mom != 0.f ? bc[j] : 0.f, bo);
    if (mom != 0.f) bc[j] = bo;
    pc[j] = po;
    if (sc) sc[j] = f2bf(po);
  }
}

}  // namespace lars
}  // namespace ddpx

using namespace ddpx::lars;

// Workgroups per chunk in ddpx_sgd_flat_chunks (1, 2, 4 or 8); returns the value in force.
DDPX_API int ddpx_lars_set_split(int split) {
  if (split == 1 || split == 2 || split == 4 || split == 8) g_update_split = split;
  return g_update_split;
}

// Two partials per chunk of ``table`` (FlatChunk[n_chunks], device) into partials_out[2 * n_chunks]; the caller
// guarantees that every chunk lies inside both buffers (the host builder checks it against the store's size).
DDPX_API int ddpx_lars_sumsq(const float* w, const void* g, int g_bf16, const void* table, int n_chunks,
                             float* partials_out, hipStream_t s) {
  if (n_chunks <= 0) return 0;
  if (!w || !g || !table || !partials_out) return -1;
  if (ddpx::misaligned(15, w, g, table) || ddpx::misaligned(3, partials_out)) return -1;
  const ddpx::FlatChunk* t = reinterpret_cast<const ddpx::FlatChunk*>(table);
  ddpx::with_flags([&](auto gb) {
    hipLaunchKernelGGL(lars_sumsq_kernel<gb()>, dim3(n_chunks), dim3(256), 0, s, w, g, t, partials_out);
  }, g_bf16 != 0);
  return (int)hipGetLastError();
}

// sq[0 .. P) (=|+=) per-parameter sums of w^2, sq[P .. 2P) of g^2, from the partials of the chunks
// order[segments[pid].first ...] (segments: LarsSegment[P]).
DDPX_API int ddpx_lars_segment_reduce(const float* partials, const int* order, const void* segments, int P,
                                      float* sq, int accumulate, hipStream_t s) {
  if (P <= 0) return 0;
  if (!partials || !order || !segments || !sq) return -1;
  if (ddpx::misaligned(7, segments) || ddpx::misaligned(3, partials, order, sq)) return -1;
  hipLaunchKernelGGL(lars_segment_reduce_kernel, dim3(P), dim3(64), 0, s, partials, order,
                     reinterpret_cast<const LarsSegment*>(segments), P, sq, accumulate);
  return (int)hipGetLastError();
}

// trust[P] from sq[2P]; plain[i] != 0: parameter i keeps plain SGD.  max_norm > 0: also the global clip factor
// into res3 = {sum of squares, norm, factor} (required then), which scales every gradient norm.  hyper (may be
// null): ParamHyper[P] (device, 8-B aligned); parameter i's ratio is trust_coef * wn / (gn + hyper[i].wd * wn + eps)
// and weight_decay is ignored.
DDPX_API int ddpx_lars_trust(const float* sq, const int* plain, const void* hyper, int P, float trust_coef,
                             float weight_decay, float eps, float max_norm, float* res3, float* trust,
                             hipStream_t s) {
  if (P <= 0) return 0;
  if (!sq || !plain || !trust) return -1;
  if (ddpx::misaligned(7, hyper)) return -1;
  if (max_norm > 0.f && !res3) return -1;
  if (!(max_norm > 0.f)) max_norm = 0.f;
  hipLaunchKernelGGL(lars_trust_kernel, dim3(1), dim3(256), 0, s, sq, plain,
                     reinterpret_cast<const ddpx::ParamHyper*>(hyper), P, trust_coef, hyper ? 0.f : weight_decay, eps,
                     max_norm, res3, trust);
  return (int)hipGetLastError();
}

// The SGD update over ``n_chunks`` chunks of ``table``.  p, buf, g, shadow are the WHOLE store's buffers (chunk
// starts are flat indices); buf may be null when momentum == 0, shadow may be null.  lr_dev (device scalar) wins
// over lr_host; clip_dev: optional device factor on the gradient, on top of grad_scale.
// hyper == null: LARS's update, every parameter's step scaled by trust[pid] (required).  hyper: ParamHyper[P]
// (device, 8-B aligned); the chunk's parameter takes wd = hyper[pid].wd (weight_decay is ignored) and
// lr = lr * hyper[pid].lr_mul, and trust may be null (plain SGD: every ratio 1).  Rows {1, wd} give the bits of
// hyper == null with that weight_decay.
DDPX_API int ddpx_sgd_flat_chunks(float* p, float* buf, const void* g, int g_bf16, void* shadow, const void* table,
                                  int n_chunks, const float* trust, const void* hyper, const float* lr_dev,
                                  float lr_host, float momentum, float weight_decay, float grad_scale,
                                  const float* clip_dev, int nesterov, int first, hipStream_t s) {
  if (n_chunks <= 0) return 0;
  if (!p || !g || !table || (!hyper && !trust)) return -1;
  if (momentum != 0.f && !buf) return -1;
  if (ddpx::misaligned(15, p, buf, table) || ddpx::misaligned(g_bf16 ? 7 : 15, g) ||
      ddpx::misaligned(7, shadow, hyper) || ddpx::misaligned(3, trust, lr_dev, clip_dev))
    return -1;
  const ddpx::FlatChunk* t = reinterpret_cast<const ddpx::FlatChunk*>(table);
  const ddpx::ParamHyper* h = reinterpret_cast<const ddpx::ParamHyper*>(hyper);
  const dim3 grid(n_chunks, g_update_split), block(256);
  ddpx::with_flags([&](auto gb, auto hyp) {
    hipLaunchKernelGGL((sgd_flat_chunks_kernel<gb(), hyp()>), grid, block, 0, s, p, buf, g, (unsigned short*)shadow,
                       t, trust, h, lr_dev, lr_host, momentum, hyp() ? 0.f : weight_decay, grad_scale, clip_dev,
                       nesterov, first);
  }, g_bf16 != 0, hyper != nullptr);
  return (int)hipGetLastError();
}
