// ddpx — global gradient norm over the flat gradient buffer (clip_grad_norm_).
//
// The flat store keeps every gradient in one fp32 or bf16 buffer whose parameters start 64-element
// aligned, with padding in between that nobody writes.  The host cuts the parameters (intersected with
// the flat ranges this rank owns: the whole store, a DDP bucket, a ZeRO-1 shard) into chunks of at most
// kChunk elements, each inside ONE parameter, and the norm is computed in the store-and-sum form:
//
//   grad_sumsq_kernel     one 256-thread workgroup per chunk -> one fp32 partial per chunk (plain store)
//   sumsq_reduce_kernel   one workgroup sums the partials in a fixed order in fp64 -> device fp32 scalar
//   clip_coef_kernel      norm = sqrt(sq), coef = min(1, max_norm / (norm + 1e-6))  (torch's formula)
//
// No float atomics: every partial and the total depend only on the chunk table, never on the grid or on
// arrival order, so two calls give the same bits.  The clip factor stays on the device; the flat SGD
// kernel folds it into its gradient scale (ddpx_sgd_flat_clip), so no pass rewrites the gradients and
// nothing goes to the host (graph-capturable).
//
// Summation shape of one partial (the tests derive their tolerance from it; thread_sumsq and block_store_sums in
// ddpx_flat_optim.h, which lars.hip and lamb.hip share): a thread owns 4 accumulators,
// accumulator k takes the 16-B vectors tid + (4 j + k) * 256 of the chunk with one fma per element:
// kChunk / (4 * 256) = 32 elements per accumulator for both dtypes, + 1 for the scalar tail on accumulator
// 0; then (a0 + a1) + (a2 + a3), a 6-level butterfly over the wave, and (w0 + w1) + (w2 + w3) through LDS.
#include "ddpx_flat_optim.h"

namespace ddpx {

constexpr int kChunk = 32768;

static int g_sumsq_nt = 0;  // non-temporal loads in the norm pass (ddpx_grad_sumsq_set_nt; benchmarks)

template <bool GBF16, bool NT>
__global__ void __launch_bounds__(256)
grad_sumsq_kernel(const void* __restrict__ g, const FlatChunk* __restrict__ table,
                  float* __restrict__ partials) {
  __shared__ float red[1][4];
  const FlatChunk c = table[blockIdx.x];
  const int tid = threadIdx.x;
  const char* x = reinterpret_cast<const char*>(g) + c.start * (GBF16 ? 2 : 4);
  const float t[1] = {thread_sumsq<GBF16, NT>(x, c.len, tid)};
  block_store_sums(t, red, tid, partials + blockIdx.x);
}

// thread t sums partials t, t + 256, ... in fp64, then a fixed LDS tree: the same bits for the same input
__global__ void __launch_bounds__(256)
sumsq_reduce_kernel(const float* __restrict__ partials, int n, float* __restrict__ sq, int accumulate) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)partials[i];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) *sq = (float)(accumulate ? (double)*sq + red[0] : red[0]);
}

// out2[0] = total norm, out2[1] = clip factor.  torch.nn.utils.clip_grad_norm_ with error_if_nonfinite=False:
// clamp(max_norm / (norm + 1e-6), max=1.0), which keeps a NaN factor NaN (the comparison below is false for it)
__global__ void clip_coef_kernel(const float* __restrict__ sq, float max_norm, float* __restrict__ out2) {
  const float norm = sqrtf(*sq);
  const float c = max_norm / (norm + 1e-6f);
  out2[0] = norm;
  out2[1] = c > 1.f ? 1.f : c;
}

template <bool XBF16>
__global__ void __launch_bounds__(256)
scale_dev_kernel(void* __restrict__ x, int64_t n, const float* __restrict__ scale_ptr) {
  const float s = *scale_ptr;
  constexpr int W = XBF16 ? 8 : 4;
  const int64_t nv = n / W;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    if constexpr (XBF16) {
      u32x4 r = reinterpret_cast<u32x4*>(x)[i];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        r[q] = pack_bf2(__uint_as_float(r[q] << 16) * s, __uint_as_float(r[q] & 0xffff0000u) * s);
      reinterpret_cast<u32x4*>(x)[i] = r;
    } else {
      f32x4 v = reinterpret_cast<f32x4*>(x)[i];
      v *= s;
      reinterpret_cast<f32x4*>(x)[i] = v;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < n - nv * W) {
    const int64_t j = nv * W + threadIdx.x;
    if constexpr (XBF16) {
      unsigned short* xs = reinterpret_cast<unsigned short*>(x);
      xs[j] = f2bf(bf2f(xs[j]) * s);
    } else {
      reinterpret_cast<float*>(x)[j] *= s;
    }
  }
}

}  // namespace ddpx

using namespace ddpx;

DDPX_API int ddpx_grad_chunk() { return kChunk; }

DDPX_API void ddpx_grad_sumsq_set_nt(int nt) { g_sumsq_nt = nt ? 1 : 0; }

// One partial per chunk of ``table`` (FlatChunk[n_chunks], device); the caller guarantees that every chunk
// lies inside the gradient buffer (the host builder checks it against the store's size).
DDPX_API int ddpx_grad_sumsq(const void* g, int g_bf16, const void* table, int n_chunks, float* partials_out,
                             hipStream_t s) {
  if (n_chunks <= 0) return 0;
  if (!g || !table || !partials_out) return -1;
  if (misaligned(15, g, table)) return -1;
  const FlatChunk* t = reinterpret_cast<const FlatChunk*>(table);
  with_flags([&](auto gb, auto nt) {
    hipLaunchKernelGGL((grad_sumsq_kernel<gb(), nt()>), dim3(n_chunks), dim3(256), 0, s, g, t, partials_out);
  }, g_bf16 != 0, g_sumsq_nt != 0);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_grad_sumsq_reduce(const float* partials, int n, float* sq_out, int accumulate, hipStream_t s) {
  if (n < 0 || !sq_out || (n > 0 && !partials)) return -1;
  hipLaunchKernelGGL(sumsq_reduce_kernel, dim3(1), dim3(256), 0, s, partials, n, sq_out, accumulate);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_clip_coef(const float* sq, float max_norm, float* out2, hipStream_t s) {
  if (!sq || !out2) return -1;
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(1), 0, s, sq, max_norm, out2);
  return (int)hipGetLastError();
}

// x *= *scale_ptr in place (fp32 or bf16), the functional clip_grad_norm_'s scaling pass.
DDPX_API int ddpx_scale_dev(void* x, int x_bf16, int64_t n, const float* scale_ptr, hipStream_t s) {
  if (n <= 0) return 0;
  if (!x || !scale_ptr || misaligned(15, x)) return -1;
  const int64_t nv = n / (x_bf16 ? 8 : 4) + 1;
  int64_t blocks = (nv + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (x_bf16)
    hipLaunchKernelGGL(scale_dev_kernel<true>, dim3((int)blocks), dim3(256), 0, s, x, n, scale_ptr);
  else
    hipLaunchKernelGGL(scale_dev_kernel<false>, dim3((int)blocks), dim3(256), 0, s, x, n, scale_ptr);
  return (int)hipGetLastError();
}
