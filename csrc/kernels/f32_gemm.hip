// ddpx — the GEMM core of the reference's fp32 recipe on MI355X (``--dtype fp32``; singlegpu.py trains its VGG
// in fp32 and reports "fp32 model has accuracy").  The BatchNorm passes are in f32_bn.hip, the pooling and the
// classifier head in f32_head.hip.
//
// One exact-fp32 GEMM for Linear fwd / dgrad / wgrad and the 3x3 convolutions as implicit GEMMs (NHWC, the im2col
// never materialised): v_mfma_f32_16x16x4_f32 — f32 in, f32 accumulate, bitwise an fmaf chain, 64 FLOP/clk/SIMD =
// the f32 vector peak (gfx950 has no xf32).  256-thread workgroups of 2x2 waves, 128x128 / 128x64 / 64x128 /
// 64x64 tiles, BK = 16, XCD-aware tile order.  Two kernels run the same fragments and MFMA sequence:
//
//   * gemm_f32_dma_kernel (default): operand tiles go global -> LDS by LDS-DMA into a 4-slot ring (3 slots for
//     the image's first convolution), three K-steps in flight, one barrier per K-step;
//   * gemm_f32_kernel: register-staged loads into double-buffered LDS.  The fallback for operands beyond 32-bit
//     buffer offsets, and the oracle the ring kernel is held to bitwise (DDPX_F32_STAGING=reg selects it).
//
// Summation: plain (one MFMA chain over K: the Linear layers) or blocked (a fresh accumulator per 64 k added to
// the running sum: the convolutions; 16-k blocks = the register-staged kernel's order) — see f32_sum_mode().
// Epilogues: per element bias, accumulate, ReLU, mask (epilogue()), stored in fragment order (4-B lanes) or, on
// the ring kernel, staged through the idle ring and stored as 16-B row vectors (F_VEC); raw split-K slabs
// (F_SPLIT) finished by splitk_reduce / splitk_epi / wgrad_reduce in fixed order — deterministic, no float
// atomics; and on the ring kernel the BatchNorm tile statistics of a conv forward, and the fused SGD update of a
// weight gradient that is never stored.
#include <cstdlib>

#include "ddpx_common.h"
#include "ddpx_f32.h"

namespace ddpx {
namespace f32k {

enum Mode { DENSE_KC = 0, DENSE_OC = 1, IM2COL_KC = 2, IM2COL_OC = 3 };

// A logical operand X(o, k): o = row of A / column of B ("outer"), k = reduction index.
//   DENSE_KC : p[o * ld + k]           (contiguous along k; K % 4 == 0)
//   DENSE_OC : p[k * ld + o]           (contiguous along o; O % 4 == 0)
//   IM2COL_KC: o = pixel m, k = (r*3+s)*C + c -> x[n][h+sgn(r-1)][w+sgn(s-1)][c]   (forward / data gradient A)
//   IM2COL_OC: o = (r*3+s)*C + c, k = pixel m  (same element)                         (weight gradient B)
// Out-of-range rows / k / padding taps read as 0.  C, H, W are powers of two (log2 given).
struct Operand {
  const float* p;
  int ld, O;
  int lc, lh, lw, sgn;
};

__device__ __forceinline__ f32x4 im2col4(const Operand& X, int m, int k) {
  const int n = m >> (X.lh + X.lw);
  const int h = (m >> X.lw) & ((1 << X.lh) - 1);
  const int w = m & ((1 << X.lw) - 1);
  const int rs = k >> X.lc;
  const int c = k & ((1 << X.lc) - 1);
  const int r = (rs * 11) >> 5;  // rs / 3 for rs < 9
  const int s = rs - 3 * r;
  const int ih = h + X.sgn * (r - 1), iw = w + X.sgn * (s - 1);
  if (rs >= 9 || ih < 0 || iw < 0 || ih >= (1 << X.lh) || iw >= (1 << X.lw)) return (f32x4){0.f, 0.f, 0.f, 0.f};
  const size_t off = ((((size_t)n << X.lh | ih) << X.lw | iw) << X.lc) | c;
  return *reinterpret_cast<const f32x4*>(X.p + off);
}

template <int MODE>
__device__ __forceinline__ f32x4 load4(const Operand& X, int o, int k, int kend) {
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  if (o >= X.O || k >= kend) return zero;
  if constexpr (MODE == DENSE_KC) return *reinterpret_cast<const f32x4*>(X.p + (size_t)o * X.ld + k);
  if constexpr (MODE == DENSE_OC) return *reinterpret_cast<const f32x4*>(X.p + (size_t)k * X.ld + o);
  if constexpr (MODE == IM2COL_KC) return im2col4(X, o, k);
  return im2col4(X, k, o);
}

constexpr int BK = 16, PAD = 20, NT = 256;  // Stage<KC> maps 4 float4 per row: BK is 16

template <int MODE, int BO>
struct Stage {
  static constexpr int NV = BO * BK / 4 / NT;  // float4 per thread per tile
  static constexpr bool KC = (MODE == DENSE_KC || MODE == IM2COL_KC);
  f32x4 r[NV];
  __device__ __forceinline__ void load(const Operand& X, int o0, int kt, int kend, int tid) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int idx = tid + NT * v;
      if constexpr (KC) r[v] = load4<MODE>(X, o0 + (idx >> 2), kt + (idx & 3) * 4, kend);
      else r[v] = load4<MODE>(X, o0 + (idx % (BO / 4)) * 4, kt + idx / (BO / 4), kend);
    }
  }
  __device__ __forceinline__ void store(float (*S)[BO + PAD], int tid) const {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const int idx = tid + NT * v;
      if constexpr (KC) {
        const int o = idx >> 2, kq = (idx & 3) * 4;
#pragma unroll
        for (int e = 0; e < 4; ++e) S[kq + e][o] = r[v][e];
      } else {
        *reinterpret_cast<f32x4*>(&S[idx / (BO / 4)][(idx % (BO / 4)) * 4]) = r[v];
      }
    }
  }
};

enum Flags { F_RELU = 1, F_ACCUM = 2, F_SPLIT = 4, F_VEC = 8 };  // F_VEC: LDS-DMA core's 16-B store epilogue

// The output epilogue of one element, in this order: + bias, + the value already there (F_ACCUM), ReLU, mask.
// A raw split-K slab (F_SPLIT) takes none of it.  b(), prev() and mk() give the element's bias, previous value and
// mask; each is called only where its term applies, so a store path may hand in the load itself.
template <class Bias, class Prev, class Mask>
__device__ __forceinline__ float epilogue(float v, int flags, bool has_bias, bool has_mask, Bias b, Prev prev,
                                          Mask mk) {
  if (!(flags & F_SPLIT)) {
    if (has_bias) v += b();
    if (flags & F_ACCUM) v += prev();
    if (flags & F_RELU) v = fmaxf(v, 0.f);
    if (has_mask && !(mk() > 0.f)) v = 0.f;
  }
  return v;
}

// The accumulators of a workgroup's tile to out, fragment by fragment: a lane's 4 values of a 16x16 fragment are 4
// rows of one column (4-B stores, 64-B row pieces per wave instruction).
template <int FM, int FN>
__device__ __forceinline__ void store_fragments(const f32x4 (&acc)[FM][FN], float* __restrict__ out, int ldc, int M,
                                                int N, int row0, int col0, int lr, int lc,
                                                const float* __restrict__ bias, const float* __restrict__ mask,
                                                int flags) {
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int row = row0 + i * 16 + lr * 4 + e;
        const int col = col0 + j * 16 + lc;
        if (row >= M || col >= N) continue;
        const size_t o = (size_t)row * ldc + col;
        out[o] = epilogue(
            acc[i][j][e], flags, bias, mask, [&] { return bias[col]; }, [&] { return out[o]; },
            [&] { return mask[o]; });
      }
}

// C[m][n] (+)= sum_k A(m,k) B(k,n)  [+ bias[n]] [relu] [* (mask[m][n] > 0)]; F_SPLIT: the K range of
// blockIdx's split z goes to the raw slab C + z * split_stride.
template <int BM, int BN, int AM, int BMD, bool PLAIN>
__global__ void __launch_bounds__(NT)
gemm_f32_kernel(const Operand A, const Operand B, int M, int N, int K, int kchunk, float* __restrict__ C, int ldc,
                long split_stride, const float* __restrict__ bias, const float* __restrict__ mask, int flags,
                int tiles_m, int tiles_n) {
  __shared__ __attribute__((aligned(16))) float As[2][BK][BM + PAD];
  __shared__ __attribute__((aligned(16))) float Bs[2][BK][BN + PAD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave & 1, wn = wave >> 1;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int per = tiles_m * tiles_n;
  const int z = bid / per, t2 = bid - z * per;
  // consecutive ids (one XCD's range) walk down M inside one column panel of B: the B panel stays in L2
  const int tm = t2 % tiles_m, tn = t2 / tiles_m;
  const int m0 = tm * BM, n0 = tn * BN;
  const int k0 = z * kchunk, k1 = min(K, k0 + kchunk);
  const int nk = (k1 - k0 + BK - 1) / BK;

  constexpr int FM = BM / 32, FN = BN / 32;
  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  Stage<AM, BM> sa;
  Stage<BMD, BN> sb;
  if (nk > 0) {
    sa.load(A, m0, k0, k1, tid);
    sb.load(B, n0, k0, k1, tid);
    sa.store(As[0], tid);
    sb.store(Bs[0], tid);
  }
  __syncthreads();
  const int lr = lane >> 4, lc = lane & 15;
  for (int it = 0; it < nk; ++it) {
    const int cur = it & 1;
    const bool more = it + 1 < nk;
    if (more) {
      sa.load(A, m0, k0 + (it + 1) * BK, k1, tid);
      sb.load(B, n0, k0 + (it + 1) * BK, k1, tid);
    }
    // blocked summation (PLAIN = false): each K step's 16 products go into a fresh accumulator that is then
    // added to the running sum — the rounding chain is K/16 long instead of K (4x smaller error at K = 4608,
    // where a plain MFMA chain left the conv7 output 4e-6 from fp64).  PLAIN: one MFMA chain over K, the
    // summation order of the fp32 library kernels (held to their error vs fp64: tests/test_gpu_f32.py).
    f32x4 part[FM][FN];
    if constexpr (PLAIN) {
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) part[i][j] = acc[i][j];
    }
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {
      float a[FM], b[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) a[i] = As[cur][kk + lr][wm * (BM / 2) + i * 16 + lc];
#pragma unroll
      for (int j = 0; j < FN; ++j) b[j] = Bs[cur][kk + lr][wn * (BN / 2) + j * 16 + lc];
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          part[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
              a[i], b[j], (PLAIN || kk) ? part[i][j] : (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        if constexpr (PLAIN) acc[i][j] = part[i][j];
        else acc[i][j] += part[i][j];
      }
    if (more) {
      sa.store(As[cur ^ 1], tid);
      sb.store(Bs[cur ^ 1], tid);
    }
    __syncthreads();
  }

  float* out = (flags & F_SPLIT) ? C + (size_t)z * split_stride : C;
  store_fragments(acc, out, ldc, M, N, m0 + wm * (BM / 2), n0 + wn * (BN / 2), lr, lc, bias, mask, flags);
}

// ------------------------------------------------------------------ LDS-DMA ring variant
// Same tiles, fragments, MFMA sequence and summation order as gemm_f32_kernel (bitwise-identical results), but the
// operand tiles go global -> LDS by `buffer_load_dword ... lds` (LDS-DMA: no staging VGPRs, no ds_write pass, no
// per-element transposing stores) into an S-stage ring with S-1 K-steps in flight, one raw s_barrier per K-step
// and counted vmcnt waits — the register-staged kernel above exposed a whole K-step of global-load latency per
// barrier with only 2 waves per SIMD (244 VGPRs) to hide it.
// LDS images (16-B chunks = 4 floats, lane-linear DMA writes, bank swizzles applied to the SOURCE chunk):
//   KC operand  [rows][16 k]   row = 64 B, chunk c at c ^ ((row >> 2) & 3)        (conflict-free b32 fragment reads)
//   OC operand  [16 k][rows]   row = 4*rows B, chunk c at c ^ (4 * (k & 3))        (rows >= 64)
constexpr unsigned kOOB32 = 0x80000000u;

template <int MODE>
__device__ __forceinline__ unsigned f32_chunk_off(const Operand& X, int o, int k, int kend) {
  if (o >= X.O || k >= kend) return kOOB32;
  if constexpr (MODE == DENSE_KC) return (unsigned)(((size_t)o * X.ld + k) * 4);
  if constexpr (MODE == DENSE_OC) return (unsigned)(((size_t)k * X.ld + o) * 4);
  const int m = MODE == IM2COL_KC ? o : k, q = MODE == IM2COL_KC ? k : o;
  const int n = m >> (X.lh + X.lw);
  const int h = (m >> X.lw) & ((1 << X.lh) - 1);
  const int w = m & ((1 << X.lw) - 1);
  const int rs = q >> X.lc;
  const int c = q & ((1 << X.lc) - 1);
  const int r = (rs * 11) >> 5;
  const int s2 = rs - 3 * r;
  const int ih = h + X.sgn * (r - 1), iw = w + X.sgn * (s2 - 1);
  if (rs >= 9 || ih < 0 || iw < 0 || ih >= (1 << X.lh) || iw >= (1 << X.lw)) return kOOB32;
  return (unsigned)((((((size_t)n << X.lh | ih) << X.lw | iw) << X.lc) | c) * 4);
}

// Stage one operand tile (ROWS x 16 k) of K-step k0 into an LDS slot: ROWS*64/1024 wave-instructions over 4 waves.
template <int MODE, int ROWS>
__device__ __forceinline__ void f32_stage(__amdgpu_buffer_rsrc_t rs, char* slot, const Operand& X, int o0, int k0,
                                          int kend, int wave, int lane) {
  constexpr bool KC = (MODE == DENSE_KC || MODE == IM2COL_KC);
  constexpr int NI = ROWS * 64 / 1024 / 4;  // instructions per wave
  static_assert(NI * 4 * 1024 == ROWS * 64, "tile must split over 4 waves");
#pragma unroll
  for (int j = 0; j < NI; ++j) {
    const int inst = j * 4 + wave;
    const int pc = inst * 64 + lane;  // LDS chunk position
    unsigned off;
    if constexpr (KC) {
      const int row = pc >> 2, cpos = pc & 3;
      const int kc = cpos ^ ((row >> 2) & 3);
      off = f32_chunk_off<MODE>(X, o0 + row, k0 + 4 * kc, kend);
    } else {
      constexpr int CPR = ROWS / 4;  // chunks per k-row
      const int krow = pc / CPR, cpos = pc % CPR;
      const int oc = cpos ^ (4 * (krow & 3));
      off = f32_chunk_off<MODE>(X, o0 + 4 * oc, k0 + krow, kend);
    }
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (LDS_AS void*)(slot + inst * 1024), 16, off, 0, 0, 0);
  }
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

// KB (blocked summation only): K-steps of 16 per fresh block accumulator.  1 = the register-staged kernel's order
// (bitwise equal); 4 = 64-k blocks (the default: f32_block()).
template <int BM, int BN, int AM, int BMD, bool PLAIN, int STAGES, int KB>
__global__ void __launch_bounds__(NT)
gemm_f32_dma_kernel(const Operand A, const Operand B, int M, int N, int K, int kchunk, float* __restrict__ C,
                    int ldc, long split_stride, const float* __restrict__ bias, const float* __restrict__ mask,
                    int flags, int tiles_m, int tiles_n, unsigned a_bytes, unsigned b_bytes,
                    float* __restrict__ stats, SgdArgs sgd) {
  constexpr int A_SUB = BM * 64, B_SUB = BN * 64, SLOT = A_SUB + B_SUB;
  constexpr int LW = (BM + BN) * 64 / 1024 / 4;  // DMA instructions per wave per stage
  __shared__ __attribute__((aligned(1024))) char smem[STAGES * SLOT];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int per = tiles_m * tiles_n;
  const int z = bid / per, t2 = bid - z * per;
  const int tm = t2 % tiles_m, tn = t2 / tiles_m;
  const int m0 = tm * BM, n0 = tn * BN;
  const int k0 = z * kchunk, k1 = min(K, k0 + kchunk);
  const int nk = (k1 - k0 + BK - 1) / BK;
  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)A.p, 0, a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)B.p, 0, b_bytes, 0x00020000);

  constexpr int FM = BM / 32, FN = BN / 32;
  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  auto issue = [&](int t) {
    char* slot = smem + (t % STAGES) * SLOT;
    f32_stage<AM, BM>(ra, slot, A, m0, k0 + t * BK, k1, wave, lane);
    f32_stage<BMD, BN>(rb, slot + A_SUB, B, n0, k0 + t * BK, k1, wave, lane);
  };
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nk) issue(s);
  const int lr = lane >> 4, lc = lane & 15;
  constexpr int KBE = PLAIN ? 1 : KB;
  for (int it0 = 0; it0 < nk; it0 += KBE) {
    f32x4 part[FM][FN];
    if constexpr (PLAIN) {
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) part[i][j] = acc[i][j];
    }
#pragma unroll
    for (int u = 0; u < KBE; ++u) {
      const int it = it0 + u;
      if (KBE > 1 && it >= nk) break;
      const int ahead = min(STAGES - 2, nk - 1 - it);  // younger stages allowed in flight
      if (STAGES >= 4 && ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LW) : "memory");
      else if (ahead >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LW) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (it + STAGES - 1 < nk) issue(it + STAGES - 1);
      const char* sa = smem + (it % STAGES) * SLOT;
      const char* sb = sa + A_SUB;
      // every fragment of the K-step read up front (one LDS-latency exposure per K-step; reading them kk by kk
      // into reused registers made hipcc wait lgkmcnt(0) every 8 MFMAs)
      float a[BK / 4][FM], b[BK / 4][FN];
#pragma unroll
      for (int q = 0; q < BK / 4; ++q) {
#pragma unroll
        for (int i = 0; i < FM; ++i) a[q][i] = f32_frag<AM, BM>(sa, wm * (BM / 2) + i * 16 + lc, 4 * q + lr);
#pragma unroll
        for (int j = 0; j < FN; ++j) b[q][j] = f32_frag<BMD, BN>(sb, wn * (BN / 2) + j * 16 + lc, 4 * q + lr);
      }
      __builtin_amdgcn_sched_barrier(0);  // keep every read issued before the first MFMA (counted lgkmcnt waits)
#pragma unroll
      for (int q = 0; q < BK / 4; ++q)
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j)
            part[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                a[q][i], b[q][j], (PLAIN || u || q) ? part[i][j] : (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        if constexpr (PLAIN) acc[i][j] = part[i][j];
        else acc[i][j] += part[i][j];
      }
  }

  if (stats) {
    // BatchNorm training statistics of this output tile, straight from the accumulators (the conv forward's raw
    // output): per column, the tile mean and M2 over its valid rows -> stats[tile_m][0 / 1][col] (the chunk
    // statistics bn_finalize merges with Chan's formula; chunk = BM rows).  Fixed reduction order: the 4 lanes
    // sharing a column (xor 16, 32), then the two row-halves of the tile in order.
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave is done with the LDS ring: reuse it
    float* red = reinterpret_cast<float*>(smem);  // [4][BN]: sums of the 2 row halves, then their M2
    const int rows_t = min(BM, M - m0);
    float mean[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      float sm = 0.f;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (m0 + wm * (BM / 2) + i * 16 + lr * 4 + e < M) sm += acc[i][j][e];
      sm += __shfl_xor(sm, 16, 64);
      sm += __shfl_xor(sm, 32, 64);
      if (lr == 0) red[wm * BN + wn * (BN / 2) + j * 16 + lc] = sm;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int col = wn * (BN / 2) + j * 16 + lc;
      mean[j] = (red[col] + red[BN + col]) / (float)rows_t;
      float q = 0.f;
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (m0 + wm * (BM / 2) + i * 16 + lr * 4 + e < M) {
            const float d = acc[i][j][e] - mean[j];
            q = fmaf(d, d, q);
          }
      q += __shfl_xor(q, 16, 64);
      q += __shfl_xor(q, 32, 64);
      if (lr == 0) red[(2 + wm) * BN + col] = q;
    }
    __syncthreads();
    if (wm == 0 && lr == 0) {
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        const int col = wn * (BN / 2) + j * 16 + lc;
        if (n0 + col < N) {
          stats[(size_t)tm * 2 * N + n0 + col] = mean[j];
          stats[(size_t)tm * 2 * N + N + n0 + col] = red[2 * BN + col] + red[3 * BN + col];
        }
      }
    }
  }
  float* out = (flags & F_SPLIT) ? C + (size_t)z * split_stride : C;
  using TS = TileStage<BM, BN, STAGES * SLOT>;  // both row-vector epilogues below walk the tile through the ring
  float* T = reinterpret_cast<float*>(smem);
  if (sgd.p && !(flags & F_SPLIT)) {
    // fused optimizer (single-process weight gradients): the tile's gradient updates the parameter it belongs to
    // right here, with sgd_apply's fma sequence (bitwise the flat SGD's); the gradient is never stored.  The
    // accumulators are staged through the (now idle) LDS ring in row parts so every thread streams 16-B vectors
    // of the master / momentum rows (per-element 4-B accesses ran the update at a fraction of the HBM rate).
    constexpr int TLD = TS::TLD, EH = TS::EH, BMH = TS::BMH, Q = TS::Q, RSTEP = TS::RSTEP, NV = TS::NV;
    constexpr int CH = NV < 4 ? NV : 4;
    const float slr = *sgd.lr;
    const bool has_mom = sgd.mom != 0.f;
    const int cq = tid % Q, r0 = tid / Q;
    const int col = n0 + 4 * cq;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int h = 0; h < EH; ++h) {
      TS::put(T, acc, h, wm, wn, lr, lc);
      const int mh = m0 + h * BMH;
#pragma unroll
      for (int i0 = 0; i0 < NV; i0 += CH) {
        f32x4 pv[CH], bv[CH];
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const int row = mh + r0 + (i0 + i) * RSTEP;
          pv[i] = bv[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
          if (row >= M || col >= N) continue;
          const size_t o = (size_t)row * ldc + col;
          pv[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(sgd.p + o));
          if (has_mom) bv[i] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(sgd.buf + o));
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const int r = r0 + (i0 + i) * RSTEP;
          const int row = mh + r;
          if (row >= M || col >= N) continue;
          const size_t o = (size_t)row * ldc + col;
          const f32x4 g = *reinterpret_cast<const f32x4*>(T + r * TLD + 4 * cq);
          f32x4 po, bo;
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            float d = fmaf(sgd.wd, pv[i][q], g[q]);
            if (has_mom) d = fmaf(sgd.mom, bv[i][q], d);
            bo[q] = d;
            po[q] = fmaf(-slr, d, pv[i][q]);
          }
          __builtin_nontemporal_store(po, reinterpret_cast<f32x4*>(sgd.p + o));
          if (has_mom) __builtin_nontemporal_store(bo, reinterpret_cast<f32x4*>(sgd.buf + o));
          if (sgd.shadow)
            *reinterpret_cast<u32x2*>(sgd.shadow + o) = (u32x2){pack_bf2(po[0], po[1]), pack_bf2(po[2], po[3])};
        }
      }
    }
    return;
  }
  if (flags & F_VEC) {
    // Output tile staged through the idle LDS ring in row parts, then stored as 16-B row vectors (a 128-wide tile
    // row is 512 contiguous bytes).  The fragment-order stores below write 4-B lanes in 64-B row pieces: DeepNN's
    // first conv (K = 36, 256 MB of output) ran 171 us, store-bound, on them (profiles/r6_deepnn).  Same values,
    // same epilogue order (bias, accumulate, ReLU, mask) — bitwise the scalar form.
    constexpr int TLD = TS::TLD, EH = TS::EH, BMH = TS::BMH, Q = TS::Q, RSTEP = TS::RSTEP, NV = TS::NV;
    const int cq = tid % Q, r0 = tid / Q;
    const int col = n0 + 4 * cq;
    const bool epi = !(flags & F_SPLIT);
    f32x4 bv = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (epi && bias && col < N) bv = *reinterpret_cast<const f32x4*>(bias + col);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int h = 0; h < EH; ++h) {
      TS::put(T, acc, h, wm, wn, lr, lc);
      const int mh = m0 + h * BMH;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int r = r0 + i * RSTEP;
        const int row = mh + r;
        if (row >= M || col >= N) continue;
        const size_t o = (size_t)row * ldc + col;
        f32x4 v = *reinterpret_cast<const f32x4*>(T + r * TLD + 4 * cq);
        if (epi) {
          const f32x4 prev = (flags & F_ACCUM) ? *reinterpret_cast<const f32x4*>(out + o) : bv;
          const f32x4 mk = mask ? *reinterpret_cast<const f32x4*>(mask + o) : (f32x4){1.f, 1.f, 1.f, 1.f};
#pragma unroll
          for (int q = 0; q < 4; ++q)
            v[q] = epilogue(
                v[q], flags, bias, true, [&] { return bv[q]; }, [&] { return prev[q]; }, [&] { return mk[q]; });
        }
        *reinterpret_cast<f32x4*>(out + o) = v;
      }
    }
    return;
  }
  store_fragments(acc, out, ldc, M, N, m0 + wm * (BM / 2), n0 + wn * (BN / 2), lr, lc, bias, mask, flags);
}

// Summation order of the f32 core (DDPX_F32_SUM=plain|blocked|auto, default auto).  The bar is the stock fp32
// libraries' own error vs fp64 on the same inputs (tests/test_gpu_f32.py::test_error_no_worse_than_stock,
// MI355X: profiles/r3_f32): the plain chain matches hipBLASLt on the MLP's fc1 (1.15e-6 vs 1.15e-6 rel-L2)
// and is 1.15-1.3x MIOpen's error on VGG's conv7 / conv4, where a few max-pool routing flips then move the
// gradients below them 4x further than torch's own fp32 run does; the blocked form is 2-4x MORE accurate
// than the libraries.  auto: plain for dense GEMMs (Linear layers: 1.056 vs 1.150 ms per toy-MLP step),
// blocked for the im2col convolution GEMMs.
static int f32_sum_mode() {  // 0 auto, 1 plain, 2 blocked
  static const int v = [] {
    const char* e = getenv("DDPX_F32_SUM");
    return !e ? 0 : e[0] == 'p' ? 1 : e[0] == 'b' ? 2 : 0;
  }();
  return v;
}

// 3-slot ring for im2col GEMMs with K <= 48 (DDPX_F32_SMALLK=0 disables; A/B).  Same summation: bitwise equal.
static bool f32_small_k_ring() {
  static const bool v = [] {
    const char* e = getenv("DDPX_F32_SMALLK");
    return !(e && e[0] == '0');
  }();
  return v;
}

// Operand staging: DDPX_F32_STAGING=dma (LDS-DMA ring, default) | reg (register-staged, double-buffered LDS).
static int g_f32_staging = -1;  // -1: from the environment; ddpx_f32_set_staging() overrides (tests, A/B)
static bool f32_dma() {
  if (g_f32_staging < 0) {
    const char* e = getenv("DDPX_F32_STAGING");
    g_f32_staging = (e && e[0] == 'r') ? 0 : 1;
  }
  return g_f32_staging == 1;
}
constexpr int kF32Stages = 4;
// Output stores of the LDS-DMA core: 16-B row vectors staged through LDS (default) or the fragment-order 4-B
// stores (DDPX_F32_EPI=scalar; A/B).  Bitwise the same results.
static bool f32_vec_epi() {
  static const bool v = [] {
    const char* e = getenv("DDPX_F32_EPI");
    return !(e && e[0] == 's');
  }();
  return v;
}
// Summation block of the LDS-DMA core's blocked mode, in 16-k K-steps (DDPX_F32_BLOCK=1|4, default 4): a fresh
// block accumulator per 64 k, added to the running sum.  Measured on MI355X (profiles/r4_f32): the rounding
// error of a length-K dot product is smallest near blocks of sqrt(K) (~64 at VGG's K = 2304-4608: conv7 / conv4
// outputs 0.26x MIOpen's own error vs fp64, against 0.42x / 0.37x with 16-k blocks), and the adds of fewer
// blocks cost less (VGG fp32 step 19.07 ms vs 21.35 ms with 16-k blocks).  1 = the register-staged kernel's
// exact summation order (bitwise equal to it).
static int g_f32_block = -1;
static int f32_block() {
  if (g_f32_block < 0) {
    const char* e = getenv("DDPX_F32_BLOCK");
    g_f32_block = (e && e[0] == '1') ? 1 : 4;
  }
  return g_f32_block;
}

template <int BM, int BN, int AM, int BMD>
static void launch(const Operand& A, const Operand& B, int M, int N, int K, int splits, float* C, int ldc,
                   long split_stride, const float* bias, const float* mask, int flags, hipStream_t s,
                   unsigned a_bytes, unsigned b_bytes, float* stats = nullptr, SgdArgs sgd = SgdArgs{}) {
  const int tm = (M + BM - 1) / BM, tn = (N + BN - 1) / BN;
  int kchunk = (K + splits - 1) / splits;
  kchunk = (kchunk + BK - 1) / BK * BK;
  const int nwg = tm * tn * splits;
  const int mode = f32_sum_mode();
  const bool conv = AM == IM2COL_KC || BMD == IM2COL_OC;
  const bool plain = mode == 1 || (mode == 0 && !conv);
  if (!(f32_dma() && a_bytes && b_bytes)) {
    const auto reg = plain ? gemm_f32_kernel<BM, BN, AM, BMD, true> : gemm_f32_kernel<BM, BN, AM, BMD, false>;
    hipLaunchKernelGGL(reg, dim3(nwg), dim3(NT), 0, s, A, B, M, N, K, kchunk, C, ldc, split_stride, bias, mask, flags,
                       tm, tn);
    return;
  }
  const auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  if (f32_vec_epi() && N % 4 == 0 && ldc % 4 == 0 && split_stride % 4 == 0 && al16(C) && al16(bias) && al16(mask))
    flags |= F_VEC;
  auto ring = gemm_f32_dma_kernel<BM, BN, AM, BMD, true, kF32Stages, 1>;
  if (!plain && f32_block() == 4) ring = gemm_f32_dma_kernel<BM, BN, AM, BMD, false, kF32Stages, 4>;
  if (!plain && f32_block() == 1) ring = gemm_f32_dma_kernel<BM, BN, AM, BMD, false, kF32Stages, 1>;
  if constexpr (AM == IM2COL_KC) {
    // the image's first convolution (K = 36: 3 K-steps): a 3-slot ring holds the whole K range, and the smaller
    // LDS footprint (48 KB at 128x128, not 64) fits 3 workgroups per CU instead of 2
    if (!plain && kchunk <= 3 * BK && f32_block() == 4 && f32_small_k_ring())
      ring = gemm_f32_dma_kernel<BM, BN, AM, BMD, false, 3, 4>;
  }
  hipLaunchKernelGGL(ring, dim3(nwg), dim3(NT), 0, s, A, B, M, N, K, kchunk, C, ldc, split_stride, bias, mask, flags,
                     tm, tn, a_bytes, b_bytes, stats, sgd);
}

template <int AM, int BMD>
static void dispatch_tile(int tile, const Operand& A, const Operand& B, int M, int N, int K, int splits, float* C,
                          int ldc, long ss, const float* bias, const float* mask, int flags, hipStream_t s,
                          unsigned ab, unsigned bb, float* stats = nullptr, SgdArgs sgd = SgdArgs{}) {
  switch (tile) {
    case 0: launch<128, 128, AM, BMD>(A, B, M, N, K, splits, C, ldc, ss, bias, mask, flags, s, ab, bb, stats, sgd); break;
    case 1: launch<128, 64, AM, BMD>(A, B, M, N, K, splits, C, ldc, ss, bias, mask, flags, s, ab, bb, stats, sgd); break;
    case 3: launch<64, 128, AM, BMD>(A, B, M, N, K, splits, C, ldc, ss, bias, mask, flags, s, ab, bb, stats, sgd); break;
    default: launch<64, 64, AM, BMD>(A, B, M, N, K, splits, C, ldc, ss, bias, mask, flags, s, ab, bb, stats, sgd); break;
  }
}

// Bytes an operand spans (the LDS-DMA buffer resource's bound; 0 = too large for 32-bit offsets: register path)
static unsigned operand_bytes(int mode, int ld, int O, int K, int C, int npix) {
  size_t n;
  if (mode == DENSE_KC) n = ((size_t)(O - 1) * ld + K) * 4;
  else if (mode == DENSE_OC) n = ((size_t)(K - 1) * ld + O) * 4;
  else n = (size_t)npix * C * 4;
  return n >= 0x80000000ull ? 0u : (unsigned)n;
}

// ------------------------------------------------------------------ conv helpers
// Forward / data-gradient GEMM weights from torch's [Co][Ci][3][3] fp32 master:
//   wf[(r*3+s)*Cp + ci][co]  (Cp >= Ci zero-padded input channels)     — B of the forward
//   wd[(r*3+s)*Co + co][ci]  (only when wd != null)                     — B of the data gradient
__global__ void __launch_bounds__(256) wprep_kernel(const float* __restrict__ w, int Co, int Ci, int Cp,
                                                     float* __restrict__ wf, float* __restrict__ wd) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // over 9 * Cp * Co
  if (i >= 9 * Cp * Co) return;
  const int co = i % Co, k = i / Co, ci = k % Cp, rs = k / Cp;
  const float v = ci < Ci ? w[((size_t)co * Ci + ci) * 9 + rs] : 0.f;
  wf[i] = v;
  if (wd && ci < Ci) wd[((size_t)rs * Co + co) * Ci + ci] = v;
}

// grad[co][ci][r][s] (+)= sum_z part[z][co][(r*3+s)*Cp + ci]   (fixed order over z)
// Threads walk the slab layout (ci fastest: coalesced reads of every slab, 8 slabs' loads in flight) and scatter
// into torch's [Co][Ci][3][3] order; the sum over z runs in the same order as before (bitwise unchanged).
__global__ void __launch_bounds__(256) wgrad_reduce_kernel(const float* __restrict__ part, int S, int Co, int Ci,
                                                            int Cp, float* __restrict__ grad, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;  // over Co * 9 * Ci, slab order
  if (i >= Co * Ci * 9) return;
  const int ci = i % Ci, rs = (i / Ci) % 9, co = i / (9 * Ci);
  const size_t stride = (size_t)Co * 9 * Cp;
  const float* p = part + (size_t)co * 9 * Cp + rs * Cp + ci;
  float acc = 0.f;
  int z = 0;
  // 32 slabs' loads in flight: the first conv (3 input channels: 14 workgroups, 512 slabs) was latency-bound at
  // 8 (28 us in the DeepNN fp32 step); same adds in the same order
  for (; z + 32 <= S; z += 32) {
    float v[32];
#pragma unroll
    for (int u = 0; u < 32; ++u) v[u] = p[(size_t)(z + u) * stride];
#pragma unroll
    for (int u = 0; u < 32; ++u) acc += v[u];
  }
  for (; z + 8 <= S; z += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(z + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += v[u];
  }
  for (; z < S; ++z) acc += p[(size_t)z * stride];
  const size_t o = ((size_t)co * Ci + ci) * 9 + rs;
  grad[o] = accumulate ? grad[o] + acc : acc;
}

// out[i] (+)= sum_z part[z][i]
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const float* __restrict__ part, int S, long n,
                                                             float* __restrict__ out, int accumulate) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float acc = 0.f;
  for (int z = 0; z < S; ++z) acc += part[z * n + i];
  out[i] = accumulate ? out[i] + acc : acc;
}

// Split-K finish of a [M][N] fp32 GEMM with its epilogue: out = relu?(sum_z part[z] + bias[n]) * (mask > 0)?,
// 16-B vectors (N % 4 == 0), slabs summed in split order.
__global__ void __launch_bounds__(256) splitk_epi_kernel(const float* __restrict__ part, int S, int M, int N,
                                                          float* __restrict__ out, const float* __restrict__ bias,
                                                          const float* __restrict__ mask, int relu) {
  const long nv = (long)M * N / 4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= nv) return;
  const long n4 = (long)M * N / 4;
  f32x4 acc = reinterpret_cast<const f32x4*>(part)[i];
  for (int z = 1; z < S; ++z) {
    const f32x4 v = reinterpret_cast<const f32x4*>(part)[z * n4 + i];
    acc += v;
  }
  const int col = (int)((i * 4) % N);
  f32x4 mk = {1.f, 1.f, 1.f, 1.f};
  if (mask) mk = reinterpret_cast<const f32x4*>(mask)[i];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float v = acc[q];
    if (bias) v += bias[col + q];
    if (relu) v = fmaxf(v, 0.f);
    if (mask && !(mk[q] > 0.f)) v = 0.f;
    acc[q] = v;
  }
  reinterpret_cast<f32x4*>(out)[i] = acc;
}

// 0 = 128x128, 1 = 128x64, 2 = 64x64, 3 = 64x128.  Thin operands get the tile that does not compute padding:
// M <= 64 (the weight gradients of 64-channel layers: M = Co) takes 64-row tiles.
static int auto_tile(int M, int N, int splits) {
  if (M <= 64) return N <= 64 ? 2 : 3;
  const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128) * splits;
  return N <= 64 ? 1 : (t128 >= 512 ? 0 : 2);
}

static int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return (1 << l) == v ? l : -1;
}

}  // namespace f32k
}  // namespace ddpx

using namespace ddpx;
using namespace ddpx::f32k;

// C (+)= A B on the f32 MFMA core.  amode/bmode: Mode; conv geometry (C, H, W of the NHWC tensor an
// IM2COL operand reads, and the tap sign) applies to whichever operand is IM2COL.  splits > 1: raw partial
// slabs C + z*split_stride (no epilogue).  tile: 0 = 128x128, 1 = 128x64, 2 = 64x64, 3 = 64x128, -1 = auto.
DDPX_API int ddpx_f32_gemm(int amode, const float* a, int lda, int bmode, const float* b, int ldb, int M, int N, int K,
                           int gc, int gh, int gw, int sgn, int splits, float* c, int ldc, int64_t split_stride,
                           const float* bias, const float* mask, int flags, int tile, hipStream_t s) {
  if (M <= 0 || N <= 0) return 0;
  const bool kc = amode == DENSE_KC || amode == IM2COL_KC || bmode == DENSE_KC;
  if ((kc && K % 4) || splits < 1) return -1;  // k-contiguous operands load 4 consecutive k
  const bool im = amode >= IM2COL_KC || bmode >= IM2COL_KC;
  int lc = 0, lh = 0, lw = 0;
  if (im) {
    lc = ilog2(gc), lh = ilog2(gh), lw = ilog2(gw);
    if (lc < 2 || lh < 0 || lw < 0) return -2;  // channels: power of two >= 4 (16-B taps)
    if ((amode == IM2COL_KC && K != 9 * gc) || (bmode == IM2COL_OC && N != 9 * gc)) return -2;
  }
  if ((amode == DENSE_OC && M % 4) || (bmode == DENSE_OC && N % 4) || (bmode == IM2COL_OC && N % 4)) return -3;
  if ((amode == DENSE_KC && lda % 4) || (bmode == DENSE_KC && ldb % 4) || (amode == DENSE_OC && lda % 4) ||
      (bmode == DENSE_OC && ldb % 4))
    return -4;
  if (splits > 1) flags |= F_SPLIT;
  Operand A{a, lda, M, lc, lh, lw, sgn}, B{b, ldb, N, lc, lh, lw, sgn};
  const unsigned ab = operand_bytes(amode, lda, M, K, gc, M), bb = operand_bytes(bmode, ldb, N, K, gc, K);
  if (tile < 0) {
    tile = auto_tile(M, N, splits);
    // first convolution (K <= 48, 3-slot ring): 128x64 tiles, 105 vs 128 us at 3 -> 128 channels, batch 512
    // (benchmarks/f32_first_conv_probe.py, profiles/r6_f32epi)
    if (amode == IM2COL_KC && K <= 3 * BK && splits == 1 && tile == 0) tile = 1;
  }
  auto run = dispatch_tile<DENSE_KC, DENSE_KC>;
  switch (amode * 4 + bmode) {
    case DENSE_KC * 4 + DENSE_KC: break;
    case DENSE_KC * 4 + DENSE_OC: run = dispatch_tile<DENSE_KC, DENSE_OC>; break;
    case DENSE_OC * 4 + DENSE_OC: run = dispatch_tile<DENSE_OC, DENSE_OC>; break;
    case IM2COL_KC * 4 + DENSE_OC: run = dispatch_tile<IM2COL_KC, DENSE_OC>; break;
    case DENSE_OC * 4 + IM2COL_OC: run = dispatch_tile<DENSE_OC, IM2COL_OC>; break;
    default: return -5;
  }
  run(tile, A, B, M, N, K, splits, c, ldc, split_stride, bias, mask, flags, s, ab, bb, nullptr, SgdArgs{});
  return (int)hipGetLastError();
}

// Weight gradient dW [N][K] = dy^T x (dy [M][N], x [M][K], both DENSE_OC) applied straight to the parameter by an
// SGD epilogue (single process, SGD(fused_backward)): no gradient stored.  LDS-DMA core only (-6 otherwise).
DDPX_API int ddpx_f32_wgrad_sgd(const float* dy, int ldy, const float* x, int ldx, int M, int N, int K, int tile,
                                float* sgd_p, float* sgd_buf, void* sgd_shadow, const float* lr, float mom, float wd,
                                hipStream_t s) {
  if (M <= 0 || N <= 0) return 0;
  if (!f32_dma()) return -6;
  if (!sgd_p || !lr || (mom != 0.f && !sgd_buf)) return -1;
  if (N % 4 || K % 4 || ldy % 4 || ldx % 4) return -3;
  // output [N rows][K cols]: A = dy^T (rows = N, reduction = M), B = x (cols = K)
  Operand A{dy, ldy, N, 0, 0, 0, 1}, B{x, ldx, K, 0, 0, 0, 1};
  const unsigned ab = operand_bytes(DENSE_OC, ldy, N, M, 0, 0), bb = operand_bytes(DENSE_OC, ldx, K, M, 0, 0);
  if (!ab || !bb) return -4;
  if (tile < 0) tile = auto_tile(N, K, 1);
  dispatch_tile<DENSE_OC, DENSE_OC>(tile, A, B, N, K, M, 1, sgd_p, K, 0, nullptr, nullptr, 0, s, ab, bb, nullptr,
                                    SgdArgs{sgd_p, sgd_buf, (unsigned short*)sgd_shadow, lr, mom, wd});
  return (int)hipGetLastError();
}

DDPX_API int ddpx_f32_splitk_reduce(const float* part, int S, int64_t n, float* out, int accumulate, hipStream_t s) {
  hipLaunchKernelGGL(splitk_reduce_kernel, dim3(nblk(n)), dim3(256), 0, s, part, S, (long)n, out, accumulate);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_f32_splitk_epi(const float* part, int S, int M, int N, float* out, const float* bias,
                                 const float* mask, int relu, hipStream_t s) {
  if (N % 4 || S < 1) return -1;
  const long nv = (long)M * N / 4;
  hipLaunchKernelGGL(splitk_epi_kernel, dim3((unsigned)((nv + 255) / 256)), dim3(256), 0, s, part, S, M, N, out, bias,
                     mask, relu);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_f32_conv_wprep(const float* w, int Co, int Ci, int Cp, float* wf, float* wd, hipStream_t s) {
  if (Cp < Ci || (wd && Cp != Ci)) return -1;
  hipLaunchKernelGGL(wprep_kernel, dim3(nblk((long)9 * Cp * Co)), dim3(256), 0, s, w, Co, Ci, Cp, wf, wd);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_f32_conv_wgrad_reduce(const float* part, int S, int Co, int Ci, int Cp, float* grad, int accumulate,
                                        hipStream_t s) {
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(nblk((long)Co * Ci * 9)), dim3(256), 0, s, part, S, Co, Ci, Cp, grad,
                     accumulate);
  return (int)hipGetLastError();
}

// Summation block (1 or 4 K-steps of 16) of the LDS-DMA core; returns the previous setting.
DDPX_API int ddpx_f32_set_block(int kb) {
  const int prev = f32_block();
  g_f32_block = kb == 1 ? 1 : 4;
  return prev;
}

// 1 = LDS-DMA ring GEMM core, 0 = register-staged; returns the previous setting.
DDPX_API int ddpx_f32_set_staging(int dma) {
  const int prev = f32_dma() ? 1 : 0;
  g_f32_staging = dma ? 1 : 0;
  return prev;
}

// Forward 3x3 convolution y [N*H*W][Co] = conv(x NHWC [N][H][W][C], wf) on the LDS-DMA core with the BatchNorm
// tile statistics emitted by its epilogue: stats[tiles_m][2][Co] (tile mean, M2).  Returns the tile's row count
// (the chunk size bn_finalize needs), or a negative code when the fused path does not apply (register-staged
// core selected, or an operand beyond 32-bit offsets): the caller then runs the separate statistics pass.
DDPX_API int ddpx_f32_conv_fwd_stats(const float* x, const float* wf, float* y, int N, int H, int W, int C, int Co,
                                     float* stats, hipStream_t s) {
  if (!f32_dma()) return -10;
  const int lc = ilog2(C), lh = ilog2(H), lw = ilog2(W);
  if (lc < 2 || lh < 0 || lw < 0 || Co % 4) return -2;
  const int M = N * H * W, K = 9 * C;
  Operand A{x, 0, M, lc, lh, lw, 1}, B{wf, Co, Co, lc, lh, lw, 1};
  const unsigned ab = operand_bytes(IM2COL_KC, 0, M, K, C, M), bb = operand_bytes(DENSE_OC, Co, Co, K, C, K);
  if (!ab || !bb) return -11;
  const int tile = auto_tile(M, Co, 1);
  dispatch_tile<IM2COL_KC, DENSE_OC>(tile, A, B, M, Co, K, 1, y, Co, 0, nullptr, nullptr, 0, s, ab, bb, stats);
  const int err = (int)hipGetLastError();
  return err ? -err : ((tile == 2 || tile == 3) ? 64 : 128);
}
