// ddpx — 1x1 / stride-1 convolution in bf16 (the projection shortcut of a Wide ResNet's first block): forward,
// data gradient and weight gradient as weight-stationary streaming kernels.
//
// The shapes are far from what the tiled GEMM core serves: P = N*H*W rows in the hundreds of thousands against
// C = 16 input and Co = 64..512 output channels, so the reduction is one to a few MFMA steps and the kernels are
// bound by the one pass over the big operand.  There is no K ring and no tile of the weight: the whole prepared
// weight [Co][C] (ddpx_conv1x1_weight_prep, at most 64 KiB) sits in a workgroup's LDS and rows are streamed past it.
//
//   forward : y[P][Co]  = x[P][C]   . W[Co][C]^T     (LDS image W,   rows = co, K = c)
//   dgrad   : dx[P][C]  = dy[P][Co] . W[Co][C]       (LDS image W^T, rows = c,  K = co; transposed while filling)
//   wgrad   : dW[Co][C] = dy[P][Co]^T . x[P][C]      over K = P, split into slabs of rows
//
// Forward and dgrad are one kernel, out[P][N] = in[P][K] . L[N][K]^T with L the LDS image.  v_mfma_f32_32x32x8_bf16
// with the roles swapped (M = output column, N = pixel row), because then both operand fragments are plain 16-byte
// reads: lane (i = lane % 32, g = lane / 32) of a K-step of 16 channels reads the 8 channels 16s + 8g .. + 7 of
// row i, its low four go to one MFMA and its high four to a second one (the sum over k does not care which slot a
// channel sits in, as long as both operands agree).  For C = 16 a wave's load of one 32-row tile is 1 KiB of
// consecutive memory.  The MFMA's M rows are dealt to output columns in the order that leaves each lane with two
// runs of 8 consecutive columns in its 16 accumulators, so a tile is stored as 16-byte chunks, 32 B per pixel row
// per instruction; fp32 accumulation, one rounding to bf16.  A wave owns a contiguous range of 32-row tiles, holds
// the A fragments of up to 64 channels (KB K-steps) in registers, sweeps the 32-wide column tiles NG at a time from
// them, and issues the next block's loads before it multiplies the current one (one block ahead per wave; the
// other waves of the CU supply the rest of the loads in flight).  With C <= 64 and N <= 128 (the WRN shapes) every
// input element is loaded once.  An output narrower than 32 columns (the data gradient's N = C = 16) is one column
// tile whose upper MFMA rows multiply zeros: nothing is padded in memory and nothing extra is stored; the idle half
// of the 32x32 instruction is hidden behind the stream.
//
// Weight gradient: a workgroup walks its slab of rows in chunks of 32 pixels.  The chunk of dy and of x goes
// global -> registers -> LDS as 16-byte pieces (the next chunk's loads are issued before the current chunk is
// multiplied), and the fragments are read back transposed (k = pixel) with 2-byte LDS reads; the row strides are
// 16 mod 32 bytes so the two lane halves, four pixels apart, use different banks.  Each wave keeps TPW 32x32 fp32
// tiles of dW[Co][Cp] in registers for the whole slab and writes them once to part[slab][Co][Cp];
// ddpx_conv1x1_wgrad_reduce (conv_igemm_s2.hip) sums the slabs in order: no atomics, bitwise reproducible.
// The slab count (wgrad_slabs) aims at two workgroups per CU with at least two chunks each: an unmeasured choice.
//
// Supported: C, Co multiples of 8, Co * C * 2 B <= 64 KiB, operands below 2 GiB; the weight gradient also needs
// its staging chunk 32 * (2 (Co + C) + 32) + 64 B within 64 KiB (16 -> 512 and 128 -> 256 are inside).  Anything
// else is a negative return code.  No BatchNorm-statistics epilogue: a Wide ResNet's shortcut has no BatchNorm.
//
// Build (hipcc -O3, gfx950; VGPR / AGPR / waves per SIMD): stream_kernel<false> and <true> 128 / 64 / 2;
// wgrad_kernel<1,3> 58 / 16 / 6, <2,3> 136 / 32 / 3, <4,16> 218 / 64 / 1, <8,16> 254 / 132 / 1.  No scratch in any.
// LDS is dynamic: the weight image (at most 64 KiB), or the staging chunk.
#include "ddpx_common.h"

namespace ddpx {
namespace c1 {

constexpr int KB = 4;  // K-steps of 16 channels whose A fragments a wave holds at once
constexpr int NG = 4;  // 32-wide column tiles swept per held block (64 accumulator registers)

struct StreamParams {
  const unsigned short* in;   // [P][K]
  const unsigned short* w;    // prepared weight as stored, [wrows][wcols]
  unsigned short* out;        // [P][N]
  int P, K, N;
  int wrows, wcols;
  int ld16;                   // row stride of the LDS image in 16-byte chunks
  int tiles, tpw;             // 32-row tiles, tiles per wave
};

struct Iter {
  int t, grp, kb;  // row tile, column-tile group, K block
};

union Frag {
  u32x4 q;
  short4v h[2];
  unsigned short e[8];
};

// TR = false: the LDS image is the stored weight (forward).  TR = true: its transpose (data gradient).
template <bool TR>
__global__ void __launch_bounds__(256) stream_kernel(StreamParams p) {
  extern __shared__ __attribute__((aligned(16))) char wl[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  {
    const int cpr = p.wcols >> 3, n = p.wrows * cpr;
    for (int i = tid; i < n; i += 256) {
      const int r = i / cpr, ch = i - r * cpr;
      Frag v;
      v.q = *reinterpret_cast<const u32x4*>(p.w + (size_t)i * 8);
      if (!TR) {
        *reinterpret_cast<u32x4*>(wl + ((size_t)r * p.ld16 + ch) * 16) = v.q;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          *reinterpret_cast<unsigned short*>(wl + (size_t)(ch * 8 + j) * p.ld16 * 16 + r * 2) = v.e[j];
      }
    }
  }
  __syncthreads();

  const int kc = p.K >> 3;                  // 16-byte chunks per input row
  const int nks = (kc + 1) >> 1;            // K-steps of 16 channels
  const int nkb = (nks + KB - 1) / KB;
  const int nct = (p.N + 31) >> 5;
  const int ngrp = (nct + NG - 1) / NG;
  const int t0 = (blockIdx.x * 4 + wave) * p.tpw;
  const int t1 = min(p.tiles, t0 + p.tpw);
  if (t0 >= t1) return;
  const int i32 = lane & 31, g = lane >> 5;
  // MFMA row i32 = 8a + 4h + b carries output column 16 (a / 2) + 8h + 4 (a % 2) + b of its tile: lane half g then
  // holds columns 8g .. 8g + 7 in accumulators 0..7 and 16 + 8g .. in 8..15
  const int wcol = 16 * (i32 >> 4) + 8 * ((i32 >> 2) & 1) + 4 * ((i32 >> 3) & 1) + (i32 & 3);

  auto advance = [&](Iter& it) {
    if (++it.kb == nkb) {
      it.kb = 0;
      if (++it.grp == ngrp) {
        it.grp = 0;
        ++it.t;
      }
    }
  };
  auto load = [&](const Iter& it, Frag (&a)[KB]) {
    const int row = it.t * 32 + i32;
    const bool ok = it.t < t1 && row < p.P;
    const unsigned short* src = p.in + (size_t)row * p.K;
#pragma unroll
    for (int s = 0; s < KB; ++s) {
      const int ch = 2 * (it.kb * KB + s) + g;
      a[s].q = u32x4{0u, 0u, 0u, 0u};
      if (ok && ch < kc) a[s].q = *reinterpret_cast<const u32x4*>(src + ch * 8);
    }
  };

  f32x16 acc[NG];
  auto compute = [&](const Iter& it, const Frag (&a)[KB]) {
    if (it.kb == 0) {
#pragma unroll
      for (int c = 0; c < NG; ++c)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;
    }
#pragma unroll
    for (int s = 0; s < KB; ++s) {
      const int ks = it.kb * KB + s;
      if (ks < nks) {
        const int ch = 2 * ks + g;
#pragma unroll
        for (int c = 0; c < NG; ++c) {
          const int ct = it.grp * NG + c;
          if (ct < nct) {
            const int col = ct * 32 + wcol;
            Frag w;
            w.q = u32x4{0u, 0u, 0u, 0u};
            if (col < p.N && ch < kc) w.q = *reinterpret_cast<const u32x4*>(wl + ((size_t)col * p.ld16 + ch) * 16);
            acc[c] = __builtin_amdgcn_mfma_f32_32x32x8bf16_1k(w.h[0], a[s].h[0], acc[c], 0, 0, 0);
            acc[c] = __builtin_amdgcn_mfma_f32_32x32x8bf16_1k(w.h[1], a[s].h[1], acc[c], 0, 0, 0);
          }
        }
      }
    }
    if (it.kb == nkb - 1) {
      const int row = it.t * 32 + i32;
      if (row < p.P) {
        unsigned short* dst = p.out + (size_t)row * p.N;
#pragma unroll
        for (int c = 0; c < NG; ++c) {
          const int ct = it.grp * NG + c;
          if (ct < nct) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const int col = ct * 32 + 16 * h + 8 * g;
              if (col < p.N) {
                u32x4 o;
                o.x = pack_bf2(acc[c][8 * h + 0], acc[c][8 * h + 1]);
                o.y = pack_bf2(acc[c][8 * h + 2], acc[c][8 * h + 3]);
                o.z = pack_bf2(acc[c][8 * h + 4], acc[c][8 * h + 5]);
                o.w = pack_bf2(acc[c][8 * h + 6], acc[c][8 * h + 7]);
                *reinterpret_cast<u32x4*>(dst + col) = o;
              }
            }
          }
        }
      }
    }
  };

  Frag a0[KB], a1[KB];
  Iter cur{t0, 0, 0}, nxt;
  load(cur, a0);
  while (true) {
    nxt = cur;
    advance(nxt);
    load(nxt, a1);
    compute(cur, a0);
    cur = nxt;
    if (cur.t >= t1) break;
    advance(nxt);
    load(nxt, a0);
    compute(cur, a1);
    cur = nxt;
    if (cur.t >= t1) break;
  }
}

struct WgradParams {
  const unsigned short* dy;  // [P][Co]
  const unsigned short* x;   // [P][Cp]
  float* part;               // [S][Co][Cp]
  int P, Co, Cp;
  int klen;                  // rows per slab, a multiple of 32
  int sD, sX, xoff;          // LDS row strides (bytes) of the dy / x chunk, byte offset of the x chunk
  int nct, ntile;            // column tiles (over Cp), all 32x32 tiles of dW
};

// TPW: dW tiles per wave (wave w owns tiles w, w + 4, ...).  NST: 16-byte pieces of a chunk per thread.
template <int TPW, int NST>
__global__ void __launch_bounds__(256) wgrad_kernel(WgradParams p) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i32 = lane & 31, g = lane >> 5;
  const int cD = p.Co >> 3, cX = p.Cp >> 3, nD = 32 * cD, nAll = nD + 32 * cX;
  // this thread's pieces of a chunk: source offset (elements from the chunk's first row) and
  // LDS offset | pixel << 16 | (x operand) << 24 | valid << 25
  int soff[NST];
  unsigned dst[NST];
#pragma unroll
  for (int q = 0; q < NST; ++q) {
    const int idx = q * 256 + tid;
    soff[q] = 0;
    dst[q] = 0;
    if (idx < nD) {
      const int px = idx / cD, ch = idx - px * cD;
      soff[q] = px * p.Co + ch * 8;
      dst[q] = (unsigned)(px * p.sD + ch * 16) | (unsigned)px << 16 | 1u << 25;
    } else if (idx < nAll) {
      const int j = idx - nD, px = j / cX, ch = j - px * cX;
      soff[q] = px * p.Cp + ch * 8;
      dst[q] = (unsigned)(p.xoff + px * p.sX + ch * 16) | (unsigned)px << 16 | 3u << 24;
    }
  }
  const int p0 = blockIdx.x * p.klen, pend = min(p.P, p0 + p.klen);

  u32x4 st[NST];
  auto load = [&](int pc) {
#pragma unroll
    for (int q = 0; q < NST; ++q) {
      st[q] = u32x4{0u, 0u, 0u, 0u};
      const unsigned d = dst[q];
      if ((d >> 25) & 1) {
        const int px = (d >> 16) & 31;
        if (pc + px < pend) {
          const unsigned short* base = (d >> 24) & 1 ? p.x + (size_t)pc * p.Cp : p.dy + (size_t)pc * p.Co;
          st[q] = *reinterpret_cast<const u32x4*>(base + soff[q]);
        }
      }
    }
  };

  f32x16 acc[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  load(p0);
  for (int pc = p0; pc < pend; pc += 32) {
#pragma unroll
    for (int q = 0; q < NST; ++q)
      if ((dst[q] >> 25) & 1) *reinterpret_cast<u32x4*>(lds + (dst[q] & 0xffffu)) = st[q];
    __syncthreads();
    if (pc + 32 < pend) load(pc + 32);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int prow = ks * 8 + 4 * g;  // this lane's four pixels of the K-step
      short4v b;
      int bct = -1;
#pragma unroll
      for (int i = 0; i < TPW; ++i) {
        const int t = wave + 4 * i;
        if (t < p.ntile) {
          const int cot = t / p.nct, ct = t - cot * p.nct;
          if (ct != bct) {
            const char* xs = lds + p.xoff + prow * p.sX + (ct * 32 + i32) * 2;
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = *reinterpret_cast<const short*>(xs + j * p.sX);
            bct = ct;
          }
          const char* ds = lds + prow * p.sD + (cot * 32 + i32) * 2;
          short4v a;
#pragma unroll
          for (int j = 0; j < 4; ++j) a[j] = *reinterpret_cast<const short*>(ds + j * p.sD);
          acc[i] = __builtin_amdgcn_mfma_f32_32x32x8bf16_1k(a, b, acc[i], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }

  float* slab = p.part + (size_t)blockIdx.x * p.Co * p.Cp;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int t = wave + 4 * i;
    if (t < p.ntile) {
      const int cot = t / p.nct, ct = t - cot * p.nct;
      const int c = ct * 32 + i32;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int co = cot * 32 + 8 * (r >> 2) + 4 * g + (r & 3);
        if (co < p.Co && c < p.Cp) slab[(size_t)co * p.Cp + c] = acc[i][r];
      }
    }
  }
}

// ------------------------------------------------------------------ host side
static bool chk16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

constexpr long long kLdsBudget = 64 * 1024;

// 0 on a supported problem: P rows in *P
static int make_shape(int N, int H, int W, int C, int Co, long long* P) {
  if (N < 1 || H < 1 || W < 1 || C < 8 || Co < 8 || C % 8 || Co % 8) return -1;
  *P = (long long)N * H * W;
  const long long lim = 0x80000000ll;
  if (*P * C * 2 >= lim || *P * Co * 2 >= lim) return -4;
  if ((long long)Co * C * 2 > kLdsBudget) return -2;
  return 0;
}

// out [P][Nn] = in [P][K] . L[Nn][K]^T, L = w (tr = false, w stored [Nn][K]) or w^T (tr = true, w stored [K][Nn])
static int launch_stream(bool tr, const void* in, const void* w, void* out, long long P, int K, int Nn,
                         hipStream_t st) {
  StreamParams p{};
  p.in = (const unsigned short*)in; p.w = (const unsigned short*)w; p.out = (unsigned short*)out;
  p.P = (int)P; p.K = K; p.N = Nn;
  p.wrows = tr ? K : Nn; p.wcols = tr ? Nn : K;
  // an odd stride in 16-byte chunks keeps the 32 rows of a fragment read on different banks; taken when it fits
  const int kc = K / 8;
  p.ld16 = ((long long)Nn * (kc | 1) * 16 <= kLdsBudget) ? (kc | 1) : kc;
  p.tiles = (int)((P + 31) / 32);
  const int waves = 4 * 1024;  // four workgroups per CU
  p.tpw = (p.tiles + waves - 1) / waves;
  const int grid = (p.tiles + 4 * p.tpw - 1) / (4 * p.tpw);
  const size_t lds = (size_t)Nn * p.ld16 * 16;
  if (tr) hipLaunchKernelGGL(stream_kernel<true>, dim3(grid), dim3(256), lds, st, p);
  else hipLaunchKernelGGL(stream_kernel<false>, dim3(grid), dim3(256), lds, st, p);
  return (int)hipGetLastError();
}

static int pad_stride(int bytes) { return bytes % 32 == 0 ? bytes + 16 : bytes; }

static int wgrad_geometry(int C, int Co, WgradParams* p) {
  p->Co = Co; p->Cp = C;
  p->sD = pad_stride(Co * 2); p->sX = pad_stride(C * 2);
  p->xoff = 32 * p->sD;
  p->nct = (C + 31) / 32;
  p->ntile = (Co + 31) / 32 * p->nct;
  if (32ll * (p->sD + p->sX) + 64 > kLdsBudget || p->ntile > 32) return -2;
  return 0;
}

// two workgroups per CU when the rows allow it, never fewer than two 32-pixel chunks per slab; every slab has rows
static int wgrad_slabs(long long P, int* klen) {
  long long S = (P + 63) / 64;
  S = S > 512 ? 512 : (S < 1 ? 1 : S);
  const long long k = ((P + S - 1) / S + 31) / 32 * 32;
  *klen = (int)k;
  return (int)((P + k - 1) / k);
}

}  // namespace c1
}  // namespace ddpx

using namespace ddpx;

// y [N*H*W][Co] = x [N*H*W][C] . wf [Co][C]^T (1x1, stride 1, pad 0)
DDPX_API int ddpx_conv1x1_s1_fwd(const void* x, const void* wf, void* y, int N, int H, int W, int C, int Co,
                                 hipStream_t st) {
  long long P;
  if (int e = c1::make_shape(N, H, W, C, Co, &P)) return e;
  if (!x || !wf || !y) return -1;
  if (!c1::chk16(x) || !c1::chk16(wf) || !c1::chk16(y)) return -3;
  return c1::launch_stream(false, x, wf, y, P, C, Co, st);
}

// dx [N*H*W][C] = dy [N*H*W][Co] . wd [Co][C]
DDPX_API int ddpx_conv1x1_s1_dgrad(const void* dy, const void* wd, void* dx, int N, int H, int W, int C, int Co,
                                   hipStream_t st) {
  long long P;
  if (int e = c1::make_shape(N, H, W, C, Co, &P)) return e;
  if (!dy || !wd || !dx) return -1;
  if (!c1::chk16(dy) || !c1::chk16(wd) || !c1::chk16(dx)) return -3;
  return c1::launch_stream(true, dy, wd, dx, P, Co, C, st);
}

// slabs of the weight gradient (the leading extent of its part buffer), or a negative code
DDPX_API int ddpx_conv1x1_s1_wgrad_slabs(int N, int H, int W, int C, int Co) {
  long long P;
  if (int e = c1::make_shape(N, H, W, C, Co, &P)) return e;
  c1::WgradParams p{};
  if (int e = c1::wgrad_geometry(C, Co, &p)) return e;
  int klen;
  return c1::wgrad_slabs(P, &klen);
}

// part [S][Co][C] (fp32) = per-slab partial weight gradients, S = ddpx_conv1x1_s1_wgrad_slabs(...); summed by
// ddpx_conv1x1_wgrad_reduce
DDPX_API int ddpx_conv1x1_s1_wgrad(const void* dy, const void* x, float* part, int S, int N, int H, int W, int C,
                                   int Co, hipStream_t st) {
  long long P;
  if (int e = c1::make_shape(N, H, W, C, Co, &P)) return e;
  c1::WgradParams p{};
  if (int e = c1::wgrad_geometry(C, Co, &p)) return e;
  if (!dy || !x || !part) return -1;
  if (!c1::chk16(dy) || !c1::chk16(x) || !c1::chk16(part)) return -3;
  if (S != c1::wgrad_slabs(P, &p.klen)) return -1;
  p.dy = (const unsigned short*)dy; p.x = (const unsigned short*)x; p.part = part; p.P = (int)P;
  const size_t lds = (size_t)32 * (p.sD + p.sX) + 64;
  const int tpw = (p.ntile + 3) / 4;
  const int pieces = (32 * (Co + C) / 8 + 255) / 256;
  const dim3 grid(S), block(256);
#define DDPX_C1_WGRAD(T, Q) hipLaunchKernelGGL((c1::wgrad_kernel<T, Q>), grid, block, lds, st, p)
  if (pieces <= 3 && tpw <= 1) DDPX_C1_WGRAD(1, 3);
  else if (pieces <= 3 && tpw <= 2) DDPX_C1_WGRAD(2, 3);
  else if (tpw <= 4) DDPX_C1_WGRAD(4, 16);
  else DDPX_C1_WGRAD(8, 16);
#undef DDPX_C1_WGRAD
  return (int)hipGetLastError();
}
