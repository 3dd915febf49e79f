// ddpx — stride-2 convolutions in fp32: 3x3 / pad 1 and 1x1 / pad 0, forward, data gradient and weight gradient,
// the fp32 twins of conv_igemm_s2.hip on the exact-f32 matrix instruction (v_mfma_f32_16x16x4_f32: f32 in, f32
// accumulate), with the LDS images, fragment reads and epilogue staging of f32_gemm.hip's LDS-DMA core
// (ddpx_f32.h) and a main loop and address arithmetic of their own: general H, W and any C % 4 == 0.
//
// x NHWC [N][H][W][C] fp32, Ho = (H + 1) / 2, Wo = (W + 1) / 2, P' = N*Ho*Wo, T = 9 or 1 taps, pad = 1 or 0:
//   forward : y[P'][Co]   = A . Wf[T*C][Co],  A(p', (tap, c)) = x[n][2ho + ky - pad][2wo + kx - pad][c]
//             A is a KC image (rows = output pixels), Wf an OC image (rows of Co).
//   dgrad   : the input pixels split into the four parity classes (h & 1, w & 1), which receive 1, 2, 2 and 4 of the
//             nine taps: four dense GEMMs  dx_class[Pc][C] = A_class[Pc][taps*Co] . Wd[(tap, co)][C]  with
//             A_class(r, (tap, co)) = dy[n][i + dho][j + dwo][co], in one launch.  The workgroup index picks (class,
//             row tile), the four-tap class first; every class stores its rows of dx strided by parity, every element
//             of dx exactly once.  No MFMA multiplies an inserted zero.  1x1: class (0, 0) has its one tap (B is the
//             fp32 master [Co][C] itself), the other three have K = 0 and store +0: no memset, no second pass.
//   wgrad   : dW[Co][T*C] = dy[P'][Co]^T . A[P'][T*C]: dy an OC image (rows of Co), the im2col of x an OC image whose
//             k-rows are output pixels; split over K = P' into fp32 slabs (blockIdx.y) that ddpx_f32_conv_wgrad_reduce
//             (3x3) / ddpx_f32_splitk_reduce (1x1: the slab already is torch's [Co][C]) sum in slab order: no atomics.
// Every chunk is 16 B = 4 consecutive channels moved global -> LDS by LDS-DMA; out-of-range rows, padding taps and k
// past the end get the offset 0x80000000, beyond the buffer resource's bound, and read as 0: no branch around a load.
// What depends on a lane's row alone (the anchor pixel (2ho, 2wo) and its byte base) is computed once per tile; per
// K-step of 16 a chunk costs its tap's shift and a bounds test.  With channels % 16 == 0 a K-step lies inside one
// tap and the shift is wave-uniform ("fast"); otherwise the tap comes from a per-chunk FastDiv.
// Summation: a fresh accumulator per 64 k added to the running sum, the stride-1 convolutions' default order.
// Two tiles, 256 threads (2x2 waves), 4-stage ring, three K-steps in flight, counted vmcnt + one raw barrier per
// K-step: 128x128 (64 KiB of LDS: two workgroups per CU, which is also what its 224 registers allow) and 64x64
// (32 KiB: five per CU, bounded by LDS; its 73 registers would allow more).
#include "ddpx_conv_s2.h"
#include "ddpx_f32.h"

namespace ddpx {
namespace f32s2 {

using namespace f32k;
using namespace s2;  // Shape, ClassGeom, fwd_shift, dgrad_shift, make_classes, tile_rows
using pipe::dma16;
using pipe::fdiv;

enum Kind : int { K_FWD = 0, K_DGRAD = 1, K_WGRAD = 2 };
constexpr int kStages = 4;

struct Params {
  const float* A;
  const float* B;
  float* C;
  float* stats;         // forward: [tiles_m][2][N] (mean, M2) of the tile's rows, or null
  unsigned a_bytes, b_bytes;
  int M, N, K;          // GEMM extents (dgrad: M and K per class)
  int H, W, Ho, Wo;     // input / output image
  int Cs;               // channels of the gathered tensor (x: C; dgrad's dy: Co)
  int ks;               // 3 or 1
  FastDiv dCs, dWo, dHo;
  int klen;             // wgrad: K per split (a multiple of 64)
  long long split_stride;
  int fast;             // Cs % 16 == 0: one tap per K-step
  int tiles_n;
  ClassGeom cls[4];
};

template <int KIND, int BM, int BN, int STAGES>
__global__ void __launch_bounds__(NT) conv_s2_kernel(const Params p) {
  constexpr bool AK = KIND != K_WGRAD;  // A is the gathered KC image (forward, dgrad) or dy as an OC image (wgrad)
  constexpr int AMODE = AK ? IM2COL_KC : DENSE_OC, BMODE = DENSE_OC;  // the images f32_frag reads
  constexpr int A_SUB = BM * 64, B_SUB = BN * 64, SLOT = A_SUB + B_SUB;
  constexpr int NIA = BM / 64, NIB = BN / 64, LW = NIA + NIB;  // DMA instructions per wave per stage
  constexpr int FM = BM / 32, FN = BN / 32;
  static_assert(STAGES >= 2 && STAGES <= 4 && NIA >= 1 && NIB >= 1, "ring depth / tile");
  __shared__ __attribute__((aligned(1024))) char smem[STAGES * SLOT];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave & 1, wn = wave >> 1;
  const int lr = lane >> 4, lc = lane & 15;

  // ---- tile, split, class
  int M = p.M, K = p.K, tm, tn, split = 0;
  ClassGeom cg = p.cls[0];
  if constexpr (KIND == K_DGRAD) {
    const int rt = blockIdx.x / p.tiles_n;
    tn = blockIdx.x - rt * p.tiles_n;
#pragma unroll
    for (int s = 1; s < 4; ++s)
      if (rt >= p.cls[s].tile0) cg = p.cls[s];
    tm = rt - cg.tile0;
    M = cg.rows;
    const int ntaps = p.ks == 3 ? (1 + cg.ph) * (1 + cg.pw) : (cg.ph | cg.pw ? 0 : 1);
    K = ntaps * p.Cs;
  } else {
    const int tiles_m = (M + BM - 1) / BM;
    const int ntiles = tiles_m * p.tiles_n;
    int wg;
    if (gridDim.y > 1) {  // split-major over all workgroups: an XCD owns whole K ranges
      const int lg = xcd_remap(blockIdx.y * gridDim.x + blockIdx.x, ntiles * gridDim.y);
      split = lg / ntiles;
      wg = lg - split * ntiles;
    } else {
      wg = xcd_remap(blockIdx.x, ntiles);
    }
    tm = wg % tiles_m;
    tn = wg / tiles_m;
  }
  const int m0 = tm * BM, n0 = tn * BN;
  const int kbeg = p.klen ? split * p.klen : 0;
  const int kend = p.klen ? min(K, kbeg + p.klen) : K;
  const int nk = (kend - kbeg + BK - 1) / BK;

  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)p.B, 0, p.b_bytes, 0x00020000);

  // ---- per-tile address caches
  // gathered A (forward: x, anchor (2ho, 2wo); dgrad: dy, anchor (i, j)): per DMA instruction the lane's row anchor
  // (y << 16 | x; y = 0x4000 past the last row: out of bounds for every tap), the byte offset of (anchor, this
  // lane's chunk of the K-step) and that chunk's first k in the K-step
  const int Hs = KIND == K_DGRAD ? p.Ho : p.H, Ws = KIND == K_DGRAD ? p.Wo : p.W;  // the gathered image
  int ayx[NIA], ak4[NIA];
  unsigned abase[NIA];
  // an OC image of a dense [k][outer] matrix (forward B = Wf, dgrad B = Wd, wgrad A = dy): the lane's k-row in the
  // K-step and the byte offset of its 4 outer elements in a matrix row, or -1 past the last one
  int akrow[NIA], acol[NIA], bkrow[NIB], bcol[NIB];
  // wgrad B (im2col of x, k-rows = output pixels): the lane's column (tap, channel) is fixed for the tile:
  // (da + 1) | (db + 1) << 2, and the byte shift of its tap and channel from the anchor pixel (bcol < 0: no column)
  int bcd[NIB], bsh[NIB];
  if constexpr (AK) {
    const FastDiv dw = KIND == K_DGRAD ? cg.dWc : p.dWo, dh = KIND == K_DGRAD ? cg.dHc : p.dHo;
    const int wr = KIND == K_DGRAD ? cg.Wc : p.Wo, hr = KIND == K_DGRAD ? cg.Hc : p.Ho;
    const int sc = KIND == K_DGRAD ? 1 : 2;
#pragma unroll
    for (int j = 0; j < NIA; ++j) {
      int r, kc;
      f32_kc_chunk((j * 4 + wave) * 64 + lane, r, kc);
      const int row = m0 + r;
      const int t = fdiv(row, dw), xw = row - t * wr;
      const int n = fdiv(t, dh), yh = t - n * hr;
      const int y = sc * yh, x = sc * xw;
      ayx[j] = row < M ? ((y << 16) | x) : (0x4000 << 16);
      ak4[j] = 4 * kc;
      abase[j] = ((((unsigned)n * Hs + y) * Ws + x) * p.Cs + 4 * kc) * 4u;
    }
  } else {
#pragma unroll
    for (int j = 0; j < NIA; ++j) {
      int oc;
      f32_oc_chunk<BM>((j * 4 + wave) * 64 + lane, akrow[j], oc);
      acol[j] = m0 + 4 * oc < p.M ? (m0 + 4 * oc) * 4 : -1;
    }
  }
#pragma unroll
  for (int j = 0; j < NIB; ++j) {
    int oc;
    f32_oc_chunk<BN>((j * 4 + wave) * 64 + lane, bkrow[j], oc);
    const int col = n0 + 4 * oc;
    bcol[j] = col < p.N ? col * 4 : -1;
    if constexpr (KIND == K_WGRAD) {
      const int tl = fdiv(col, p.dCs), c = col - tl * p.Cs;
      int da, db;
      fwd_shift(p.ks, tl, da, db);
      bcd[j] = ((da + 1) & 3) | (((db + 1) & 3) << 2);  // masked: past N the tap index is out of fwd_shift's range
      bsh[j] = ((da * p.W + db) * p.Cs + c) * 4;
    }
  }

  auto issue = [&](int t) {
    char* slot = smem + (t % STAGES) * SLOT;
    const int k0 = kbeg + t * BK;
    // ---------------- A
    if constexpr (AK) {
      int da_u = 0, db_u = 0, sh_u = 0;
      if (p.fast) {  // one tap per K-step: its shift is wave-uniform
        const int tl = fdiv(k0, p.dCs);
        int tap;
        if constexpr (KIND == K_DGRAD) dgrad_shift(p.ks, cg.ph, cg.pw, tl, da_u, db_u, tap);
        else fwd_shift(p.ks, tl, da_u, db_u);
        sh_u = ((da_u * Ws + db_u) * p.Cs + (k0 - tl * p.Cs)) * 4;
      }
#pragma unroll
      for (int j = 0; j < NIA; ++j) {
        int da = da_u, db = db_u, sh = sh_u;
        const int k = k0 + ak4[j];
        if (!p.fast) {
          const int tl = fdiv(k, p.dCs);
          int tap;
          if constexpr (KIND == K_DGRAD) dgrad_shift(p.ks, cg.ph, cg.pw, tl, da, db, tap);
          else fwd_shift(p.ks, tl, da, db);
          sh = ((da * Ws + db) * p.Cs + (k - tl * p.Cs) - ak4[j]) * 4;
        }
        const int yy = (ayx[j] >> 16) + da, xx = (ayx[j] & 0xffff) + db;
        const bool ok = k < kend && (unsigned)yy < (unsigned)Hs && (unsigned)xx < (unsigned)Ws;
        dma16(ra, slot + (j * 4 + wave) * 1024, ok ? abase[j] + (unsigned)sh : kOOB32);
      }
    } else {  // wgrad: dy [P'][Co], k-row = output pixel
#pragma unroll
      for (int j = 0; j < NIA; ++j) {
        const int k = k0 + akrow[j];
        const bool ok = k < kend && acol[j] >= 0;
        dma16(ra, slot + (j * 4 + wave) * 1024, ok ? (unsigned)k * p.M * 4u + acol[j] : kOOB32);
      }
    }
    // ---------------- B
    char* sb = slot + A_SUB;
#pragma unroll
    for (int j = 0; j < NIB; ++j) {
      const int k = k0 + bkrow[j];
      unsigned off;
      if constexpr (KIND == K_FWD) {  // Wf [T*C][Co]
        off = (k < kend && bcol[j] >= 0) ? (unsigned)k * p.N * 4u + bcol[j] : kOOB32;
      } else if constexpr (KIND == K_DGRAD) {  // Wd [(tap, co)][C]: the class's k-th row is row (tap(k), co)
        const int tl = fdiv(k, p.dCs), co = k - tl * p.Cs;
        int da, db, tap;
        dgrad_shift(p.ks, cg.ph, cg.pw, tl, da, db, tap);
        off = (k < kend && bcol[j] >= 0) ? (unsigned)(tap * p.Cs + co) * p.N * 4u + bcol[j] : kOOB32;
      } else {  // im2col of x: k-row = output pixel k, column = (tap, channel)
        const int t2 = fdiv(k, p.dWo), wo = k - t2 * p.Wo;
        const int n = fdiv(t2, p.dHo), ho = t2 - n * p.Ho;
        const int yy = 2 * ho + (bcd[j] & 3) - 1, xx = 2 * wo + ((bcd[j] >> 2) & 3) - 1;
        const bool ok = k < kend && bcol[j] >= 0 && (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W;
        off = ok ? (((unsigned)n * p.H + 2 * ho) * p.W + 2 * wo) * p.Cs * 4u + (unsigned)bsh[j] : kOOB32;
      }
      dma16(rb, sb + (j * 4 + wave) * 1024, off);
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ---- ring: STAGES - 1 K-steps in flight, a counted vmcnt for the oldest, one raw barrier, the refill of the slot
  // freed one K-step ago, then the fragments and 4 * FM * FN MFMAs; a fresh block accumulator every 4 K-steps
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nk) issue(s);
  for (int it0 = 0; it0 < nk; it0 += 4) {
    f32x4 part[FM][FN];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int it = it0 + u;
      if (it >= nk) break;
      const int ahead = min(STAGES - 2, nk - 1 - it);  // younger stages allowed in flight
      if (STAGES >= 4 && ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * LW) : "memory");
      else if (STAGES >= 3 && ahead >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(LW) : "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      if (it + STAGES - 1 < nk) issue(it + STAGES - 1);
      const char* sa = smem + (it % STAGES) * SLOT;
      const char* sb = sa + A_SUB;
      float a[BK / 4][FM], b[BK / 4][FN];
#pragma unroll
      for (int q = 0; q < BK / 4; ++q) {
#pragma unroll
        for (int i = 0; i < FM; ++i) a[q][i] = f32_frag<AMODE, BM>(sa, wm * (BM / 2) + i * 16 + lc, 4 * q + lr);
#pragma unroll
        for (int j = 0; j < FN; ++j) b[q][j] = f32_frag<BMODE, BN>(sb, wn * (BN / 2) + j * 16 + lc, 4 * q + lr);
      }
      __builtin_amdgcn_sched_barrier(0);  // every read issued before the first MFMA
#pragma unroll
      for (int q = 0; q < BK / 4; ++q)
#pragma unroll
        for (int i = 0; i < FM; ++i)
#pragma unroll
          for (int j = 0; j < FN; ++j)
            part[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                a[q][i], b[q][j], (u || q) ? part[i][j] : (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] += part[i][j];
  }

  if constexpr (KIND == K_FWD) {
    if (p.stats) {
      // BatchNorm training statistics of this output tile from the accumulators, in gemm_f32_dma_kernel's format
      // and reduction order: per column the tile mean and M2 over its valid rows -> stats[tile_m][0 / 1][col]; the
      // 4 lanes sharing a column (xor 16, 32), then the two row-halves of the tile in order
      __builtin_amdgcn_s_barrier();  // every wave is done with the LDS ring: reuse it
      asm volatile("" ::: "memory");
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
          if (n0 + col < p.N) {
            p.stats[(size_t)tm * 2 * p.N + n0 + col] = mean[j];
            p.stats[(size_t)tm * 2 * p.N + p.N + n0 + col] = red[2 * BN + col] + red[3 * BN + col];
          }
        }
      }
    }
  }

  // ---- epilogue: the tile through the idle ring in row parts, then 16-B row vectors
  using TS = TileStage<BM, BN, STAGES * SLOT>;
  constexpr int TLD = TS::TLD, EH = TS::EH, BMH = TS::BMH, Q = TS::Q, RSTEP = TS::RSTEP, NV = TS::NV;
  float* T = reinterpret_cast<float*>(smem);
  const int cq = tid % Q, r0 = tid / Q;
  const int col = n0 + 4 * cq;
#pragma unroll
  for (int h = 0; h < EH; ++h) {
    TS::put(T, acc, h, wm, wn, lr, lc);
    const int mh = m0 + h * BMH;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int r = r0 + i * RSTEP;
      const int m = mh + r;
      if (m >= M || col >= p.N) continue;  // N % 4 == 0: a chunk is all in or all out
      size_t row = m;
      if constexpr (KIND == K_DGRAD) {  // class row -> its pixel of dx
        const int t = fdiv(m, cg.dWc), j = m - t * cg.Wc;
        const int img = fdiv(t, cg.dHc), ii = t - img * cg.Hc;
        row = ((size_t)img * p.H + 2 * ii + cg.ph) * p.W + 2 * j + cg.pw;
      }
      float* d = p.C + (size_t)split * p.split_stride + row * p.N + col;
      *reinterpret_cast<f32x4*>(d) = *reinterpret_cast<const f32x4*>(T + r * TLD + 4 * cq);
    }
  }
}

// torch's 1x1 weight [Co][Ci] -> the forward's B [C][Co] (C >= Ci zero-padded input channels)
__global__ void __launch_bounds__(256) wprep_1x1_kernel(const float* __restrict__ w, int Co, int Ci, int C,
                                                         float* __restrict__ wf) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= C * Co) return;
  const int co = i % Co, ci = i / Co;
  wf[i] = ci < Ci ? w[(size_t)co * Ci + ci] : 0.f;
}

// ------------------------------------------------------------------ host side
static bool al16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// 0 on a supported problem.  Every tensor stays below 2 GiB (buffer offsets are 32-bit); H, W below 2^14 (the row
// anchors pack (y, x) into one register).
static int make_shape(int N, int H, int W, int C, int Co, int ks, Shape* s) {
  if ((ks != 3 && ks != 1) || N < 1 || H < 1 || W < 1 || C < 4 || Co < 4 || C % 4 || Co % 4) return -1;
  if (H >= 0x4000 || W >= 0x4000) return -1;
  s->N = N; s->H = H; s->W = W; s->C = C; s->Co = Co; s->ks = ks;
  s->Ho = (H + 1) / 2; s->Wo = (W + 1) / 2; s->T = ks * ks;
  s->Po = (long long)N * s->Ho * s->Wo;
  const long long lim = 0x80000000ll;
  if ((long long)N * H * W * C * 4 >= lim || s->Po * Co * 4 >= lim || (long long)Co * s->T * C * 4 >= lim) return -4;
  return 0;
}

// tile 0: 128x128, tile 1: 64x64; -1: the default, from the measurements at batch 512 on the ResNet-18 transitions
// (README, "Stride-2 convolutions in fp32"); fitted to those three shapes, nothing is known beyond them.  The 64x64 tile (five workgroups per CU) for the weight gradient and the
// 1x1 kernels, where it was never the slower one; 128x128 for the 3x3 forward from 512 such tiles, and for the 3x3
// data gradient, whose row tiles average 9/4 taps of work, not 9, from 1024.
static int pick_tile32(int kind, int ks, long long rows, int cols, int tile) {
  if (tile >= 0) return tile <= 1 ? tile : -2;
  if (tile != -1) return -2;
  if (kind == K_WGRAD || ks == 1 || cols <= 64 || rows <= 64) return 1;
  const long long t128 = ((rows + 127) / 128) * ((cols + 127) / 128);
  return t128 >= (kind == K_DGRAD ? 1024 : 512) ? 0 : 1;
}

template <int KIND>
static int launch(const Params& p, int tile, dim3 grid, hipStream_t st) {
  if (tile == 0) hipLaunchKernelGGL((conv_s2_kernel<KIND, 128, 128, kStages>), grid, dim3(NT), 0, st, p);
  else hipLaunchKernelGGL((conv_s2_kernel<KIND, 64, 64, kStages>), grid, dim3(NT), 0, st, p);
  return (int)hipGetLastError();
}

static void common_params(Params& p, const Shape& s) {
  p.H = s.H; p.W = s.W; p.Ho = s.Ho; p.Wo = s.Wo; p.ks = s.ks;
  p.dWo = make_fastdiv(s.Wo);
  p.dHo = make_fastdiv(s.Ho);
}

// Splits of the weight gradient over K = P': enough workgroups for every CU's residency (two 128x128 or five
// 64x64 workgroups on 256 CUs), each split at least one 64-k summation block and a multiple of it.
static int wgrad_splits(const Shape& s, int tile) {
  const int bm = tile_rows(tile);
  const long long tiles = (long long)((s.Co + bm - 1) / bm) * ((s.T * s.C + bm - 1) / bm);
  const long long slots = 256 * (tile == 0 ? 2 : 5);
  const long long maxS = (s.Po + 63) / 64;
  long long S = (slots + tiles - 1) / tiles;
  S = S < 1 ? 1 : (S > maxS ? maxS : S);
  const long long klen = ((s.Po + S - 1) / S + 63) / 64 * 64;
  return (int)((s.Po + klen - 1) / klen);  // every split has a K range: no slab needs zeroing
}

}  // namespace f32s2
}  // namespace ddpx

using namespace ddpx;
using namespace ddpx::f32s2;

// torch's fp32 1x1 weight [Co][Ci][1][1] -> wf [C][Co], the forward's B (C >= Ci, zero-padded).  The data
// gradient reads the master itself.
DDPX_API int ddpx_f32_conv1x1_wprep(const float* w, int Co, int Ci, int C, float* wf, hipStream_t st) {
  if (C % 4 || Co % 4 || Co < 4 || Ci < 1 || C < Ci || !w || !wf) return -1;
  hipLaunchKernelGGL(wprep_1x1_kernel, dim3(f32k::nblk((long)C * Co)), dim3(256), 0, st, w, Co, Ci, C, wf);
  return (int)hipGetLastError();
}

// Rows per tile / row tiles of the forward (the statistics rows bn_finalize merges).
DDPX_API int ddpx_f32_conv_s2_fwd_tile_rows(int N, int H, int W, int C, int Co, int ks, int tile) {
  Shape s;
  if (int e = make_shape(N, H, W, C, Co, ks, &s)) return e;
  const int t = pick_tile32(K_FWD, ks, s.Po, Co, tile);
  return t < 0 ? t : tile_rows(t);
}
DDPX_API int ddpx_f32_conv_s2_fwd_tiles_m(int N, int H, int W, int C, int Co, int ks, int tile) {
  const int bm = ddpx_f32_conv_s2_fwd_tile_rows(N, H, W, C, Co, ks, tile);
  if (bm < 0) return bm;
  return (int)(((long long)N * ((H + 1) / 2) * ((W + 1) / 2) + bm - 1) / bm);
}

// y [N*Ho*Wo][Co] = conv(x, W), stride 2.  ks = 3: wf [9*C][Co] (ddpx_f32_conv_wprep), pad 1; ks = 1: wf [C][Co]
// (ddpx_f32_conv1x1_wprep), pad 0.  stats (nullable): [tiles_m][2][Co].
DDPX_API int ddpx_f32_conv_s2_fwd(const float* x, const float* wf, float* y, float* stats, int N, int H, int W, int C,
                                  int Co, int ks, int tile, hipStream_t st) {
  Shape s;
  if (int e = make_shape(N, H, W, C, Co, ks, &s)) return e;
  if (!al16(x) || !al16(wf) || !al16(y)) return -3;
  const int t = pick_tile32(K_FWD, ks, s.Po, Co, tile);
  if (t < 0) return t;
  const int bm = tile_rows(t);
  Params p{};
  common_params(p, s);
  p.A = x; p.B = wf; p.C = y; p.stats = stats;
  p.a_bytes = (unsigned)((size_t)N * H * W * C * 4);
  p.b_bytes = (unsigned)((size_t)Co * s.T * C * 4);
  p.M = (int)s.Po; p.N = Co; p.K = s.T * C;
  p.Cs = C; p.dCs = make_fastdiv(C); p.fast = C % 16 == 0;
  p.tiles_n = (Co + bm - 1) / bm;
  return launch<K_FWD>(p, t, dim3((p.M + bm - 1) / bm * p.tiles_n), st);
}

// Row tiles of the data gradient over its four parity classes.
DDPX_API int ddpx_f32_conv_s2_dgrad_tiles_m(int N, int H, int W, int C, int Co, int ks, int tile) {
  Shape s;
  if (int e = make_shape(N, H, W, C, Co, ks, &s)) return e;
  const int t = pick_tile32(K_DGRAD, ks, (long long)N * H * W, C, tile);
  if (t < 0) return t;
  ClassGeom cls[4];
  return make_classes(s, tile_rows(t), cls);
}

// dx [N][H][W][C] = dgrad(dy [N*Ho*Wo][Co], W).  ks = 3: wd [9][Co][C] (ddpx_f32_conv_wprep); ks = 1: the fp32
// master [Co][C].  Every element of dx is written once (1x1: +0 off the even / even pixels).
DDPX_API int ddpx_f32_conv_s2_dgrad(const float* dy, const float* wd, float* dx, int N, int H, int W, int C, int Co,
                                    int ks, int tile, hipStream_t st) {
  Shape s;
  if (int e = make_shape(N, H, W, C, Co, ks, &s)) return e;
  if (!al16(dy) || !al16(wd) || !al16(dx)) return -3;
  const int t = pick_tile32(K_DGRAD, ks, (long long)N * H * W, C, tile);
  if (t < 0) return t;
  const int bm = tile_rows(t);
  Params p{};
  common_params(p, s);
  p.A = dy; p.B = wd; p.C = dx;
  p.a_bytes = (unsigned)((size_t)s.Po * Co * 4);
  p.b_bytes = (unsigned)((size_t)Co * s.T * C * 4);
  p.N = C;
  p.Cs = Co; p.dCs = make_fastdiv(Co); p.fast = Co % 16 == 0;
  p.tiles_n = (C + bm - 1) / bm;
  const int row_tiles = make_classes(s, bm, p.cls);
  return launch<K_DGRAD>(p, t, dim3(row_tiles * p.tiles_n), st);
}

DDPX_API int ddpx_f32_conv_s2_wgrad_splits(int N, int H, int W, int C, int Co, int ks, int tile) {
  Shape s;
  if (int e = make_shape(N, H, W, C, Co, ks, &s)) return e;
  const int t = pick_tile32(K_WGRAD, ks, Co, s.T * C, tile);
  return t < 0 ? t : wgrad_splits(s, t);
}

// part [S][Co][T*C] = split-K partial weight gradients, S = ddpx_f32_conv_s2_wgrad_splits(...); reduced by
// ddpx_f32_conv_wgrad_reduce (3x3) or ddpx_f32_splitk_reduce (1x1).
DDPX_API int ddpx_f32_conv_s2_wgrad(const float* dy, const float* x, float* part, int S, int N, int H, int W, int C,
                                    int Co, int ks, int tile, hipStream_t st) {
  Shape s;
  if (int e = make_shape(N, H, W, C, Co, ks, &s)) return e;
  if (!al16(dy) || !al16(x) || !al16(part)) return -3;
  const int t = pick_tile32(K_WGRAD, ks, Co, s.T * C, tile);
  if (t < 0) return t;
  if (S != wgrad_splits(s, t)) return -1;
  const int bm = tile_rows(t);
  Params p{};
  common_params(p, s);
  p.A = dy; p.B = x; p.C = part;
  p.a_bytes = (unsigned)((size_t)s.Po * Co * 4);
  p.b_bytes = (unsigned)((size_t)N * H * W * C * 4);
  p.M = Co; p.N = s.T * C; p.K = (int)s.Po;
  p.Cs = C; p.dCs = make_fastdiv(C);
  p.klen = (int)(((s.Po + S - 1) / S + 63) / 64 * 64);
  p.split_stride = (long long)Co * s.T * C;
  p.tiles_n = (p.N + bm - 1) / bm;
  return launch<K_WGRAD>(p, t, dim3((Co + bm - 1) / bm * p.tiles_n, S), st);
}
