// ddpx — stride-2 convolutions in bf16: 3x3 / pad 1 and 1x1 / pad 0, forward, data gradient and weight
// gradient, as implicit GEMMs with a main loop of their own on the building blocks of ddpx_pipe.h (LDS-DMA,
// the swizzled LDS images and their fragment reads, FastDiv, counted vmcnt + raw barrier ring).
//
// x NHWC [N][H][W][C] bf16, Ho = (H + 1) / 2, Wo = (W + 1) / 2 (torch's Conv2d(k=3, s=2, p=1) and
// Conv2d(k=1, s=2, p=0), odd sizes included), P' = N*Ho*Wo, T = 9 or 1 taps, pad = 1 or 0:
//   forward : y[P'][Co]    = A . Wf[Co][T*C]^T, A(p', (tap, c)) = x[n][2ho + ky - pad][2wo + kx - pad][c]
//   dgrad   : the input pixels split into four parity classes (h & 1, w & 1).  A pixel (2i + ph, 2j + pw) only
//             receives the taps with ky = 1 (ph = 0) or ky in {0, 2} (ph = 1), likewise kx: 1, 2, 2 or 4 taps.
//             Each class is a dense GEMM  dx_class[Pc][C] = A_class[Pc][taps*Co] . Wd[(tap, co)][C]  with
//             A_class(r, (tap, co)) = dy[n][i + dho][j + dwo][co]  (dho = 1 for ky = 0, else 0): 9/4 P Co C
//             multiply-adds in all and no product with an inserted zero.  One launch: the workgroup index picks
//             (class, row tile), the four-tap class first so it is not the tail; every class stores its rows of dx
//             strided by parity, every dx element exactly once.  1x1: class (0, 0) has its one tap, the other
//             three classes have none and store +0 (no memset, no second pass).
//   wgrad   : dW[Co][T*C]  = dy[P'][Co]^T . A[P'][T*C], split over K = P' into fp32 slabs (blockIdx.y) that
//             ddpx_conv_wgrad_reduce (3x3) / ddpx_conv1x1_wgrad_reduce sum in slab order: no atomics.
// Every A / B chunk is 16 B of consecutive channels, so a tile is staged with the same lane -> LDS mapping as
// the stride-1 kernels; only the source addresses differ.  What depends on a lane's row only (the anchor pixel,
// its byte base) is computed once per tile; per K-step a chunk costs its tap's shift and a bounds test.  With
// channels % 64 == 0 a 64-wide K-step lies in one tap and the shift is wave-uniform ("fast"); otherwise the tap
// comes from a per-chunk division.
// Two tiles: 128x128 on a 2-deep ring (64 KiB: two workgroups per CU) and 64x64 on a 3-deep ring (48 KiB:
// three per CU); 4 waves (2x2), v_mfma_f32_16x16x32_bf16, fp32 accumulation, one rounding to bf16.
#include "ddpx_conv_s2.h"
#include "ddpx_pipe.h"

namespace ddpx {
namespace s2 {

using namespace pipe;

enum Kind : int { K_FWD = 0, K_DGRAD = 1, K_WGRAD = 2 };

struct Params {
  const unsigned short* A;
  const unsigned short* B;
  void* C;
  float* stats;         // forward: [tiles_m][2][N] (mean, M2) of the stored outputs, or null
  unsigned a_bytes, b_bytes;
  int M, N, K;          // GEMM extents (dgrad: M and K per class)
  int H, W, Ho, Wo;     // input / output image
  int Cs;               // channels of the gathered tensor (x: C; dgrad's dy: Co)
  int Ci;               // input channels (dgrad: leading dimension of dx and Wd)
  int ks;               // 3 or 1
  FastDiv dCs, dWo, dHo;
  int klen;             // wgrad: K per split
  long long split_stride;
  int fast;             // Cs % 64 == 0: one tap per K-step
  int tiles_n;
  ClassGeom cls[4];
};

// lane's (row, first k) of wave-instruction `inst` of a K-contig ROWS x 64 tile / (k-row, column) of an
// M/N-contig one: the LDS images of ddpx_pipe.h's tile_voff
__device__ __forceinline__ void kc_pos(int inst, int lane, int& r, int& c8) {
  r = inst * 8 + (lane >> 3);
  c8 = ((lane & 7) ^ ((r >> 1) & 7)) * 8;
}
template <int ROWS>
__device__ __forceinline__ void nc_pos(int inst, int lane, int& kr, int& col) {
  constexpr int ROWB = ROWS * 2, CPR = ROWB / 16;
  kr = inst * (1024 / ROWB) + lane / CPR;
  const int q = lane % CPR;
  col = (((q >> 1) ^ tr_swz<ROWB>(kr)) << 4) + (q & 1) * 8;
}

// rows of a K-contig gathered operand: anchor pixel (y << 16 | x; y = 0x4000 past the last row: out of
// bounds for every tap) and the byte offset of (anchor pixel, this lane's chunk of a 64-channel block)
template <int ROWS>
struct RowCache {
  static constexpr int NI = ROWS / 32;
  int yx[NI];
  unsigned base[NI];
};

template <int KIND, int BM, int BN, int STAGES>
__global__ void __launch_bounds__(256) s2_kernel(Params p) {
  constexpr int NW = 4, NT = 256;
  constexpr bool AK = KIND != K_WGRAD, BKc = KIND == K_FWD;
  constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, SLOT = A_BYTES + B_BYTES;
  constexpr int FM = BM / 32, FN = BN / 32;
  constexpr int NIA = BM / 32, NIB = BN / 32;
  constexpr int LPW = NIA + NIB;  // DMA instructions per wave per stage
  constexpr int TLD = BN + 4, BMH = 64, EH = BM / BMH, RG = NT / BN;
  constexpr int EPI_BYTES = (BMH * TLD + RG * BN + 2 * BN) * 4;
  static_assert(EPI_BYTES <= STAGES * SLOT, "epilogue staging must fit in the ring");
  static_assert(BM == 64 || BM == 128, "row parts are one wave row (128) or the whole tile (64)");
  __shared__ __attribute__((aligned(1024))) char smem[STAGES * SLOT];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

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
    if (gridDim.y > 1) {  // split-major over all workgroups: an XCD owns whole K ranges (as ddpx_pipe.h)
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
  const int nk = (kend - kbeg + 63) / 64;

  const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc((void*)p.A, 0, p.a_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc((void*)p.B, 0, p.b_bytes, 0x00020000);
  const ConvGeom nogeom{};

  // ---- per-tile address caches
  // A of forward / dgrad: the anchor of every row (forward: x pixel (2ho, 2wo); dgrad: dy pixel (i, j))
  const int Hs = KIND == K_DGRAD ? p.Ho : p.H, Ws = KIND == K_DGRAD ? p.Wo : p.W;  // the gathered image
  RowCache<AK ? BM : 32> arow;
  if constexpr (AK) {
    const FastDiv dw = KIND == K_DGRAD ? cg.dWc : p.dWo, dh = KIND == K_DGRAD ? cg.dHc : p.dHo;
    const int wr = KIND == K_DGRAD ? cg.Wc : p.Wo, hr = KIND == K_DGRAD ? cg.Hc : p.Ho;
    const int sc = KIND == K_DGRAD ? 1 : 2;
#pragma unroll
    for (int j = 0; j < NIA; ++j) {
      int r, c8;
      kc_pos(j * NW + wave, lane, r, c8);
      const int row = m0 + r;
      const int t = fdiv(row, dw), xw = row - t * wr;
      const int n = fdiv(t, dh), yh = t - n * hr;
      const int y = sc * yh, x = sc * xw;
      arow.yx[j] = row < M ? ((y << 16) | x) : (0x4000 << 16);
      arow.base[j] = (unsigned)((((n * Hs + y) * Ws + x) * p.Cs + c8) * 2);
    }
  }
  // B of wgrad: a lane's column (tap, channel) is fixed for the tile: (da + 1) | (db + 1) << 2 | valid << 4 and
  // the byte shift of the tap and channel; B of dgrad: the column's byte offset in a Wd row, or -1
  int bcd[NIB], boff[NIB];
  if constexpr (KIND != K_FWD) {
#pragma unroll
    for (int j = 0; j < NIB; ++j) {
      int kr, col;
      nc_pos<BN>(j * NW + wave, lane, kr, col);
      col += n0;
      if constexpr (KIND == K_WGRAD) {
        const int tl = fdiv(col, p.dCs), c = col - tl * p.Cs;
        int da, db;
        fwd_shift(p.ks, tl, da, db);
        bcd[j] = (da + 1) | ((db + 1) << 2) | ((col < p.N) << 4);
        boff[j] = ((da * p.W + db) * p.Cs + c) * 2;
      } else {
        bcd[j] = kr;
        boff[j] = col < p.N ? col * 2 : -1;
      }
    }
  }

  auto issue = [&](int t) {
    char* slot = smem + (t % STAGES) * SLOT;
    const int k0 = kbeg + t * 64;
    // ---------------- A
    if constexpr (AK) {
      int tl_u = 0, sh_u = 0, da_u = 0, db_u = 0;
      if (p.fast) {  // one tap per K-step: its shift is wave-uniform
        tl_u = fdiv(k0, p.dCs);
        int tap;
        if constexpr (KIND == K_DGRAD) dgrad_shift(p.ks, cg.ph, cg.pw, tl_u, da_u, db_u, tap);
        else fwd_shift(p.ks, tl_u, da_u, db_u);
        sh_u = ((da_u * Ws + db_u) * p.Cs + (k0 - tl_u * p.Cs)) * 2;
      }
#pragma unroll
      for (int j = 0; j < NIA; ++j) {
        int r, c8;
        kc_pos(j * NW + wave, lane, r, c8);
        int da = da_u, db = db_u, sh = sh_u;
        if (!p.fast) {
          const int k = k0 + c8;
          const int tl = fdiv(k, p.dCs);
          int tap;
          if constexpr (KIND == K_DGRAD) dgrad_shift(p.ks, cg.ph, cg.pw, tl, da, db, tap);
          else fwd_shift(p.ks, tl, da, db);
          sh = ((da * Ws + db) * p.Cs + (k - tl * p.Cs) - c8) * 2;
        }
        const int yy = (arow.yx[j] >> 16) + da, xx = (arow.yx[j] & 0xffff) + db;
        const bool ok = k0 + c8 < kend && (unsigned)yy < (unsigned)Hs && (unsigned)xx < (unsigned)Ws;
        dma16(ra, slot + (j * NW + wave) * 1024, ok ? arow.base[j] + (unsigned)sh : kOOB);
      }
    } else {  // wgrad: dy [P'][Co], M-contig
#pragma unroll
      for (int j = 0; j < NIA; ++j)
        dma16(ra, slot + (j * NW + wave) * 1024,
              tile_voff<BM, false, MODE_PLAIN, NW>(nogeom, p.M, m0, p.M, k0, kend, wave, lane, j));
    }
    // ---------------- B
    char* sb = slot + A_BYTES;
#pragma unroll
    for (int j = 0; j < NIB; ++j) {
      unsigned off;
      if constexpr (KIND == K_FWD) {  // Wf [Co][T*C], K-contig
        off = tile_voff<BN, true, MODE_PLAIN, NW>(nogeom, p.K, n0, p.N, k0, kend, wave, lane, j);
      } else if constexpr (KIND == K_DGRAD) {  // Wd [(tap, co)][C]: the class's k-th row is row (tap(k), co)
        const int k = k0 + bcd[j];
        const int tl = fdiv(k, p.dCs), co = k - tl * p.Cs;
        int da, db, tap;
        dgrad_shift(p.ks, cg.ph, cg.pw, tl, da, db, tap);
        off = (k < kend && boff[j] >= 0) ? (unsigned)((tap * p.Cs + co) * p.Ci * 2 + boff[j]) : kOOB;
      } else {  // im2col of x, N-contig: k-row = output pixel
        int kr, col;
        nc_pos<BN>(j * NW + wave, lane, kr, col);
        const int pix = k0 + kr;
        const int t = fdiv(pix, p.dWo), wo = pix - t * p.Wo;
        const int n = fdiv(t, p.dHo), ho = t - n * p.Ho;
        const int yy = 2 * ho + (bcd[j] & 3) - 1, xx = 2 * wo + ((bcd[j] >> 2) & 3) - 1;
        const bool ok = pix < kend && (bcd[j] >> 4) && (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W;
        off = ok ? (unsigned)(((n * p.H + 2 * ho) * p.W + 2 * wo) * p.Cs * 2 + boff[j]) : kOOB;
      }
      dma16(rb, sb + (j * NW + wave) * 1024, off);
    }
  };

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ---- ring: STAGES - 1 K-steps in flight, counted vmcnt for the oldest, raw barrier, refill, MFMA
#pragma unroll
  for (int s = 0; s < STAGES - 1; ++s)
    if (s < nk) issue(s);
  for (int t = 0; t < nk; ++t) {
    if (STAGES >= 3 && t + 1 < nk) wait_vmcnt<(STAGES >= 3 ? LPW : 0)>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + STAGES - 1 < nk) issue(t + STAGES - 1);
    const char* sa = smem + (t % STAGES) * SLOT;
    const char* sb = sa + A_BYTES;
#pragma unroll
    for (int kk = 0; kk < 64; kk += 32) {
      bf16x8 a[FM], b[FN];
      load_frags<BM, AK, FM, BN, BKc, FN>(sa, wm * (BM / 2), sb, wn * (BN / 2), kk, lane, a, b);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }

  // ---- epilogue: 64-row parts of the fp32 tile through LDS, 8-column (16-B bf16 / 2 x 16-B fp32) vectors
  float* T = reinterpret_cast<float*>(smem);
  float* red = T + BMH * TLD;
  float* colres = red + RG * BN;  // [2][BN]
  constexpr int CQ = BN / 8, RSTEP = NT / CQ, NV = BMH / RSTEP;
  const int cq = tid % CQ, r0 = tid / CQ;
  const int n = n0 + 8 * cq;
  float st_n = 0.f, st_mean = 0.f, st_m2 = 0.f;
#pragma unroll
  for (int h = 0; h < EH; ++h) {
    if (h == 0) __builtin_amdgcn_s_barrier();  // every wave is done reading the last slot
    else __syncthreads();
    if (EH == 1 || wm == h) {
      const int mr = (EH == 1 ? wm * (BM / 2) : 0) + 4 * (lane >> 4);
      const int nc = wn * (BN / 2) + (lane & 15);
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) T[(mr + i * 16 + r) * TLD + nc + j * 16] = acc[i][j][r];
    }
    __syncthreads();
    const int mh = m0 + h * BMH;
    if (n < p.N) {  // N % 8 == 0: a chunk is all in or all out
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int r = r0 + i * RSTEP, m = mh + r;
        if (m >= M) continue;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(T + r * TLD + 8 * cq);
        const f32x4 v1 = *reinterpret_cast<const f32x4*>(T + r * TLD + 8 * cq + 4);
        if constexpr (KIND == K_WGRAD) {
          float* d = reinterpret_cast<float*>(p.C) + (size_t)split * p.split_stride + (size_t)m * p.N + n;
          *reinterpret_cast<f32x4*>(d) = v0;
          *reinterpret_cast<f32x4*>(d + 4) = v1;
        } else {
          size_t row = m;
          if constexpr (KIND == K_DGRAD) {  // class row -> its pixel of dx
            const int t = fdiv(m, cg.dWc), j = m - t * cg.Wc;
            const int img = fdiv(t, cg.dHc), ii = t - img * cg.Hc;
            row = ((size_t)img * p.H + 2 * ii + cg.ph) * p.W + 2 * j + cg.pw;
          }
          *reinterpret_cast<u32x4*>(reinterpret_cast<unsigned short*>(p.C) + row * p.N + n) =
              (u32x4){pack_bf2(v0[0], v0[1]), pack_bf2(v0[2], v0[3]), pack_bf2(v1[0], v1[1]), pack_bf2(v1[2], v1[3])};
        }
      }
    }
    if constexpr (KIND == K_FWD) {
      if (p.stats) {
        // BatchNorm statistics of the stored (bf16-rounded) values of this part: column sums over RG row groups,
        // the part's mean, M2 about it; the parts are Chan-merged in order and the tile writes one row
        const int col = tid % BN, rg = tid / BN;
        const int rows_valid = min(BMH, M - mh);
        float s = 0.f;
        for (int r = rg; r < rows_valid; r += RG) s += bf2f(f2bf(T[r * TLD + col]));
        red[rg * BN + col] = s;
        __syncthreads();
        if (tid < BN) {
          float tot = 0.f;
#pragma unroll
          for (int g = 0; g < RG; ++g) tot += red[g * BN + tid];
          colres[tid] = rows_valid > 0 ? tot / (float)rows_valid : 0.f;
        }
        __syncthreads();
        const float mean = colres[col];
        float q = 0.f;
        for (int r = rg; r < rows_valid; r += RG) {
          const float d = bf2f(f2bf(T[r * TLD + col])) - mean;
          q += d * d;
        }
        red[rg * BN + col] = q;
        __syncthreads();
        if (tid < BN && rows_valid > 0) {
          float qb = 0.f;
#pragma unroll
          for (int g = 0; g < RG; ++g) qb += red[g * BN + tid];
          const float nb = (float)rows_valid, mb = colres[tid];
          if (st_n == 0.f) {
            st_n = nb;
            st_mean = mb;
            st_m2 = qb;
          } else {
            const float nn = st_n + nb, d = mb - st_mean;
            st_mean += d * (nb / nn);
            st_m2 += qb + d * d * (st_n * nb / nn);
            st_n = nn;
          }
        }
        if (h == EH - 1 && tid < BN && n0 + tid < p.N) {
          p.stats[((size_t)tm * 2) * p.N + n0 + tid] = st_mean;
          p.stats[((size_t)tm * 2 + 1) * p.N + n0 + tid] = st_m2;
        }
      }
    }
  }
}

// fp32 torch weight [Co][Cr] (1x1) -> bf16 [Co][Cp], zero padded: the forward's Wf and the data gradient's Wd
__global__ void __launch_bounds__(256) weight_prep_1x1_kernel(const float* __restrict__ w, int Co, int Cr, int Cp,
                                                              unsigned short* __restrict__ wf,
                                                              unsigned short* __restrict__ wd) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Co * Cp) return;
  const int c = i % Cp, o = i / Cp;
  const unsigned short h = f2bf(c < Cr ? w[(size_t)o * Cr + c] : 0.f);
  wf[i] = h;
  if (wd != wf) wd[i] = h;
}

// out [Co][Cr] (=|+=) sum_s part[s][Co][Cp] in slab order, or the fused SGD of the parameter: one thread per
// element, 8 slabs' loads in flight
__global__ void __launch_bounds__(256) wgrad1_reduce_kernel(const float* __restrict__ part, int S, int Co, int Cr,
                                                            int Cp, void* __restrict__ out, int out_bf16,
                                                            int accumulate, SgdArgs sgd) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Co * Cr) return;
  const int o = i / Cr, c = i - o * Cr;
  const float* src = part + (size_t)o * Cp + c;
  const size_t slab = (size_t)Co * Cp;
  float acc = 0.f;
  for (int k0 = 0; k0 < S; k0 += 8) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) v[q] = k0 + q < S ? src[(size_t)(k0 + q) * slab] : 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (k0 + q < S) acc += v[q];
  }
  if (sgd.p) {
    sgd_apply(sgd, i, acc, *sgd.lr);
  } else if (out_bf16) {
    unsigned short* d = reinterpret_cast<unsigned short*>(out) + i;
    *d = f2bf(accumulate ? acc + bf2f(*d) : acc);
  } else {
    float* d = reinterpret_cast<float*>(out) + i;
    *d = accumulate ? acc + *d : acc;
  }
}

// ------------------------------------------------------------------ host side
static bool chk16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// 0 on a supported problem.  Every tensor stays below 2 GiB (buffer offsets are 32-bit).
static int make_shape(int N, int H, int W, int C, int Co, int ks, Shape* s) {
  if ((ks != 3 && ks != 1) || N < 1 || H < 1 || W < 1 || C < 8 || Co < 8 || C % 8 || Co % 8) return -1;
  if (H >= 0x4000 || W >= 0x4000) return -1;
  s->N = N; s->H = H; s->W = W; s->C = C; s->Co = Co; s->ks = ks;
  s->Ho = (H + 1) / 2; s->Wo = (W + 1) / 2; s->T = ks * ks;
  s->Po = (long long)N * s->Ho * s->Wo;
  const long long lim = 0x80000000ll;
  if ((long long)N * H * W * C * 2 >= lim || s->Po * Co * 2 >= lim || (long long)Co * s->T * C * 2 >= lim) return -4;
  return 0;
}

// tile 0: 128x128 (two workgroups per CU), tile 1: 64x64 (three per CU).  Default: the large tile when it alone
// gives every CU a workgroup, or (wgrad, whose splits fill the chip either way) when both extents exceed 64.
static int pick_tile(long long rows, int cols, int tile, bool split) {
  if (tile >= 0) return tile <= 1 ? tile : -2;
  if (tile != -1) return -2;
  if (cols <= 64 || rows <= 64) return 1;
  const long long t128 = ((rows + 127) / 128) * ((cols + 127) / 128);
  return (split || t128 >= 256) ? 0 : 1;
}

template <int KIND>
static int launch(const Params& p, int tile, dim3 grid, hipStream_t st) {
  if (tile == 0) hipLaunchKernelGGL((s2_kernel<KIND, 128, 128, 2>), grid, dim3(256), 0, st, p);
  else hipLaunchKernelGGL((s2_kernel<KIND, 64, 64, 3>), grid, dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

static void common_params(Params& p, const Shape& s) {
  p.H = s.H; p.W = s.W; p.Ho = s.Ho; p.Wo = s.Wo; p.ks = s.ks; p.Ci = s.C;
  p.dWo = make_fastdiv(s.Wo);
  p.dHo = make_fastdiv(s.Ho);
}

static int wgrad_splits(const Shape& s, int tile) {
  const int bm = tile_rows(tile);
  const long long tiles = (long long)((s.Co + bm - 1) / bm) * ((s.T * s.C + bm - 1) / bm);
  const long long slots = 256 * (tile == 0 ? 2 : 3);
  const long long maxS = (s.Po + 127) / 128;  // >= 2 K-steps per split
  long long S = (slots + tiles - 1) / tiles;
  S = S < 1 ? 1 : (S > maxS ? maxS : S);
  const long long klen = ((s.Po + S - 1) / S + 63) / 64 * 64;
  return (int)((s.Po + klen - 1) / klen);  // every split has a K range: no slab needs zeroing
}

}  // namespace s2
}  // namespace ddpx

using namespace ddpx;
using ddpx::pipe::make_fastdiv;

DDPX_API int ddpx_conv1x1_weight_prep(const float* w, int Co, int Cr, int Cp, void* wf, void* wd, hipStream_t st) {
  if (Cp % 8 || Cp < Cr || Co < 1 || Cr < 1 || !wf || !wd) return -1;
  hipLaunchKernelGGL(s2::weight_prep_1x1_kernel, dim3((Co * Cp + 255) / 256), dim3(256), 0, st, w, Co, Cr, Cp,
                     (unsigned short*)wf, (unsigned short*)wd);
  return (int)hipGetLastError();
}

// Row tiles / rows per tile of the forward (the statistics rows bn_finalize merges).
DDPX_API int ddpx_conv_s2_fwd_tile_rows(int N, int H, int W, int C, int Co, int ks, int tile) {
  s2::Shape s;
  if (int e = s2::make_shape(N, H, W, C, Co, ks, &s)) return e;
  const int t = s2::pick_tile(s.Po, Co, tile, false);
  return t < 0 ? t : s2::tile_rows(t);
}
DDPX_API int ddpx_conv_s2_fwd_tiles_m(int N, int H, int W, int C, int Co, int ks, int tile) {
  const int bm = ddpx_conv_s2_fwd_tile_rows(N, H, W, C, Co, ks, tile);
  if (bm < 0) return bm;
  return (int)(((long long)N * ((H + 1) / 2) * ((W + 1) / 2) + bm - 1) / bm);
}

// y [N*Ho*Wo][Co] = conv(x, W), stride 2.  ks = 3: wf [Co][9][C], pad 1; ks = 1: wf [Co][C], pad 0.
DDPX_API int ddpx_conv_s2_fwd(const void* x, const void* wf, void* y, float* stats, int N, int H, int W, int C, int Co,
                              int ks, int tile, hipStream_t st) {
  s2::Shape s;
  if (int e = s2::make_shape(N, H, W, C, Co, ks, &s)) return e;
  if (!s2::chk16(x) || !s2::chk16(wf) || !s2::chk16(y)) return -3;
  const int t = s2::pick_tile(s.Po, Co, tile, false);
  if (t < 0) return t;
  const int bm = s2::tile_rows(t);
  s2::Params p{};
  s2::common_params(p, s);
  p.A = (const unsigned short*)x; p.B = (const unsigned short*)wf; p.C = y; p.stats = stats;
  p.a_bytes = (unsigned)((size_t)N * H * W * C * 2);
  p.b_bytes = (unsigned)((size_t)Co * s.T * C * 2);
  p.M = (int)s.Po; p.N = Co; p.K = s.T * C;
  p.Cs = C; p.dCs = make_fastdiv(C); p.fast = C % 64 == 0;
  p.tiles_n = (Co + bm - 1) / bm;
  return s2::launch<s2::K_FWD>(p, t, dim3((p.M + bm - 1) / bm * p.tiles_n), st);
}

// Row tiles of the data gradient over its four parity classes.
DDPX_API int ddpx_conv_s2_dgrad_tiles_m(int N, int H, int W, int C, int Co, int ks, int tile) {
  s2::Shape s;
  if (int e = s2::make_shape(N, H, W, C, Co, ks, &s)) return e;
  const int t = s2::pick_tile((long long)N * H * W, C, tile, false);
  if (t < 0) return t;
  s2::ClassGeom cls[4];
  return s2::make_classes(s, s2::tile_rows(t), cls);
}

// dx [N][H][W][C] = dgrad(dy [N*Ho*Wo][Co], W).  ks = 3: wd [9][Co][C]; ks = 1: wd [Co][C].  Every element of dx
// is written once (1x1: +0 off the even / even pixels).
DDPX_API int ddpx_conv_s2_dgrad(const void* dy, const void* wd, void* dx, int N, int H, int W, int C, int Co, int ks,
                                int tile, hipStream_t st) {
  s2::Shape s;
  if (int e = s2::make_shape(N, H, W, C, Co, ks, &s)) return e;
  if (!s2::chk16(dy) || !s2::chk16(wd) || !s2::chk16(dx)) return -3;
  // (the default weighs the tiles of all four classes together: about P / 128 row tiles)
  const int t = s2::pick_tile((long long)N * H * W, C, tile, false);
  if (t < 0) return t;
  const int bm = s2::tile_rows(t);
  s2::Params p{};
  s2::common_params(p, s);
  p.A = (const unsigned short*)dy; p.B = (const unsigned short*)wd; p.C = dx;
  p.a_bytes = (unsigned)((size_t)s.Po * Co * 2);
  p.b_bytes = (unsigned)((size_t)Co * s.T * C * 2);
  p.N = C;
  p.Cs = Co; p.dCs = make_fastdiv(Co); p.fast = Co % 64 == 0;
  p.tiles_n = (C + bm - 1) / bm;
  const int row_tiles = s2::make_classes(s, bm, p.cls);
  return s2::launch<s2::K_DGRAD>(p, t, dim3(row_tiles * p.tiles_n), st);
}

DDPX_API int ddpx_conv_s2_wgrad_splits(int N, int H, int W, int C, int Co, int ks, int tile) {
  s2::Shape s;
  if (int e = s2::make_shape(N, H, W, C, Co, ks, &s)) return e;
  const int t = s2::pick_tile(Co, s.T * C, tile, true);
  return t < 0 ? t : s2::wgrad_splits(s, t);
}

// part [S][Co][T*C] (fp32) = split-K partial weight gradients, S = ddpx_conv_s2_wgrad_splits(...).
DDPX_API int ddpx_conv_s2_wgrad(const void* dy, const void* x, float* part, int S, int N, int H, int W, int C, int Co,
                                int ks, int tile, hipStream_t st) {
  s2::Shape s;
  if (int e = s2::make_shape(N, H, W, C, Co, ks, &s)) return e;
  if (!s2::chk16(dy) || !s2::chk16(x) || !s2::chk16(part)) return -3;
  const int t = s2::pick_tile(Co, s.T * C, tile, true);
  if (t < 0) return t;
  if (S != s2::wgrad_splits(s, t)) return -1;
  const int bm = s2::tile_rows(t);
  s2::Params p{};
  s2::common_params(p, s);
  p.A = (const unsigned short*)dy; p.B = (const unsigned short*)x; p.C = part;
  p.a_bytes = (unsigned)((size_t)s.Po * Co * 2);
  p.b_bytes = (unsigned)((size_t)N * H * W * C * 2);
  p.M = Co; p.N = s.T * C; p.K = (int)s.Po;
  p.Cs = C; p.dCs = make_fastdiv(C);
  p.klen = (int)(((s.Po + S - 1) / S + 63) / 64 * 64);
  p.split_stride = (long long)Co * s.T * C;
  p.tiles_n = (p.N + bm - 1) / bm;
  return s2::launch<s2::K_WGRAD>(p, t, dim3((Co + bm - 1) / bm * p.tiles_n, S), st);
}

DDPX_API int ddpx_conv1x1_wgrad_reduce(const float* part, int S, int Co, int Cr, int Cp, void* out, int out_bf16,
                                       int accumulate, float* sgd_p, float* sgd_buf, void* sgd_shadow,
                                       const float* sgd_lr, float sgd_mom, float sgd_wd, hipStream_t st) {
  if (S < 1 || Co < 1 || Cr < 1 || Cp < Cr || (!out && !sgd_p) || (sgd_p && !sgd_lr)) return -1;
  hipLaunchKernelGGL(s2::wgrad1_reduce_kernel, dim3((Co * Cr + 255) / 256), dim3(256), 0, st, part, S, Co, Cr, Cp, out,
                     out_bf16, accumulate, SgdArgs{sgd_p, sgd_buf, (unsigned short*)sgd_shadow, sgd_lr, sgd_mom, sgd_wd});
  return (int)hipGetLastError();
}
