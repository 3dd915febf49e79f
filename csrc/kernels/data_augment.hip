// ddpx — GPU-resident data pipeline: gather + RandomCrop(32, padding=4) +
// RandomHorizontalFlip + ToTensor in one kernel.
//
// Replaces the reference's per-sample CPU PIL transforms and the blocking
// pinned H2D copy of every batch (/root/reference/singlegpu.py:155-159 train
// transform, :114-115 `source.to(gpu_id)`).  The uint8
// dataset ([N][3][32][32], 150 MiB for CIFAR-10 train) stays resident in HBM
// (and mostly in the 256 MiB Infinity Cache); each step gathers the sampler's
// indices, applies a per-sample crop offset and flip drawn from a counter-based
// hash, scales by 1/255 (no mean/std, as in the reference) and writes the batch
// in the layout the model consumes.
#include "ddpx_common.h"

namespace ddpx {

enum OutLayout : int { OUT_NCHW_F32 = 0, OUT_NCHW_BF16 = 1, OUT_NHWC_BF16 = 2, OUT_NHWC_F32 = 3, OUT_NHWC8_BF16 = 4,
                       OUT_NHWC4_F32 = 5 };

// x mod m for a small m (the crop range 2 * pad + 1) with 32-bit operations only: x = hi * 2^32 + lo, so
// x mod m = ((hi mod m) * (2^32 mod m) + lo mod m) mod m — exactly the 64-bit remainder the CPU twin takes.
__device__ __forceinline__ unsigned mod64(uint64_t x, int m) {
  const unsigned um = (unsigned)m;
  const unsigned p32 = (0xFFFFFFFFu % um + 1u) % um;
  const unsigned hi = (unsigned)(x >> 32) % um, lo = (unsigned)x % um;
  return (hi * p32 + lo) % um;  // < m * m + m: no overflow for the small m used here (m < 65536)
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// NCHW / flat layouts: one thread per (sample, channel, row, 8-pixel group);
// each thread gathers its 8 source bytes (L2/Infinity-Cache hits) and writes
// 8 contiguous outputs with one 16-B (bf16) or two 16-B (fp32) stores.
// NHWC layouts: one thread per (sample, row, pixel), C channels each.
// Per-sample crop offsets and flip, from the counter-based hash (the CPU twin draws the same).
// Cutout (cut = the square's side S > 0, training only): the centre (cy, cx) of the sample's erased square, in
// output coordinates, from a second hash of the sample's crop / flip hash: the CutMix centre's arithmetic.
constexpr uint64_t kCutSalt = 0xA0761D6478BD642Full;
constexpr int kPrm = 5;  // ints per sample in a workgroup's LDS parameter block: dy, dx, flip, cy, cx

__device__ __forceinline__ void sample_params(uint64_t seed, int b, int pad, int train, int cut, int H, int W, int& dy,
                                              int& dx, int& flip, int& cy, int& cx) {
  dy = pad;
  dx = pad;
  flip = 0;
  cy = cx = 0;
  if (train) {
    const uint64_t r = splitmix64(seed ^ (0xD1B54A32D192ED03ull * (uint64_t)(b + 1)));
    dy = (int)mod64(r, 2 * pad + 1);
    dx = (int)mod64(r >> 16, 2 * pad + 1);
    flip = (int)((r >> 40) & 1);
    if (cut > 0) {
      const uint64_t rc = splitmix64(r ^ kCutSalt);
      cy = (int)mod64(rc, H);
      cx = (int)mod64(rc >> 20, W);
    }
  }
}

// Whether output pixel (y, x) lies in the sample's Cutout square: rows [cy - S / 2, cy - S / 2 + S), the same for the
// columns; the image bounds cut the square off (a square centred near the border is not shifted inwards).
// S = 0: never.
__device__ __forceinline__ bool cut_hit(int S, int cy, int cx, int y, int x) {
  const int y0 = cy - S / 2, x0 = cx - S / 2;
  return y >= y0 && y < y0 + S && x >= x0 && x < x0 + S;
}

// 8 consecutive output pixels [xg * 8, +8) of one source row (`row`: the row's first byte, row 0 when the crop
// put the row outside the image: row_ok false), cropped, flipped and scaled to [0, 1].
__device__ __forceinline__ void gather_row8(const uint8_t* __restrict__ row, int W, int xg, int dx, int pad, int flip,
                                            bool row_ok, float (&v)[8]) {
  const float inv = 1.f / 255.f;
  if (W == 32 && (((uintptr_t)row) & 15) == 0) {
    // CIFAR rows: the whole 32-B source row in two 16-B loads (2 address operations per lane instead of 8
    // byte loads), bytes picked in registers
    const u32x4 lo = *reinterpret_cast<const u32x4*>(row), hi = *reinterpret_cast<const u32x4*>(row + 16);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ox = xg * 8 + j;
      const int x = flip ? (W - 1 - ox) : ox;
      const int sx = x + dx - pad;
      const int d = (sx >> 2) & 7;
      const unsigned w = d < 4 ? (d < 2 ? (d == 0 ? lo[0] : lo[1]) : (d == 2 ? lo[2] : lo[3]))
                               : (d < 6 ? (d == 4 ? hi[0] : hi[1]) : (d == 6 ? hi[2] : hi[3]));
      const unsigned byte = (w >> (8 * (sx & 3))) & 0xFFu;
      v[j] = (row_ok && sx >= 0 && sx < W) ? (float)byte * inv : 0.f;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ox = xg * 8 + j;                 // output column
      const int x = flip ? (W - 1 - ox) : ox;    // column of the cropped image
      const int sx = x + dx - pad;
      v[j] = (row_ok && sx >= 0 && sx < W) ? (float)row[sx] * inv : 0.f;
    }
  }
}

// NCHW / flat: 8 outputs at element offset o, one 16-B (bf16) or two 16-B (fp32) stores.
__device__ __forceinline__ void store_row8(int layout, void* __restrict__ out, size_t o, const float (&v)[8]) {
  if (layout == OUT_NCHW_BF16) {
    u32x4 pk = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
    *reinterpret_cast<u32x4*>(reinterpret_cast<unsigned short*>(out) + o) = pk;
  } else {
    f32x4* d = reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + o);
    d[0] = (f32x4){v[0], v[1], v[2], v[3]};
    d[1] = (f32x4){v[4], v[5], v[6], v[7]};
  }
}

// NHWC layouts: pixel number p of the batch, val(cc) = channel cc's value (cc < C).
template <class V>
__device__ __forceinline__ void store_pixel(int layout, void* __restrict__ out, size_t p, int C, V val) {
  if (layout == OUT_NHWC8_BF16) {
    // NHWC with the channels zero-padded to 8 (16-B pixels: the conv0 implicit-GEMM input)
    float v[8];
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) v[cc] = cc < C ? val(cc) : 0.f;
    u32x4 pk = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
    *reinterpret_cast<u32x4*>(reinterpret_cast<unsigned short*>(out) + p * 8) = pk;
    return;
  }
  if (layout == OUT_NHWC4_F32) {
    // NHWC fp32 with the channels zero-padded to 4 (16-B pixels: the fp32 conv0 implicit-GEMM input)
    f32x4 v;
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) v[cc] = cc < C ? val(cc) : 0.f;
    *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + p * 4) = v;
    return;
  }
  for (int cc = 0; cc < C; ++cc) {
    const float v = val(cc);
    if (layout == OUT_NHWC_BF16) reinterpret_cast<unsigned short*>(out)[p * C + cc] = f2bf(v);
    else reinterpret_cast<float*>(out)[p * C + cc] = v;
  }
}

// prm (optional, LDS): [dy, dx, flip, cy, cx] of samples b0, b0 + 1, ... drawn once per workgroup (the hash and its
// 64-bit remainders cost more VALU than the rest of a thread's work, and up to 384 threads share a sample).
// cut: the Cutout side S (0: off; the entry points pass 0 for an evaluation batch): the sample's square is written
// as 0.0 after crop and flip.
__device__ __forceinline__ void augment_body(const uint8_t* __restrict__ images, const int64_t* __restrict__ labels,
                                             const int64_t* __restrict__ idx, int B, int C, int H, int W, int pad,
                                             uint64_t seed, int train, int cut, int layout, void* __restrict__ out,
                                             int64_t* __restrict__ tgt_out, const int* prm = nullptr, int b0 = 0) {
  const bool nhwc = (layout == OUT_NHWC_BF16 || layout == OUT_NHWC_F32 || layout == OUT_NHWC8_BF16 ||
                     layout == OUT_NHWC4_F32);
  const int G = W / 8;  // 8-pixel groups per row (W % 8 == 0 checked on the host)
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = nhwc ? B * H * W : B * C * H * G;
  if (t >= total) return;
  int b, c = 0, y, xg = 0, xo = 0;
  if (nhwc) {
    xo = t % W;
    y = (t / W) % H;
    b = t / (W * H);
  } else {
    xg = t % G;
    y = (t / G) % H;
    c = (t / (G * H)) % C;
    b = t / (G * H * C);
  }
  const int64_t src = idx ? idx[b] : b;
  int dy, dx, flip, cy, cx;
  if (prm) {
    const int* p = prm + (b - b0) * kPrm;
    dy = p[0], dx = p[1], flip = p[2], cy = p[3], cx = p[4];
  } else {
    sample_params(seed, b, pad, train, cut, H, W, dy, dx, flip, cy, cx);
  }
  if (tgt_out && y == 0 && c == 0 && xg == 0 && xo == 0) tgt_out[b] = labels[src];
  const int sy = y + dy - pad;
  const bool row_ok = (sy >= 0) && (sy < H);
  const float inv = 1.f / 255.f;
  const uint8_t* img = images + (size_t)src * C * H * W;
  if (!nhwc) {
    const uint8_t* row = img + (size_t)c * H * W + (size_t)(row_ok ? sy : 0) * W;
    float v[8];
    gather_row8(row, W, xg, dx, pad, flip, row_ok, v);
    if (cut > 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = cut_hit(cut, cy, cx, y, xg * 8 + j) ? 0.f : v[j];
    }
    store_row8(layout, out, (((size_t)b * C + c) * H + y) * W + xg * 8, v);
  } else {
    const int x = flip ? (W - 1 - xo) : xo;
    const int sx = x + dx - pad;
    const bool ok = row_ok && sx >= 0 && sx < W && !cut_hit(cut, cy, cx, y, xo);
    store_pixel(layout, out, ((size_t)b * H + y) * W + xo, C,
                [&](int cc) { return ok ? (float)img[(size_t)cc * H * W + sy * W + sx] * inv : 0.f; });
  }
}

// ---------------------------------------------------------------- Mixup / CutMix (timm's "batch" mode)
// Sample b is mixed with sample B - 1 - b of the same batch, the partner gathered with its own crop and flip.
// All mixing randomness is one draw per batch from the counter hash (seed already carries the step), so every
// workgroup derives the same draw and a captured step needs no host work.  lam ~ Beta(alpha, alpha) comes
// from a host-built quantile table (1024 equal-probability bins per mode, with the CutMix box extents worked
// out on the host in fp64): no transcendental maths here, and the CPU twin reads the same table.
struct MixRow {
  float lam;
  int cut_h, cut_w;
};
constexpr int kMixBins = 1024;
constexpr uint64_t kMixSalt = 0x8CB92BA72F3D8DD7ull;
enum MixMode : int { MIX_NONE = 0, MIX_MIXUP = 1, MIX_CUTMIX = 2 };

struct MixDraw {
  int mode;
  float wlam;            // label weight of the sample's own target (1 when not mixed)
  float lam, oml;        // Mixup: pixel weights lam and 1 - lam
  int y0, y1, x0, x1;    // CutMix: the partner's box in output coordinates, [y0, y1) x [x0, x1)
};

// modes: bit 0 Mixup enabled, bit 1 CutMix enabled.  p_apply / p_switch: probabilities scaled to 2^24.
__device__ __forceinline__ MixDraw mix_draw(uint64_t seed, int H, int W, int modes, unsigned p_apply,
                                            unsigned p_switch, const MixRow* __restrict__ table) {
  MixDraw d = {MIX_NONE, 1.f, 1.f, 0.f, 0, 0, 0, 0};
  const uint64_t r = splitmix64(seed ^ kMixSalt);
  if (!modes || (unsigned)(r & 0xFFFFFFu) >= p_apply) return d;
  const bool cut = modes == 3 ? (unsigned)((r >> 24) & 0xFFFFFFu) < p_switch : modes == 2;
  const MixRow row = table[(cut ? kMixBins : 0) + (int)((r >> 48) & (uint64_t)(kMixBins - 1))];
  if (!cut) {
    d.mode = MIX_MIXUP;
    d.lam = d.wlam = row.lam;
    d.oml = 1.f - row.lam;
    return d;
  }
  const uint64_t r2 = splitmix64(r);
  const int cy = (int)mod64(r2, H), cx = (int)mod64(r2 >> 20, W);
  d.mode = MIX_CUTMIX;
  d.y0 = min(max(cy - row.cut_h / 2, 0), H);
  d.y1 = min(max(cy + row.cut_h / 2, 0), H);
  d.x0 = min(max(cx - row.cut_w / 2, 0), W);
  d.x1 = min(max(cx + row.cut_w / 2, 0), W);
  d.wlam = 1.f - (float)((d.y1 - d.y0) * (d.x1 - d.x0)) / (float)(H * W);  // correctly rounded fp32 division
  return d;
}

// lam * a + oml * b as two rounded products and a rounded sum: contraction off for these three operations (the
// __fmul_rn / __fadd_rn intrinsics are plain operators here and would still be fused into an FMA), so torch's
// separate fp32 multiply and add kernels on the CPU give the same bits.
__device__ __forceinline__ float blend_rn(float lam, float a, float oml, float b) {
#pragma clang fp contract(off)
  const float pa = lam * a;
  const float pb = oml * b;
  return pa + pb;
}

// The mixed batch (d.mode != MIX_NONE): augment_body's thread layout, two gathers per output.  Mixup blends
// the scaled fp32 pixels with separately rounded products and sum (blend_rn); CutMix takes the partner's pixel inside the box.  prm: [dy, dx, flip] of samples
// b0 .. b0 + nb - 1, then of their partners.
__device__ __forceinline__ void augment_mix_body(const uint8_t* __restrict__ images, const int64_t* __restrict__ idx,
                                                 int B, int C, int H, int W, int pad, uint64_t seed, int cut,
                                                 int layout, void* __restrict__ out, const MixDraw& d, const int* prm,
                                                 int b0, int nb) {
  const bool nhwc = (layout == OUT_NHWC_BF16 || layout == OUT_NHWC_F32 || layout == OUT_NHWC8_BF16 ||
                     layout == OUT_NHWC4_F32);
  const int G = W / 8;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int total = nhwc ? B * H * W : B * C * H * G;
  if (t >= total) return;
  int b, c = 0, y, xg = 0, xo = 0;
  if (nhwc) {
    xo = t % W;
    y = (t / W) % H;
    b = t / (W * H);
  } else {
    xg = t % G;
    y = (t / G) % H;
    c = (t / (G * H)) % C;
    b = t / (G * H * C);
  }
  const int pb = B - 1 - b;
  // Cutout: each gathered sample is erased by its own square before the mix (the partner's pixels by the partner's)
  int dy, dx, flip, cy, cx, qy, qx, qflip, qcy, qcx;
  if (prm) {
    const int* pa = prm + (b - b0) * kPrm;
    const int* pp = pa + nb * kPrm;
    dy = pa[0], dx = pa[1], flip = pa[2], cy = pa[3], cx = pa[4];
    qy = pp[0], qx = pp[1], qflip = pp[2], qcy = pp[3], qcx = pp[4];
  } else {
    sample_params(seed, b, pad, 1, cut, H, W, dy, dx, flip, cy, cx);
    sample_params(seed, pb, pad, 1, cut, H, W, qy, qx, qflip, qcy, qcx);
  }
  const uint8_t* img = images + (size_t)(idx ? idx[b] : b) * C * H * W;
  const uint8_t* pim = images + (size_t)(idx ? idx[pb] : pb) * C * H * W;
  const int sy = y + dy - pad, ty = y + qy - pad;
  const bool row_ok = sy >= 0 && sy < H, prow_ok = ty >= 0 && ty < H;
  const bool cutmix = d.mode == MIX_CUTMIX;
  const bool row_in = cutmix && y >= d.y0 && y < d.y1;
  const float inv = 1.f / 255.f;
  if (!nhwc) {
    float v[8];
    gather_row8(img + (size_t)c * H * W + (size_t)(row_ok ? sy : 0) * W, W, xg, dx, pad, flip, row_ok, v);
    if (cut > 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = cut_hit(cut, cy, cx, y, xg * 8 + j) ? 0.f : v[j];
    }
    if (!cutmix || row_in) {
      float u[8];
      gather_row8(pim + (size_t)c * H * W + (size_t)(prow_ok ? ty : 0) * W, W, xg, qx, pad, qflip, prow_ok, u);
      if (cut > 0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) u[j] = cut_hit(cut, qcy, qcx, y, xg * 8 + j) ? 0.f : u[j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ox = xg * 8 + j;
        if (cutmix) v[j] = (ox >= d.x0 && ox < d.x1) ? u[j] : v[j];
        else v[j] = blend_rn(d.lam, v[j], d.oml, u[j]);
      }
    }
    store_row8(layout, out, (((size_t)b * C + c) * H + y) * W + xg * 8, v);
  } else {
    const int sx = (flip ? (W - 1 - xo) : xo) + dx - pad;
    const int tx = (qflip ? (W - 1 - xo) : xo) + qx - pad;
    const bool ok = row_ok && sx >= 0 && sx < W && !cut_hit(cut, cy, cx, y, xo);
    const bool pok = prow_ok && tx >= 0 && tx < W && !cut_hit(cut, qcy, qcx, y, xo);
    const bool in_box = row_in && xo >= d.x0 && xo < d.x1;
    auto own = [&](int cc) { return ok ? (float)img[(size_t)cc * H * W + sy * W + sx] * inv : 0.f; };
    auto partner = [&](int cc) { return pok ? (float)pim[(size_t)cc * H * W + ty * W + tx] * inv : 0.f; };
    store_pixel(layout, out, ((size_t)b * H + y) * W + xo, C, [&](int cc) {
      if (cutmix) return in_box ? partner(cc) : own(cc);
      return blend_rn(d.lam, own(cc), d.oml, partner(cc));
    });
  }
}

// cursor (optional): device-side step counter k (read only).  The batch is rows [k % nbatch * B, +B) of
// the epoch's index permutation `idx` and the augmentation seed is seed + k (DeviceLoader.batch_seed(k)),
// so a captured training step draws a new batch on every replay with no host work.  The counter is
// advanced by its owner (the training step's LR-table kernel); advancing it here would need a
// completion counter every workgroup hits with an atomic — measured 26 vs 6.6 us for 768 workgroups.
__global__ void __launch_bounds__(256)
augment_kernel(const uint8_t* __restrict__ images, const int64_t* __restrict__ labels,
               const int64_t* __restrict__ idx, int B, int C, int H, int W, int pad, uint64_t seed,
               int train, int cut, int layout, void* __restrict__ out, int64_t* __restrict__ tgt_out,
               const int* __restrict__ cursor, int nbatch) {
  if (cursor) {
    const int k = *cursor;
    idx += (size_t)(k % nbatch) * B;
    seed += (uint64_t)k;
  }
  constexpr int kMaxSamples = 8;
  __shared__ int prm[kMaxSamples * kPrm];
  const bool nhwc = (layout == OUT_NHWC_BF16 || layout == OUT_NHWC_F32 || layout == OUT_NHWC8_BF16 ||
                     layout == OUT_NHWC4_F32);
  const int per = nhwc ? H * W : C * H * (W / 8);  // threads per sample
  const int total = B * per;
  const int t0 = blockIdx.x * blockDim.x;
  const int t1 = min(total, t0 + (int)blockDim.x) - 1;
  const int b0 = t0 / per, nb = t1 >= t0 ? t1 / per - b0 + 1 : 0;
  if (nb > kMaxSamples) {  // tiny images: every thread draws its own sample's parameters
    augment_body(images, labels, idx, B, C, H, W, pad, seed, train, cut, layout, out, tgt_out);
    return;
  }
  if ((int)threadIdx.x < nb) {
    int* p = prm + threadIdx.x * kPrm;
    sample_params(seed, b0 + (int)threadIdx.x, pad, train, cut, H, W, p[0], p[1], p[2], p[3], p[4]);
  }
  __syncthreads();
  augment_body(images, labels, idx, B, C, H, W, pad, seed, train, cut, layout, out, tgt_out, prm, b0);
}

// augment_kernel with the batch's Mixup / CutMix draw.  The draw (one thread) and the crop / flip parameters of
// the workgroup's samples and of their partners go to LDS once.  A batch that draws "no mix" runs augment_body
// itself, so it writes the plain kernel's bits; a mixed one runs augment_mix_body.  Either way the first thread
// of each sample also writes the partner's label and the label weight.
__global__ void __launch_bounds__(256)
augment_mix_kernel(const uint8_t* __restrict__ images, const int64_t* __restrict__ labels,
                   const int64_t* __restrict__ idx, int B, int C, int H, int W, int pad, uint64_t seed, int cut,
                   int layout, void* __restrict__ out, int64_t* __restrict__ tgt_out, const int* __restrict__ cursor,
                   int nbatch,
                   const MixRow* __restrict__ table, int modes, unsigned p_apply, unsigned p_switch,
                   int64_t* __restrict__ tgt_b_out, float* __restrict__ lam_out) {
  if (cursor) {
    const int k = *cursor;
    idx += (size_t)(k % nbatch) * B;
    seed += (uint64_t)k;
  }
  constexpr int kMaxSamples = 8;
  __shared__ int prm[2 * kMaxSamples * kPrm];
  __shared__ MixDraw draw;
  const bool nhwc = (layout == OUT_NHWC_BF16 || layout == OUT_NHWC_F32 || layout == OUT_NHWC8_BF16 ||
                     layout == OUT_NHWC4_F32);
  const int per = nhwc ? H * W : C * H * (W / 8);  // threads per sample
  const int total = B * per;
  const int t0 = blockIdx.x * blockDim.x;
  const int t1 = min(total, t0 + (int)blockDim.x) - 1;
  const int b0 = t0 / per, nb = t1 >= t0 ? t1 / per - b0 + 1 : 0;
  const bool shared_prm = nb <= kMaxSamples;  // else tiny images: every thread draws its own parameters
  const int tid = threadIdx.x;
  if (tid == (int)blockDim.x - 1) draw = mix_draw(seed, H, W, modes, p_apply, p_switch, table);
  if (shared_prm && tid < 2 * nb) {
    int* p = prm + tid * kPrm;
    sample_params(seed, tid < nb ? b0 + tid : B - 1 - (b0 + tid - nb), pad, 1, cut, H, W, p[0], p[1], p[2], p[3], p[4]);
  }
  __syncthreads();
  const MixDraw d = draw;
  const int t = t0 + tid;
  if (t < total && t % per == 0) {
    const int b = t / per;
    tgt_b_out[b] = labels[idx ? idx[B - 1 - b] : B - 1 - b];
    lam_out[b] = d.wlam;
  }
  if (d.mode == MIX_NONE) {
    augment_body(images, labels, idx, B, C, H, W, pad, seed, 1, cut, layout, out, tgt_out, shared_prm ? prm : nullptr,
                 b0);
    return;
  }
  if (t < total && t % per == 0) tgt_out[t / per] = labels[idx ? idx[t / per] : t / per];
  augment_mix_body(images, idx, B, C, H, W, pad, seed, cut, layout, out, d, shared_prm ? prm : nullptr, b0, nb);
}

}  // namespace ddpx

using namespace ddpx;

// cutout: the side S of the Cutout square (0: off), 0 <= S <= 2 * max(H, W), -7 beyond (and, for S > 0, image sides
// in 1..4096: the centre's mod64).  An evaluation batch (train == 0) is never erased.
static int cutout_check(int cutout, int H, int W) {
  if (cutout < 0 || cutout > 2 * (H > W ? H : W)) return -7;
  if (cutout > 0 && (H < 1 || H > 4096 || W < 1 || W > 4096)) return -7;
  return 0;
}

DDPX_API int ddpx_augment(const void* images, const int64_t* labels, const int64_t* idx, int B, int C, int H,
                          int W, int pad, uint64_t seed, int train, int cutout, int layout, void* out,
                          int64_t* tgt_out, hipStream_t s) {
  if (B <= 0) return 0;
  if (W % 8) return -1;
  if (pad < 0 || pad > 4096) return -4;  // mod64's 32-bit arithmetic assumes a small crop range
  if (cutout_check(cutout, H, W)) return -7;
  const bool nhwc = (layout == OUT_NHWC_BF16 || layout == OUT_NHWC_F32 || layout == OUT_NHWC8_BF16 ||
                     layout == OUT_NHWC4_F32);
  if ((layout == OUT_NHWC8_BF16 && C > 8) || (layout == OUT_NHWC4_F32 && C > 4)) return -2;
  const int n = nhwc ? B * H * W : B * C * H * (W / 8);
  hipLaunchKernelGGL(augment_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const uint8_t*)images, labels,
                     idx, B, C, H, W, pad, seed, train, train ? cutout : 0, layout, out, tgt_out, (const int*)nullptr,
                     1);
  return (int)hipGetLastError();
}

// Training batch with Mixup / CutMix.  table: device MixRow[2][1024] (row 0 Mixup, row 1 CutMix quantiles);
// modes: bit 0 Mixup, bit 1 CutMix; p_apply / p_switch: probabilities scaled to 2^24; tgt_b_out [B] int64 and
// lam_out [B] fp32 receive the partner's label and the label weight.  cursor / nbatch as ddpx_augment_cursor
// (cursor null: idx is the batch itself).
static int augment_mix_launch(const void* images, const int64_t* labels, const int64_t* idx, int nbatch, int B, int C,
                              int H, int W, int pad, uint64_t seed, int cutout, int layout, void* out,
                              int64_t* tgt_out, const int* cursor, const void* table, int modes, unsigned p_apply,
                              unsigned p_switch, int64_t* tgt_b_out, float* lam_out, hipStream_t s) {
  if (W % 8) return -1;
  if (pad < 0 || pad > 4096 || H < 1 || H > 4096 || W > 4096) return -4;  // mod64's 32-bit arithmetic
  if (modes < 0 || modes > 3 || (modes && !table) || !tgt_out || !tgt_b_out || !lam_out) return -5;
  if (p_apply > (1u << 24) || p_switch > (1u << 24)) return -6;
  if (cutout_check(cutout, H, W)) return -7;
  const bool nhwc = (layout == OUT_NHWC_BF16 || layout == OUT_NHWC_F32 || layout == OUT_NHWC8_BF16 ||
                     layout == OUT_NHWC4_F32);
  if ((layout == OUT_NHWC8_BF16 && C > 8) || (layout == OUT_NHWC4_F32 && C > 4)) return -2;
  const int n = nhwc ? B * H * W : B * C * H * (W / 8);
  hipLaunchKernelGGL(augment_mix_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const uint8_t*)images, labels, idx,
                     B, C, H, W, pad, seed, cutout, layout, out, tgt_out, cursor, nbatch, (const MixRow*)table, modes,
                     p_apply, p_switch, tgt_b_out, lam_out);
  return (int)hipGetLastError();
}

DDPX_API int ddpx_augment_mix(const void* images, const int64_t* labels, const int64_t* idx, int B, int C, int H,
                              int W, int pad, uint64_t seed, int cutout, int layout, void* out, int64_t* tgt_out,
                              const void* table, int modes, unsigned p_apply, unsigned p_switch, int64_t* tgt_b_out,
                              float* lam_out, hipStream_t s) {
  if (B <= 0) return 0;
  return augment_mix_launch(images, labels, idx, 1, B, C, H, W, pad, seed, cutout, layout, out, tgt_out, nullptr,
                            table, modes, p_apply, p_switch, tgt_b_out, lam_out, s);
}

DDPX_API int ddpx_augment_mix_cursor(const void* images, const int64_t* labels, const int64_t* idx_all, int nbatch,
                                     int B, int C, int H, int W, int pad, uint64_t seed, int cutout, int layout,
                                     void* out, int64_t* tgt_out, const int* cursor, const void* table, int modes,
                                     unsigned p_apply, unsigned p_switch, int64_t* tgt_b_out, float* lam_out,
                                     hipStream_t s) {
  if (B <= 0 || nbatch <= 0 || !cursor) return -3;
  return augment_mix_launch(images, labels, idx_all, nbatch, B, C, H, W, pad, seed, cutout, layout, out, tgt_out,
                            cursor, table, modes, p_apply, p_switch, tgt_b_out, lam_out, s);
}

// Batch k = *cursor of a device-resident epoch permutation (idx_all: nbatch x B indices), seed + k.
// The cursor is read, not advanced.  Graph-capturable.
DDPX_API int ddpx_augment_cursor(const void* images, const int64_t* labels, const int64_t* idx_all, int nbatch,
                                 int B, int C, int H, int W, int pad, uint64_t seed, int train, int cutout, int layout,
                                 void* out, int64_t* tgt_out, const int* cursor, hipStream_t s) {
  if (B <= 0 || nbatch <= 0 || !cursor) return -3;
  if (W % 8) return -1;
  if (pad < 0 || pad > 4096) return -4;  // mod64's 32-bit arithmetic assumes a small crop range
  if (cutout_check(cutout, H, W)) return -7;
  const bool nhwc = (layout == OUT_NHWC_BF16 || layout == OUT_NHWC_F32 || layout == OUT_NHWC8_BF16 ||
                     layout == OUT_NHWC4_F32);
  if ((layout == OUT_NHWC8_BF16 && C > 8) || (layout == OUT_NHWC4_F32 && C > 4)) return -2;
  const int n = nhwc ? B * H * W : B * C * H * (W / 8);
  hipLaunchKernelGGL(augment_kernel, dim3((n + 255) / 256), dim3(256), 0, s, (const uint8_t*)images, labels,
                     idx_all, B, C, H, W, pad, seed, train, train ? cutout : 0, layout, out, tgt_out, cursor, nbatch);
  return (int)hipGetLastError();
}
