// ddpx — the fused classifier head for up to 128 classes (CIFAR-100 and the like): Linear(K -> C) + softmax
// cross-entropy forward, and the backward fused with the preceding ReLU's mask, the bias gradients and SGD.
// ONE launch each way, as head_xent.hip's 10-class kernels, whose structure these keep:
//   forward  = (16-row block x K slice) workgroups on v_mfma_f32_16x16x32_bf16: the A fragment (16 rows of H) is
//              loaded once per K step and reused for CT = ceil(C / 16) class tiles of W, each wave holds CT
//              accumulators; write-through partials + agent-scope tickets, the last slice of a row block sums the
//              partials in slice order and finishes its rows with 16 lanes per row (lane j: classes j, j + 16, ...;
//              max / sum-of-exponentials / sum_c q_c z_c over the 16 lanes in a fixed DPP pattern), the last row
//              block sums the row losses in row order and advances the LR table;
//   backward = one workgroup per 16-column slab over ALL rows.  dlogits stay fp32: both products run on the exact-f32
//              matrix instruction v_mfma_f32_16x16x4_f32 (the bf16 operands H and W widened, which is exact), so
//              dW and dH carry fp32 accumulation error only.  A three-way bf16 split of dlogits on the bf16 MFMA
//              would need 3x the (16x faster) instructions plus the split's VALU work and a second LDS image;
//              at 2 x 4 x CT f32 MFMAs per 16 rows the instruction count is not what bounds a 16-column slab, so
//              the exact form was taken.
// Both kernels are templates on CT (1..8), picked by the entry points from C.
// Fixed summation orders, no float atomics: two launches on the same inputs give the same bits.
#include "ddpx_common.h"

namespace ddpx {
namespace wide {

constexpr int kMaxC = 128;
constexpr int kCols = 16;           // backward: columns per workgroup

// head_xent.hip's SoftArgs: q_c = (1 - smoothing) * (lam_m [c == tgt_m] + (1 - lam_m) [c == tgt_b_m]) + smoothing / C
struct Soft {
  const int64_t* tgt_b;
  const float* lam;
  float smoothing;
};

// Reductions over the 16 lanes of a DPP row (every lane gets the result, the same bits in each: every step
// combines two lanes' values symmetrically): quad xor 1, quad xor 2, half-row mirror, row mirror.
template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x141>(v);
  v += dpp_f<0x140>(v);
  return v;
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  v = fmaxf(v, dpp_f<0x141>(v));
  v = fmaxf(v, dpp_f<0x140>(v));
  return v;
}
__device__ __forceinline__ int row16_min(int v) {
  v = min(v, dpp_i<0xB1>(v));
  v = min(v, dpp_i<0x4E>(v));
  v = min(v, dpp_i<0x141>(v));
  v = min(v, dpp_i<0x140>(v));
  return v;
}

// Forward.  Grid, K split, hand-offs and the batch tail are head_fwd_kernel's (MI355X_MICROARCH.md "Valid forms",
// row 1: sc1 stores drained before the ticket, sc1 loads after it).  Thread t of the workgroup owns row t / 16 and
// the classes t % 16 + 16 i of the [16][16 CT] block: in the cross-wave sum, in the slice partials (stored as
// [CT][256], coalesced) and in the row finish, so the summed logits never leave its registers.
// CT is a template parameter: the CT accumulators are then plain registers (with a run-time CT the guarded MFMAs
// made the compiler copy the whole accumulator tuple around every guard).
template <bool SOFT, int CT>
__global__ void __launch_bounds__(256)
head_wide_fwd_kernel(const unsigned short* __restrict__ H, const unsigned short* __restrict__ W,
                     const float* __restrict__ b, const int64_t* __restrict__ tgt, int M, int K, int C, int ldh,
                     int KS, int kslice, float inv_m, float* __restrict__ logits, float* __restrict__ dlogits,
                     int* __restrict__ correct, float* part, float* loss_rows, int* tickets,
                     float* __restrict__ loss_mean, const float* __restrict__ lr_table, int lr_n,
                     int* __restrict__ lr_counter, float* __restrict__ lr_out, Soft sa) {
  constexpr int kFwdLd = 16 * CT + 1;
  __shared__ float lds[4 * 16 * kFwdLd + 4];
  int* flag = reinterpret_cast<int*>(lds + 4 * 16 * kFwdLd);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int rb = blockIdx.x / KS, ks = blockIdx.x - rb * KS;
  const int nrb = gridDim.x / KS;
  const int m0 = rb * 16;
  const int kw = kslice / 4;  // multiple of 32
  const int kb = ks * kslice + wave * kw;
  const int ke = min(K, kb + kw);
  const int row = m0 + (lane & 15);
  const int cls = lane & 15;
  const int ko = 8 * (lane >> 4);
  int lr_k = 0;
  float lr_next = 0.f;
  if (lr_counter && loss_mean) {  // loaded now by every workgroup: no dependent round trips in the tail
    lr_k = *lr_counter;
    lr_next = lr_table[lr_k < lr_n ? lr_k : lr_n - 1];
  }
  const bool rok = row < M;
  const unsigned short* hp = H + (size_t)(rok ? row : 0) * ldh;
  f32x4 acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
  constexpr int KST = 2;  // MFMA steps whose loads (1 + CT fragments each) are in flight together
  for (int k = kb; k < ke; k += 32 * KST) {
    u32x4 av[KST], bv[KST][CT];
#pragma unroll
    for (int i = 0; i < KST; ++i) {
      const int kk = k + 32 * i + ko;
      av[i] = (u32x4){0u, 0u, 0u, 0u};
      if (rok && kk < ke) av[i] = *reinterpret_cast<const u32x4*>(hp + kk);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        bv[i][ct] = (u32x4){0u, 0u, 0u, 0u};  // classes >= C: zero fragments
        if (ct * 16 + cls < C && kk < ke)
          bv[i][ct] = *reinterpret_cast<const u32x4*>(W + (size_t)(ct * 16 + cls) * K + kk);
      }
    }
#pragma unroll
    for (int i = 0; i < KST; ++i)
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, av[i]),
                                                          __builtin_bit_cast(bf16x8, bv[i][ct]), acc[ct], 0, 0, 0);
  }
  // C/D map: col (class within the tile) = lane & 15, row = 4 * (lane >> 4) + r
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) lds[(wave * 16 + 4 * (lane >> 4) + r) * kFwdLd + ct * 16 + (lane & 15)] = acc[ct][r];
  __syncthreads();
  const int t = threadIdx.x;
  const int rr = t >> 4, j = t & 15;
  float z[CT];
#pragma unroll
  for (int i = 0; i < CT; ++i) {
    const int cc = j + 16 * i;
    z[i] = (lds[rr * kFwdLd + cc] + lds[(16 + rr) * kFwdLd + cc]) +
           (lds[(32 + rr) * kFwdLd + cc] + lds[(48 + rr) * kFwdLd + cc]);
  }
  if (KS > 1) {
#pragma unroll
    for (int i = 0; i < CT; ++i)
      __hip_atomic_store(part + ((size_t)blockIdx.x * CT + i) * 256 + t, z[i], __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (t == 0) *flag = __hip_atomic_fetch_add(tickets + rb, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == KS - 1;
    __syncthreads();
    if (!*flag) return;
    // sc1 buffer loads, 8 slices x CT values in flight together; summed in slice order, whichever slice was last
    const __amdgpu_buffer_rsrc_t rp = __builtin_amdgcn_make_buffer_rsrc((void*)(part + (size_t)rb * KS * CT * 256), 0,
                                                                          (unsigned)(KS * CT * 256 * 4), 0x00020000);
#pragma unroll
    for (int i = 0; i < CT; ++i) z[i] = 0.f;
    for (int s0 = 0; s0 < KS; s0 += 8) {
      float v[8][CT];
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int i = 0; i < CT; ++i)
          v[q][i] = s0 + q < KS ? __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
                                      rp, (((s0 + q) * CT + i) * 256 + t) * 4, 0, 16))
                                : 0.f;
#pragma unroll
      for (int q = 0; q < 8; ++q)
#pragma unroll
        for (int i = 0; i < CT; ++i) z[i] += v[q][i];
    }
    if (t == 0) __hip_atomic_store(tickets + rb, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // row finish: 16 lanes per row (one DPP row), lane j holds the classes j + 16 i
  const int m = m0 + rr;
  const bool mok = m < M;
  float mx = -INFINITY;
  int am = 0x7fffffff;
#pragma unroll
  for (int i = 0; i < CT; ++i) {
    const int c = j + 16 * i;
    if (c < C) {
      z[i] += b[c];
      if (z[i] > mx) { mx = z[i]; am = c; }  // lowest class of the lane's maxima
    }
  }
  const float mxr = row16_max(mx);
  am = row16_min(mx == mxr ? am : 0x7fffffff);  // ties go to the lowest class index
  float se = 0.f;
#pragma unroll
  for (int i = 0; i < CT; ++i)
    if (j + 16 * i < C) se += __expf(z[i] - mxr);
  se = row16_sum(se);
  const float lse = mxr + __logf(se);
  const int tg = (tgt && mok) ? (int)tgt[m] : 0;
  int tb = tg;
  float la = 1.f, keep = 1.f, oml = 0.f, uni = 0.f;
  if constexpr (SOFT) {
    if (sa.tgt_b && mok) tb = (int)sa.tgt_b[m];
    if (sa.tgt_b && sa.lam && mok) la = sa.lam[m];
    keep = 1.f - sa.smoothing;
    oml = 1.f - la;
    uni = sa.smoothing / (float)C;
  }
  float zt = 0.f;  // the lane's part of sum_c q_c z_c (hard: z_t on the lane that holds class t, zeros elsewhere)
#pragma unroll
  for (int i = 0; i < CT; ++i) {
    const int c = j + 16 * i;
    if (c < C) {
      float q;
      if constexpr (SOFT) {
        q = keep * ((c == tg ? la : 0.f) + (c == tb ? oml : 0.f)) + uni;
        zt += q * z[i];
      } else {
        q = c == tg ? 1.f : 0.f;
        zt += c == tg ? z[i] : 0.f;
      }
      if (mok) {
        if (logits) logits[(size_t)m * C + c] = z[i];
        if (dlogits) dlogits[(size_t)m * C + c] = (__expf(z[i] - lse) - q) * inv_m;
      }
    }
  }
  zt = row16_sum(zt);
  if (loss_mean && mok && j == 0)
    __hip_atomic_store(loss_rows + m, lse - zt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (correct) {
    const unsigned long long bal = __ballot(tgt && mok && j == 0 && am == tg);
    if (lane == 0 && bal) atomicAdd(correct, __popcll(bal));  // integer: deterministic
  }
  if (!loss_mean) return;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its sc1 stores
  __syncthreads();
  if (t == 0) flag[1] = __hip_atomic_fetch_add(tickets + nrb, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nrb - 1;
  __syncthreads();
  if (!flag[1] || wave != 0) return;
  const __amdgpu_buffer_rsrc_t rl =
      __builtin_amdgcn_make_buffer_rsrc((void*)loss_rows, 0, (unsigned)(M * 4), 0x00020000);
  float s = 0.f;
  for (int i0 = 0; i0 < M; i0 += 64 * 8) {
    float v[8];
#pragma unroll
    for (int q = 0; q < 8; ++q)  // out-of-range lanes read zeros (buffer bounds check)
      v[q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rl, (i0 + q * 64 + lane) * 4, 0, 16));
#pragma unroll
    for (int q = 0; q < 8; ++q) s += v[q];
  }
  s = wave_sum(s);  // fixed butterfly: the same order whichever row block is last
  if (lane == 0) {
    *loss_mean = s / (float)M;
    __hip_atomic_store(tickets + nrb, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lr_counter) {  // the training step's device LR schedule: lr = table[step], step += 1 (head_fwd_kernel)
      *lr_out = lr_next;
      *lr_counter = lr_k + 1;
    }
  }
}

// Backward.  Workgroup = the 16-column slab [k0, k0 + 16) over all M rows; its 4 waves take 16-row tiles in turn:
//   g[m][k]   = sum_c (go dl[m][c]) W[c][k]          A = the tile's dlogits [16 rows][4 classes per step],
//                                                     B = W's slab [4 classes][16 columns], held in registers for
//                                                     all classes from before the loop (so the fused SGD below may
//                                                     overwrite W: no other workgroup reads these columns)
//   dH[m][k]  = hscale * (relu_mask ? g * (H[m][k] > 0) : g)                     (bf16, stored)
//   dW[c][k]  = sum_m (go dl[m][c]) H[m][k]          A = dlogits^T [16 classes][4 rows], B = H [4 rows][16 columns],
//                                                     CT accumulators per wave over all its tiles
//   dprev[k]  = sum_m of the stored (bf16-rounded) dH;   db[c] = sum_m go dl[m][c]  (workgroup 0)
// The tile's dlogits (times go, zero past M and C) are staged once in the wave's LDS region and read in both
// fragment layouts.  The k slot (step s, lane group q) of the dW product stands for tile row 4 q + s, which is the
// row the lane holds in register s of the dH accumulator: the same four H values feed the B operand and the mask.
// Sums: MFMA accumulators over a wave's tiles, then the 4 waves in order through LDS: a fixed order.
template <int CT>
__global__ void __launch_bounds__(256)
head_wide_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ go_ptr,
                     const unsigned short* __restrict__ H, const unsigned short* __restrict__ W, int M, int K, int C,
                     int ldh, unsigned short* __restrict__ dH, int relu_mask, float hscale,
                     void* __restrict__ dW, void* __restrict__ db, void* __restrict__ dbprev, int out_bf16,
                     int accumulate, SgdArgs sW, SgdArgs sB, SgdArgs sP) {
  constexpr int NW = 16 * CT;       // classes, padded to whole tiles
  constexpr int kDlLd = NW + 4;
  constexpr int HH = NW > 64 ? 2 : 1;  // classes per lane when a row of dlogits is spread over the wave
  __shared__ float dls[4 * 16 * kDlLd];  // [wave][16 rows][classes]
  __shared__ float red[4 * NW * kCols];  // [wave][class][column]
  __shared__ float redp[4 * 64];         // [wave][lane]: dprev partials
  __shared__ float redh[4 * NW];         // [wave][class]: head-bias partials (workgroup 0)
  const float go = go_ptr ? *go_ptr : 1.f;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int k0 = blockIdx.x * kCols;
  const bool head_bias = blockIdx.x == 0;
  // this slab of W for all classes, widened (exact): B fragment of step s = W[4 s + q][k0 + r]
  float wf[4 * CT];
#pragma unroll
  for (int s = 0; s < 4 * CT; ++s) {
    const int c = 4 * s + q;
    wf[s] = c < C ? bf2f(W[(size_t)c * K + k0 + r]) : 0.f;
  }
  // fused SGD: master / momentum of the elements this thread finishes, loaded under the main loop
  float pre_p[CT], pre_m[CT], prev_p = 0.f, prev_m = 0.f, preh_p = 0.f, preh_m = 0.f;
#pragma unroll
  for (int i = 0; i < CT; ++i) {
    pre_p[i] = pre_m[i] = 0.f;
    const int c = (tid >> 4) + 16 * i;
    if (sW.p && c < C) {
      const size_t idx = (size_t)c * K + k0 + (tid & 15);
      pre_p[i] = __builtin_nontemporal_load(sW.p + idx);
      if (sW.mom != 0.f) pre_m[i] = __builtin_nontemporal_load(sW.buf + idx);
    }
  }
  if (sP.p && tid < kCols) {
    prev_p = __builtin_nontemporal_load(sP.p + k0 + tid);
    if (sP.mom != 0.f) prev_m = __builtin_nontemporal_load(sP.buf + k0 + tid);
  }
  if (head_bias && sB.p && tid < C) {
    preh_p = __builtin_nontemporal_load(sB.p + tid);
    if (sB.mom != 0.f) preh_m = __builtin_nontemporal_load(sB.buf + tid);
  }
  const float lr = sW.p ? *sW.lr : 0.f;
  f32x4 acc[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float dbp = 0.f, hb[2] = {0.f, 0.f};
  float* dt = dls + wave * 16 * kDlLd;
  const int ntile = (M + 15) / 16;
  for (int t0 = 0; t0 < ntile; t0 += 4) {  // uniform trip count: a wave past the last tile works on zeros
    const int m0 = (t0 + wave) * 16;
    float dv[16][HH];
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
      for (int hh = 0; hh < HH; ++hh) {
        const int c = lane + 64 * hh;
        dv[i][hh] = (m0 + i < M && c < C) ? dlogits[(size_t)(m0 + i) * C + c] : 0.f;
      }
    unsigned short hv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int m = m0 + 4 * q + s;
      hv[s] = m < M ? H[(size_t)m * ldh + k0 + r] : (unsigned short)0;
    }
#pragma unroll
    for (int i = 0; i < 16; ++i)
#pragma unroll
      for (int hh = 0; hh < HH; ++hh)
        if (lane + 64 * hh < NW) dt[i * kDlLd + lane + 64 * hh] = dv[i][hh] * go;
    __syncthreads();
    f32x4 g = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4 * CT; ++s)
      g = __builtin_amdgcn_mfma_f32_16x16x4f32(dt[r * kDlLd + 4 * s + q], wf[s], g, 0, 0, 0);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const float hf = bf2f(hv[s]);
#pragma unroll
      for (int ct = 0; ct < CT; ++ct)
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(dt[(4 * q + s) * kDlLd + ct * 16 + r], hf, acc[ct], 0, 0, 0);
    }
    // C/D map of g: column k0 + r, tile row 4 q + s
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int m = m0 + 4 * q + s;
      float v = g[s];
      if (relu_mask && !(bf2f(hv[s]) > 0.f)) v = 0.f;
      const unsigned short o = f2bf(v * hscale);
      if (dH && m < M) dH[(size_t)m * ldh + k0 + r] = o;
      dbp += bf2f(o);  // rows past M: zeros
    }
    if (head_bias) {
#pragma unroll
      for (int hh = 0; hh < HH; ++hh)
        if (lane + 64 * hh < NW) {
#pragma unroll
          for (int i = 0; i < 16; ++i) hb[hh] += dt[i * kDlLd + lane + 64 * hh];
        }
    }
    __syncthreads();  // the tile is consumed before the next one is staged
  }
  // C/D map of acc[ct]: column k0 + r, class 16 ct + 4 q + s
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int s = 0; s < 4; ++s) red[(wave * NW + ct * 16 + 4 * q + s) * kCols + r] = acc[ct][s];
  redp[wave * 64 + lane] = dbp;
  if (head_bias) {
#pragma unroll
    for (int hh = 0; hh < HH; ++hh)
      if (lane + 64 * hh < NW) redh[wave * NW + lane + 64 * hh] = hb[hh];
  }
  __syncthreads();
  auto put = [&](const SgdArgs& sg, void* base, size_t idx, float v, float pv, float mv) {
    if (sg.p) {  // fused optimizer: update the parameter instead of storing its gradient
      sgd_apply_pre(sg, idx, v, lr, pv, mv);
    } else if (out_bf16) {
      unsigned short* o = reinterpret_cast<unsigned short*>(base) + idx;
      *o = f2bf(accumulate ? v + bf2f(*o) : v);
    } else {
      float* o = reinterpret_cast<float*>(base) + idx;
      *o = accumulate ? v + *o : v;
    }
  };
  if (dW || sW.p) {
#pragma unroll
    for (int i = 0; i < CT; ++i) {
      const int c = (tid >> 4) + 16 * i, col = tid & 15;
      if (c < C) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) s += red[(w * NW + c) * kCols + col];
        put(sW, dW, (size_t)c * K + k0 + col, s, pre_p[i], pre_m[i]);
      }
    }
  }
  if (tid < kCols && (dbprev || sP.p)) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) s += redp[w * 64 + qq * 16 + tid];
    put(sP, dbprev, (size_t)(k0 + tid), s, prev_p, prev_m);
  }
  if (head_bias && tid < C && (db || sB.p)) {  // head bias: db[c] = go * sum_m dlogits[m][c]
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) s += redh[w * NW + tid];
    put(sB, db, (size_t)tid, s, preh_p, preh_m);
  }
}

}  // namespace wide
}  // namespace ddpx

using namespace ddpx;
using namespace ddpx::wide;

// head_xent.hip's split: enough (row block x slice) workgroups to fill the chip, >= one 32-wide step per wave
static int wide_ksplit(int M, int K) {
  const int rbs = (M + 15) / 16;
  const int ks = (256 + rbs - 1) / rbs;
  const int maxks = max(1, K / 128);
  return max(1, min(ks, maxks));
}

// Forward scratch (floats): slice partials [row blocks * KS][CT][256] + row losses [M].  The tickets (row blocks + 1
// ints, zero between launches) are ddpx_head_fwd_tickets' .
DDPX_API int64_t ddpx_head_wide_fwd_scratch(int M, int K, int C) {
  if (M <= 0 || C < 1 || C > kMaxC) return 0;
  const int64_t rbs = (M + 15) / 16, ct = (C + 15) / 16;
  return rbs * wide_ksplit(M, K) * ct * 256 + M;
}

template <bool SOFT>
static int wide_fwd_launch(const void* H, const void* W, const float* b, const int64_t* tgt, int M, int K, int C,
                           int ldh, float inv_m, float* logits, float* dlogits, int* correct, float* scratch,
                           int* tickets, float* loss_mean, const float* lr_table, int lr_n, int* lr_counter,
                           float* lr_out, Soft sa, hipStream_t s) {
  if (C < 1 || C > kMaxC) return -1;
  if (K < 8 || K % 8 || ldh % 8 || ldh < K) return -2;
  if (M <= 0) return 0;
  if (!scratch || !tickets) return -3;
  if (loss_mean && !tgt) return -4;
  if (lr_counter && (!loss_mean || !lr_table || !lr_out || lr_n < 1)) return -5;
  const int rbs = (M + 15) / 16;
  const int ks = wide_ksplit(M, K);
  int kslice = (K + ks - 1) / ks;
  kslice = (kslice + 127) / 128 * 128;  // whole 32-wide MFMA steps for each of the 4 waves
  const int ct = (C + 15) / 16;
  float* part = scratch;
  float* loss_rows = scratch + (size_t)rbs * ks * ct * 256;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(rbs * ks), dim3(256), 0, s, (const unsigned short*)H, (const unsigned short*)W, b,
                       tgt, M, K, C, ldh, ks, kslice, inv_m, logits, dlogits, correct, part, loss_rows, tickets,
                       loss_mean, lr_table, lr_n, lr_counter, lr_out, sa);
  };
  switch (ct) {
    case 1: launch(head_wide_fwd_kernel<SOFT, 1>); break;
    case 2: launch(head_wide_fwd_kernel<SOFT, 2>); break;
    case 3: launch(head_wide_fwd_kernel<SOFT, 3>); break;
    case 4: launch(head_wide_fwd_kernel<SOFT, 4>); break;
    case 5: launch(head_wide_fwd_kernel<SOFT, 5>); break;
    case 6: launch(head_wide_fwd_kernel<SOFT, 6>); break;
    case 7: launch(head_wide_fwd_kernel<SOFT, 7>); break;
    default: launch(head_wide_fwd_kernel<SOFT, 8>); break;
  }
  return (int)hipGetLastError();
}

DDPX_API int ddpx_head_wide_fwd(const void* H, const void* W, const float* b, const int64_t* tgt, int M, int K, int C,
                                int ldh, float inv_m, float* logits, float* dlogits, int* correct, float* scratch,
                                int* tickets, float* loss_mean, const float* lr_table, int lr_n, int* lr_counter,
                                float* lr_out, hipStream_t s) {
  return wide_fwd_launch<false>(H, W, b, tgt, M, K, C, ldh, inv_m, logits, dlogits, correct, scratch, tickets,
                                loss_mean, lr_table, lr_n, lr_counter, lr_out, Soft{nullptr, nullptr, 0.f}, s);
}

DDPX_API int ddpx_head_wide_fwd_soft(const void* H, const void* W, const float* b, const int64_t* tgt,
                                     const int64_t* tgt_b, const float* lam, float smoothing, int M, int K, int C,
                                     int ldh, float inv_m, float* logits, float* dlogits, int* correct, float* scratch,
                                     int* tickets, float* loss_mean, const float* lr_table, int lr_n, int* lr_counter,
                                     float* lr_out, hipStream_t s) {
  if (!tgt) return -4;
  if (!(smoothing >= 0.f && smoothing <= 1.f)) return -6;
  return wide_fwd_launch<true>(H, W, b, tgt, M, K, C, ldh, inv_m, logits, dlogits, correct, scratch, tickets,
                               loss_mean, lr_table, lr_n, lr_counter, lr_out, Soft{tgt_b, lam, smoothing}, s);
}

DDPX_API int ddpx_head_wide_bwd(const float* dlogits, const float* go, const void* H, const void* W, int M, int K,
                                int C, int ldh, void* dH, int relu_mask, float hscale, void* dW, void* db, void* dbprev,
                                int out_bf16, int accumulate, float* sw_p, float* sw_buf, void* sw_sh, float* sb_p,
                                float* sb_buf, void* sb_sh, float* sp_p, float* sp_buf, void* sp_sh, const float* lr,
                                float mom, float wd, hipStream_t s) {
  if (C < 1 || C > kMaxC) return -1;
  if (K < kCols || K % kCols || ldh % 8 || ldh < K) return -2;
  if (M <= 0) return 0;
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(K / kCols), dim3(256), 0, s, dlogits, go, (const unsigned short*)H,
                       (const unsigned short*)W, M, K, C, ldh, (unsigned short*)dH, relu_mask, hscale, dW, db, dbprev,
                       out_bf16, accumulate, SgdArgs{sw_p, sw_buf, (unsigned short*)sw_sh, lr, mom, wd},
                       SgdArgs{sb_p, sb_buf, (unsigned short*)sb_sh, lr, mom, wd},
                       SgdArgs{sp_p, sp_buf, (unsigned short*)sp_sh, lr, mom, wd});
  };
  switch ((C + 15) / 16) {
    case 1: launch(head_wide_bwd_kernel<1>); break;
    case 2: launch(head_wide_bwd_kernel<2>); break;
    case 3: launch(head_wide_bwd_kernel<3>); break;
    case 4: launch(head_wide_bwd_kernel<4>); break;
    case 5: launch(head_wide_bwd_kernel<5>); break;
    case 6: launch(head_wide_bwd_kernel<6>); break;
    case 7: launch(head_wide_bwd_kernel<7>); break;
    default: launch(head_wide_bwd_kernel<8>); break;
  }
  return (int)hipGetLastError();
}
