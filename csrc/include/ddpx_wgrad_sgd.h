// ddpx — weight gradient + SGD in one warp-specialised persistent kernel (gfx950).
//
//   W -= lr * sgd_direction( dY^T X )          dY [K=batch][M=out] bf16, X [K][N=in] bf16, W fp32 [M][N]
//
// The single-process optimizer fused into backward (SGD(fused_backward=True)) streams 18 B per weight
// (master + momentum in, master + momentum + bf16 shadow out) right where the weight gradient is born,
// so the gradient never round-trips through HBM.  In the tile-per-workgroup GEMM that stream ran AFTER
// each tile's MFMA main loop: both halves serialised and the fused kernels (toy MLP fc1 / fc0: 97 / 78 us,
// profiles/r2_head) were no faster than a stored fp32 gradient plus one flat SGD pass.
//
// Here every workgroup (one per CU, NMW + NSW waves) owns a list of BM x 128 tiles (n-fastest over W, so the tiles
// in flight on the chip cover whole rows of W) and splits its waves by role:
//   * waves 0..NMW-1 (math, NMW = 4 or 8): the LDS-DMA ring + v_mfma_f32_16x16x32_bf16 main loop of tile i (the
//     pipe core of ddpx_pipe.h), then its fp32 accumulators into an LDS tile buffer;
//   * waves NMW.. (stream, NSW = 4 or 8): the optimizer update of tile i-1 from the buffer the math waves filled
//     one iteration earlier, spread evenly over the K-steps, master / momentum loads a 4-vector ring ahead
//     (non-temporal, counted vmcnt waits) — so a CU's HBM stream runs while its matrix cores work on the next tile.
// Both roles execute exactly NK + 1 = 9 s_barriers per iteration (NK = 8 K-steps of 64, then the buffer hand-off)
// for nt + 1 iterations (iteration 0 fills: math only; iteration nt drains: stream only), whatever the tile
// height, so the barrier sequence matches by construction.
// The update arithmetic is sgd_apply's fma sequence, and every accumulator is one MFMA chain over K in K-step order:
// bitwise equal to the stored-gradient + flat-SGD path for every variant.
//
// Tile height BM (select_variant; DDPX_WSGD_TILE):
//   *  64 rows: two hand-off buffers (iteration parity), so the roles never share one; 3 or 4 ring stages of 24 KiB;
//      every layout (4 / 8 stream waves, 4 / 8 math waves, MX-FP8 copies).  64x128 moves 192 KiB of L2 -> LDS operand
//      traffic per tile, 704 MB for the toy MLP's pair: more than the 504 MB optimizer stream it shares the CU's
//      texture-address path with (profiles/r6_pair).
//   * 128 rows (bf16, 8 math waves of 64 x 32, 4 stream waves, 3 ring stages of 32 KiB): 256 KiB per twice the work
//      (470 MB for the pair), and each K-step's fixed costs (counted wait, barrier, DMA issue, fragment latency) are
//      spread over twice the MFMAs.  Two 64 KiB buffers do not fit the 160 KiB LDS beside the ring; ONE does (96 + 64
//      KiB, exactly the LDS).  The math waves store tile i's accumulators during the last K-step of iteration i,
//      after the barrier that opens it; the stream waves have by then taken every vector of tile i-1 out of the
//      buffer, because they read the vectors of K-step t + 1 into registers during K-step t (those of K-step 0 right
//      after the hand-off barrier), read nothing in the last K-step, and wait for their LDS reads (lgkmcnt(0)) before
//      every barrier.  Measured on the toy pair (profiles/r7_pair, median CU): math side alone 78.7 -> 53.8 us, span
//      107.7 -> 95.2 us, the stream pacing 83 us of it.  The fill and drain iterations are whole tiles: 9.0 + 9.0 us
//      against 7.1 + 3.8 us with 64 rows, which takes back 7 of the 19.6 us the steady iterations gained; half-height
//      first and last iterations (64 rows, FM = 2) would return most of that and are not built.
#pragma once

#include <cstdlib>

#include "ddpx_mx.h"
#include "ddpx_pipe.h"

namespace ddpx {
namespace wsgd {

constexpr int BN = 128;
constexpr int NK = 8;  // K-steps of 64 per tile: K == 512 (eligible())
// STAGES-deep LDS-DMA ring for the math waves + the fp32 tile buffers of the math -> stream hand-off.
//   BM = 64, 3 stages:  two buffers, row stride BN + 4 (conflict-free accumulator stores), 138 KiB;
//   BM = 64, 4 stages:  one more 24 KiB stage in flight (the math side's K-steps are L2->LDS latency bound with
//                       only 4 DMA-issuing waves), which fits the 160 KiB LDS only with unpadded rows (4-way
//                       conflicts on the once-per-tile accumulator store);
//   BM = 128, 3 stages: 3 x 32 KiB of ring + ONE 64 KiB buffer = 160 KiB.  Rows are unpadded; the 16-column group
//                       of a row is XORed with (row >> 2) & 3 (tile_col), which puts the four rows one accumulator
//                       store instruction touches on different banks and keeps every f32x4 of a row contiguous.
// Diagnostics (ddpx_gemm_set_stamps, benchmarks/pair_stamps.py): with p0.stamp set, lane 0 of wave 0 (math role)
// and of the first stream wave (stream role) write s_memrealtime (10 ns ticks) at kernel start (slot 0), on ARRIVAL at each of the
// role's s_barriers (slots 1..), and at kernel end (last slot): stamp[(block * 2 + role) * kStampSlots + slot].  A
// barrier's departure is the later of the two roles' arrivals, so the per-barrier wait of each role shows which
// side sets the pace.  Off (a null pointer) it costs a scalar test per barrier.
constexpr int kStampSlots = 256;

template <int BM, int STAGES>
struct Cfg {
  static_assert(BM == 64 || BM == 128, "tile height");
  static_assert(STAGES == 3 || (STAGES == 4 && BM == 64), "ring depth");
  static constexpr int A_SUB = BM * 64 * 2, B_SUB = BN * 64 * 2, SLOT = A_SUB + B_SUB;
  static constexpr bool SBUF = BM == 128;  // one hand-off buffer (swizzled columns) instead of two
  static constexpr int ALD = (STAGES >= 4 || SBUF) ? BN : BN + 4;
  static constexpr int ACC_BYTES = BM * ALD * 4;
  static constexpr int LDS_BYTES = STAGES * SLOT + (SBUF ? 1 : 2) * ACC_BYTES;
  static_assert(LDS_BYTES <= 160 * 1024, "LDS");
  // column of (row, col) inside the buffer's row
  __host__ __device__ static constexpr int tile_col(int row, int col) {
    return SBUF ? (col ^ (((row >> 2) & 3) << 4)) : col;
  }
};

// Two GEMMs may share one launch (p0's tiles, then p1's: the toy MLP's fc1 and fc0 weight gradients are
// independent once fc1's data gradient ran): one fill and one drain iteration instead of two, one launch
// boundary fewer.  Single GEMM: p1 = p0 and nt1 = 0.  Both must have the same K, lr, momentum, wd, alpha.
// PROBE (measurement only, DDPX_WSGD_XTRA, benchmarks/pair_stamps.py): 0 = none; 3 = math only (the stream waves keep
// the barrier sequence but load, update and store nothing); 4 = stream only (the math waves issue no DMA and no MFMA:
// zero gradients).
// NMW: math waves, 4 (2 x 2 waves of 32 x 64) or 8 (2 x 4 waves of 32 x 32: two MFMA waves per SIMD, so one wave's
// fragment reads, DMA issue and barrier wait run under the other's MFMAs — the 4-wave math side ran its K-steps at
// 11 % MFMA busy with its waves waiting 62 % of their cycles, profiles/r6_pair).
// The optimizer stream loads and stores master / momentum non-temporally; the bf16 shadow store is plain.
// BM: tile height, 64 or 128 (128: bf16 only, 8 math waves of 64 x 32, 3 stages, the single hand-off buffer).
template <int BM, int STAGES, bool FP8, int NSW, bool NORD, int NMW, int PROBE = 0>
__global__ void __launch_bounds__(64 * NMW + 64 * NSW) wgrad_sgd_ws_kernel(pipe::Params p0, pipe::Params p1, int nt1) {
  using C = Cfg<BM, STAGES>;
  constexpr int ALD = C::ALD, ACC_BYTES = C::ACC_BYTES, LDS_BYTES = C::LDS_BYTES;
  constexpr int A_SUB = C::A_SUB, SLOT = C::SLOT;
  constexpr bool SBUF = C::SBUF;
  static_assert(NMW == 4 || NMW == 8, "math waves");
  static_assert(BM == 64 || (NMW == 8 && !FP8), "the 128-row tile: 8 math waves, no MX-FP8 copy");
  static_assert(PROBE == 0 || PROBE == 3 || PROBE == 4, "probe");
  constexpr int WN = NMW / 2;                        // math waves along N
  constexpr int WMR = BM / 2;                        // math wave tile WMR x (BN / WN)
  constexpr int FM = WMR / 16, FN = BN / WN / 16;
  constexpr int LPW = (BM + BN) / (8 * NMW);         // LDS-DMA instructions per math wave per stage
  __shared__ __attribute__((aligned(1024))) char smem[LDS_BYTES];
  float* const accb = reinterpret_cast<float*>(smem + STAGES * SLOT);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles_m0 = p0.M / BM, tiles_m1 = p1.M / BM;
  const int nt0 = tiles_m0 * (p0.N / BN);
  const int ntiles = nt0 + nt1;
  const int nt = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;  // >= 1 (grid <= ntiles)
  constexpr int nk = NK;
  // tile i of this workgroup: origin and which GEMM it belongs to (uniform per workgroup)
  // NORD: the tiles running at once sweep whole rows of W (n fastest): the optimizer stream then reads and
  // writes every row's 512-B tile segments side by side instead of 64 rows x 4 segments scattered over W
  // (m fastest), which is what the HBM sees of 256 CUs streaming at once.
  auto tile_origin = [&](int i, int& m0, int& n0) -> int {
    int g = (int)blockIdx.x + i * (int)gridDim.x;
    const int sel = g >= nt0;
    if (sel) g -= nt0;
    if constexpr (NORD) {
      const int tn = (sel ? p1.N : p0.N) / BN;
      m0 = (g / tn) * BM;
      n0 = (g % tn) * BN;
    } else {
      const int tm = sel ? tiles_m1 : tiles_m0;
      m0 = (g % tm) * BM;
      n0 = (g / tm) * BN;
    }
    return sel;
  };
  const pipe::Params& p = p0;  // K, alpha, lr, momentum, wd: shared by both GEMMs
  long long* const stp = (p0.stamp && (tid == 0 || tid == 64 * NMW))
                             ? p0.stamp + ((size_t)blockIdx.x * 2 + (wave < NMW ? 0 : 1)) * kStampSlots
                             : nullptr;
  int nstamp = 1;
  auto mark = [&]() {  // arrival at the role's next barrier
    if (stp) {
      stp[nstamp < kStampSlots - 1 ? nstamp : kStampSlots - 2] = (long long)__builtin_amdgcn_s_memrealtime();
      ++nstamp;
    }
  };
  if (stp) stp[0] = (long long)__builtin_amdgcn_s_memrealtime();

  if (wave < NMW) {
    // ------------------------------------------------------------------ math waves
    const int wm = wave / WN, wn = wave % WN;
    const __amdgpu_buffer_rsrc_t ra0 = __builtin_amdgcn_make_buffer_rsrc((void*)p0.A, 0, p0.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb0 = __builtin_amdgcn_make_buffer_rsrc((void*)p0.B, 0, p0.b_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t ra1 = __builtin_amdgcn_make_buffer_rsrc((void*)p1.A, 0, p1.a_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb1 = __builtin_amdgcn_make_buffer_rsrc((void*)p1.B, 0, p1.b_bytes, 0x00020000);
    // One LDS-DMA ring across ALL of this workgroup's tiles: K-step g of the workgroup's sequence is K-step
    // g % nk of its tile g / nk, and stage g + STAGES - 1 is issued during K-step g even when it belongs to
    // the next tile, so the ring never drains and refills at a tile boundary (with K = 512 a tile is only
    // nk = 8 K-steps: a per-tile refill cost ~2 of every 10 K-steps of L2 latency).
    const int G = nt * nk;
    // the issuer walks g = 0, 1, 2, ... in order: the tile origin (integer divisions) is computed once per tile
    int iss_i = -1, iss_kt = nk - 1, iss_m0 = 0, iss_n0 = 0, iss_sel = 0;
    auto issue = [&](int g) {
      if constexpr (PROBE == 4) return;  // measurement: stream only
      if (++iss_kt >= nk) {
        iss_kt = 0;
        iss_sel = tile_origin(++iss_i, iss_m0, iss_n0);
      }
      const int m0 = iss_m0, n0 = iss_n0, sel = iss_sel, kt = iss_kt;
      const __amdgpu_buffer_rsrc_t ra = sel ? ra1 : ra0, rb = sel ? rb1 : rb0;
      const int lda = sel ? p1.lda : p0.lda, ldb = sel ? p1.ldb : p0.ldb;
      const int Mg = sel ? p1.M : p0.M, Ng = sel ? p1.N : p0.N;
      char* slot = smem + (g % STAGES) * SLOT;
      pipe::stage_tile<BM, false, pipe::MODE_PLAIN, NMW>(ra, slot, p.conv, lda, m0, Mg, kt * 64, p.K, wave, lane);
      pipe::stage_tile<BN, false, pipe::MODE_PLAIN, NMW>(rb, slot + A_SUB, p.conv, ldb, n0, Ng, kt * 64, p.K, wave,
                                                         lane);
    };
#pragma unroll
    for (int s = 0; s < STAGES - 1; ++s)
      if (s < G) issue(s);
    for (int i = 0; i <= nt; ++i) {
      if (i == nt) {  // drain iteration: the stream waves finish the last tile
        for (int t = 0; t < nk; ++t) {
          mark();
          __builtin_amdgcn_s_barrier();
        }
      } else {
        f32x4 acc[FM][FN];
#pragma unroll
        for (int a = 0; a < FM; ++a)
#pragma unroll
          for (int b = 0; b < FN; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < nk; ++t) {
          const int g = i * nk + t;
          const int ahead = min(STAGES - 2, G - 1 - g);
          // stage g landed: everything but the (up to STAGES - 2) younger stages' DMAs
          if (STAGES >= 4 && ahead >= 2) pipe::wait_vmcnt<2 * LPW>();
          else if (ahead >= 1) pipe::wait_vmcnt<LPW>();
          else pipe::wait_vmcnt<0>();
          mark();
          __builtin_amdgcn_s_barrier();
          asm volatile("" ::: "memory");
          if (g + STAGES - 1 < G) issue(g + STAGES - 1);
          const char* sa = smem + (g % STAGES) * SLOT;
          const char* sb = sa + A_SUB;
#pragma unroll
          for (int kk = 0; kk < (PROBE == 4 ? 0 : 64); kk += 32) {
            bf16x8 af[FM], bfr[FN];
            pipe::load_frags<BM, false, FM, BN, false, FN>(sa, wm * WMR, sb, wn * (BN / WN), kk, lane, af, bfr);
#pragma unroll
            for (int a = 0; a < FM; ++a)
#pragma unroll
              for (int b = 0; b < FN; ++b)
                acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bfr[b], acc[a][b], 0, 0, 0);
          }
        }
        // accumulators -> tile buffer i&1 (C/D map: row 4*(lane>>4)+r, col lane&15 of each 16x16 block).
        // Single buffer: the stream waves took the last vector of tile i-1 out of it before they arrived at this
        // iteration's last K-step barrier, which the MFMAs above have passed.
        float* T = accb + (SBUF ? 0 : (i & 1) * (ACC_BYTES / 4));
        const int mr = wm * WMR + 4 * (lane >> 4), nc = wn * (BN / WN) + (lane & 15);
#pragma unroll
        for (int a = 0; a < FM; ++a)
#pragma unroll
          for (int b = 0; b < FN; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = mr + a * 16 + r;
              T[row * ALD + C::tile_col(row, nc + b * 16)] = acc[a][b][r] * p.alpha;
            }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      mark();
      __builtin_amdgcn_s_barrier();  // hand-off: tile i's buffer complete, tile i-1's buffer released
    }
    if (stp) stp[kStampSlots - 1] = (long long)__builtin_amdgcn_s_memrealtime();
  } else {
    // ---------------------------------------------------------------- stream waves
    // Vector v of tile i-1 (row row0 + RSTEP v, columns col..col+3 of the tile) is updated in K-step v * KPU / UPK
    // of iteration i (64-row tile, 4 stream waves: one vector per K-step).  Its master / momentum loads are issued
    // DIST updates earlier — for the first DIST vectors of a tile, in the last K-steps of the previous iteration — into a
    // ring of DIST register slots.  Profiled on MI355X (benchmarks/stream_probe.hip): 4 waves per CU stream the
    // optimizer's 18 B per weight at 6.2 TB/s with 4 vectors in flight per thread, against 3.5 TB/s holding a
    // whole tile (8 vectors, 128 VGPRs of state) ahead, which also pushed this kernel into register spills.
    // NSW stream waves (4, or 8 with DDPX_WSGD_STREAM_WAVES=8): SV vectors per stream thread per tile, spread evenly
    // over the tile's NK K-steps: UPK updates per K-step (SV >= NK) or one update every KPU K-steps (SV < NK); a
    // ring of DIST = 4 vectors in flight per thread (a ring of 8 measured no faster).
    //   BM  64: SV = 8 (NSW 4: one update per K-step) or 4 (NSW 8: one every second K-step);
    //   BM 128: SV = 16 (NSW 4: two updates per K-step).
    // Single hand-off buffer (SBUF): the math waves refill the buffer during the LAST K-step of an iteration, so the
    // stream waves read the gradient vectors of K-step t + 1 during K-step t (those of K-step 0 right after the
    // hand-off barrier) into UPK register vectors and read nothing in the last K-step; every read has landed
    // (lgkmcnt(0)) before the thread arrives at the next barrier.
    constexpr int DIST = 4;
    constexpr int SV = BM * BN / 4 / (NSW * 64);
    constexpr int UPK = SV >= NK ? SV / NK : 1;   // updates per K-step
    constexpr int KPU = SV >= NK ? 1 : NK / SV;   // K-steps per update
    constexpr int RSTEP = NSW * 2;                // tile rows between a thread's consecutive vectors
    static_assert(SV % DIST == 0 && DIST % UPK == 0 && SV * KPU == NK * UPK, "ring");
    static_assert(!SBUF || KPU == 1, "single buffer: at least one update per K-step");
    const int st = tid - 64 * NMW;
    const int row0 = st >> 5, col = 4 * (st & 31);  // row0 < RSTEP
    const float lr = *p.sgd.lr;
    const float mom = p.sgd.mom, wd = p.sgd.wd;
    const bool has_mom = mom != 0.f;
    f32x4 rp[DIST], rm[DIST];  // the ring (statically indexed: every loop over it is unrolled)
    // per-GEMM pointers selected as scalars (a reference to p0.sgd / p1.sgd picked at run time put the structs
    // on the stack: scratch loads, which also count in vmcnt)
    float* const P0 = p0.sgd.p;
    float* const P1 = p1.sgd.p;
    float* const M0 = has_mom ? p0.sgd.buf : p0.sgd.p;
    float* const M1 = has_mom ? p1.sgd.buf : p1.sgd.p;
    unsigned short* const S0 = p0.sgd.shadow;
    unsigned short* const S1 = p1.sgd.shadow;
    unsigned char* const Q0 = p0.sgd.q8;
    unsigned char* const Q1 = p1.sgd.q8;
    unsigned char* const E0 = p0.sgd.s8;
    unsigned char* const E1 = p1.sgd.s8;
    // transposed MX copy (FP8, 8 stream waves): each updated vector is staged as fp32 in the gradient tile it
    // replaced (the thread's own, already consumed slot), and once a 32-row block of the tile is complete (after
    // the barrier that follows its last vector's update) every stream thread quantises 8 rows of one column:
    // quad = 32 rows of a column = one MX block along M, its 4 lanes write 32 contiguous code bytes of W^T
    unsigned char* const QT0 = p0.sgd.q8t;
    unsigned char* const QT1 = p1.sgd.q8t;
    unsigned char* const ET0 = p0.sgd.s8t;
    unsigned char* const ET1 = p1.sgd.s8t;
    const bool qt_on = FP8 && NSW == 8 && (QT0 != nullptr || QT1 != nullptr);  // (either GEMM may skip its copy)
    unsigned qt_e0 = 0;  // block 0's E8M0 byte until block 1's: the column's two scales as one 2-byte store
    const int ldc0 = p0.ldc, ldc1 = p1.ldc;
    auto vec_off = [&](int j, int v, int& sel) -> size_t {
      int m0, n0;
      sel = tile_origin(j, m0, n0);
      return (size_t)(m0 + row0 + RSTEP * v) * (sel ? ldc1 : ldc0) + n0 + col;
    };
    // load vector v of tile j into a ring slot
    auto load_vec = [&](int j, int v, f32x4& pv, f32x4& mv) {
      int sel;
      const size_t off = vec_off(j, v, sel);
      pv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>((sel ? P1 : P0) + off));
      mv = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>((sel ? M1 : M0) + off));
    };
    auto grad_vec = [&](const float* T, int v) -> f32x4 {
      const int row = row0 + RSTEP * v;
      return *reinterpret_cast<const f32x4*>(T + row * ALD + C::tile_col(row, col));
    };
    // update vector v of tile j with gradient g, then refill the slot with the vector DIST ahead
    auto update_vec_g = [&](int j, int v, const f32x4 g, f32x4& pv, f32x4& mv, float* stage) {
      int sel;
      const size_t off = vec_off(j, v, sel);
      f32x4 po, bo;
#pragma unroll
      for (int q = 0; q < 4; ++q) {  // sgd_apply's fma sequence
        float d = fmaf(wd, pv[q], g[q]);
        if (has_mom) d = fmaf(mom, mv[q], d);
        po[q] = fmaf(-lr, d, pv[q]);
        bo[q] = has_mom ? d : po[q];
      }
      if (stage) *reinterpret_cast<f32x4*>(stage) = po;
      const u32x2 sh = (u32x2){pack_bf2(po[0], po[1]), pack_bf2(po[2], po[3])};
      __builtin_nontemporal_store(po, reinterpret_cast<f32x4*>((sel ? P1 : P0) + off));
      __builtin_nontemporal_store(bo, reinterpret_cast<f32x4*>((sel ? M1 : M0) + off));
      *reinterpret_cast<u32x2*>((sel ? S1 : S0) + off) = sh;
      if constexpr (FP8) {  // MX-FP8 weight copy for the next forward: 8 lanes = one 32-column block
        unsigned e8;
        const unsigned q = mx::e4m3_group8(po, &e8);
        *reinterpret_cast<unsigned*>((sel ? Q1 : Q0) + off) = q;
        // the row's 4 block scales (lanes 0/8/16/24 of each half-wave) as two 2-byte stores by lanes 0 and 16 of
        // each half-wave, the neighbouring block's byte fetched by DPP row_ror:8 (plain VALU, no LDS permute on
        // the stream's per-update path); byte stores scattered over the tile's rows cost more than the codes
        const unsigned e1 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)e8, 0x128, 0xF, 0xF, false);
        if ((lane & 15) == 0)
          *reinterpret_cast<unsigned short*>((sel ? E1 : E0) + (off >> 5)) = (unsigned short)(e8 | (e1 << 8));
      }
      // refill: vector v + DIST of tile j, or vector v + DIST - SV of tile j + 1, or (past the last tile)
      // vector v of tile j again — a harmless reload that keeps the per-update operation count fixed
      const int vn = v + DIST;
      const bool same = vn < SV, next = !same && j + 1 < nt;
      load_vec(same ? j : (next ? j + 1 : j), same ? vn : (next ? vn - SV : v), pv, mv);
    };
    // update vector v of tile j from the gradient tile T
    auto update_vec = [&](int j, int v, const float* T, f32x4& pv, f32x4& mv) {
      if constexpr (FP8 && NSW == 8) {
        if (qt_on) {  // the updated vector back into its (consumed) gradient slot: the transposed copy's staging
          float* slot = const_cast<float*>(T) + (row0 + RSTEP * v) * ALD + col;
          const f32x4 g = *reinterpret_cast<const f32x4*>(slot);
          update_vec_g(j, v, g, pv, mv, slot);
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // visible to the other waves after the next barrier
          return;
        }
      }
      update_vec_g(j, v, grad_vec(T, v), pv, mv, nullptr);
    };
    // quantise rows [32 b, 32 b + 32) of tile j (staged in T) into the transposed copy
    auto quant_t = [&](int j, int b, const float* T) {
      int m0, n0;
      const int sel = tile_origin(j, m0, n0);
      unsigned char* const qd = sel ? QT1 : QT0;
      if (!qd) return;  // uniform: this GEMM writes no transposed copy
      const int c = st >> 2, sub = st & 3;
      float v[8];
      float am = 0.f;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        v[r] = bf2f(f2bf(T[(32 * b + 8 * sub + r) * ALD + c]));  // the bf16 copy's value, as the quantiser sees it
        am = fmaxf(am, fabsf(v[r]));
      }
      am = fmaxf(am, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, am), 0xB1, 0xF, 0xF, false)));
      am = fmaxf(am, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, am), 0x4E, 0xF, 0xF, false)));
      const int e = mx::block_exp(am, mx::kMaxE4M3);
      const float inv = ldexpf(1.f, -e);
      const unsigned lo = mx::quant4(v[0], v[1], v[2], v[3], inv, mx::kMaxE4M3, false);
      const unsigned hi = mx::quant4(v[4], v[5], v[6], v[7], inv, mx::kMaxE4M3, false);
      const int Mg = sel ? p1.M : p0.M;
      *reinterpret_cast<u32x2*>(qd + (size_t)(n0 + c) * Mg + m0 + 32 * b + 8 * sub) = (u32x2){lo, hi};
      unsigned char* const ed = sel ? ET1 : ET0;  // (null: codes only — measurement, benchmarks/pair_fp8t.py)
      if (sub == 0 && ed) {
        if (b == 0) {
          qt_e0 = (unsigned)(e + 127);
        } else {
          *reinterpret_cast<unsigned short*>(ed + (size_t)(n0 + c) * (Mg / 32) + m0 / 32) =
              (unsigned short)(qt_e0 | ((unsigned)(e + 127) << 8));
        }
      }
    };
    // iteration 0 (math fills the first tile): prefetch tile 0's first DIST vectors
#pragma unroll
    for (int v = 0; v < DIST; ++v)
      if constexpr (PROBE != 3) load_vec(0, v, rp[v], rm[v]);
    for (int t = 0; t < nk; ++t) {
      mark();
      __builtin_amdgcn_s_barrier();
    }
    mark();
    __builtin_amdgcn_s_barrier();
    // trip r = DIST K-steps: iteration i = 1 + r / TPI updates tile i - 1, vectors (r % TPI) * DIST .. + DIST - 1;
    // the first trip is peeled so the loop is entered with the same memory operations in flight as on its back
    // edge (the compiler then counts every update's ring wait, e.g. vmcnt(15) at DIST = 4, instead of the
    // entry path's smaller count)
    constexpr int TPI = SV / DIST;  // trips per iteration
    f32x4 gq[UPK];                  // single buffer: the next K-step's gradient vectors
    auto read_ahead = [&](int v0) {
      if constexpr (SBUF && PROBE != 3) {
#pragma unroll
        for (int k = 0; k < UPK; ++k) gq[k] = grad_vec(accb, v0 + k);
      }
    };
    read_ahead(0);  // (after the first hand-off barrier)
    auto trip = [&](int r) {
      const int i = 1 + r / TPI, t = (r % TPI) * DIST;
      const float* T = accb + (SBUF ? 0 : ((i - 1) & 1) * (ACC_BYTES / 4));
      f32x4 gc[UPK];
#pragma unroll
      for (int u = 0; u < DIST; ++u) {
        // sched_barrier: keep each update's register work (which waits for its ring slot) inside its K-step
        if (u % UPK == 0) {  // a K-step begins
          if constexpr (SBUF) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          mark();
          __builtin_amdgcn_s_barrier();
          __builtin_amdgcn_sched_barrier(0);
          if constexpr (SBUF && PROBE != 3) {
#pragma unroll
            for (int k = 0; k < UPK; ++k) gc[k] = gq[k];
            // not in the iteration's last K-step (uniform; known at compile time except for the trip's last K-step)
            if (u + UPK < DIST || r % TPI != TPI - 1) read_ahead(t + u + UPK);
          }
        }
        if constexpr (PROBE != 3) {  // (3: measurement, math only)
          if constexpr (SBUF) update_vec_g(i - 1, t + u, gc[u % UPK], rp[u], rm[u], nullptr);
          else update_vec(i - 1, t + u, T, rp[u], rm[u]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 1; k < KPU; ++k) {
          mark();
          __builtin_amdgcn_s_barrier();
        }
        if constexpr (FP8 && NSW == 8) {  // SV = 4, TPI = 1: rows 0-31 are vectors 0-1, rows 32-63 vectors 2-3
          if (qt_on && (t + u) % 2 == 1) {
            quant_t(i - 1, (t + u) / 2, T);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
          }
        }
      }
      if (r % TPI == TPI - 1) {  // end of iteration i: the buffer hand-off barrier
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        mark();
        __builtin_amdgcn_s_barrier();
        read_ahead(0);  // the next tile's first vectors (after the last iteration: a read nobody uses)
      }
    };
    trip(0);
#pragma unroll 1
    for (int r = 1; r < TPI * nt; ++r) trip(r);
    if (stp) stp[kStampSlots - 1] = (long long)__builtin_amdgcn_s_memrealtime();
  }
}

// Eligible shapes: the plain weight-gradient layout (A M-contig, B N-contig), M % 64 == 0, N % 128 == 0,
// K == 512 (the batch: NK = 8 K-steps of 64, a tile's optimizer vectors spread evenly over them; the two roles'
// barrier counts are NK + 1 per iteration), ldc % 4 == 0.  The 128-row tile also needs M % 128 == 0 (select_variant).
static inline bool eligible(const pipe::Params& p, bool ak, bool bk) {
  return !ak && !bk && p.M % 64 == 0 && p.N % BN == 0 && p.K == 64 * NK && (p.ldc & 3) == 0 && p.sgd.p &&
         p.sgd.lr && (p.sgd.mom == 0.f || p.sgd.buf) && p.sgd.shadow && (!p.sgd.q8 || (p.sgd.s8 && (p.ldc & 127) == 0 && !((uintptr_t)p.sgd.q8 & 3) && !((uintptr_t)p.sgd.s8 & 3))) &&
         (!p.sgd.q8t || (p.sgd.q8 && !((uintptr_t)p.sgd.q8t & 7) && !((uintptr_t)p.sgd.s8t & 1)));
}

// Which instantiation a launch runs: the kernel's template arguments.
struct Variant {
  int bm;      // tile height, 64 or 128
  int stages;  // LDS-DMA ring depth, 3 or 4
  bool fp8;    // the stream waves also write the MX-FP8 copy
  int nsw;     // stream waves, 4 or 8
  bool nord;   // tile order: n fastest
  int nmw;     // math waves, 4 or 8
  int probe;   // 0, or 3 (math only) / 4 (stream only)
};

static inline int env_digit(const char* name) {
  const char* e = getenv(name);
  return e && e[0] >= '0' && e[0] <= '9' ? e[0] - '0' : -1;
}

// The variant of a launch over ntiles 64x128 tiles (qt: a transposed MX copy is requested; m128: every GEMM of the
// launch has M % 128 == 0).  "Large" is every CU owning >= 64 such tiles (the wide MLP, ~150 per CU); the toy MLP
// has 14 per CU.
//   bm:     128 exists in one layout (bf16, no MX copies, 3 stages, 4 stream waves, n order, 8 math waves) and needs
//           m128; a sibling knob that asks for another layout keeps 64 rows.  DDPX_WSGD_TILE=64|128 forces it where
//           that holds; else 128 when every CU gets a 128-row tile (toy pair, 7 per CU: 0.2105-0.2118 vs 0.2259-0.2270
//           ms/step; wide MLP, 76 per CU, instead of its 4-stage 8-stream-wave 64-row kernel; profiles/r7_pair).
//           The three entries below describe the 64-row kernel.
//   stages: DDPX_WSGD_STAGES=3|4 forces it; else 4 when large (wide MLP: 2.434 vs 2.469 ms/step), 3 below (toy MLP:
//           0.2398 vs 0.2502 ms/step; profiles/r2_stages).
//   nsw:    8 with the transposed MX copy (only that layout emits it); else DDPX_WSGD_STREAM_WAVES=4|8 forces it; else
//           8 when large (wide MLP: 2.108 vs 2.175 ms/step; with the MX-FP8 copy 2.055 / 2.059 ms with 8 / 4 math waves
//           vs 2.195 / 2.160 ms at 4 stream waves, profiles/r6_fp8), 4 below (toy pair 115.9 vs 120.4 us;
//           profiles/r3_wsgd).
//   nord:   DDPX_WSGD_ORDER=n (default) | m.
//   nmw:    8 beside 4 n-ordered stream waves unless DDPX_WSGD_MATH_WAVES=4 (profiles/r6_pair); else 4.
//   probe:  DDPX_WSGD_XTRA=3|4, honoured for the toy pair's layout only (bf16, 3 stages, 4 stream waves, n order).
static inline Variant select_variant(long long ntiles, int num_cus, bool fp8, bool qt, bool m128) {
  static const int env_stages = env_digit("DDPX_WSGD_STAGES"), env_nsw = env_digit("DDPX_WSGD_STREAM_WAVES");
  static const int env_nmw = env_digit("DDPX_WSGD_MATH_WAVES");
  static const int env_probe = [] {
    const char* e = getenv("DDPX_WSGD_XTRA");
    return e ? atoi(e) : 0;
  }();
  static const int env_tile = [] {
    const char* e = getenv("DDPX_WSGD_TILE");
    return e ? atoi(e) : 0;
  }();
  static const bool env_nord = [] {
    const char* e = getenv("DDPX_WSGD_ORDER");
    return !(e && e[0] == 'm');
  }();
  const bool large = ntiles >= 64LL * num_cus;
  Variant v;
  v.bm = 64;
  v.stages = (env_stages == 3 || env_stages == 4) ? env_stages : (large ? 4 : 3);
  v.fp8 = fp8;
  v.nsw = qt ? 8 : (env_nsw == 4 || env_nsw == 8) ? env_nsw : (large ? 8 : 4);
  v.nord = env_nord;
  v.nmw = (env_nmw != 4 && v.nsw == 4 && v.nord) ? 8 : 4;
  // the 128-row tile has one layout; a sibling knob that asks for another one keeps 64 rows
  const bool can128 = m128 && !fp8 && !qt && env_stages != 4 && env_nsw != 8 && env_nmw != 4 && env_nord;
  const bool want128 = env_tile == 128 || (env_tile != 64 && ntiles >= 2LL * num_cus);
  if (want128 && can128) v.bm = 128, v.stages = 3, v.nsw = 4, v.nmw = 8;
  const bool toy = !fp8 && v.stages == 3 && v.nsw == 4 && v.nord;
  v.probe = (toy && (env_probe == 3 || env_probe == 4)) ? env_probe : 0;
  return v;
}

using Kernel = void (*)(pipe::Params, pipe::Params, int);

// The (stream waves, order, math waves) layouts of one ring depth and precision.
template <int STAGES, bool FP8>
static inline Kernel layout_kernel(const Variant& v) {
  // (the 64-row kernel's defaults: where the 128-row tile does not apply)
  if (v.nmw == 8) return wgrad_sgd_ws_kernel<64, STAGES, FP8, 4, true, 8>;  // default below 64 tiles per CU
  if (v.nsw == 8) return v.nord ? wgrad_sgd_ws_kernel<64, STAGES, FP8, 8, true, 4>  // default from 64 tiles per CU
                                : wgrad_sgd_ws_kernel<64, STAGES, FP8, 8, false, 4>;
  return v.nord ? wgrad_sgd_ws_kernel<64, STAGES, FP8, 4, true, 4> : wgrad_sgd_ws_kernel<64, STAGES, FP8, 4, false, 4>;
}

static inline Kernel kernel_of(const Variant& v) {
  if (v.bm == 128) {  // one layout: bf16, 3 stages, 4 stream waves, n order, 8 math waves (select_variant)
    if (v.probe == 3) return wgrad_sgd_ws_kernel<128, 3, false, 4, true, 8, 3>;
    if (v.probe == 4) return wgrad_sgd_ws_kernel<128, 3, false, 4, true, 8, 4>;
    return wgrad_sgd_ws_kernel<128, 3, false, 4, true, 8>;  // default for the toy and the wide MLP's pairs
  }
  if (v.probe == 3)
    return v.nmw == 8 ? wgrad_sgd_ws_kernel<64, 3, false, 4, true, 8, 3> : wgrad_sgd_ws_kernel<64, 3, false, 4, true, 4, 3>;
  if (v.probe == 4)
    return v.nmw == 8 ? wgrad_sgd_ws_kernel<64, 3, false, 4, true, 8, 4> : wgrad_sgd_ws_kernel<64, 3, false, 4, true, 4, 4>;
  if (v.stages == 4) return v.fp8 ? layout_kernel<4, true>(v) : layout_kernel<4, false>(v);
  return v.fp8 ? layout_kernel<3, true>(v) : layout_kernel<3, false>(v);
}

// The variant a launch of one (pair = false: p0 only) or two GEMMs runs.
static inline Variant plan(const pipe::Params& p0, const pipe::Params& p1, bool pair, bool qt, int num_cus) {
  const long long nt64 = (long long)(p0.M / 64) * (p0.N / BN) + (pair ? (long long)(p1.M / 64) * (p1.N / BN) : 0);
  const bool m128 = p0.M % 128 == 0 && (!pair || p1.M % 128 == 0);
  return select_variant(nt64, num_cus, p0.sgd.q8 != nullptr, qt, m128);
}

// p0's tiles then p1's (a single GEMM passes p1 = p0, pair = false), one workgroup per CU.
static inline hipError_t launch_variant(const pipe::Params& p0, const pipe::Params& p1, bool pair, bool qt,
                                        int num_cus, hipStream_t s) {
  const Variant v = plan(p0, p1, pair, qt, num_cus);
  const int nt1 = pair ? (p1.M / v.bm) * (p1.N / BN) : 0;
  const int ntiles = (p0.M / v.bm) * (p0.N / BN) + nt1;
  const int grid = ntiles < num_cus ? ntiles : num_cus;
  hipLaunchKernelGGL(kernel_of(v), dim3(grid), dim3(64 * (v.nmw + v.nsw)), 0, s, p0, p1, nt1);
  return hipGetLastError();
}

static inline hipError_t launch(const pipe::Params& p, int num_cus, hipStream_t s) {
  return launch_variant(p, p, false, false, num_cus, s);
}

// Both weight gradients (+ their SGD updates) in one launch; the caller checked eligible() for both and equal
// K / alpha / lr / momentum / wd (pair_compatible).
static inline bool pair_compatible(const pipe::Params& a, const pipe::Params& b) {
  return a.K == b.K && a.alpha == b.alpha && a.sgd.lr == b.sgd.lr && a.sgd.mom == b.sgd.mom && a.sgd.wd == b.sgd.wd;
}

static inline hipError_t launch_pair(const pipe::Params& p0, const pipe::Params& p1, int num_cus, hipStream_t s) {
  if ((p0.sgd.q8 != nullptr) != (p1.sgd.q8 != nullptr)) return hipErrorInvalidValue;  // both or neither
  const bool qt = p0.sgd.q8t != nullptr || p1.sgd.q8t != nullptr;
  if (qt && !p0.sgd.q8) return hipErrorInvalidValue;
  return launch_variant(p0, p1, true, qt, num_cus, s);
}

}  // namespace wsgd
}  // namespace ddpx
