// gemm_bf16_t256.h — the 8-wave persistent 256x256x64 kernel's body; gemm_bf16_t256.hip (batched rows, conv3x3) and gemm_bf16_t256_pair.hip
// (two row segments) instantiate it: together the three instantiations compile longer than any other source of the library.
#pragma once
#include "gemm_bf16_kernels.h"

namespace drag_gemm {

// --------------------------------------------------------------------------------------------
// gemm_bf16_t256 — 256x256x64 tile, 8 waves (2 along M x 4 along N), wave tile 128x64 as 8x4
// v_mfma_f32_16x16x32_bf16 (128 accumulator registers).  LDS: 2 K-tile buffers x {A0,A1,B0,B1}
// half-tiles of 128 rows x 64 k (16 KiB each) = 128 KiB, one workgroup per CU, 2 waves per SIMD.
//
// Per K-tile t (buffer t&1) TWO phases, each = load segment | barrier | 32 MFMAs | barrier (4 barriers per K-tile):
//   phase A  reads W cols 0-63 + X rows 0-63 (16 x ds_read_b128)   quadrants (0,0) (0,1)
//   phase B  reads X rows 64-127 (8)                               quadrants (1,1) (1,0)
// A wave never needs a whole K-tile at once, so the LDS-DMA stream is cut into four 16-KiB PIECES ordered by
// need-time instead of by operand:
//   alpha = A rows 0-63 of both halves          beta  = W rows {0-31, 64-95} of both halves       (read in A)
//   gamma = W rows {32-63, 96-127}   (read in A) delta = A rows 64-127 of both halves             (read in B)
// and issued into the slot whose last reader finished >= 1 phase earlier:
//   phase A(t): delta(t+1)   (2 DMA per wave)        phase B(t): alpha, beta, gamma (t+2)   (6 DMA per wave)
// -> load segments of 16 reads + 2 DMA and 8 reads + 6 DMA, both shorter than the partner group's 32-MFMA segment;
// every piece is in flight for 2 phases (one K-tile) before the wait that retires it, ~80 KiB are in flight per CU
// and the queue is never drained: both waits are the COUNTED s_waitcnt vmcnt(8) (four younger pieces stay in flight).
// (Measured alternatives, same data: four phases of 16 MFMAs with 8 barriers per K-tile -3 %; DMA issue inside the
//  MFMA segment -10 %; k-step-split fragment reads -3 %; 32x32x16 MFMA -7 %; waiting for reads after the barrier +-0.)
// The two wave groups (wr = 0 / 1: one wave of each per SIMD) run staggered by one barrier, so one group's MFMA
// segment overlaps the other's ds_read / DMA-issue segment (s_setprio favours the MFMA side).
// Hazard rules this schedule satisfies: (RAW) data read in the load segment of phase p is waited for (vmcnt) by
// EVERY wave in the load segment of phase p-1, i.e. before a barrier that the staggered group has passed before
// it reads; (WAR) every ds_read is retired (lgkmcnt(0)) before its phase's first barrier and a slot is restaged
// >= 1 phase after its last read; the compiler may not move anything across a barrier (sched_barrier).
// --------------------------------------------------------------------------------------------
constexpr int T2_HALF = 128 * BK * 2;          // 16 KiB half-tile
constexpr int T2_BUF = 4 * T2_HALF;            // A0 A1 B0 B1

#define T2_BARRIER()                      \
  do {                                    \
    __builtin_amdgcn_sched_barrier(0);    \
    __builtin_amdgcn_s_barrier();         \
    __builtin_amdgcn_sched_barrier(0);    \
  } while (0)

template <int MODE, bool SEG>   // SEG: the launch may carry a second row segment (drag_gemm_bf16_pair)
__device__ __forceinline__ void t256_body(const GemmKArgs& p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * T2_BUF + 8 * 2048];   // + one 2 KiB epilogue slab per wave
  const int w = wave_id();
  const int l = lane_id();
  const int wr = w >> 2, wc = w & 3;
  // ---- persistent: this workgroup computes tiles vb, vb + P, vb + 2P ... (P = gridDim.x, a multiple of 8 whenever a
  // workgroup has more than one tile, so every tile of a workgroup maps to the XCD the workgroup runs on).  The LDS-DMA
  // stream runs CONTINUOUSLY across tile boundaries: the last two K-steps of a tile already fetch K-steps 0 and 1 of
  // the next one, so the epilogue's stores overlap the next tile's loads and only the first tile pays a prologue.
  const int P = (int)gridDim.x;
  const int nwg = p.tiles_m * p.tiles_n;
  int vb = (int)blockIdx.x;

  // ---- load state of ONE tile (switched in place two K-steps before the tile's first MFMA)
  __amdgpu_buffer_rsrc_t rsA, rsW;
  unsigned vo[4][2];          // [piece: 0 alpha, 1 beta, 2 gamma, 3 delta][chunk] global byte offset (per lane)
  int lo[4][2];               // LDS byte offset of the chunk inside a K-tile buffer (wave-uniform, tile-independent)
  // staging role: every piece has 16 chunks of 8 rows; this wave moves chunks c = 2w, 2w+1 of each piece.
  // chunk c -> operand half (c>>3) and an 8-row group inside it:
  //   alpha: rows 8*(c&7)              delta: rows 64 + 8*(c&7)
  //   beta : sub=c&7: rows 8*sub (sub<4) | 64 + 8*(sub-4)      gamma: rows 32 + 8*sub | 96 + 8*(sub-4)
  auto chunk_row0 = [&](int pc, int sub) {
    if (pc == 0) return 8 * sub;
    if (pc == 3) return 64 + 8 * sub;
    if (pc == 1) return sub < 4 ? 8 * sub : 64 + 8 * (sub - 4);
    return sub < 4 ? 32 + 8 * sub : 96 + 8 * (sub - 4);
  };
#pragma unroll
  for (int pc = 0; pc < 4; ++pc)
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
      const int c = w * 2 + c2, half = c >> 3;
      lo[pc][c2] = ((pc == 0 || pc == 3 ? 0 : 2) + half) * T2_HALF + chunk_row0(pc, c & 7) * 128;
    }
  auto load_state = [&](int tile) {
    int tm, tn;
    pick_tile(p, tile, tm, tn);
    const bf16_t* A = p.A;
    const bf16_t* W = p.W;
    int M = p.M;
    RowMap am = p.am;
    if (SEG && p.seg_tiles_m > 0 && tm >= p.seg_tiles_m) { tm -= p.seg_tiles_m; A = p.A2; W = p.W2; M = p.M2; am = p.am2; }
    const int m0 = tm * 256, n0 = tn * 256;
    // descriptors are based at the tile's first row, so operands of any size work with 32-bit in-tile offsets
    const long long a0 = MODE == 0 ? am.off(m0) : p.cv.off(m0);
    rsA = __builtin_amdgcn_make_buffer_rsrc((void*)(A + a0), 0, 0x7ffffff0u, 0x00020000);
    const int wrows = min(256, p.N - n0);
    rsW = __builtin_amdgcn_make_buffer_rsrc((void*)(W + (long long)n0 * p.K), 0, (unsigned)((long long)wrows * p.K * 2),
                                            0x00020000);
#pragma unroll
    for (int pc = 0; pc < 4; ++pc)
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        const int c = w * 2 + c2, half = c >> 3;
        const int row = chunk_row0(pc, c & 7) + (l >> 3);      // this lane's row inside the half
        const int slot = (l & 7) ^ ((row >> 1) & 7);
        if (pc == 0 || pc == 3) {
          const int ra = min(m0 + half * 128 + row, M - 1);    // clamp: rows past the edge are never stored
          vo[pc][c2] = (unsigned)(((MODE == 0 ? am.off(ra) : p.cv.off(ra)) - a0 + slot * 8) * 2);
        } else {
          const int rw = min(half * 128 + row, wrows - 1);
          vo[pc][c2] = (unsigned)(((long long)rw * p.K + slot * 8) * 2);
        }
      }
  };
  const int cchunks = MODE == 1 ? p.cv.Cin / BK : 1;
  const int nk = p.K / BK;                          // >= 4 (use_t256)
  auto issue = [&](int pc, int kt, int buf) {       // K-step kt of the tile in the load state -> LDS buffer buf
    int soff = kt * (BK * 2);
    if (MODE == 1 && (pc == 0 || pc == 3)) {
      const int tap = kt / cchunks, cc = kt - tap * cchunks;
      const int r = tap / 3, sx = tap - r * 3;
      soff = ((r * p.cv.Wp + sx) * p.cv.Cin + cc * BK) * 2;
    }
    DRAG_LDS char* d = (DRAG_LDS char*)smem + buf * T2_BUF;
    if (pc == 0 || pc == 3) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (DRAG_LDS void*)(d + lo[pc][0]), 16, vo[pc][0], soff, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (DRAG_LDS void*)(d + lo[pc][1]), 16, vo[pc][1], soff, 0, 0);
    } else {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (DRAG_LDS void*)(d + lo[pc][0]), 16, vo[pc][0], soff, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (DRAG_LDS void*)(d + lo[pc][1]), 16, vo[pc][1], soff, 0, 0);
    }
  };

  // fragment read offsets inside this wave's A half (wr) and B half (wc>>1)
  const int p0 = (l >> 4) ^ ((l & 15) >> 1);
  const int fx = wr * T2_HALF + (l & 15) * 128;                                   // + mi*2048
  const int fw = (2 + (wc >> 1)) * T2_HALF + ((wc & 1) * 64 + (l & 15)) * 128;    // + ni*2048

  // ---- TWO phases per K-step (32 MFMAs each), 4 barriers per K-step:
  //   phase A: reads W cols 0-63 + X rows 0-63 (16 x b128), issues delta(g+1),            quadrants (0,0) (0,1)
  //   phase B: reads X rows 64-127 (8),                     issues alpha,beta,gamma(g+2), quadrants (1,1) (1,0)
  // (16 reads + 2 DMA | 8 reads + 6 DMA: both load segments fit under the partner group's 32-MFMA segment.)
  // stream:  B(g): a,b,g(g+2)   A(g+1): d(g+2)   B(g+1): a,b,g(g+3) ...   every wait leaves 4 younger pieces: vmcnt(8).
  // g counts K-steps over ALL tiles of this workgroup (buffer = g & 1).
  load_state(vb);
  issue(0, 0, 0); issue(1, 0, 0); issue(2, 0, 0); issue(3, 0, 0);
  issue(0, 1, 1); issue(1, 1, 1); issue(2, 1, 1);
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");     // alpha, beta, gamma (0) landed
  T2_BARRIER();
  if (wr == 1) T2_BARRIER();                       // stagger the second wave group by one barrier

  bf16x8_t xf[4][2], w0[2][2], w1[2][2];
  f32x4_t acc[8][4];
#define T2_MMA(wsel, mh, nh) _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) _Pragma("unroll") for (int mi = 0; mi < 4; ++mi) \
    _Pragma("unroll") for (int ni = 0; ni < 2; ++ni) \
      acc[4 * (mh) + mi][2 * (nh) + ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wsel[ni][ks], xf[mi][ks], \
                                                                                  acc[4 * (mh) + mi][2 * (nh) + ni], 0, 0, 0)
  // wait until at most `8 + extra` VMEM operations are outstanding; with nothing younger in the stream: drain.
  // Right after an interior tile's epilogue the >= 16 stores it issued sit between the piece waited for and the
  // youngest pieces (VMEM operations of a wave retire in issue order), so 16 more may stay in flight.
#define T2_WAIT(more, relaxed) do { if (!(more)) asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); \
                                    else if (relaxed) asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); \
                                    else asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); } while (0)

  int g = 0;
  bool after_interior_epilogue = false;
  for (;;) {
    const bool have_next = vb + P < nwg;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
    for (int t = 0; t < nk; ++t, ++g) {
      const char* sb = smem + (g & 1) * T2_BUF;
      const bool more1 = t + 1 < nk || have_next;      // K-step g+1 exists
      const bool more2 = t + 2 < nk || have_next;      // K-step g+2 exists
      const bool relaxed = after_interior_epilogue && t == 0;
      // ================= phase A =================
#pragma unroll
      for (int ni = 0; ni < 2; ++ni)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
          w0[ni][ks] = *(const bf16x8_t*)(sb + fw + ni * 2048 + ((p0 ^ (ks * 4)) << 4));
          w1[ni][ks] = *(const bf16x8_t*)(sb + fw + (2 + ni) * 2048 + ((p0 ^ (ks * 4)) << 4));
        }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) xf[mi][ks] = *(const bf16x8_t*)(sb + fx + mi * 2048 + ((p0 ^ (ks * 4)) << 4));
      if (more1) issue(3, t + 1 < nk ? t + 1 : 0, (g + 1) & 1);   // delta(g+1): A rows 64-127 of the other buffer, last read in B(g-1)
      T2_WAIT(more1, relaxed);                          // delta(g) landed (read in phase B)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      T2_BARRIER();
      __builtin_amdgcn_s_setprio(1);
      T2_MMA(w0, 0, 0);
      T2_MMA(w1, 0, 1);
      __builtin_amdgcn_s_setprio(0);
      T2_BARRIER();
      // ================= phase B =================
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) xf[mi][ks] = *(const bf16x8_t*)(sb + fx + (4 + mi) * 2048 + ((p0 ^ (ks * 4)) << 4));
      // every later load of this tile has been issued: from here on the stream fetches the next tile
      if (t == nk - 2 && have_next) load_state(vb + P);
      if (more2) {                                     // slots last read in phase A of this K-step
        const int kt = t + 2 < nk ? t + 2 : t + 2 - nk;
        issue(0, kt, g & 1); issue(1, kt, g & 1); issue(2, kt, g & 1);
      }
      T2_WAIT(more2, relaxed);                          // alpha, beta, gamma (g+1) landed (read in A of the next K-step)
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      T2_BARRIER();
      __builtin_amdgcn_s_setprio(1);
      T2_MMA(w1, 1, 1);
      T2_MMA(w0, 1, 0);
      __builtin_amdgcn_s_setprio(0);
      T2_BARRIER();
    }
    if (!have_next && wr == 0) T2_BARRIER();         // balance the stagger before the last epilogue
    int tm, tn;
    pick_tile(p, vb, tm, tn);
    GemmKArgs pd = p;
    if (SEG) pick_segment(pd, tm);
    const int m0 = tm * 256, n0 = tn * 256;
    pd = dest_of(pd, n0);
    if (pd.wide) staged_epilogue<8, 256>(pd, m0, m0 + wr * 128, n0, n0 + wc * 64, l, acc, smem + 2 * T2_BUF + w * 2048);
    else wave_epilogue<8, 256>(pd, m0, m0 + wr * 128 + (l & 15), n0, n0 + wc * 64 + (l >> 4) * 4, acc);
    if (!have_next) break;
    after_interior_epilogue = m0 + 256 <= pd.M && n0 + 256 <= p.N;
    vb += P;
  }
#undef T2_MMA
#undef T2_WAIT
}

template <int MODE>
__global__ __launch_bounds__(512, 2) void gemm_bf16_t256(GemmKArgs p) { t256_body<MODE, false>(p); }

}  // namespace drag_gemm
