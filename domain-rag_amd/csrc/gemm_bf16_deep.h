// gemm_bf16_deep.h — the ring kernel's body; gemm_bf16_deep_n128.hip / _n192a.hip / _n192b.hip instantiate it (the 17 instantiations
// compile longer than any other source of the library, so they are spread over three objects).
#pragma once
#include "gemm_bf16_kernels.h"

namespace drag_gemm {

// --------------------------------------------------------------------------------------------
// gemm_bf16_deep — (32*MI) x 128 x 64 tile, 4 waves (2x2), wave tile (16*MI) x 64, ST-stage LDS-DMA ring with COUNTED waits.
// For the launches that cannot fill the chip with 256x256 tiles (BASELINE configs[1]: 512 / 1024 / 1536 rows): there a
// workgroup's K loop is a latency chain — the double-buffered t128 loop above exposes one L2/HBM round trip per K-step
// (0.9 us per step measured at K = 12288 / 15360, 28 % of a CU's MFMA rate) — so the ring keeps ST-1 K-steps in flight per
// workgroup and smaller M tiles put more workgroups on the chip.  Same MFMA, same k order per output element as the other
// two kernels: bit-identical results, so the choice may depend on the launch's shape (batch invariance is kept).
// Stage = A tile (32*MI rows) then W tile (128 rows), 128 B per row, same XOR swizzle as t128.  Per stage a wave issues
// MI A chunks... (32*MI / 8 / 4) + 4 W chunks of 8 rows.  The epilogue slabs alias stage memory after the loop's last barrier.
// --------------------------------------------------------------------------------------------
// Round 3: the N extent of the tile is a template parameter too (NI column blocks of 16 per wave: 128- or 192-column tiles).
// A launch of this family is bound by what ONE CU can ingest from L2 (measured ~70 GB/s per CU through LDS-DMA, whatever the
// ring depth): its time is (K-steps) x (tile rows + tile columns) x 128 B x (tiles on the busiest CU) / that rate.  BASELINE
// configs[1]'s two heaviest shapes sit badly on 128-column tiles: (1536, 3072, 15360) is 288 128x128 tiles on 256 CUs (32 CUs
// carry two: 660 TFLOP/s) and (1536, 12288, 3072) is 1152 of them; 96x192 tiles make the first exactly 256 workgroups (one per
// CU, 44 % fewer bytes on the busiest CU) and 128x192 tiles make the second exactly 3 rounds of 256.  Same MFMA, same k order per
// output element: the bits cannot tell (test_gemm_kernels_are_bit_identical), so the choice stays a function of the launch shape.
template <int MI, int ST, int NI = 4>
// The ring is DYNAMIC shared memory and the kernel asks for two waves per SIMD: told the static LDS size of a one-workgroup-per-CU ring,
// hipcc sees a lone wave per SIMD, takes its 512-register budget, parks the accumulators in AGPRs and shuttles the loop-carried fragment
// set of the pipelined loop through ~300 v_accvgpr moves per K-step; inside 256 unified registers everything stays in arch VGPRs.
__global__ __launch_bounds__(256, 2) void gemm_bf16_deep(GemmKArgs p) {
  constexpr int TBM = 32 * MI, TBN = 32 * NI;
  constexpr int A_BYTES = TBM * 128, W_BYTES = TBN * 128, STAGE = A_BYTES + W_BYTES;
  constexpr int CA = TBM / 32;                 // A chunks (8 rows, 1 KiB) per wave per stage
  constexpr int CW = TBN / 32;                 // W chunks per wave per stage
  constexpr int CH = CA + CW;                  // DMA instructions per wave per stage
  static_assert(ST >= 2 && ST <= 4 && ST * STAGE >= 4 * 2048 && ST * STAGE <= 160 * 1024 && (NI == 4 || NI == 6), "ring depth / tile");
  extern __shared__ __attribute__((aligned(16))) char smem[];       // ST * STAGE bytes (deep_lds_bytes)
  const int w = wave_id();
  const int l = lane_id();
  const int wr = w >> 1, wc = w & 1;
  int tm, tn;
  pick_tile(p, (int)blockIdx.x, tm, tn);
  pick_segment(p, tm);
  const int m0 = tm * TBM, n0 = tn * TBN;

  const long long a0 = p.am.off(m0);
  __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)(p.A + a0), 0, 0x7ffffff0u, 0x00020000);
  const int wrows = min(TBN, p.N - n0);
  __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)(p.W + (long long)n0 * p.K), 0,
                                                                 (unsigned)((long long)wrows * p.K * 2), 0x00020000);
  unsigned voffA[4], voffW[6];      // (an array of template-dependent bound captured by the lambda below loses the host stub in hipcc 7.2)
#pragma unroll
  for (int i = 0; i < CA; ++i) {
    const int row = (w * CA + i) * 8 + (l >> 3);
    const int slot = (l & 7) ^ ((row >> 1) & 7);
    const int ra = min(m0 + row, p.M - 1);                 // clamp: rows past the edge are never stored
    voffA[i] = (unsigned)((p.am.off(ra) - a0 + slot * 8) * 2);
  }
#pragma unroll
  for (int i = 0; i < CW; ++i) {
    const int row = (w * CW + i) * 8 + (l >> 3);
    const int slot = (l & 7) ^ ((row >> 1) & 7);
    const int rw = min(row, wrows - 1);
    voffW[i] = (unsigned)(((long long)rw * p.K + slot * 8) * 2);
  }
  auto stage = [&](int buf, int kt) {
    const int soff = kt * (BK * 2);
    DRAG_LDS char* d = (DRAG_LDS char*)smem + buf * STAGE;
#pragma unroll
    for (int i = 0; i < CA; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (DRAG_LDS void*)(d + (w * CA + i) * 1024), 16, voffA[i], soff, 0, 0);
#pragma unroll
    for (int i = 0; i < CW; ++i)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (DRAG_LDS void*)(d + A_BYTES + (w * CW + i) * 1024), 16, voffW[i], soff, 0, 0);
  };

  const int p0 = (l >> 4) ^ ((l & 15) >> 1);
  const int fa = (wr * (TBM / 2) + (l & 15)) * 128;            // + mi*2048
  const int fb = A_BYTES + (wc * (TBN / 2) + (l & 15)) * 128;  // + ni*2048

  f32x4_t acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  // ---- main loop, software-pipelined ACROSS the barrier.  One workgroup per CU means one wave per SIMD, all four in the same phase:
  // with "barrier | ds_read | MFMA" per K-step the LDS phase (72 KiB of fragment reads per K-step for a 96x192 tile = the MFMA time)
  // and the MFMA phase never overlap — (1536, 3072, 15360) ran 167 us where its operand stream alone takes 96 us and its MFMAs 58
  // (scripts/probe/probe_ingest.hip).  So the fragments live in two register sets (a lone wave per SIMD has 512 VGPRs): the k-half-1
  // reads of K-step kt issue before its k-half-0 MFMAs, the barrier of K-step kt+1 sits BETWEEN the two MFMA halves, and the k-half-0
  // reads of K-step kt+1 issue before the k-half-1 MFMAs of kt.  At that barrier every wave has finished reading buffer kt, so K-step
  // kt+ST is staged into it: ST K-steps in flight instead of ST-1 from the same LDS.  Same MFMA order per accumulator: same bits.
  const int nk = p.K / BK;
#pragma unroll
  for (int s2 = 0; s2 < ST; ++s2)
    if (s2 < nk) stage(s2, s2);
  auto wait_landed = [&](int younger) {      // the K-step awaited has `younger` stages behind it in this wave's (in-order) VMEM queue
    if (younger >= 3) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * CH) : "memory");
    else if (younger == 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * CH) : "memory");
    else if (younger == 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(CH) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };
  // The fragment reads are inline asm and the waits that retire them are counted by hand: left to the compiler, the older register set
  // is awaited with lgkmcnt(0) — which also drains the reads just issued for the other set, i.e. no overlap at all.  LDS returns in
  // order, so lgkmcnt(MI + NI) after issuing one set's reads means the previous set has landed.
  bf16x8_t xa0[MI], wb0[NI], xa1[MI], wb1[NI];
  const unsigned lds0 = (unsigned)(size_t)(DRAG_LDS char*)smem;
  const unsigned adA = lds0 + (unsigned)fa, adB = lds0 + (unsigned)(fb - A_BYTES);     // + buffer * STAGE + k-half slot
  auto read_half = [&](int b, int ks, bf16x8_t* xa, bf16x8_t* wb) {
    const unsigned so = (unsigned)(b * STAGE + ((p0 ^ (ks * 4)) << 4));
    lds_read_frags<MI, 0>(xa, adA + so);
    lds_read_frags<NI, A_BYTES>(wb, adB + so);
  };
  auto landed = [&](bf16x8_t* xa, bf16x8_t* wb) {      // after a wait: what was read into these registers may be used from here on
#pragma unroll
    for (int i = 0; i < MI; ++i) asm volatile("" : "+v"(xa[i]));
#pragma unroll
    for (int i = 0; i < NI; ++i) asm volatile("" : "+v"(wb[i]));
  };
  wait_landed(min(ST - 1, nk - 1));
  // A bare s_barrier: __syncthreads() carries a release fence, i.e. s_waitcnt vmcnt(0), which would drain the ring.
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
  read_half(0, 0, xa0, wb0);
  int buf = 0;
#define DRAG_DEEP_MMA(XA, WB) _Pragma("unroll") for (int mi = 0; mi < MI; ++mi) _Pragma("unroll") for (int ni = 0; ni < NI; ++ni) \
    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(WB[ni], XA[mi], acc[mi][ni], 0, 0, 0)
  int kt = 0;
  // steady state: K-steps kt+1 .. kt+ST-1 are issued and K-step kt+ST exists — one basic block per K-step, nothing conditional
  for (; kt + ST < nk; ++kt) {
    const int nb = buf + 1 == ST ? 0 : buf + 1;
    read_half(buf, 1, xa1, wb1);
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(MI + NI) : "memory");      // k-half 0 of this K-step (read one MFMA half ago) landed
    landed(xa0, wb0);
    DRAG_DEEP_MMA(xa0, wb0);
    __builtin_amdgcn_sched_barrier(0);                           // (the waits below must not rise above the MFMAs)
    // K-step kt+1 landed for this wave (ST-2 younger stages stay in flight) and its own reads of buffer kt are complete ...
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((ST - 2) * CH) : "memory");
    // ... for every wave
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    stage(buf, kt + ST);
    read_half(nb, 0, xa0, wb0);
    landed(xa1, wb1);                      // (volatile asm keeps its order: this half's MFMAs cannot rise above the reads just issued)
    DRAG_DEEP_MMA(xa1, wb1);
    buf = nb;
  }
  // the last ST K-steps: nothing left to stage, the ring drains
  for (; kt < nk; ++kt) {
    const int nb = buf + 1 == ST ? 0 : buf + 1;
    read_half(buf, 1, xa1, wb1);
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(MI + NI) : "memory");
    landed(xa0, wb0);
    DRAG_DEEP_MMA(xa0, wb0);
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 1 < nk) {
      wait_landed(min(ST - 2, nk - 2 - kt));
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      read_half(nb, 0, xa0, wb0);
      landed(xa1, wb1);
    } else {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      landed(xa1, wb1);
    }
    DRAG_DEEP_MMA(xa1, wb1);
    buf = nb;
  }
#undef DRAG_DEEP_MMA
  const GemmKArgs pd = dest_of(p, n0);
  if (p.wide) {
    __syncthreads();                              // the slabs alias the ring
    staged_epilogue<MI, TBM, TBN, NI>(pd, m0, m0 + wr * (TBM / 2), n0, n0 + wc * (TBN / 2), l, acc, smem + w * 2048);
  } else {
    wave_epilogue<MI, TBM, TBN, NI>(pd, m0, m0 + wr * (TBM / 2) + (l & 15), n0, n0 + wc * (TBN / 2) + (l >> 4) * 4, acc);
  }
}

}  // namespace drag_gemm
