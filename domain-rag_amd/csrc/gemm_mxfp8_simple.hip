// gemm_mxfp8_simple.hip — the 128x128 kernel of drag_gemm_mxfp8 (gemm_mxfp8.hip launches it): correctness first.
//
// 256 threads = 4 waves (2x2), 128x128 tile, K-step 128 (= 128 bytes per row: the bytes of the bf16 kernels' K-step of 64, so the LDS
// image and its XOR swizzle are gemm_bf16_t128's).  Each wave a 64x64 sub-tile as 4x4 v_mfma_scale_f32_16x16x128_f8f6f4.  Operand tiles
// go HBM -> registers -> LDS with ordinary 16-byte loads and stores, double-buffered: the loads of step k + 1 are in flight under the MFMAs
// of step k, one barrier per K-step.  Scales go global -> register as the row's dword of the K-step (4 e8m0 bytes), one step ahead; the lane's
// byte is shifted into place (OPSEL 0).
// Rows past an edge are clamped on the load and never stored.  The operand map: gemm_mxfp8.h.
#include "gemm_mxfp8.h"

namespace drag_gemm {

__global__ __launch_bounds__(256, 2) void gemm_mxfp8_simple(MxKArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE_BYTES + 4 * 2048];  // A0 A1 W0 W1 + one epilogue slab per wave
  const GemmKArgs& g = p.g;
  const int w = wave_id();
  const int l = lane_id();
  const int t = (int)threadIdx.x;
  const int wr = w >> 1, wc = w & 1;
  int tm, tn;
  pick_tile(g, (int)blockIdx.x, tm, tn);
  const int m0 = tm * BM, n0 = tn * BN;
  const int K = g.K, kb = K >> 5;                          // kb: scale bytes per row

  // ---- staging: thread t moves 16-byte chunks {t, t + 256, t + 512, t + 768} of each 128-row x 128-byte operand tile ----
  const uint8_t* ga[4];
  const uint8_t* gw[4];
  int lofs[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = i * 256 + t;
    const int row = c >> 3, slot = c & 7;
    ga[i] = p.Aq + (long long)min(m0 + row, g.M - 1) * K + slot * 16;
    gw[i] = p.Wq + (long long)min(n0 + row, g.N - 1) * K + slot * 16;
    lofs[i] = row * 128 + ((slot ^ ((row >> 1) & 7)) << 4);
  }
  // ---- fragments: lane l reads row (l & 15) + 16 i of its wave's rows, logical 16-byte slots (l >> 4) and 4 + (l >> 4) of the K-step ----
  const int r16 = l & 15, blk = l >> 4;
  const int sw = (r16 >> 1) & 7;                           // the swizzle term of rows 16 i + r16 (16 i adds a multiple of 8 to row >> 1)
  const int so0 = (blk ^ sw) << 4, so1 = ((4 + blk) ^ sw) << 4;
  const int fa = (wr * 64 + r16) * 128;                    // + i * 2048
  const int fb = (wc * 64 + r16) * 128;
  const uint32_t* sa[4];                                   // the scale dword of K-step 0 of this lane's rows (kb % 4 == 0: aligned)
  const uint32_t* sb[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    sa[i] = (const uint32_t*)(p.As + (long long)min(m0 + wr * 64 + i * 16 + r16, g.M - 1) * kb);
    sb[i] = (const uint32_t*)(p.Ws + (long long)min(n0 + wc * 64 + i * 16 + r16, g.N - 1) * kb);
  }

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  u32x4_t ra[4], rw[4];
  int xs[4], ws[4];
  auto load = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = *(const u32x4_t*)(ga[i] + kt * 128);
      rw[i] = *(const u32x4_t*)(gw[i] + kt * 128);
      xs[i] = (int)sa[i][kt];
      ws[i] = (int)sb[i][kt];
    }
  };

  const int nk = K >> 7;
  load(0);
  for (int kt = 0; kt < nk; ++kt) {
    char* sA = smem + (kt & 1) * TILE_BYTES;
    char* sB = smem + (2 + (kt & 1)) * TILE_BYTES;
    // (this buffer was last read in step kt - 2; every wave has passed step kt - 1's barrier since)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *(u32x4_t*)(sA + lofs[i]) = ra[i];
      *(u32x4_t*)(sB + lofs[i]) = rw[i];
    }
    int xsc[4], wsc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { xsc[i] = (int)((unsigned)xs[i] >> (8 * blk)); wsc[i] = (int)((unsigned)ws[i] >> (8 * blk)); }
    __syncthreads();
    if (kt + 1 < nk) load(kt + 1);
    i32x8_t xa[4], wb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const u32x4_t a0 = *(const u32x4_t*)(sA + fa + i * 2048 + so0), a1 = *(const u32x4_t*)(sA + fa + i * 2048 + so1);
      const u32x4_t b0 = *(const u32x4_t*)(sB + fb + i * 2048 + so0), b1 = *(const u32x4_t*)(sB + fb + i * 2048 + so1);
      xa[i] = (i32x8_t){(int)a0[0], (int)a0[1], (int)a0[2], (int)a0[3], (int)a1[0], (int)a1[1], (int)a1[2], (int)a1[3]};
      wb[i] = (i32x8_t){(int)b0[0], (int)b0[1], (int)b0[2], (int)b0[3], (int)b1[0], (int)b1[1], (int)b1[2], (int)b1[3]};
    }
#pragma unroll
    for (int mi = 0; mi < 4; ++mi)
#pragma unroll
      for (int ni = 0; ni < 4; ++ni)
        acc[mi][ni] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wb[ni], xa[mi], acc[mi][ni], 0, 0, 0, wsc[ni], 0, xsc[mi]);
  }

  // ---- epilogue (the bf16 GEMM's): lane holds C[m = .. + (l & 15)][n = .. + (l >> 4) * 4 + 0..3] ----
  if (g.wide) staged_epilogue<4, BM>(g, m0, m0 + wr * 64, n0, n0 + wc * 64, l, acc, smem + 4 * TILE_BYTES + w * 2048);
  else wave_epilogue<4, BM>(g, m0, m0 + wr * 64 + (l & 15), n0, n0 + wc * 64 + (l >> 4) * 4, acc);
}

}  // namespace drag_gemm
