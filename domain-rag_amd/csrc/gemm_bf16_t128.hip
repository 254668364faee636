// gemm_bf16_t128.hip — the 128x128x64 kernel of drag_gemm_bf16 / drag_conv3x3_bf16 (gemm_bf16.hip launches it).
//
// Structure (kernel "t128"): 256 threads = 4 waves (2x2), 128x128x64 tile, each wave a 64x64
// sub-tile as 4x4 v_mfma_f32_16x16x32_bf16.  Operand tiles go HBM -> LDS by LDS-DMA
// (buffer_load_dwordx4 ... lds, 1 KiB per wave-instruction), double-buffered, one barrier
// per K-tile.  The LDS image is lane-linear, so the bank-conflict XOR swizzle is applied to
// the per-lane *source* address and again on the ds_read_b128 (involution).
// MFMA operands are swapped (a = W fragment, b = A fragment) so each lane ends up holding 4
// consecutive output columns -> 8-byte bf16 stores and vector bias/gate/residual loads.
#include "gemm_bf16_kernels.h"

namespace drag_gemm {

template <int MODE>  // 0: batched rows, 1: conv3x3 implicit GEMM
__global__ __launch_bounds__(256, 2) void gemm_bf16_t128(GemmKArgs p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE_BYTES + 4 * 2048];  // A0 A1 B0 B1 + one epilogue slab per wave
  const int w = wave_id();
  const int l = lane_id();
  const int wr = w >> 1, wc = w & 1;

  // ---- tile selection: XCD-contiguous, grouped along M for L2 reuse of the W panel ----
  const int nwg = p.tiles_m * p.tiles_n;
  int wg = xcd_remap((int)blockIdx.x, nwg);
  constexpr int GROUP_M = 8;
  const int in_group = GROUP_M * p.tiles_n;
  const int gid = wg / in_group;
  const int first_m = gid * GROUP_M;
  const int gsz = min(p.tiles_m - first_m, GROUP_M);
  const int rem = wg - gid * in_group;
  int tm = first_m + rem % gsz;
  const int tn = rem / gsz;
  if (MODE == 0) pick_segment(p, tm);
  const int m0 = tm * BM, n0 = tn * BN;

  // ---- staging addresses: wave w stages 8-row chunks {4w..4w+3} of both tiles ----
  // descriptors are based at the tile's first row (addresses grow with the row index), so operands
  // of any size work with 32-bit in-tile offsets; rows are clamped, so no access leaves the tensor
  const long long a0 = MODE == 0 ? p.am.off(m0) : p.cv.off(m0);
  __amdgpu_buffer_rsrc_t rsA = __builtin_amdgcn_make_buffer_rsrc((void*)(p.A + a0), 0, 0x7ffffff0u, 0x00020000);
  // W descriptor is based at this tile's first row, so stacked weights of any size work
  const int wrows = min(BN, p.N - n0);
  __amdgpu_buffer_rsrc_t rsW = __builtin_amdgcn_make_buffer_rsrc((void*)(p.W + (long long)n0 * p.K), 0,
                                                                 (unsigned)((long long)wrows * p.K * 2), 0x00020000);
  unsigned voffA[4], voffW[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (w * 4 + i) * 8 + (l >> 3);           // row within tile
    const int slot = (l & 7) ^ ((row >> 1) & 7);           // logical 16-B slot this lane fetches
    int ra = min(m0 + row, p.M - 1);                       // clamp: rows past the edge are never stored
    int rw = min(row, wrows - 1);
    voffA[i] = (unsigned)(((MODE == 0 ? p.am.off(ra) : p.cv.off(ra)) - a0 + slot * 8) * 2);
    voffW[i] = (unsigned)(((long long)rw * p.K + slot * 8) * 2);
  }

  const int cchunks = MODE == 1 ? p.cv.Cin / BK : 1;
  auto stage = [&](int buf, int kt) {
    const int soff = kt * (BK * 2);
    int soffA = soff;
    if (MODE == 1) {
      const int tap = kt / cchunks, cc = kt - tap * cchunks;
      const int r = tap / 3, sx = tap - r * 3;
      soffA = ((r * p.cv.Wp + sx) * p.cv.Cin + cc * BK) * 2;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      DRAG_LDS char* dA = (DRAG_LDS char*)smem + buf * TILE_BYTES + (w * 4 + i) * 1024;
      DRAG_LDS char* dB = (DRAG_LDS char*)smem + (2 + buf) * TILE_BYTES + (w * 4 + i) * 1024;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (DRAG_LDS void*)dA, 16, voffA[i], soffA, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (DRAG_LDS void*)dB, 16, voffW[i], soff, 0, 0);
    }
  };

  // ---- fragment read addresses (bytes within a tile) ----
  const int p0 = (l >> 4) ^ ((l & 15) >> 1);
  const int fa = (wr * 64 + (l & 15)) * 128;   // + mi*2048, slot (p0 ^ 4ks)*16
  const int fb = (wc * 64 + (l & 15)) * 128;

  f32x4_t acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int nk = p.K / BK;
  stage(0, 0);
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < nk) stage(buf ^ 1, kt + 1);
    const char* sA = smem + buf * TILE_BYTES;
    const char* sB = smem + (2 + buf) * TILE_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int so = ((p0 ^ (ks * 4)) << 4);
      bf16x8_t xa[4], wb[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        xa[i] = *(const bf16x8_t*)(sA + fa + i * 2048 + so);
        wb[i] = *(const bf16x8_t*)(sB + fb + i * 2048 + so);
      }
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[ni], xa[mi], acc[mi][ni], 0, 0, 0);
    }
  }

  // ---- epilogue: lane holds C[m = .. + (l&15)][n = .. + (l>>4)*4 + 0..3] ----
  const GemmKArgs pd = dest_of(p, n0);
  if (p.wide) staged_epilogue<4, BM>(pd, m0, m0 + wr * 64, n0, n0 + wc * 64, l, acc, smem + 4 * TILE_BYTES + w * 2048);
  else wave_epilogue<4, BM>(pd, m0, m0 + wr * 64 + (l & 15), n0, n0 + wc * 64 + (l >> 4) * 4, acc);
}

template __global__ void gemm_bf16_t128<0>(GemmKArgs);
template __global__ void gemm_bf16_t128<1>(GemmKArgs);

}  // namespace drag_gemm
