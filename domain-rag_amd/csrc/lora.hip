// lora.hip — drag_lora_merge_bf16: w[n,k] = bf16( f32(w0[n,k]) + sum_{r<R} scale[r] * up[n,r] * down[r,k] ), in place or out of place.
//
// The pass that folds LoRA adapters into the resident bf16 weights of the Flux DiT (domain-rag_amd/lora.py states the rule on the host,
// include/domainrag_hip.h the contract).  HBM-bound: w0 is read once and w written once, 16 bytes per lane; up, down and scale are small
// and come from L2.
//
// Tiling: a workgroup of 4 waves owns 128 rows (n) x 128 columns (k) of W; a wave owns 32 rows of it.  The product is computed TRANSPOSED,
// D'[k][n] = sum_r down[r][k] * (scale[r] up[n][r]), on v_mfma_f32_16x16x32_bf16 (A = down^T, B = scaled up^T), so that a lane's
// accumulator registers are consecutive k of ONE row n: the C/D map of the instruction puts column n = lane & 15 on the lane and rows
// 4 (lane >> 4) + reg in its four registers.  Which k a row of A stands for is free, so a 32 k x 16 n subtile is two MFMAs whose row
// m = 4 a + b means k = 8 a + b (first) and k = 8 a + 4 + b (second): lane (a, n) then holds k = 8 a ... 8 a + 7 of row n, one 16-byte
// piece of W.
//
// down arrives [R, K], r-major, but the A operand wants 8 consecutive r of one k per lane.  A chunk of 32 ranks x 128 k is staged in LDS
// as it lies in memory (rows of r, 16-byte pieces) and read with ds_read_b64_tr_b16: within a 16-lane group, source lane 4 q + p gives
// the address of 4 consecutive k of rank row q, and result lane 4 p + e receives that k-column e of the four rows (the map
// attention_d128.h uses for V).  Two reads (rank rows 8 g ... + 3 and + 4 ... + 7) make one operand; the source address of lane (q, p) is
// k = 8 p + 4 u of the subtile for MFMA u, which is exactly the row permutation above.  LDS rows are 320 bytes (256 + 64): the 16
// source pieces of a group (4 rows x 4 p, 16-byte pitch) fall into 16 different 16-byte slots of a bank row.
//
// The per-rank scale is float32 and must not cost a rounding: scale[r] * up[n][r] is formed in float32 and fed to the matrix core as
// the sum of two bf16 values (hi = bf16(x), lo = bf16(x - hi)), two MFMAs per step, which keeps 16 mantissa bits of every scaled factor;
// down enters exactly, products and sums are float32 in the accumulator, and the one rounding to bf16 is the final store.
//
// Rank padding and edges: ranks >= R are ZERO on both sides (LDS rows of down are zero-filled, up elements are never read there), so
// whatever a padded up row holds — NaN included — never reaches a product.  Rows >= N and columns >= K are neither read nor written.
// Every lane runs every LDS read (the transposed read needs the whole wave): edges are handled by zero operands and guarded
// global accesses only.
#include "drag_common.h"

namespace drag_lora {

constexpr int NT = 128;                 // rows of W per workgroup (32 per wave)
constexpr int KT = 128;                 // columns of W per workgroup
constexpr int RC = 32;                  // ranks per staging chunk = the depth of one MFMA
constexpr int ROWB = KT * 2 + 64;       // bytes per LDS row of the down chunk

typedef short s16x4_t __attribute__((ext_vector_type(4)));
typedef short s16x8_t __attribute__((ext_vector_type(8)));

struct Args {
  const bf16_t* w0;
  bf16_t* w;
  const bf16_t* up;
  const bf16_t* down;
  const float* scale;
  long long ldw0, ldw;
  int N, K, R, ldup, lddown, ktiles;
};

__global__ __launch_bounds__(256) void lora_merge_kernel(Args p) {
  __shared__ __attribute__((aligned(16))) char dn[RC * ROWB];
  __shared__ __attribute__((aligned(16))) float sc[RC];
  const int tid = (int)threadIdx.x, l = tid & 63, wv = tid >> 6;
  const int g = l >> 4, c = l & 15;
  const int tile = (int)blockIdx.x;
  const int k0 = (tile % p.ktiles) * KT;
  const int n0 = (tile / p.ktiles) * NT + wv * 32;

  // this lane's pieces of W0: row n0 + 16 i + c, columns k0 + 32 s + 8 g ... + 7; loaded first, consumed last
  u32x4_t wreg[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int n = n0 + 16 * i + c, k = k0 + 32 * s + 8 * g;
      wreg[i][s] = u32x4_t{0u, 0u, 0u, 0u};
      if (n < p.N && k < p.K) wreg[i][s] = *(const u32x4_t*)(p.w0 + (long long)n * p.ldw0 + k);
    }

  f32x4_t acc[2][4][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int u = 0; u < 2; ++u) acc[i][s][u] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // transposed-read source address of this lane inside the chunk: rank row 8 g + q, k = 8 p of a subtile (q = c >> 2, p = c & 3)
  const int tr_off = (8 * g + (c >> 2)) * ROWB + (c & 3) * 16;

  for (int r0 = 0; r0 < p.R; r0 += RC) {
    __syncthreads();                                        // the previous chunk's reads are done
    // stage down[r0 ... r0 + 31][k0 ... k0 + 127]: 512 pieces of 16 bytes, two per thread; zero beyond R and beyond K
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int id = tid + 256 * j, rr = id >> 4, kp = (id & 15) * 8;
      u32x4_t v = {0u, 0u, 0u, 0u};
      if (r0 + rr < p.R && k0 + kp < p.K) v = *(const u32x4_t*)(p.down + (long long)(r0 + rr) * p.lddown + k0 + kp);
      *(u32x4_t*)(dn + rr * ROWB + kp * 2) = v;
    }
    if (tid < RC) sc[tid] = r0 + tid < p.R ? p.scale[r0 + tid] : 0.f;
    __syncthreads();

    // B operand: scale[r] * up[n][r] for r = r0 + 8 g ... + 7 of row n0 + 16 i + c, split hi + lo
    float s8[8];
    *(f32x4_t*)&s8[0] = *(const f32x4_t*)&sc[8 * g];
    *(f32x4_t*)&s8[4] = *(const f32x4_t*)&sc[8 * g + 4];
    bf16x8_t bhi[2], blo[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int n = n0 + 16 * i + c, r = r0 + 8 * g;
      s16x8_t raw = {0, 0, 0, 0, 0, 0, 0, 0};
      if (n < p.N) {
        const bf16_t* src = p.up + (long long)n * p.ldup + r;
        if (r + 8 <= p.R) {
          raw = *(const s16x8_t*)src;
        } else {                                            // the piece that straddles R: element by element, nothing past R is read
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (r + j < p.R) raw[j] = (short)src[j];
        }
      }
      s16x8_t hi, lo;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float x = s8[j] * bf2f((bf16_t)raw[j]);
        const bf16_t h = f2bf(x);
        hi[j] = (short)h;
        lo[j] = (short)f2bf(x - bf2f(h));
      }
      bhi[i] = __builtin_bit_cast(bf16x8_t, hi);
      blo[i] = __builtin_bit_cast(bf16x8_t, lo);
    }

#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        DRAG_LDS char* a = (DRAG_LDS char*)dn + (tr_off + s * 64 + u * 8);
        const s16x4_t a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((DRAG_LDS s16x4_t*)a);
        const s16x4_t a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((DRAG_LDS s16x4_t*)(a + 4 * ROWB));
        const bf16x8_t af = __builtin_bit_cast(bf16x8_t, (s16x8_t)__builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          acc[i][s][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bhi[i], acc[i][s][u], 0, 0, 0);
          acc[i][s][u] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, blo[i], acc[i][s][u], 0, 0, 0);
        }
      }
  }

  // w = bf16(w0 + delta): registers 0..3 of MFMA u are k = 8 g + 4 u ... + 3 of this lane's row
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int n = n0 + 16 * i + c, k = k0 + 32 * s + 8 * g;
      if (n >= p.N || k >= p.K) continue;
      const u32x4_t v = wreg[i][s];
      u32x4_t o;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        const f32x4_t d = acc[i][s][h >> 1];
        const float lo = __uint_as_float(v[h] << 16) + d[2 * (h & 1)];
        const float hi = __uint_as_float(v[h] & 0xffff0000u) + d[2 * (h & 1) + 1];
        o[h] = pack2bf(lo, hi);
      }
      *(u32x4_t*)(p.w + (long long)n * p.ldw + k) = o;
    }
}

}  // namespace drag_lora

extern "C" int drag_lora_merge_bf16(const void* w0, int64_t ldw0, void* w, int64_t ldw, int32_t N, int32_t K, const void* up, int32_t ldup,
                                    const void* down, int32_t lddown, const float* scale, int32_t R, void* stream) {
  DRAG_CHECK(w0 && w && up && down && scale, "drag_lora_merge_bf16: null pointer");
  DRAG_CHECK(N >= 1 && R >= 1, "drag_lora_merge_bf16: N >= 1 and R >= 1 required");
  DRAG_CHECK(N <= 0x7fffff00 && R <= 0x7fffff00, "drag_lora_merge_bf16: N and R must leave room for a tile below 2^31");
  DRAG_CHECK(K >= 8 && K % 8 == 0, "drag_lora_merge_bf16: K a positive multiple of 8 required");
  DRAG_CHECK(ldw >= K && ldw0 >= K && lddown >= K && ldw % 8 == 0 && ldw0 % 8 == 0 && lddown % 8 == 0,
             "drag_lora_merge_bf16: ldw, ldw0 and lddown must be >= K and multiples of 8");
  DRAG_CHECK(ldup >= R && ldup % 8 == 0, "drag_lora_merge_bf16: ldup must be >= R and a multiple of 8");
  DRAG_CHECK((((uintptr_t)w0 | (uintptr_t)w | (uintptr_t)up | (uintptr_t)down) & 15) == 0,
             "drag_lora_merge_bf16: w0, w, up and down must be 16-byte aligned");
  DRAG_CHECK(((uintptr_t)scale & 3) == 0, "drag_lora_merge_bf16: scale must be 4-byte aligned");
  drag_lora::Args p;
  p.w0 = (const bf16_t*)w0; p.w = (bf16_t*)w; p.up = (const bf16_t*)up; p.down = (const bf16_t*)down; p.scale = scale;
  p.ldw0 = ldw0; p.ldw = ldw; p.N = N; p.K = K; p.R = R; p.ldup = ldup; p.lddown = lddown;
  p.ktiles = (K + drag_lora::KT - 1) / drag_lora::KT;
  const long long blocks = (long long)p.ktiles * ((N + drag_lora::NT - 1) / drag_lora::NT);
  DRAG_CHECK(blocks < (1ll << 31), "drag_lora_merge_bf16: too many tiles for one launch");
  hipLaunchKernelGGL(drag_lora::lora_merge_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p);
  DRAG_LAUNCH_CHECK();
  return 0;
}
