// attention_mxfp8.hip — drag_attention_mxfp8: flash attention over the MXFP8 images of drag_qkv_prep_mxfp8 (head_dim 128), the kernel and
// its host side.  attention_mxfp8.h describes the structure and the operand map; compiled HIP with builtins throughout.
#include "attention_mxfp8.h"
#include "gemm_mxfp8.h"

namespace drag_attn {

using drag_gemm::i32x8_t;

__device__ __forceinline__ i32x8_t mx_frag(const u32x4_t a, const u32x4_t b) {
  return (i32x8_t){(int)a[0], (int)a[1], (int)a[2], (int)a[3], (int)b[0], (int)b[1], (int)b[2], (int)b[3]};
}

template <int NQ, int NW>       // NW waves, each NQ blocks of 16 queries
__global__ __launch_bounds__(NW * 64, NW == 8 ? 1 : 2) void attention_mxfp8_kernel(MxAttnArgs p) {
  constexpr int CH = 1024 / (NW * 64);                    // 16-byte chunks of a tile per thread
  __shared__ __attribute__((aligned(16))) char smem[4 * MX_TILE_BYTES];     // K0 K1 V0 V1
  const int w = wave_id(), l = lane_id(), t = (int)threadIdx.x;
  const int c16 = l & 15, g = l >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const long long bh = (long long)b * p.H + h;
  const int sp = p.s_pad;
  const uint8_t* kq = p.kq + bh * sp * 128;
  const uint8_t* ks = p.ks + bh * sp * 4;
  const uint8_t* vq = p.vq + bh * 128 * sp;
  const uint8_t* vs = p.vs + bh * 128 * (sp >> 5);
  const int q0 = ((int)blockIdx.x * NW + w) * 16 * NQ;

  // ---- Q fragments and scales: lane (c16, g) supplies bytes 16 g .. and 64 + 16 g .. of query row q0 + 16 n + c16, and scale byte g ----
  i32x8_t qf[NQ];
  int qsc[NQ];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    const int row = min(q0 + 16 * n + c16, sp - 1);        // (rows S .. s_pad - 1 are the zero padding; nothing of them is stored)
    const uint8_t* qp = p.qq + (bh * sp + row) * 128 + 16 * g;
    qf[n] = mx_frag(*(const u32x4_t*)qp, *(const u32x4_t*)(qp + 64));
    qsc[n] = (int)p.qs[(bh * sp + row) * 4 + g];
  }

  // ---- staging: thread t moves the 16-byte chunks {t, t + threads, ...} of each 128-row x 128-byte tile ----
  // K row n of the tile goes to LDS row rho(n) = 16 (4 (n >> 6) + ((n >> 2) & 3)) + 4 ((n >> 4) & 3) + (n & 3): score block tt reads rows
  // 16 tt .. 16 tt + 15 and finds the keys kappa(tt, i) of attention_mxfp8.h there.  V^T rows (d) stay in order.
  // (global offsets are unsigned and the bases uniform: the loads address as scalar base + 32-bit lane offset)
  unsigned gk[CH], gv[CH];
  int lk[CH], lv[CH];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = i * (NW * 64) + t;
    const int row = c >> 3, slot = c & 7;
    const int rho = 16 * (4 * (row >> 6) + ((row >> 2) & 3)) + 4 * ((row >> 4) & 3) + (row & 3);
    gk[i] = (unsigned)(row * 128 + slot * 16);
    gv[i] = (unsigned)(row * sp + slot * 16);
    lk[i] = rho * 128 + ((slot ^ ((rho >> 1) & 7)) << 4);
    lv[i] = row * 128 + ((slot ^ ((row >> 1) & 7)) << 4);
  }
  // ---- fragments: lane reads row 16 i + c16 of a tile, logical 16-byte slots g and 4 + g ----
  const int sw = (c16 >> 1) & 7;
  const int f0 = c16 * 128 + ((g ^ sw) << 4), f1 = c16 * 128 + (((4 + g) ^ sw) << 4);     // + i * 2048
  // the scale bytes of the lane's rows: k row kappa(tt, c16) of the tile = a constant per tt past kso; V^T row 16 dt + c16 = dt uniform
  // steps of 16 rows past vso
  const unsigned kso = (unsigned)((16 * (c16 >> 2) + (c16 & 3)) * 4 + g);                // + tile * 512 + (64 (tt >> 2) + 4 (tt & 3)) * 4
  const unsigned vso = (unsigned)(c16 * (sp >> 5) + g);                                  // + tile * 4 + dt * 16 * (sp >> 5)
  const unsigned vstep = (unsigned)(16 * (sp >> 5));

  f32x4_t o[NQ][8];
  float mrow[NQ], lrow[NQ];
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    mrow[n] = -INFINITY;
    lrow[n] = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) o[n][i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }

  u32x4_t rk[CH], rv[CH];
  int ksc[8];
  auto load = [&](int T) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      rk[i] = *(const u32x4_t*)(kq + (size_t)T * MX_TILE_BYTES + gk[i]);
      rv[i] = *(const u32x4_t*)(vq + (size_t)T * MX_KV + gv[i]);
    }
  };
  auto load_kscales = [&](int T) {
#pragma unroll
    for (int i = 0; i < 8; ++i) ksc[i] = (int)(ks + (size_t)T * (MX_KV * 4) + (64 * (i >> 2) + 4 * (i & 3)) * 4)[kso];
  };

  const int nT = sp / MX_KV;
  load(0);
  load_kscales(0);
  for (int T = 0; T < nT; ++T) {
    char* sK = smem + (T & 1) * MX_TILE_BYTES;
    char* sV = smem + (2 + (T & 1)) * MX_TILE_BYTES;
    // (this buffer was last read in tile T - 2; every wave has passed tile T - 1's barrier since)
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      *(u32x4_t*)(sK + lk[i]) = rk[i];
      *(u32x4_t*)(sV + lv[i]) = rv[i];
    }
    __syncthreads();
    if (T + 1 < nT) load(T + 1);
    int vsc[8];                                            // this tile's V^T scales: first used after the softmax
#pragma unroll
    for (int i = 0; i < 8; ++i) vsc[i] = (int)(vs + (size_t)T * 4 + (size_t)i * vstep)[vso];

    // ---- per block of 16 queries: S^T = K Q^T, one MFMA per 16 keys x 16 queries, then the online softmax of the lane's query column;
    // the rounded p are the second product's b operand.  (NQ = 2 with 4 waves spilled 272 bytes per lane to scratch when this was written; the 8-wave
    // form with one query block per wave needs 180 registers and none.) ----
    const bool tail = (T + 1) * MX_KV > p.S;               // the last tile holds padded keys: masked to -inf
    i32x8_t pf[NQ];
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
      __builtin_amdgcn_sched_barrier(0);                   // (keeps the next block's fragment reads from rising above this point: registers)
      f32x4_t s[8];
#pragma unroll
      for (int tt = 0; tt < 8; ++tt) {
        const i32x8_t kf = mx_frag(*(const u32x4_t*)(sK + tt * 2048 + f0), *(const u32x4_t*)(sK + tt * 2048 + f1));
        s[tt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(kf, qf[n], (f32x4_t){0.f, 0.f, 0.f, 0.f}, 0, 0, 0, ksc[tt], 0, qsc[n]);
      }
      if (n == NQ - 1 && T + 1 < nT) load_kscales(T + 1);  // (this tile's are dead; the loads fly under the softmax and the second product)
      if (tail) {
#pragma unroll
        for (int tt = 0; tt < 8; ++tt)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (T * MX_KV + 64 * (tt >> 2) + 16 * g + 4 * (tt & 3) + r >= p.S) s[tt][r] = -INFINITY;
      }
      // the row maximum of the raw products: the scale is positive (checked on the host), so max(s c) = c max(s)
      float mx = -INFINITY;
#pragma unroll
      for (int tt = 0; tt < 8; ++tt)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[tt][r]);
      mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      // (every tile's first key is < S and scores are finite: mnew is finite, so no inf - inf below)
      const float mnew = fmaxf(mrow[n], mx * p.c);
      const float alpha = __builtin_amdgcn_exp2f(mrow[n] - mnew);
      mrow[n] = mnew;
      const float off = 8.0f - mnew;                       // p * 2^8 straight from the exponent: the row sum carries the same exact factor
      float sum = 0.f;
#pragma unroll
      for (int tt = 0; tt < 8; ++tt) {
        float e[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          e[r] = __builtin_amdgcn_exp2f(fmaf(s[tt][r], p.c, off));
          sum += e[r];
        }
        // e4m3(p * 2^8), round to nearest even, four keys to a register in key order
        int pk = __builtin_amdgcn_cvt_pk_fp8_f32(e[0], e[1], 0, false);
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(e[2], e[3], pk, true);
        pf[n][tt] = pk;
      }
      lrow[n] = lrow[n] * alpha + sum;
#pragma unroll
      for (int i = 0; i < 8; ++i) o[n][i] *= alpha;
    }

    __builtin_amdgcn_sched_barrier(0);
    // ---- O^T += V^T P^T: one MFMA per 16 d x 16 queries x 128 keys; P under the constant scale byte 119 = 2^-8 ----
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) {
      const i32x8_t vf = mx_frag(*(const u32x4_t*)(sV + dt * 2048 + f0), *(const u32x4_t*)(sV + dt * 2048 + f1));
#pragma unroll
      for (int n = 0; n < NQ; ++n)
        o[n][dt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(vf, pf[n], o[n][dt], 0, 0, 0, vsc[dt], 0, 119);
    }
  }

  // ---- epilogue: lane holds O^T[d = 16 dt + 4 g + r][query c16]: 8 bytes per store ----
#pragma unroll
  for (int n = 0; n < NQ; ++n) {
    float lt = lrow[n];
    lt += __shfl_xor(lt, 16, 64);
    lt += __shfl_xor(lt, 32, 64);
    const float inv = 256.0f / lt;                         // lt = 2^8 * the sum of p; the accumulators hold the sum of p v
    const int row = q0 + 16 * n + c16;
    if (row < p.S) {
      bf16_t* op = p.out + (long long)b * p.o_bs + (long long)row * p.ld_o + h * 128 + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 8; ++dt) {
        u32x2_t v;
        v[0] = pack2bf(o[n][dt][0] * inv, o[n][dt][1] * inv);
        v[1] = pack2bf(o[n][dt][2] * inv, o[n][dt][3] * inv);
        *(u32x2_t*)(op + 16 * dt) = v;
      }
    }
  }
}


}  // namespace drag_attn

using namespace drag_attn;

constexpr int MX_NQ = 1, MX_NW = 8;  // 8 waves x one block of 16 queries = 128 queries per workgroup

extern "C" int drag_attention_mxfp8_s_pad(int32_t S) { return S > 0 && S <= (1 << 23) ? mx_s_pad(S) : 0; }

extern "C" int drag_attention_mxfp8_supported(int32_t B, int32_t S, int32_t H) { return mx_shape_ok(B, S, H) ? 1 : 0; }

extern "C" const char* drag_attention_mxfp8_kernel_name(int32_t S) {
  (void)S;                           // one kernel so far
  return "attention_mxfp8_kernel<1, 8>";
}

extern "C" int drag_attention_mxfp8(const void* qq, const void* qs, const void* kq, const void* ks, const void* vq, const void* vs, void* out,
                                    int32_t B, int32_t S, int32_t H, int32_t ld_o, int64_t o_batch_stride, float scale, void* stream) {
  DRAG_CHECK(qq && qs && kq && ks && vq && vs && out, "drag_attention_mxfp8: null pointer");
  DRAG_CHECK(mx_shape_ok(B, S, H), "drag_attention_mxfp8: unsupported shape (B, H in 1 .. 65535, S in 1 .. 2^23)");
  DRAG_CHECK(scale > 0.f, "drag_attention_mxfp8: a positive softmax scale is required");
  DRAG_CHECK(ld_o % 4 == 0 && ld_o >= H * 128, "drag_attention_mxfp8: ld_o %% 4 == 0 and ld_o >= H * 128 required");
  DRAG_CHECK(((uintptr_t)out & 7) == 0 && o_batch_stride % 4 == 0 && o_batch_stride >= 0, "drag_attention_mxfp8: out must be 8-byte aligned, o_batch_stride %% 4 == 0 and >= 0");
  DRAG_CHECK((((uintptr_t)qq | (uintptr_t)kq | (uintptr_t)vq) & 15) == 0 && (((uintptr_t)qs | (uintptr_t)ks | (uintptr_t)vs) & 3) == 0,
             "drag_attention_mxfp8: element images must be 16-byte and scale images 4-byte aligned");
  MxAttnArgs p;
  p.qq = (const uint8_t*)qq; p.qs = (const uint8_t*)qs; p.kq = (const uint8_t*)kq; p.ks = (const uint8_t*)ks;
  p.vq = (const uint8_t*)vq; p.vs = (const uint8_t*)vs; p.out = (bf16_t*)out;
  p.B = B; p.S = S; p.H = H; p.s_pad = mx_s_pad(S); p.ld_o = ld_o; p.o_bs = o_batch_stride;
  p.c = scale * 1.4426950408889634f;
  const int QB = 16 * MX_NQ * MX_NW;
  hipLaunchKernelGGL((attention_mxfp8_kernel<MX_NQ, MX_NW>), dim3((S + QB - 1) / QB, H, B), dim3(MX_NW * 64), 0, (hipStream_t)stream, p);
  DRAG_LAUNCH_CHECK();
  return 0;
}
