// attention_kernels.h — the attention kernels of Flux joint attention on gfx950: q/k RMSNorm + RoPE + V^T repack, then a
// flash-style MFMA attention (head_dim 128, bf16, no mask).
//
// Replaces FluxAttnProcessor2_0 (diffusers 0.33.1, un-vendored): norm_q/norm_k(/norm_added_*),
// apply_rotary_emb and F.scaled_dot_product_attention, reached on every denoise step from
// batch_generate_flux_kshot.py:467-474 and outpainting_updown_sampling_redux.py:1246-1257.
//
// Attention structure: block = 8 waves x 32 queries (4 waves for short sequences); KV tile = 64 keys; K tile [64][128] and
// V^T tile [128][64] arrive by LDS-DMA (buffer_load ... lds), double-buffered, one barrier per
// tile, XOR-swizzled on the source address + on the ds_read_b128.  QK^T is computed swapped
// (S^T = K Q^T, v_mfma_f32_32x32x16_bf16) so each lane owns ONE query column: the online
// softmax is lane-local apart from one lane<->lane^32 exchange, and the packed P registers are
// directly the B operand of O^T += V^T P^T.  The V^T image is stored with keys permuted inside
// groups of 16 so that a plain 16-byte read yields exactly the keys a lane's P registers hold
// (no transposes, no cross-lane traffic in the loop).
//
// This header is what the attention kernels share: the launch arguments, the tile constants and the declarations of every kernel
// instantiation the library builds.  Each kernel is compiled from its own source(s): attention_prep.hip; attention_d128.h instantiated in
// attention_d128_w8.hip / _w4.hip; attention_q64.hip; attention_q64g.hip (the only source that includes the generated attn_q64_tile.h).
// attention.hip is the host side (kernel policy, launch, the C ABI) and reaches the kernels through the declarations at the end.
// The library is linked without relocatable device code: nothing here may be a device-side global.
#pragma once
#include "drag_common.h"
// The asm statements that write m0 (one s_add_u32 m0 per LDS-DMA piece) list "m0" as a clobber: hipcc then re-materialises m0 before its own
// next LDS-DMA builtin (checked on a two-builtin probe: without the clobber the second builtin ran on the asm's stale m0).  clang warns that m0
// is a reserved register on every such statement; the clobber is what is wanted here.
#pragma clang diagnostic ignored "-Winline-asm"
#include <stdlib.h>
#include <type_traits>

namespace drag_attn {

struct PrepArgs {
  bf16_t* qkv;
  bf16_t* vt;
  const bf16_t *wq_txt, *wk_txt, *wq_img, *wk_img;
  const float *cosT, *sinT;
  int B, S, H, ld, s_txt, s_pad;
  float eps;
  int skip_q;      // q is normalised / rotated by the attention kernel as it loads its Q fragments (drag_attention_qprep_bf16)
};

struct AttnArgs {
  const bf16_t *q, *k, *vt;
  const bf16_t* v;            // VROW kernels: V as the Linear wrote it (rows of ld_qk elements, like k); vt is then unused
  bf16_t* out;
  int B, S, H, ld_qk, ld_o, s_pad;
  long long qk_bs, o_bs;
  float c;  // scale * log2(e)
  unsigned k_bytes, vt_bytes;          // span of ONE (batch, head) in the K tensor / the V^T tensor (attention_q64_kernel's descriptors)
  unsigned k_bytes_all, vt_bytes_all;  // span of the whole K tensor (all batches, all heads) / the whole V^T tensor (attention_d128_kernel)
  // optional Q preparation fused into the fragment load (all null / 0 = q is used as stored):
  const bf16_t *wq_txt, *wq_img;   // RMSNorm weights [128] of the text / image stream (rows < s_txt are text)
  const float *cosT, *sinT;        // RoPE tables [S, 64]
  int s_txt;
  float eps;
  int tune;       // measurement bits: 1 = static priority for the younger wave half, 2 = 16-byte epilogue stores
  int items;      // attention_q64_kernel: (batch-head, query block) items in all = the one-item grid; a smaller grid walks them (persistent)
};
constexpr float DEFER_THR = 8.0f;     // log2 units; 0 = rescale on every increase (classic online softmax)
constexpr int KT_BYTES = 64 * 256;   // K tile   [64 keys][128 d] bf16
constexpr int VT_BYTES = 128 * 128;  // V^T tile [128 d][64 keys] bf16

// ---- device code the two prep passes share (qk_norm_rope_vt_kernel and qkv_prep_mxfp8_kernel) ----
// Per-head RMSNorm(128) + interleaved RoPE of one q (which = 0) or k (which = 1) row, 16 lanes per row: lane sub of the sixteen holds the raw
// elements d = 8 sub + 0..7 and gets their prepared bf16 pairs back.  sc = the row (clamped to S - 1).  Every lane of the sixteen must call it.
__device__ __forceinline__ u32x4_t qk_norm_rope8(const PrepArgs& p, const int which, const int sc, const int sub, const u32x4_t raw,
                                                 const bool do_norm, const bool do_rope) {
  float x[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    x[2 * j] = bf2f((bf16_t)(raw[j] & 0xffff));
    x[2 * j + 1] = bf2f((bf16_t)(raw[j] >> 16));
  }
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) ss += x[j] * x[j];
  ss += __shfl_xor(ss, 8, 64);
  ss += __shfl_xor(ss, 4, 64);
  ss += __shfl_xor(ss, 2, 64);
  ss += __shfl_xor(ss, 1, 64);
  const float rs = rsqrtf(ss * (1.0f / 128.0f) + p.eps);
  u32x4_t wr = (u32x4_t){0u, 0u, 0u, 0u};
  if (do_norm) {
    const bf16_t* wsel = which == 0 ? (sc < p.s_txt ? p.wq_txt : p.wq_img) : (sc < p.s_txt ? p.wk_txt : p.wk_img);
    wr = *(const u32x4_t*)(wsel + sub * 8);
  }
  f32x4_t c4 = (f32x4_t){1.f, 1.f, 1.f, 1.f}, s4 = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  if (do_rope) {
    c4 = *(const f32x4_t*)(p.cosT + (long long)sc * 64 + sub * 4);
    s4 = *(const f32x4_t*)(p.sinT + (long long)sc * 64 + sub * 4);
  }
  u32x4_t o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    // diffusers RMSNorm: (x * rsqrt(var+eps)).to(bf16) * weight(bf16) -> bf16
    float a0 = x[2 * j], a1 = x[2 * j + 1];
    if (do_norm) {
      a0 = rbf(rbf(a0 * rs) * bf2f((bf16_t)(wr[j] & 0xffff)));
      a1 = rbf(rbf(a1 * rs) * bf2f((bf16_t)(wr[j] >> 16)));
    }
    // apply_rotary_emb (use_real, unbind_dim=-1): out = x*cos + rot(x)*sin in fp32
    const float r0 = a0 * c4[j] - a1 * s4[j];
    const float r1 = a1 * c4[j] + a0 * s4[j];
    o[j] = pack2bf(r0, r1);
  }
  return o;
}

// ---- device code the three attention kernels share ----
// Per-head RMSNorm(128) + interleaved RoPE of one query row's share of a lane — raw[ks] = the row's elements d = 16 ks + 8 hh + 0..7, lane ^ 32
// holds the other 64; RoPE pairs (2j, 2j+1) never straddle lanes — with the rounding points of the separate pass (qk_norm_rope_vt_kernel):
// rbf(rbf(x * rs) * w), rotation in fp32, one rounding to bf16.  qr = the row (clamped to S - 1), hh = the lane's half-wave.
// store(ks, j, word) takes the packed pair j of piece ks: every kernel keeps its fragments in another register layout.
// FOLD: scale * log2(e) inside the rotation's one rounding (attention_q64g_kernel).
// The weight and table rows are loaded before anything is consumed: one memory latency (a per-ks `if (table != null)` form compiled to
// eight serialised load-wait-branch rounds: +91 us per B=8 launch).
template <bool FOLD, class Store>
__device__ __forceinline__ void q_norm_rope(const AttnArgs& p, const u32x4_t (&raw)[8], const int qr, const int hh, Store&& store) {
  const bf16_t* wsel = (qr < p.s_txt ? p.wq_txt : p.wq_img) + hh * 8;
  const float* cp = p.cosT + (long long)qr * 64 + hh * 4;
  const float* sp = p.sinT + (long long)qr * 64 + hh * 4;
  u32x4_t wr[8];
  f32x4_t c4[8], s4[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks) {
    wr[ks] = *(const u32x4_t*)(wsel + ks * 16);
    c4[ks] = *(const f32x4_t*)(cp + ks * 8);
    s4[ks] = *(const f32x4_t*)(sp + ks * 8);
  }
  float ss = 0.f;
#pragma unroll
  for (int ks = 0; ks < 8; ++ks)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a0 = bf2f((bf16_t)(raw[ks][j] & 0xffff)), a1 = bf2f((bf16_t)(raw[ks][j] >> 16));
      ss += a0 * a0;
      ss += a1 * a1;
    }
  ss += __shfl_xor(ss, 32, 64);
  const float rs = rsqrtf(ss * (1.0f / 128.0f) + p.eps);
#pragma unroll
  for (int ks = 0; ks < 8; ++ks)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a0 = rbf(rbf(bf2f((bf16_t)(raw[ks][j] & 0xffff)) * rs) * bf2f((bf16_t)(wr[ks][j] & 0xffff)));
      const float a1 = rbf(rbf(bf2f((bf16_t)(raw[ks][j] >> 16)) * rs) * bf2f((bf16_t)(wr[ks][j] >> 16)));
      float r0 = a0 * c4[ks][j] - a1 * s4[ks][j], r1 = a1 * c4[ks][j] + a0 * s4[ks][j];
      if constexpr (FOLD) { r0 *= p.c; r1 *= p.c; }        // scale * log2(e) inside the rotation's one rounding
      store(ks, j, pack2bf(r0, r1));
    }
}

// One query row's 128 outputs, normalised: lane ll (hh = ll >> 5) holds O[query][d = 32dt + 8(r>>2) + 4hh + (r&3)] as oa(dt, r), lane ll ^ 32 the
// other half.  (ll, not hh, is the parameter: with hh passed in, hipcc's address arithmetic in attention_q64g_kernel came out six instructions different.)
template <class Acc>
__device__ __forceinline__ void store_out_row(const AttnArgs& p, const int b, const int h, const int qrow, const int ll, const float inv, Acc&& oa) {
  if (p.tune & 2) {
    // T21: lanes l and l + 32 hold the two 8-byte halves of each 16-byte output chunk.  One v_permlane32_swap per dword
    // regroups a pair of chunks (g, g + 1) so that the lower half-wave stores chunk g and the upper one chunk g + 1 as
    // whole 16-byte pieces: 8 store instructions per lane instead of 16 (the tail is store-ISSUE bound).
    bf16_t* op = p.out + (long long)b * p.o_bs + (long long)qrow * p.ld_o + h * 128 + 8 * (ll >> 5);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int g = 0; g < 4; g += 2) {
        uint32_t a0 = pack2bf(oa(dt, 4 * g) * inv, oa(dt, 4 * g + 1) * inv);
        uint32_t a1 = pack2bf(oa(dt, 4 * g + 2) * inv, oa(dt, 4 * g + 3) * inv);
        uint32_t b0 = pack2bf(oa(dt, 4 * g + 4) * inv, oa(dt, 4 * g + 5) * inv);
        uint32_t b1 = pack2bf(oa(dt, 4 * g + 6) * inv, oa(dt, 4 * g + 7) * inv);
        const auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
        const auto r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
        // lower lanes: (r[0], r[1]) = (own chunk-g half, upper lane's chunk-g half); upper lanes: (lower's chunk g+1 half, own)
        const u32x4_t o = {r0[0], r1[0], r0[1], r1[1]};
        if (qrow < p.S) *(u32x4_t*)(op + 32 * dt + 8 * g) = o;
      }
  } else if (qrow < p.S) {
    bf16_t* op = p.out + (long long)b * p.o_bs + (long long)qrow * p.ld_o + h * 128 + 4 * (ll >> 5);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        u32x2_t o;
        o[0] = pack2bf(oa(dt, 4 * g) * inv, oa(dt, 4 * g + 1) * inv);
        o[1] = pack2bf(oa(dt, 4 * g + 2) * inv, oa(dt, 4 * g + 3) * inv);
        *(u32x2_t*)(op + 32 * dt + 8 * g) = o;
      }
  }
}

// ---- the kernels: one definition each, in the source named; every other object reaches them through these declarations ----
__global__ __launch_bounds__(256) void qk_norm_rope_vt_kernel(PrepArgs p);                    // attention_prep.hip

template <int NW, int SCHED, bool QPREP, bool PMAX, bool VROW = false, bool PERSIST = false>   // NW: waves per block (4 or 8), 32 queries each; QPREP: RMSNorm + RoPE of q on load
__global__ __launch_bounds__(512, 2) void attention_d128_kernel(AttnArgs p);                  // attention_d128.h, instantiated in:
// attention_d128_w8.hip
extern template __global__ void attention_d128_kernel<8, 0, false, false>(AttnArgs);
extern template __global__ void attention_d128_kernel<8, 0, true, false>(AttnArgs);
extern template __global__ void attention_d128_kernel<8, 1, false, false>(AttnArgs);
extern template __global__ void attention_d128_kernel<8, 1, true, false>(AttnArgs);
extern template __global__ void attention_d128_kernel<8, 1, false, true>(AttnArgs);
extern template __global__ void attention_d128_kernel<8, 1, true, true>(AttnArgs);
extern template __global__ void attention_d128_kernel<8, 1, false, true, true>(AttnArgs);
extern template __global__ void attention_d128_kernel<8, 1, true, true, true>(AttnArgs);
// attention_d128_w4.hip
extern template __global__ void attention_d128_kernel<4, 0, false, false>(AttnArgs);
extern template __global__ void attention_d128_kernel<4, 0, true, false>(AttnArgs);
extern template __global__ void attention_d128_kernel<4, 1, false, false>(AttnArgs);
extern template __global__ void attention_d128_kernel<4, 1, true, false>(AttnArgs);
extern template __global__ void attention_d128_kernel<4, 1, false, true>(AttnArgs);
extern template __global__ void attention_d128_kernel<4, 1, true, true>(AttnArgs);
extern template __global__ void attention_d128_kernel<4, 1, false, true, true>(AttnArgs);
extern template __global__ void attention_d128_kernel<4, 1, true, true, true>(AttnArgs);
#if DRAG_EXP
// attention_d128_w8.hip: "attn_sched" 3 (both block sizes) and the persistent form
extern template __global__ void attention_d128_kernel<8, 2, false, true>(AttnArgs);
extern template __global__ void attention_d128_kernel<8, 2, true, true>(AttnArgs);
extern template __global__ void attention_d128_kernel<4, 2, false, true>(AttnArgs);
extern template __global__ void attention_d128_kernel<4, 2, true, true>(AttnArgs);
extern template __global__ void attention_d128_kernel<8, 1, false, true, false, true>(AttnArgs);
extern template __global__ void attention_d128_kernel<8, 1, true, true, false, true>(AttnArgs);
#endif

template <bool QPREP>
__global__ __launch_bounds__(256, 1) void attention_q64_kernel(AttnArgs p);                   // attention_q64.hip
extern template __global__ void attention_q64_kernel<true>(AttnArgs);
extern template __global__ void attention_q64_kernel<false>(AttnArgs);

template <bool QPREP, bool FOLD, int VAR = 0>      // VAR > 0: schedule variants of the fold form (DRAG_EXPERIMENTS builds: "attn_gen" = 10 + VAR)
__global__ __launch_bounds__(256, 1) void attention_q64g_kernel(AttnArgs p);                  // attention_q64g.hip
extern template __global__ void attention_q64g_kernel<true, true>(AttnArgs);
extern template __global__ void attention_q64g_kernel<true, false>(AttnArgs);
extern template __global__ void attention_q64g_kernel<false, false>(AttnArgs);
#if DRAG_EXP
#define DRAG_ATTN_Q64G_VARIANTS(X)                                                                                                 \
  X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17) X(18) X(19)
#define DRAG_AQV_EXTERN(V_) extern template __global__ void attention_q64g_kernel<true, true, V_>(AttnArgs);
DRAG_ATTN_Q64G_VARIANTS(DRAG_AQV_EXTERN)
#undef DRAG_AQV_EXTERN
#endif

}  // namespace drag_attn
