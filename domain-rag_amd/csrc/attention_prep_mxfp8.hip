// attention_prep_mxfp8.hip — drag_qkv_prep_mxfp8: the pass in front of drag_attention_mxfp8.  Reads the raw q | k | v projection under
// qk_norm_rope_vt_kernel's layout contract, leaves it untouched, and writes the six MXFP8 images of attention_mxfp8.h, every byte of them.
//
// grid (s_pad / 64, H, B), block 256.  q and k: 16 lanes per row, 8 elements per lane — the RMSNorm + RoPE arithmetic of the bf16 pass
// (qk_norm_rope8, attention_kernels.h: the values are what that pass would have stored) and then the block quantiser of
// quantize_mxfp8_kernel (quantize8, mx_quant.h), whose lane layout is the same: a quad holds one MX block, sixteen lanes the row's four.
// V: the 64 x 128 tile is staged in LDS as in the bf16 pass; one thread then owns one (d, block of 32 keys): amax, exponent, 32 bytes.
#include "attention_mxfp8.h"
#include "mx_quant.h"

namespace drag_attn {

__global__ __launch_bounds__(256) void qkv_prep_mxfp8_kernel(MxPrepArgs m) {
  __shared__ __attribute__((aligned(16))) bf16_t sv[64 * 136];  // V tile, row padded to 136 (272 B)
  const PrepArgs& p = m.a;
  const int tid = threadIdx.x;
  const int s0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;   // s0 + 63 < s_pad
  const int HD = p.H * 128;
  const bf16_t* base = p.qkv + (long long)b * p.S * p.ld;
  const long long bh = (long long)b * p.H + h;

  // ---- q and k: 16 lanes per row, 8 elements per lane ----
  const int sub = tid & 15;        // which 8-element group of the 128
  const int rloc = tid >> 4;       // 0..15
  const bool do_norm = p.wq_txt != nullptr, do_rope = p.cosT != nullptr;
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    uint8_t* eq = (which == 0 ? m.qq : m.kq) + bh * p.s_pad * 128;
    uint8_t* es = (which == 0 ? m.qs : m.ks) + bh * p.s_pad * 4;
    for (int it = 0; it < 4; ++it) {
      const int s = s0 + it * 16 + rloc;
      const bool ok = s < p.S;
      const int sc = ok ? s : p.S - 1;
      const u32x4_t raw = *(const u32x4_t*)(base + (long long)sc * p.ld + which * HD + h * 128 + sub * 8);
      u32x4_t v = (do_norm || do_rope) ? qk_norm_rope8(p, which, sc, sub, raw, do_norm, do_rope) : raw;
      if (!ok) v = (u32x4_t){0u, 0u, 0u, 0u};              // padding rows: zero bytes, scale byte 127
      u32x2_t o;
      uint32_t sw;
      drag_mx::quantize8(v, o, sw);
      *(u32x2_t*)(eq + (long long)s * 128 + sub * 8) = o;
      if (sub == 0) *(uint32_t*)(es + (long long)s * 4) = sw;
    }
  }

  // ---- v: stage [64 keys][128 d] in LDS (keys >= S as zeros), quantise along the keys ----
  for (int i = tid; i < 64 * 16; i += 256) {
    const int r = i >> 4, c = i & 15;
    const int s = s0 + r;
    u32x4_t v = (u32x4_t){0u, 0u, 0u, 0u};
    if (s < p.S) v = *(const u32x4_t*)(base + (long long)s * p.ld + 2 * HD + h * 128 + c * 8);
    *(u32x4_t*)(sv + r * 136 + c * 8) = v;
  }
  __syncthreads();
  const int d = tid & 127, blk = tid >> 7;                 // the thread's V^T row and which 32 of the tile's 64 keys
  uint32_t amax = 0;
#pragma unroll
  for (int j = 0; j < 32; ++j) amax = max(amax, (uint32_t)sv[(32 * blk + j) * 136 + d] & 0x7FFFu);
  const int e = drag_mx::block_exponent(amax);
  const float inv = drag_mx::block_inverse(e);
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    w[j] = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) w[j] |= drag_mx::e4m3_byte(sv[(32 * blk + 4 * j + i) * 136 + d], inv) << (8 * i);
  }
  uint8_t* vrow = m.vq + (bh * 128 + d) * p.s_pad + s0 + 32 * blk;
  *(u32x4_t*)vrow = (u32x4_t){w[0], w[1], w[2], w[3]};
  *(u32x4_t*)(vrow + 16) = (u32x4_t){w[4], w[5], w[6], w[7]};
  m.vs[(bh * 128 + d) * (p.s_pad >> 5) + (s0 >> 5) + blk] = (uint8_t)(e + 127);
}

}  // namespace drag_attn

using namespace drag_attn;

extern "C" int drag_qkv_prep_mxfp8(const void* qkv, const void* wq_txt, const void* wk_txt, const void* wq_img, const void* wk_img,
                                   const float* rope_cos, const float* rope_sin, int32_t B, int32_t S, int32_t H, int32_t ld, int32_t s_txt,
                                   float eps, void* qq, void* qs, void* kq, void* ks, void* vq, void* vs, void* stream) {
  DRAG_CHECK(qkv && qq && qs && kq && ks && vq && vs, "drag_qkv_prep_mxfp8: null pointer");
  DRAG_CHECK((wq_txt && wk_txt && wq_img && wk_img) || (!wq_txt && !wk_txt && !wq_img && !wk_img),
             "drag_qkv_prep_mxfp8: norm weights are all-or-none");
  DRAG_CHECK((rope_cos == nullptr) == (rope_sin == nullptr), "drag_qkv_prep_mxfp8: cos/sin come in pairs");
  DRAG_CHECK(mx_shape_ok(B, S, H), "drag_qkv_prep_mxfp8: unsupported shape (B, H in 1 .. 65535, S in 1 .. 2^23)");
  DRAG_CHECK(ld >= 3 * H * 128 && ld % 8 == 0 && ((uintptr_t)qkv & 15) == 0, "drag_qkv_prep_mxfp8: ld >= 3 * H * 128, ld %% 8 == 0 and a 16-byte aligned qkv required");
  DRAG_CHECK((((uintptr_t)qq | (uintptr_t)kq | (uintptr_t)vq) & 15) == 0 && (((uintptr_t)qs | (uintptr_t)ks | (uintptr_t)vs) & 3) == 0,
             "drag_qkv_prep_mxfp8: element images must be 16-byte and scale images 4-byte aligned");
  MxPrepArgs m;
  PrepArgs& p = m.a;
  p.qkv = (bf16_t*)qkv; p.vt = nullptr;
  p.wq_txt = (const bf16_t*)wq_txt; p.wk_txt = (const bf16_t*)wk_txt; p.wq_img = (const bf16_t*)wq_img; p.wk_img = (const bf16_t*)wk_img;
  p.cosT = rope_cos; p.sinT = rope_sin;
  p.B = B; p.S = S; p.H = H; p.ld = ld; p.s_txt = s_txt; p.s_pad = mx_s_pad(S); p.eps = eps; p.skip_q = 0;
  m.qq = (uint8_t*)qq; m.qs = (uint8_t*)qs; m.kq = (uint8_t*)kq; m.ks = (uint8_t*)ks; m.vq = (uint8_t*)vq; m.vs = (uint8_t*)vs;
  hipLaunchKernelGGL(qkv_prep_mxfp8_kernel, dim3(p.s_pad / 64, H, B), dim3(256), 0, (hipStream_t)stream, m);
  DRAG_LAUNCH_CHECK();
  return 0;
}
