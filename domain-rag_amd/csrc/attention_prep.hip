// attention_prep.hip — qk_norm_rope_vt_kernel: the pass in front of the attention kernels.
#include "attention_kernels.h"

namespace drag_attn {

// --------------------------------------------------------------------------------------------
// q/k RMSNorm + RoPE in place, V -> V^T.   grid (ceil(S/64), H, B), block 256.
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void qk_norm_rope_vt_kernel(PrepArgs p) {
  __shared__ __attribute__((aligned(16))) bf16_t sv[64 * 136];  // V tile, row padded to 136 (272 B)
  const int tid = threadIdx.x;
  const int s0 = blockIdx.x * 64, h = blockIdx.y, b = blockIdx.z;
  const int HD = p.H * 128;
  bf16_t* base = p.qkv + (long long)b * p.S * p.ld;

  // ---- q and k: 16 lanes per row, 8 elements per lane ----
  const int sub = tid & 15;        // which 8-element group of the 128
  const int rloc = tid >> 4;       // 0..15
  const bool do_norm = p.wq_txt != nullptr, do_rope = p.cosT != nullptr;
  if (do_norm || do_rope)
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    if (which == 0 && p.skip_q) continue;
    for (int it = 0; it < 4; ++it) {
      const int s = s0 + it * 16 + rloc;
      const bool ok = s < p.S;
      const int sc = ok ? s : p.S - 1;
      bf16_t* ptr = base + (long long)sc * p.ld + which * HD + h * 128 + sub * 8;
      const u32x4_t raw = *(const u32x4_t*)ptr;
      const u32x4_t o = qk_norm_rope8(p, which, sc, sub, raw, do_norm, do_rope);
      if (ok) *(u32x4_t*)ptr = o;
    }
  }

  if (p.vt == nullptr) return;        // k only: the attention kernel reads V row-major
  // ---- v: stage [64 keys][128 d] in LDS, write V^T[d][pos(key)] ----
  for (int i = tid; i < 64 * 16; i += 256) {
    const int r = i >> 4, c = i & 15;
    const int s = s0 + r;
    u32x4_t v = (u32x4_t){0u, 0u, 0u, 0u};
    if (s < p.S) v = *(const u32x4_t*)(base + (long long)s * p.ld + 2 * HD + h * 128 + c * 8);
    *(u32x4_t*)(sv + r * 136 + c * 8) = v;
  }
  __syncthreads();
  bf16_t* vtb = p.vt + ((long long)(b * p.H + h) * 128) * p.s_pad + s0;
  for (int i = tid; i < 128 * 8; i += 256) {
    const int d = i >> 3, g8 = i & 7;  // 8 positions [8*g8, 8*g8+8) of row d
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 8; j += 2) {
      // position q = 8*g8 + j  ->  group = q>>4, within = q&15 = 8h+jj -> key offset 8*(jj>>2)+4h+(jj&3)
      const int q0 = 8 * g8 + j, q1 = q0 + 1;
      const int k0 = (q0 & ~15) + 8 * (((q0 & 15) & 7) >> 2) + 4 * ((q0 & 15) >> 3) + (q0 & 3);
      const int k1 = (q1 & ~15) + 8 * (((q1 & 15) & 7) >> 2) + 4 * ((q1 & 15) >> 3) + (q1 & 3);
      w[j >> 1] = (uint32_t)sv[k0 * 136 + d] | ((uint32_t)sv[k1 * 136 + d] << 16);
    }
    *(u32x4_t*)(vtb + (long long)d * p.s_pad + 8 * g8) = (u32x4_t){w[0], w[1], w[2], w[3]};
  }
}

}  // namespace drag_attn
