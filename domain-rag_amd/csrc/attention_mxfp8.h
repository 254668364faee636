// attention_mxfp8.h — what the MXFP8 attention path shares: the prep pass (attention_prep_mxfp8.hip), the kernel and its host side
// (attention_mxfp8.hip).  Opt-in; the bf16 path (attention_kernels.h) calls none of this.
//
// Operands (include/domainrag_hip.h and domain-rag_amd/mx.py state the format): per (batch, head), dense,
//   q, k : [s_pad][128] e4m3fn bytes + [s_pad][4] e8m0 bytes (MX blocks along head_dim), s_pad = S rounded up to 128; rows >= S are
//          zero bytes under scale byte 127;
//   V^T  : [128][s_pad] e4m3fn bytes + [128][s_pad / 32] e8m0 bytes (MX blocks of 32 consecutive keys, NATURAL key order; keys >= S zero).
//
// The kernel: block = 4 waves, a wave owns NQ blocks of 16 queries, KV tile = 128 keys, K tile [128][128 B] and V^T tile [128][128 B]
// staged HBM -> registers -> LDS (16-byte pieces, XOR-swizzled, double-buffered, one barrier per tile).  Both products run on
// v_mfma_scale_f32_16x16x128_f8f6f4 under the operand map of gemm_mxfp8.h (lane (c, g) = (l & 15, l >> 4) supplies the 16 bytes at
// contraction offsets 16 g and 64 + 16 g of its row, and the scale byte of MX block g).
//   S^T = K Q^T: a = K fragment, b = Q fragment, one instruction per 16 keys x 16 queries (head_dim = 128 = one K-step).  Lane (c, g) gets
//     S^T[key row 4 g + r][query c], r = 0..3.  Score block t of a tile is computed over the 16 keys
//         kappa(t, i) = 64 (t >> 2) + 16 (i >> 2) + 4 (t & 3) + (i & 3),     i = 0..15 the block's row,
//     (the K tile's rows are stored in LDS in that order), so that lane (c, g) holds, in block t and register r, the tile's key
//         64 (t >> 2) + 16 g + 4 (t & 3) + r
//     — exactly the contraction offsets (16 g + j, 64 + 16 g + j) a lane supplies as the b operand of the second product: the 32 values
//     exp2(s - m) of a lane, rounded to e4m3 and packed four to a register in block order, ARE the P fragment.  No LDS, no lane exchange,
//     and V^T stays in natural key order.
//   O^T += V^T P^T: a = V^T fragment (row d, keys of the tile), b = P; one instruction per 16 d x 16 queries x 128 keys.  P's scale byte
//     is the constant 119 (2^-8): the operand is e4m3(p * 256), p <= 1.
// A lane owns one query column: the online softmax is lane-local apart from two exchanges (lane ^ 16, lane ^ 32: the four lane groups hold
// different keys of the same query).  Row sums add the float32 p before the rounding.  Keys >= S are masked to -inf (a zero k row scores 0).
#pragma once
#include "attention_kernels.h"

namespace drag_attn {

struct MxPrepArgs {
  PrepArgs a;              // qkv (read only here), the norm weights, the RoPE tables, B, S, H, ld, s_txt, eps; s_pad = S rounded up to 128
  uint8_t *qq, *qs, *kq, *ks, *vq, *vs;
};

struct MxAttnArgs {
  const uint8_t *qq, *qs, *kq, *ks, *vq, *vs;
  bf16_t* out;
  int B, S, H, s_pad, ld_o;
  long long o_bs;
  float c;                 // scale * log2(e)
};

constexpr int MX_KV = 128;           // keys per tile = one K-step of the second product
constexpr int MX_TILE_BYTES = 128 * 128;

// S rounded up to a whole KV tile: the row count of the q / k images and the row length of the V^T image
inline int mx_s_pad(int S) { return (S + MX_KV - 1) / MX_KV * MX_KV; }
// the shapes both entry points take: one (batch, head)'s images are addressed with 32-bit offsets, heads and batches are grid dimensions
inline bool mx_shape_ok(int B, int S, int H) { return B > 0 && S > 0 && H > 0 && B <= 65535 && H <= 65535 && S <= (1 << 23); }

}  // namespace drag_attn
