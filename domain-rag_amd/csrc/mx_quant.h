// mx_quant.h — the MXFP8 block quantiser's device arithmetic, stated once: the shared exponent of a block from its largest bf16 magnitude,
// and one element's e4m3fn byte.  quantize_mxfp8_kernel (mxfp8.hip) and qkv_prep_mxfp8_kernel (attention_prep_mxfp8.hip) are built from
// these; domain-rag_amd/mx.py restates the rule on the host and the tests hold both kernels to it byte for byte.
#pragma once
#include "drag_common.h"

namespace drag_mx {

// |v| <= 448 as float32 bits (sign cleared) -> the 7 magnitude bits of e4m3fn, round to nearest even
__device__ __forceinline__ uint32_t e4m3_mag(float a) {
  const uint32_t b = __float_as_uint(a);
  if (a >= 0.015625f) {                                   // normal e4m3 (>= 2^-6): round the mantissa to 3 bits; a carry moves the exponent
    const uint32_t r = (b + 0x7FFFFu + ((b >> 20) & 1u)) >> 20;
    return r - (120u << 3);                               // exponent bias 127 -> 7
  }
  // subnormal: multiples of 2^-9; the sum with 2^23 rounds to nearest even and leaves the integer 0..8 in the low bits (8 = 2^-6)
  return __float_as_uint(a * 512.0f + 8388608.0f) & 0xFFu;
}

// the shared exponent e of a block whose largest magnitude has the bf16 bits amax (sign cleared): the smallest integer with
// amax * 2^-e <= 448, from the exponent and mantissa bits; 0 for an all-zero block.  The scale byte is e + 127.
__device__ __forceinline__ int block_exponent(uint32_t amax) {
  int e = (int)(amax >> 7) - 127 - 8 + ((amax & 0x7Fu) > 0x60u ? 1 : 0);     // (a subnormal amax reads E = -127: clamped either way)
  e = max(e, -127);                                       // bf16's largest exponent gives e = 120: the upper clamp is never reached
  return amax == 0 ? 0 : e;
}

// 2^-e as a float (exponent field 7 .. 254)
__device__ __forceinline__ float block_inverse(int e) { return __uint_as_float((uint32_t)(127 - e) << 23); }

// the e4m3fn byte of the bf16 bits h under the block's inv = 2^-e
__device__ __forceinline__ uint32_t e4m3_byte(uint32_t h, float inv) {
  const float a = fminf(__uint_as_float((h & 0x7FFFu) << 16) * inv, 448.0f);
  return ((h >> 8) & 0x80u) | e4m3_mag(a);
}

// One lane's 8 consecutive bf16 of a row (v), the four lanes of an aligned quad holding one MX block and sixteen lanes 128 columns:
// the lane's 8 element bytes, and — in the first lane of sixteen — the four scale bytes of those 128 columns.  Every lane of the
// sixteen must call it (two exchanges inside the quad, two across it).
__device__ __forceinline__ void quantize8(const u32x4_t v, u32x2_t& o, uint32_t& s) {
  // bf16 magnitudes order like their bit patterns
  uint32_t amax = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    amax = max(amax, v[i] & 0x7FFFu);
    amax = max(amax, (v[i] >> 16) & 0x7FFFu);
  }
  amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1, 64));
  amax = max(amax, (uint32_t)__shfl_xor((int)amax, 2, 64));
  const int e = block_exponent(amax);
  const float inv = block_inverse(e);
  o = (u32x2_t){0u, 0u};
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t h = (v[i >> 1] >> ((i & 1) * 16)) & 0xFFFFu;
    o[i >> 2] |= e4m3_byte(h, inv) << ((i & 3) * 8);
  }
  // the four scale bytes of this 16-lane group's 128 columns, gathered into its first lane
  s = (uint32_t)(e + 127);
  s |= (uint32_t)__shfl_down((int)s, 4, 64) << 8;
  s |= (uint32_t)__shfl_down((int)s, 8, 64) << 16;
}

}  // namespace drag_mx
