// mxfp8.hip — drag_quantize_mxfp8: bf16 rows -> OCP MXFP8 (e4m3fn elements + one e8m0 scale per 32 consecutive K elements).
//
// One pass, HBM-bound: a lane loads 16 bytes (8 bf16), four neighbouring lanes hold one MX block and take its maximum with two lane
// exchanges inside the quad (no LDS); a lane stores its 8 element bytes, one lane of 16 the 4 scale bytes of its 128 columns.
// The rule (domain-rag_amd/mx.py restates it on the host, and the tests hold this kernel to that byte for byte): amax over the block,
// e = the smallest integer with amax * 2^-e <= 448 — from amax's exponent and mantissa bits: E - 8, or E - 7 when the mantissa exceeds
// 1.75 — clamped to [-127, 127]; an all-zero block stores byte 127; elements are x * 2^-e rounded to nearest-even to e4m3fn, saturated at
// +-448 (reachable only under a clamped e).  Non-finite inputs are outside the contract.
#include "gemm_bf16_kernels.h"
#include "mx_quant.h"

namespace drag_mx {

__global__ __launch_bounds__(256) void quantize_mxfp8_kernel(const bf16_t* __restrict__ x, long long rows, int K, drag_gemm::RowMap xm,
                                                             uint8_t* __restrict__ q, uint8_t* __restrict__ scales) {
  const int cpr = K >> 3;                                 // 16-byte chunks per row; K % 128 == 0: a 16-lane group never straddles a row
  const long long total = rows * cpr;
  const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
  const bool live = gid < total;                          // total % 16 == 0: quads and 16-lane groups are live or idle as a whole
  const long long c = live ? gid : 0;
  const long long row = c / cpr;
  const int ch = (int)(c - row * cpr);
  const int bt = (int)(row / xm.rpb);
  const long long xoff = (long long)bt * xm.bs + (row - (long long)bt * xm.rpb) * xm.ld + ch * 8;
  const u32x4_t v = *(const u32x4_t*)(x + xoff);
  u32x2_t o;
  uint32_t s;
  quantize8(v, o, s);                                      // mx_quant.h: the rule, shared with the attention prep pass
  if (!live) return;
  *(u32x2_t*)(q + row * K + ch * 8) = o;
  if ((threadIdx.x & 15) == 0) *(uint32_t*)(scales + row * (K >> 5) + (ch >> 2)) = s;
}

}  // namespace drag_mx

extern "C" int drag_quantize_mxfp8(const void* x, int64_t rows, int32_t K, int32_t ldx, int32_t rows_per_batch, int64_t batch_stride,
                                   void* q, void* scales, void* stream) {
  DRAG_CHECK(x && q && scales, "drag_quantize_mxfp8: null pointer");
  DRAG_CHECK(rows > 0 && K > 0 && K % 128 == 0, "drag_quantize_mxfp8: rows > 0 and K a positive multiple of 128 required");
  DRAG_CHECK(ldx >= K && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0, "drag_quantize_mxfp8: ldx >= K, ldx %% 8 == 0 and a 16-byte aligned input required");
  DRAG_CHECK(((uintptr_t)q & 7) == 0 && ((uintptr_t)scales & 3) == 0, "drag_quantize_mxfp8: q must be 8-byte and scales 4-byte aligned");
  drag_gemm::RowMap xm;
  xm.rpb = rows_per_batch > 0 && rows_per_batch < rows ? rows_per_batch : (int)(rows < 0x7fffffff ? rows : 0x7fffffff);
  xm.bs = batch_stride; xm.ld = ldx;
  DRAG_CHECK(rows < (1ll << 31) || rows_per_batch > 0, "drag_quantize_mxfp8: more than 2^31 rows need a row map");
  DRAG_CHECK(xm.rpb >= rows || batch_stride % 8 == 0, "drag_quantize_mxfp8: batch_stride %% 8 == 0 required");
  const long long blocks = (rows * (K >> 3) + 255) / 256;
  DRAG_CHECK(blocks < (1ll << 31), "drag_quantize_mxfp8: too many elements for one launch");
  hipLaunchKernelGGL(drag_mx::quantize_mxfp8_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, (long long)rows, K,
                     xm, (uint8_t*)q, (uint8_t*)scales);
  DRAG_LAUNCH_CHECK();
  return 0;
}
