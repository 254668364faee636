// gemm_mxfp8.h — what the MXFP8 GEMM's host side (gemm_mxfp8.hip) and its kernels (one per source, as the bf16 GEMM is split) share.
//
// drag_gemm_mxfp8 multiplies OCP MXFP8 operands (e4m3fn bytes + one e8m0 scale byte per 32 consecutive K elements, both dense) on
// v_mfma_scale_f32_16x16x128_f8f6f4 and hands the accumulators to the bf16 GEMM's epilogue (gemm_bf16_kernels.h) unchanged: the scaled
// instruction's C/D layout is that of v_mfma_f32_16x16x32_bf16.
//
// Operand map of the scaled 16x16x128 instruction as these kernels use it (confirmed by the exact-integer test of
// tests/test_gpu_mxfp8.py): the instruction is two K = 64 halves.  Lane l = (row / column l & 15, group g = l >> 4) supplies in its first four
// registers the 16 bytes at K offset 16 g of the step and in its last four those at 64 + 16 g — the two fragment reads of a bf16 K-step
// of 64, byte for byte — and in byte 0 of its scale register (OPSEL 0) the e8m0 byte of MX block g (K offsets 32 g .. 32 g + 31) of its
// row: the hardware scales by K position, so a lane's two halves fall under the scales that lane groups g >> 1 and 2 + (g >> 1) supply.
// Operands are swapped as in the bf16 kernels (a = W fragment, b = A fragment): a lane owns 4 consecutive output columns.  One MFMA covers one 128-K step of a 16x16 output block, K-steps ascending: every output element has one
// accumulation chain.
#pragma once
#include "gemm_bf16_kernels.h"

namespace drag_gemm {

typedef __attribute__((ext_vector_type(8))) int i32x8_t;     // 32 fp8 bytes: one lane's operand of the scaled MFMA

struct MxKArgs {
  GemmKArgs g;             // M, N, K, the output's row map and every epilogue operand (A / W and their row maps unused)
  const uint8_t* Aq;       // [M, K] e4m3fn
  const uint8_t* As;       // [M, K / 32] e8m0
  const uint8_t* Wq;       // [N, K]
  const uint8_t* Ws;       // [N, K / 32]
};

__global__ __launch_bounds__(256, 2) void gemm_mxfp8_simple(MxKArgs p);                       // gemm_mxfp8_simple.hip

}  // namespace drag_gemm
