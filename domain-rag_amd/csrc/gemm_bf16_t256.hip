// gemm_bf16_t256.hip — gemm_bf16_t256<MODE>: batched rows (drag_gemm_bf16) and the conv3x3 implicit GEMM (drag_conv3x3_bf16).
#include "gemm_bf16_t256.h"

namespace drag_gemm {

template __global__ void gemm_bf16_t256<0>(GemmKArgs);
template __global__ void gemm_bf16_t256<1>(GemmKArgs);

}  // namespace drag_gemm
