// gemm_bf16_deep_n128.hip — gemm_bf16_deep<MI, ST, 4>: the 128-column tiles.
#include "gemm_bf16_deep.h"

namespace drag_gemm {

template __global__ void gemm_bf16_deep<4, 2, 4>(GemmKArgs);
template __global__ void gemm_bf16_deep<4, 3, 4>(GemmKArgs);
template __global__ void gemm_bf16_deep<3, 2, 4>(GemmKArgs);
template __global__ void gemm_bf16_deep<3, 3, 4>(GemmKArgs);
template __global__ void gemm_bf16_deep<2, 2, 4>(GemmKArgs);
template __global__ void gemm_bf16_deep<2, 3, 4>(GemmKArgs);
template __global__ void gemm_bf16_deep<2, 4, 4>(GemmKArgs);
template __global__ void gemm_bf16_deep<1, 3, 4>(GemmKArgs);
template __global__ void gemm_bf16_deep<1, 4, 4>(GemmKArgs);

}  // namespace drag_gemm
