// gemm_bf16_deep_n192b.hip — gemm_bf16_deep<MI, ST, 6>: 192-column tiles, 2- and 4-stage rings.
#include "gemm_bf16_deep.h"

namespace drag_gemm {

template __global__ void gemm_bf16_deep<3, 2, 6>(GemmKArgs);
template __global__ void gemm_bf16_deep<4, 2, 6>(GemmKArgs);
template __global__ void gemm_bf16_deep<3, 4, 6>(GemmKArgs);
template __global__ void gemm_bf16_deep<4, 4, 6>(GemmKArgs);

}  // namespace drag_gemm
