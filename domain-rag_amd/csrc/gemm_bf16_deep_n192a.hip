// gemm_bf16_deep_n192a.hip — gemm_bf16_deep<MI, ST, 6>: 192-column tiles, 3-stage ring.
#include "gemm_bf16_deep.h"

namespace drag_gemm {

template __global__ void gemm_bf16_deep<1, 3, 6>(GemmKArgs);
template __global__ void gemm_bf16_deep<2, 3, 6>(GemmKArgs);
template __global__ void gemm_bf16_deep<3, 3, 6>(GemmKArgs);
template __global__ void gemm_bf16_deep<4, 3, 6>(GemmKArgs);

}  // namespace drag_gemm
