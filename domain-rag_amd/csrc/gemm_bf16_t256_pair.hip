// gemm_bf16_t256_pair.hip — the 256x256 kernel over the two row segments of drag_gemm_bf16_pair.
#include "gemm_bf16_t256.h"

namespace drag_gemm {

__global__ __launch_bounds__(512, 2) void gemm_bf16_t256_pair(GemmKArgs p) { t256_body<0, true>(p); }

}  // namespace drag_gemm
