// gemm_bf16_deep_n128.hip — gemm_bf16_deep<MI, ST, 4>: the 128-column tiles.
#include "gemm_bf16_deep.h"

namespace drag_gemm {

DRAG_GEMM_DEEP_N128(DRAG_GEMM_DEEP_DEFINE)

}  // namespace drag_gemm
