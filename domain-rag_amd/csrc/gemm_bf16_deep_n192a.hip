// gemm_bf16_deep_n192a.hip — gemm_bf16_deep<MI, ST, 6>: 192-column tiles, 3-stage ring.
#include "gemm_bf16_deep.h"

namespace drag_gemm {

DRAG_GEMM_DEEP_N192A(DRAG_GEMM_DEEP_DEFINE)

}  // namespace drag_gemm
