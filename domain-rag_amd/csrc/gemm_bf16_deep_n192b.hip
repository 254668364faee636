// gemm_bf16_deep_n192b.hip — gemm_bf16_deep<MI, ST, 6>: 192-column tiles, 2- and 4-stage rings.
#include "gemm_bf16_deep.h"

namespace drag_gemm {

DRAG_GEMM_DEEP_N192B(DRAG_GEMM_DEEP_DEFINE)

}  // namespace drag_gemm
