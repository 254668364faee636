// attention_d128_w8.hip — attention_d128_kernel<8, ...>: the 8-wave blocks (S >= 4096 when the 64-query kernels do not run), and, in experiment
// builds, the "attn_sched" 3 form of both block sizes and the persistent form.
#include "attention_d128.h"

namespace drag_attn {

template __global__ void attention_d128_kernel<8, 0, false, false>(AttnArgs);
template __global__ void attention_d128_kernel<8, 0, true, false>(AttnArgs);
template __global__ void attention_d128_kernel<8, 1, false, false>(AttnArgs);
template __global__ void attention_d128_kernel<8, 1, true, false>(AttnArgs);
template __global__ void attention_d128_kernel<8, 1, false, true>(AttnArgs);
template __global__ void attention_d128_kernel<8, 1, true, true>(AttnArgs);
template __global__ void attention_d128_kernel<8, 1, false, true, true>(AttnArgs);
template __global__ void attention_d128_kernel<8, 1, true, true, true>(AttnArgs);
#if DRAG_EXP
template __global__ void attention_d128_kernel<8, 2, false, true>(AttnArgs);
template __global__ void attention_d128_kernel<8, 2, true, true>(AttnArgs);
template __global__ void attention_d128_kernel<4, 2, false, true>(AttnArgs);
template __global__ void attention_d128_kernel<4, 2, true, true>(AttnArgs);
template __global__ void attention_d128_kernel<8, 1, false, true, false, true>(AttnArgs);
template __global__ void attention_d128_kernel<8, 1, true, true, false, true>(AttnArgs);
#endif

}  // namespace drag_attn
