// attention_d128_w4.hip — attention_d128_kernel<4, ...>: the 4-wave blocks of the short sequences.
#include "attention_d128.h"

namespace drag_attn {

template __global__ void attention_d128_kernel<4, 0, false, false>(AttnArgs);
template __global__ void attention_d128_kernel<4, 0, true, false>(AttnArgs);
template __global__ void attention_d128_kernel<4, 1, false, false>(AttnArgs);
template __global__ void attention_d128_kernel<4, 1, true, false>(AttnArgs);
template __global__ void attention_d128_kernel<4, 1, false, true>(AttnArgs);
template __global__ void attention_d128_kernel<4, 1, true, true>(AttnArgs);
template __global__ void attention_d128_kernel<4, 1, false, true, true>(AttnArgs);
template __global__ void attention_d128_kernel<4, 1, true, true, true>(AttnArgs);

}  // namespace drag_attn
