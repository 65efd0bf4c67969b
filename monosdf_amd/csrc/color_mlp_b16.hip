// bf16x3 / bf16x6 instantiations of the colour-network kernels (color_kernels.h on CoreB16N, mlp_core_b16.h).
#include "mlp_launch.h"

MLP_B16_KERNEL msdf_color_forward_b16_k(const msdf_plan_t plan, const ColorFwdArgs a) {
  extern __shared__ v8bf lds16[];
  color_forward_body<CoreB16N<NS>>(plan, a, lds16);
}

MLP_B16_KERNEL msdf_color_backward_b16_k(const msdf_plan_t plan, const ColorBwdArgs a) {
  extern __shared__ v8bf lds16[];
  color_backward_body<CoreB16N<NS>>(plan, a, lds16);
}

// what this translation unit exports (declared in mlp_launch.h, launched by the C entry points of color_mlp.hip)
template __global__ void msdf_color_forward_b16_k<2>(const msdf_plan_t, const ColorFwdArgs);
template __global__ void msdf_color_forward_b16_k<3>(const msdf_plan_t, const ColorFwdArgs);
template __global__ void msdf_color_backward_b16_k<2>(const msdf_plan_t, const ColorBwdArgs);
template __global__ void msdf_color_backward_b16_k<3>(const msdf_plan_t, const ColorBwdArgs);
