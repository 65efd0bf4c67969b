// Host side of the fused MLP kernels: the one mapping from plan->precision to a matrix core, and the one way a kernel
// of a core is launched.  The fp32 kernels are defined in sdf_mlp.hip / color_mlp.hip beside the C entry points; the
// bf16 kernels are defined and instantiated (2 and 3 planes) in sdf_mlp_b16.hip / color_mlp_b16.hip and declared
// here, which is all those translation units export.
#pragma once
#include "sdf_kernels.h"
#include "color_kernels.h"
#include "mlp_core_b16.h"

// head of a bf16 MLP kernel, here and at its definition
#define MLP_B16_KERNEL template <int NS> __global__ void __launch_bounds__(CoreB16N<NS>::THREADS, CoreB16N<NS>::WGS_PER_CU)
template <int NS>
__global__ void __launch_bounds__(256) msdf_pack_b16_kernel(const msdf_plan_t plan, const msdf_packrule_t* __restrict__ rules,
                                                            const int* __restrict__ maps, const float* __restrict__ flat_w,
                                                            const float* __restrict__ flat_b, v8bf* __restrict__ wpack,
                                                            float* __restrict__ bpack);
MLP_B16_KERNEL msdf_sdf_forward_b16_k(const msdf_plan_t plan, const v8bf* __restrict__ wpack, const float* __restrict__ bpack,
                                      const float* __restrict__ x, const float* __restrict__ aux, const AuxView av, const int P,
                                      const float clamp_radius, const float sphere_scale, float* __restrict__ sdf_out,
                                      const uint32_t* __restrict__ run_flag);
MLP_B16_KERNEL msdf_sdf_fwd_grad_b16_k(const msdf_plan_t plan, const FgArgs a);
MLP_B16_KERNEL msdf_sdf_backward_b16_k(const msdf_plan_t plan, const BwArgs a);
MLP_B16_KERNEL msdf_color_forward_b16_k(const msdf_plan_t plan, const ColorFwdArgs a);
MLP_B16_KERNEL msdf_color_backward_b16_k(const msdf_plan_t plan, const ColorBwdArgs a);

// f(Core()) with the core plan->precision names; MSDF_ERR_ARG for a value that names none
template <class F>
static int mlp_with_core(const msdf_plan_t* plan, F&& f) {
  switch (plan->precision) {
    case MSDF_PRECISION_F32: return f(CoreF32());
    case MSDF_PRECISION_BF16X3: return f(CoreB16N<2>());
    case MSDF_PRECISION_BF16X6: return f(CoreB16N<3>());
    default: return MSDF_ERR_ARG;
  }
}

// n_wgs workgroups of a kernel of `Core` on `stream`, with the core's threads and dynamic LDS
template <class Core, class... Params, class... Args>
static int mlp_launch(void (*kernel)(Params...), const int n_wgs, void* stream, const Args&... args) {
  if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, Core::LDS_BYTES) != hipSuccess)
    return MSDF_ERR_LAUNCH;
  kernel<<<n_wgs, Core::THREADS, Core::LDS_BYTES, (hipStream_t)stream>>>(args...);
  return msdf_check_launch();
}
