// Colour-network kernels for gfx950 (RenderingNetwork, reference: code/model/network.py:389-470,
// mode 'idr' / 'nerf', ReLU hidden layers, sigmoid or ReLU output, no `spec` branch).
//
// Same register-resident scheme as the SDF network (mlp_core.h).  The first layer's
// 289-wide input is split into two GEMM passes over the same accumulators: the
// feature tiles (256 slots, read from the SDF kernel's output) and a small "misc"
// block [x | PE(view) | normal | (per-image code)] built in registers.
//
// The plan's "layers" are pack units: unit 0 = first layer, feature columns;
// unit 1 = first layer, misc columns; units 2.. = the remaining layers.
#include "mlp_launch.h"

__global__ void __launch_bounds__(CoreF32::THREADS, CoreF32::WGS_PER_CU)
msdf_color_forward_k(const msdf_plan_t plan, const ColorFwdArgs a) {
  extern __shared__ v4f lds[];
  color_forward_body<CoreF32>(plan, a, lds);
}

__global__ void __launch_bounds__(CoreF32::THREADS, CoreF32::WGS_PER_CU)
msdf_color_backward_k(const msdf_plan_t plan, const ColorBwdArgs a) {
  extern __shared__ v4f lds[];
  color_backward_body<CoreF32>(plan, a, lds);
}

// the kernels of a core
static auto forward_kernel(CoreF32) { return msdf_color_forward_k; }
static auto backward_kernel(CoreF32) { return msdf_color_backward_k; }
template <int NS> static auto forward_kernel(CoreB16N<NS>) { return msdf_color_forward_b16_k<NS>; }
template <int NS> static auto backward_kernel(CoreB16N<NS>) { return msdf_color_backward_b16_k<NS>; }

// P_pad: whole workgroups (64 points on every core) that cover the P points
static bool padded_ok(const int P, const int P_pad) { return P_pad >= P && (P_pad % CoreF32::PTS_PER_WG) == 0; }

extern "C" int msdf_color_forward(const msdf_plan_t* plan, const msdf_color_fwd_args_t* a, void* stream) {
  if (plan == nullptr || a == nullptr || a->P < 0 || a->spr < 1) return MSDF_ERR_ARG;
  if (a->P == 0) return MSDF_OK;
  if (!padded_ok(a->P, a->P_pad)) return MSDF_ERR_ARG;
  return mlp_with_core(plan, [&](auto core) {
    typedef decltype(core) Core;
    return mlp_launch<Core>(forward_kernel(core), a->P_pad / Core::PTS_PER_WG, stream, *plan, *a);
  });
}

extern "C" int msdf_color_backward(const msdf_plan_t* plan, const msdf_color_bwd_args_t* a, void* stream) {
  if (plan == nullptr || a == nullptr || a->P < 0) return MSDF_ERR_ARG;
  if (a->P == 0) return MSDF_OK;
  if (!padded_ok(a->P, a->P_pad)) return MSDF_ERR_ARG;
  return mlp_with_core(plan, [&](auto core) {
    typedef decltype(core) Core;
    return mlp_launch<Core>(backward_kernel(core), a->P_pad / Core::PTS_PER_WG, stream, *plan, *a);
  });
}
