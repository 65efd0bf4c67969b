// SDF-network kernels for gfx950: weight packer, no-grad forward (sampler),
// forward + d sdf/dx (get_outputs / gradient_sdf), and the double-backward sweep.
//
// Replaces, for the hot path, the PyTorch graph built by the reference's
// ImplicitNetwork / ImplicitNetworkGrid (code/model/network.py:79-137, 247-309)
// and its autograd double backward (create_graph=True at network.py:125,285,301).
// Math: DESIGN.md "SDF network kernels".
#include "mlp_launch.h"

// ---------------------------------------------------------------------------
// weight packer: flat effective weights -> fragment-ordered packs (both orientations)
// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) msdf_pack_kernel(const msdf_plan_t plan,
                                                        const msdf_packrule_t* __restrict__ rules,
                                                        const int* __restrict__ maps,
                                                        const float* __restrict__ flat_w,
                                                        const float* __restrict__ flat_b,
                                                        v4f* __restrict__ wpack, float* __restrict__ bpack) {
  const int l = blockIdx.y;
  const int which = blockIdx.z;  // 0 forward pack, 1 transposed pack, 2 bias (+ sdf row on the last layer)
  const msdf_layer_t L = plan.layer[l];
  const msdf_packrule_t R = rules[l];
  const int* rowmap = maps + R.rowmap_off;
  const int* colmap = maps + R.colmap_off;
  const float* W = flat_w + R.w_off;
  const int stride = gridDim.x * blockDim.x;
  const int t0 = blockIdx.x * blockDim.x + threadIdx.x;
  if (which < 2) {
    // which 0: rows = out slots, k = in slots (forward);  which 1: rows = in slots, k = out slots (transposed)
    const int n_rt = which == 0 ? L.ot : L.kt;          // row tiles
    const int n_kt = which == 0 ? L.kt : L.ot;          // k tiles (true count)
    const int ktp = which == 0 ? L.ktp : L.otp;         // k tiles in the pack
    const int off = which == 0 ? L.wf_off : L.wb_off;
    const int total = ((n_rt + 1) & ~1) * ktp * 64;
    for (int i = t0; i < total; i += stride) {
      const int lane = i & 63;
      const int blk = i >> 6;
      const int kt = blk % ktp, rt = blk / ktp;
      const int rslot = 16 * rt + (lane & 15);
      v4f v;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kslot = 16 * kt + 4 * (lane >> 4) + r;
        float w = 0.f;
        if (rt < n_rt && kt < n_kt) {
          const int row = which == 0 ? rowmap[rslot] : rowmap[kslot];
          const int col = which == 0 ? colmap[kslot] : colmap[rslot];
          if (row >= 0 && col >= 0) w = R.scale * W[(size_t)row * R.cols + col];
        }
        v[r] = w;
      }
      wpack[off + i] = v;
    }
  } else {
    pack_bias_rows(plan, l, R, rowmap, colmap, W, flat_b, bpack, t0, stride);
  }
}

__global__ void __launch_bounds__(CoreF32::THREADS, CoreF32::WGS_PER_CU)
msdf_sdf_forward_k(const msdf_plan_t plan, const v4f* __restrict__ wpack, const float* __restrict__ bpack,
                   const float* __restrict__ x, const float* __restrict__ aux, const AuxView av, const int P,
                   const float clamp_radius, const float sphere_scale, float* __restrict__ sdf_out,
                   const uint32_t* __restrict__ run_flag) {
  extern __shared__ v4f lds[];
  if (run_flag != nullptr && *run_flag == 0u) return;     // a sampler round nobody asked for (uniform over the grid)
  sdf_forward_body<CoreF32>(plan, wpack, bpack, x, aux, av, P, clamp_radius, sphere_scale, sdf_out, lds);
}

// the same values, and the hidden activations of the dense-set columns saved for the forward + gradient kernel
__global__ void __launch_bounds__(CoreF32::THREADS, CoreF32::WGS_PER_CU)
msdf_sdf_forward_save_k(const msdf_plan_t plan, const v4f* __restrict__ wpack, const float* __restrict__ bpack,
                        const float* __restrict__ x, const float* __restrict__ aux, const AuxView av, const int P,
                        const float clamp_radius, const float sphere_scale, float* __restrict__ sdf_out,
                        const uint32_t* __restrict__ run_flag, const HSaveArgs hs, uint32_t* __restrict__ h_saved) {
  extern __shared__ v4f lds[];
  if (run_flag != nullptr && *run_flag == 0u) return;
  if (blockIdx.x == 0 && threadIdx.x == 0) *h_saved = 1u;
  sdf_forward_body<CoreF32, true>(plan, wpack, bpack, x, aux, av, P, clamp_radius, sphere_scale, sdf_out, lds, hs);
}

__global__ void __launch_bounds__(CoreF32::THREADS, CoreF32::WGS_PER_CU)
msdf_sdf_fwd_grad_k(const msdf_plan_t plan, const FgArgs a) {
  extern __shared__ v4f lds[];
  if (sdf_fwd_grad_reuses<CoreF32>(plan, a)) sdf_fwd_grad_body<CoreF32, true>(plan, a, lds);
  else sdf_fwd_grad_body<CoreF32>(plan, a, lds);
}

__global__ void __launch_bounds__(CoreF32::THREADS, CoreF32::WGS_PER_CU)
msdf_sdf_backward_k(const msdf_plan_t plan, const BwArgs a) {
  extern __shared__ v4f lds[];
  sdf_backward_body<CoreF32>(plan, a, lds);
}

// the kernels of a core
static auto pack_kernel(CoreF32) { return msdf_pack_kernel; }
static auto forward_kernel(CoreF32) { return msdf_sdf_forward_k; }
static auto fwd_grad_kernel(CoreF32) { return msdf_sdf_fwd_grad_k; }
static auto backward_kernel(CoreF32) { return msdf_sdf_backward_k; }
template <int NS> static auto pack_kernel(CoreB16N<NS>) { return msdf_pack_b16_kernel<NS>; }
template <int NS> static auto forward_kernel(CoreB16N<NS>) { return msdf_sdf_forward_b16_k<NS>; }
template <int NS> static auto fwd_grad_kernel(CoreB16N<NS>) { return msdf_sdf_fwd_grad_b16_k<NS>; }
template <int NS> static auto backward_kernel(CoreB16N<NS>) { return msdf_sdf_backward_b16_k<NS>; }

extern "C" int msdf_abi_version(void) { return MSDF_ABI_VERSION; }

extern "C" int msdf_pack_weights(const msdf_plan_t* plan, const msdf_packrule_t* rules_dev, const int* maps_dev,
                                 const float* flat_w, const float* flat_b, void* wpack, float* bpack,
                                 void* stream) {
  if (plan == nullptr || plan->n_layers < 1 || plan->n_layers > MSDF_MAX_LAYERS) return MSDF_ERR_ARG;
  return mlp_with_core(plan, [&](auto core) {
    typedef typename decltype(core)::wvec wvec;
    const dim3 grid(32, plan->n_layers, 3);
    pack_kernel(core)<<<grid, 256, 0, (hipStream_t)stream>>>(*plan, rules_dev, maps_dev, flat_w, flat_b, (wvec*)wpack,
                                                             bpack);
    return msdf_check_launch();
  });
}

static bool aux_layout_ok(const msdf_plan_t* plan, const int aux_C, const int aux_LC) {
  if (aux_C == 0) return true;
  return aux_C == 2 && aux_LC > 0 && (aux_LC % aux_C) == 0 &&
         aux_LC <= 16 * plan->aux_tiles;
}

// P_pad: whole workgroups (64 points on every core) that cover the P points
static bool padded_ok(const int P, const int P_pad) { return P_pad >= P && (P_pad % CoreF32::PTS_PER_WG) == 0; }

extern "C" int msdf_sdf_forward_lm(const msdf_plan_t* plan, const void* wpack, const float* bpack, const float* x,
                                   const float* aux, int aux_C, int aux_LC, int P, float clamp_radius,
                                   float sphere_scale, float* sdf, const uint32_t* run_flag, void* stream) {
  if (plan == nullptr || P < 0) return MSDF_ERR_ARG;
  if (P == 0) return MSDF_OK;
  if (plan->aux_tiles > 0 && aux == nullptr) return MSDF_ERR_ARG;
  if (!aux_layout_ok(plan, aux_C, aux_LC)) return MSDF_ERR_ARG;
  return mlp_with_core(plan, [&](auto core) {
    typedef decltype(core) Core;
    if (!Core::AUX_LEVEL_MAJOR && aux_C != 0) return MSDF_ERR_UNSUPPORTED;     // such a core takes rows
    const AuxView av = {aux_C, aux_LC, P};
    return mlp_launch<Core>(forward_kernel(core), (P + Core::PTS_PER_WG - 1) / Core::PTS_PER_WG, stream, *plan,
                            (const typename Core::wvec*)wpack, bpack, x, aux, av, P, clamp_radius, sphere_scale, sdf,
                            run_flag);
  });
}

extern "C" int msdf_sdf_forward_save(const msdf_plan_t* plan, const void* wpack, const float* bpack, const float* x,
                                     const float* aux, int aux_C, int aux_LC, int P, float clamp_radius,
                                     float sphere_scale, float* sdf, const uint32_t* run_flag, float* H, int P_pad,
                                     const int32_t* col_slot, int n_cols, int n_slots, uint32_t* h_saved,
                                     void* stream) {
  if (plan == nullptr || P < 0 || H == nullptr || col_slot == nullptr || h_saved == nullptr) return MSDF_ERR_ARG;
  if (plan->precision != MSDF_PRECISION_F32) return MSDF_ERR_UNSUPPORTED;
  // every saved row ray * n_slots + slot (slot < n_slots) lies inside the P_pad rows of H
  if (n_cols < 1 || n_slots < 1 || n_slots > n_cols || (P % n_cols) != 0 || !padded_ok(0, P_pad) ||
      (int64_t)(P / n_cols) * n_slots > (int64_t)P_pad)
    return MSDF_ERR_ARG;
  if (P == 0) return MSDF_OK;
  if (plan->aux_tiles > 0 && aux == nullptr) return MSDF_ERR_ARG;
  if (!aux_layout_ok(plan, aux_C, aux_LC)) return MSDF_ERR_ARG;
  const AuxView av = {aux_C, aux_LC, P};
  const HSaveArgs hs = {H, P_pad, col_slot, n_cols, n_slots};
  return mlp_launch<CoreF32>(msdf_sdf_forward_save_k, (P + CoreF32::PTS_PER_WG - 1) / CoreF32::PTS_PER_WG, stream, *plan,
                             (const v4f*)wpack, bpack, x, aux, av, P, clamp_radius, sphere_scale, sdf, run_flag, hs,
                             h_saved);
}

extern "C" int msdf_sdf_forward_if(const msdf_plan_t* plan, const void* wpack, const float* bpack, const float* x,
                                   const float* aux, int P, float clamp_radius, float sphere_scale, float* sdf,
                                   const uint32_t* run_flag, void* stream) {
  return msdf_sdf_forward_lm(plan, wpack, bpack, x, aux, 0, 0, P, clamp_radius, sphere_scale, sdf, run_flag, stream);
}

extern "C" int msdf_sdf_forward(const msdf_plan_t* plan, const void* wpack, const float* bpack, const float* x,
                                const float* aux, int P, float clamp_radius, float sphere_scale, float* sdf,
                                void* stream) {
  return msdf_sdf_forward_if(plan, wpack, bpack, x, aux, P, clamp_radius, sphere_scale, sdf, nullptr, stream);
}

extern "C" int msdf_sdf_fwd_grad(const msdf_plan_t* plan, const msdf_fg_args_t* a, void* stream) {
  if (plan == nullptr || a == nullptr || a->P < 0) return MSDF_ERR_ARG;
  if (a->P == 0) return MSDF_OK;
  if (!padded_ok(a->P, a->P_pad)) return MSDF_ERR_ARG;
  if (plan->aux_tiles > 0 && a->aux == nullptr) return MSDF_ERR_ARG;
  if (!aux_layout_ok(plan, a->aux_C, a->aux_LC)) return MSDF_ERR_ARG;
  if (a->dy_dx != nullptr && (a->aux_C != 2 || a->r_aux == nullptr)) return MSDF_ERR_ARG;
  // reused rows are whole workgroups of ray samples: below the rows without features (the eikonal block, which the row
  // map leaves in place -- what keeps the kernel's workgroup-uniform feature test valid in evaluation order)
  if (a->n_reuse < 0 || (a->n_reuse % CoreF32::PTS_PER_WG) != 0 || a->n_reuse > a->P) return MSDF_ERR_ARG;
  if (a->n_reuse > 0 && (a->row_map == nullptr || a->n_reuse > a->n_feat || a->h_stage == nullptr ||
                         a->stage_pad < a->n_reuse))
    return MSDF_ERR_ARG;
  // the dispatch rotation names a workgroup of this launch (eval_wg's single conditional subtraction relies on it)
  if (a->wg_first < 0 || a->wg_first >= a->P_pad / CoreF32::PTS_PER_WG) return MSDF_ERR_ARG;
  return mlp_with_core(plan, [&](auto core) {
    typedef decltype(core) Core;
    if (!Core::AUX_LEVEL_MAJOR && (a->aux_C != 0 || a->dy_dx != nullptr)) return MSDF_ERR_UNSUPPORTED;
    if (!Core::ROW_MAP && a->wg_first != 0) return MSDF_ERR_UNSUPPORTED;
    return mlp_launch<Core>(fwd_grad_kernel(core), a->P_pad / Core::PTS_PER_WG, stream, *plan, *a);
  });
}

extern "C" int msdf_sdf_backward(const msdf_plan_t* plan, const msdf_bw_args_t* a, void* stream) {
  if (plan == nullptr || a == nullptr || a->P < 0) return MSDF_ERR_ARG;
  if (a->P == 0) return MSDF_OK;
  if (!padded_ok(a->P, a->P_pad)) return MSDF_ERR_ARG;
  if (!aux_layout_ok(plan, a->aux_C, a->aux_LC)) return MSDF_ERR_ARG;
  if (a->dy_dx != nullptr && a->aux_C != 2) return MSDF_ERR_ARG;
  return mlp_with_core(plan, [&](auto core) {
    typedef decltype(core) Core;
    if (!Core::AUX_LEVEL_MAJOR && (a->aux_C != 0 || a->dy_dx != nullptr)) return MSDF_ERR_UNSUPPORTED;
    return mlp_launch<Core>(backward_kernel(core), a->P_pad / Core::PTS_PER_WG, stream, *plan, *a);
  });
}
