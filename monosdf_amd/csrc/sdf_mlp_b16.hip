// bf16x3 / bf16x6 variants of the SDF-network kernels (mlp_core_b16.h).  Same plans / slot maps as the fp32
// kernels of sdf_mlp.hip; the plan handed to these kernels carries K-BLOCK counts (32 slots) in
// ktp / otp and 16-byte offsets of the bf16 plane packs (2 or 3 planes) in wf_off / wb_off.
#include "mlp_launch.h"

// flat effective weights -> bf16 plane packs in fragment order, both orientations, + fp32 bias / sdf row
template <int NS>
__global__ void __launch_bounds__(256) msdf_pack_b16_kernel(const msdf_plan_t plan,
                                                            const msdf_packrule_t* __restrict__ rules,
                                                            const int* __restrict__ maps,
                                                            const float* __restrict__ flat_w,
                                                            const float* __restrict__ flat_b,
                                                            v8bf* __restrict__ wpack, float* __restrict__ bpack) {
  const int l = blockIdx.y;
  const int which = blockIdx.z;
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
    const int kbp = which == 0 ? L.ktp : L.otp;         // k blocks in the pack
    const int off = which == 0 ? L.wf_off : L.wb_off;
    const int rt_even = (n_rt + 1) / 2 * 2;
    const int total = rt_even * kbp * 64;
    for (int i = t0; i < total; i += stride) {
      const int lane = i & 63;
      const int blk = i >> 6;
      const int kb = blk % kbp, rt = blk / kbp;
      const int rslot = 16 * rt + (lane & 15);
      v8bf pl[NS];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ktile = 2 * kb + (j >> 2);
        const int kslot = 16 * ktile + 4 * (lane >> 4) + (j & 3);
        float w = 0.f;
        if (rt < n_rt && ktile < n_kt) {
          const int row = which == 0 ? rowmap[rslot] : rowmap[kslot];
          const int col = which == 0 ? colmap[kslot] : colmap[rslot];
          if (row >= 0 && col >= 0) w = R.scale * W[(size_t)row * R.cols + col];
        }
#pragma unroll
        for (int n = 0; n < NS; ++n) {
          const __bf16 h = (__bf16)w;
          pl[n][j] = h;
          w -= (float)h;
        }
      }
      v8bf* dst = wpack + off + ((size_t)(rt * kbp + kb) * NS) * 64 + lane;
#pragma unroll
      for (int n = 0; n < NS; ++n) dst[n * 64] = pl[n];
    }
  } else {
    pack_bias_rows(plan, l, R, rowmap, colmap, W, flat_b, bpack, t0, stride);
  }
}

MLP_B16_KERNEL msdf_sdf_forward_b16_k(const msdf_plan_t plan, const v8bf* __restrict__ wpack, const float* __restrict__ bpack,
                                      const float* __restrict__ x, const float* __restrict__ aux, const AuxView av, const int P,
                                      const float clamp_radius, const float sphere_scale, float* __restrict__ sdf_out,
                                      const uint32_t* __restrict__ run_flag) {
  extern __shared__ v8bf lds16[];
  if (run_flag != nullptr && *run_flag == 0u) return;
  sdf_forward_body<CoreB16N<NS>>(plan, wpack, bpack, x, aux, av, P, clamp_radius, sphere_scale, sdf_out, lds16);
}

MLP_B16_KERNEL msdf_sdf_fwd_grad_b16_k(const msdf_plan_t plan, const FgArgs a) {
  extern __shared__ v8bf lds16[];
  sdf_fwd_grad_body<CoreB16N<NS>>(plan, a, lds16);
}

MLP_B16_KERNEL msdf_sdf_backward_b16_k(const msdf_plan_t plan, const BwArgs a) {
  extern __shared__ v8bf lds16[];
  sdf_backward_body<CoreB16N<NS>>(plan, a, lds16);
}

// what this translation unit exports (declared in mlp_launch.h, launched by the C entry points of sdf_mlp.hip)
#define INSTANTIATE(NS)                                                                                              \
  template __global__ void msdf_pack_b16_kernel<NS>(const msdf_plan_t, const msdf_packrule_t*, const int*, const float*, \
                                                    const float*, v8bf*, float*);                                    \
  template __global__ void msdf_sdf_forward_b16_k<NS>(const msdf_plan_t, const v8bf*, const float*, const float*,    \
                                                      const float*, const AuxView, const int, const float,           \
                                                      const float, float*, const uint32_t*);                         \
  template __global__ void msdf_sdf_fwd_grad_b16_k<NS>(const msdf_plan_t, const FgArgs);                             \
  template __global__ void msdf_sdf_backward_b16_k<NS>(const msdf_plan_t, const BwArgs);
INSTANTIATE(2)
INSTANTIATE(3)
