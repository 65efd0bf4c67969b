// Shared device helpers for the MonoSDF gfx950 kernels (wave64, CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/monosdf_hip.h"

typedef float v4f __attribute__((ext_vector_type(4)));

#define MSDF_WAVE 64

static inline int msdf_check_launch() {
  return hipGetLastError() == hipSuccess ? MSDF_OK : MSDF_ERR_LAUNCH;
}

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

// Wave primitives of the ray-pipeline kernels and the mesh tools.  The order of the shuffle offsets is the summation
// order, which the results depend on bit for bit.  No fp-contract pragma here: each translation unit compiles these
// with its own flags (csrc/Makefile).
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
  return v;
}
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
  const int lane = lane_id();
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(v, d, 64);
    if (lane >= d) v += o;
  }
  return v;
}

// exclusive prefix sum, by scanning the values shifted up one lane.  (inclusive - self would cancel catastrophically
// against the 1e10 * sigma free energy of the last interval)
__device__ __forceinline__ float wave_excl_scan(const float v) {
  float prev = __shfl_up(v, 1, 64);
  if (lane_id() == 0) prev = 0.f;
  return wave_incl_scan(prev);
}
// the same; `total` = sum over the wave
__device__ __forceinline__ float wave_excl_scan(const float v, float& total) {
  const float ex = wave_excl_scan(v);
  total = __shfl(ex, 63, 64) + __shfl(v, 63, 64);
  return ex;
}

// exclusive suffix sum: sum of v over lanes > lane; `total` = sum over the wave.  Built from a shifted
// reverse scan so that a lane with nothing after it gets EXACTLY 0 (total - inclusive would leave
// rounding noise, which the 1e10 last-interval length then multiplies into the sdf / beta gradients).
__device__ __forceinline__ float wave_excl_suffix(const float v, float& total) {
  const int lane = lane_id();
  float s = __shfl_down(v, 1, 64);
  if (lane == 63) s = 0.f;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const float o = __shfl_down(s, d, 64);
    if (lane + d < 64) s += o;
  }
  total = __shfl(s, 0, 64) + __shfl(v, 0, 64);
  return s;
}

__device__ __forceinline__ float sgnf(const float v) { return (v > 0.f) ? 1.f : (v < 0.f) ? -1.f : 0.f; }

// LaplaceDensity.density_func (code/model/density.py:21-30): sigma(s) = (1/beta) (0.5 + 0.5 sign(s) expm1(-|s|/beta))
__device__ __forceinline__ float laplace_density(const float s, const float beta) {
  const float e = expm1f(-fabsf(s) / beta);
  return (1.0f / beta) * (0.5f + 0.5f * sgnf(s) * e);
}

// exp / log on the hardware transcendental unit (v_exp_f32 / v_log_f32, ~1 ulp)
__device__ __forceinline__ float fast_exp(float x) { return __expf(x); }
__device__ __forceinline__ float fast_log(float x) { return __logf(x); }

// nn.Softplus(beta=100, threshold=20): value h, derivative s = sigmoid(100 a)
// (reference: code/model/network.py:77; torch softplus forward/backward semantics).
// Branch-free on purpose (two raw transcendental ops + selects): this runs 64 times per lane per layer
// between matrix products, and divergent control flow there costs more than the arithmetic.
//   log1p(exp(t)) = max(t, 0) + log1p(exp(-|t|)),  e = exp(-|t|) in (0, 1] never overflows.
__device__ __forceinline__ void softplus100(float a, float& h, float& s) {
  const float e = __builtin_amdgcn_exp2f(-fabsf(a * 144.26950408889634f));   // exp(-|100 a|)
  const float ope = 1.0f + e;
  // log1p(e): series below 1e-4 keeps relative accuracy where 1+e rounds to 1
  const float l_series = e * fmaf(e, -0.5f, 1.0f);
  const float l_log = __builtin_amdgcn_logf(ope) * 0.6931471805599453f;      // v_log_f32 is log2
  const float l1p = (e < 1e-4f) ? l_series : l_log;
  const float hv = fmaf(0.01f, l1p, fmaxf(a, 0.0f));
  h = (a * 100.0f > 20.0f) ? a : hv;
  const float r = __builtin_amdgcn_rcpf(ope);
  s = (a >= 0.0f) ? r : e * r;
}

// from a saved post-activation h = softplus100(a) >= 0: u = 1 - sigmoid(100 a) = exp(-100 h)
__device__ __forceinline__ float one_minus_sigmoid_from_h(float h) {
  return __builtin_amdgcn_exp2f(h * -144.26950408889634f);
}

// butterfly sum over the 4 lanes {l, l^16, l^32, l^48} (same point, different k-quarter)
__device__ __forceinline__ float sum_over_quarters(float v) {
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

// sum over the 16 lanes sharing the same quarter (the 16 points of a wave tile)
__device__ __forceinline__ float sum_over_points16(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  v += __shfl_xor(v, 4, 64);
  v += __shfl_xor(v, 8, 64);
  return v;
}
