// Multi-resolution hash-grid encoder for gfx950: forward (+ dy/dx), grid backward,
// input backward and the two second-order kernels.
//
// Same arithmetic as the reference's CUDA kernels (code/hashencoder/src/hashencoder.cu:
// index function 35-72, kernel_grid 103-254, kernel_grid_backward 257-343,
// kernel_input_backward 346-372, kernel_grid_second_backward_grad 375-428,
// kernel_grid_second_backward_embedding 431-595), written for wave64: one lane per
// (point, level), level-major launch so that a level's table slice (<= 4 MiB) is the
// working set of the blocks in flight, the 8 corner reads of a point reused for the
// output AND its three directional derivatives (the reference gathers them twice),
// [L,B,C] output rows written as 8-byte-per-lane coalesced stores.
// Layouts are the reference's: inputs [B,3] in [0,1], embeddings [n,C], offsets int32 [L+1],
// outputs [L,B,C], dy_dx [B, L*3*C].  fp32 only (the reference's fp16 path is dead code).
#include "common.h"
#include <cstdlib>

#define HG_THREADS 256

struct HgCell {
  float scale;
  uint32_t gx, gy, gz;
  float sx, sy, sz;       // smoothstep(frac)
  float dx, dy, dz;       // smoothstep'(frac)
  bool oob;
};

// scale and resolution of a level, on the host as in the kernels (hg_small_levels sizes the LDS tables with it)
struct HgRes {
  float scale;
  uint32_t res;
};
__host__ __device__ __forceinline__ HgRes hg_resolution(const uint32_t level, const float S, const uint32_t H) {
  HgRes r;
  // exp2f(level * S) as the correctly rounded float (device exp2f is only ~1 ulp; one ulp of scale moves a
  // fine-level sample by 1e-4 of a cell)
  r.scale = (float)exp2((double)((float)level * S)) * (float)H - 1.0f;
  r.res = (uint32_t)ceilf(r.scale) + 1u;
  return r;
}

// per-level constants (scale, resolution, table size): uniform over a workgroup of the level-major launches.
// The reference decides the index form per corner (cu:54-72): a loop over the three axes adds p[d] * stride and
// multiplies the 32-bit running stride by the resolution while that stride still fits the level (stride <= hsize);
// if the stride has outgrown the level at the end, the index is the xor hash px ^ py * 2654435761 ^ pz * 805459861
// instead; either way it is taken modulo hsize.  The same loop runs here with the coordinates left out, once per
// level instead of once per corner: `dense` = the running stride never exceeds the table (index = x + y res +
// z res^2), otherwise the xor hash; `mask` = hsize - 1 when the table size is a power of two (every hashed level of
// the reference's configurations: the modulo becomes an AND instead of a ~40-instruction integer division per corner).
struct HgLevel {
  float scale;
  uint32_t res, hsize;
  uint32_t s1, s2, mask;
  bool dense;
};
__device__ __forceinline__ HgLevel hg_level(const int* __restrict__ offsets, const uint32_t level, const float S,
                                            const uint32_t H) {
  HgLevel v;
  v.hsize = (uint32_t)(offsets[level + 1] - offsets[level]);
  const HgRes r = hg_resolution(level, S, H);
  v.scale = r.scale;
  v.res = r.res;
  // which strides are taken, and whether the last one fits
  uint32_t stride = 1;
  v.s1 = v.s2 = 0;
  if (stride <= v.hsize) stride *= v.res;                        // d = 0 (stride 1)
  if (stride <= v.hsize) { v.s1 = stride; stride *= v.res; }     // d = 1
  if (stride <= v.hsize) { v.s2 = stride; stride *= v.res; }     // d = 2
  v.dense = !(stride > v.hsize);
  v.mask = ((v.hsize & (v.hsize - 1u)) == 0u) ? v.hsize - 1u : 0u;
  return v;
}

// the table entry of grid point (px, py, pz): the reference's index with the level's decisions taken from HgLevel
__device__ __forceinline__ uint32_t hg_index_lv(const HgLevel& lv, const uint32_t px, const uint32_t py,
                                                const uint32_t pz) {
  uint32_t index;
  if (lv.dense) index = px + py * lv.s1 + pz * lv.s2;
  else index = px ^ (py * 2654435761u) ^ (pz * 805459861u);
  if (lv.mask) return index & lv.mask;
  return (index < lv.hsize) ? index : index % lv.hsize;     // same value; dense levels skip the division
}

__device__ __forceinline__ HgCell hg_locate_xyz(const float x, const float y, const float z, const HgLevel& lv) {
  HgCell c;
  c.oob = (x < 0.f || x > 1.f || y < 0.f || y > 1.f || z < 0.f || z > 1.f);
  c.scale = lv.scale;
  float px = x * c.scale, py = y * c.scale, pz = z * c.scale;
  const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
  c.gx = (uint32_t)fx; c.gy = (uint32_t)fy; c.gz = (uint32_t)fz;
  px -= fx; py -= fy; pz -= fz;
  c.dx = 6.f * px * (1.f - px); c.dy = 6.f * py * (1.f - py); c.dz = 6.f * pz * (1.f - pz);
  c.sx = px * px * (3.f - 2.f * px); c.sy = py * py * (3.f - 2.f * py); c.sz = pz * pz * (3.f - 2.f * pz);
  return c;
}

__device__ __forceinline__ HgCell hg_locate(const float* __restrict__ inputs, const HgLevel& lv, const uint32_t b) {
  return hg_locate_xyz(inputs[(size_t)b * 3 + 0], inputs[(size_t)b * 3 + 1], inputs[(size_t)b * 3 + 2], lv);
}

// Corner k of a cell is the grid point (gx + (k & 1), gy + ((k >> 1) & 1), gz + ((k >> 2) & 1)): its table entry ...
__device__ __forceinline__ uint32_t hg_corner_index(const HgLevel& lv, const HgCell& c, const int k) {
  return hg_index_lv(lv, c.gx + (k & 1), c.gy + ((k >> 1) & 1), c.gz + ((k >> 2) & 1));
}

// ... and what it weighs, from the per-axis weights wx, wy, wz = {1 - smoothstep, smoothstep} of the cell.  k is a
// compile-time constant wherever these functions are called (unrolled loops), so the arrays are registers.  The
// association and order of every product and sum here is what the values of the table gradient are made of:
// hashgrid.o is built with -ffp-contract=off.
// w_k, the trilinear weight                                           (kernel_grid, kernel_grid_backward, cu:257-343)
__device__ __forceinline__ float hg_corner_weight(const float (&wx)[2], const float (&wy)[2], const float (&wz)[2],
                                                  const int k) {
  return wx[k & 1] * wy[(k >> 1) & 1] * wz[(k >> 2) & 1];
}
// the second-order coefficient: sum over axes of +/- the other axes' weights * q_d, q_d = gg_d * smoothstep'_d * scale
//                                                                     (kernel_grid_second_backward_embedding, cu:431-595)
__device__ __forceinline__ float hg_corner_coefficient(const float (&wx)[2], const float (&wy)[2], const float (&wz)[2],
                                                       const float q0, const float q1, const float q2, const int k) {
  const int bx = k & 1, by = (k >> 1) & 1, bz = (k >> 2) & 1;
  return (bx ? 1.f : -1.f) * wy[by] * wz[bz] * q0 + (by ? 1.f : -1.f) * wx[bx] * wz[bz] * q1 +
         (bz ? 1.f : -1.f) * wx[bx] * wy[by] * q2;
}
// what one channel adds to corner k of the table gradient, from wk = hg_corner_weight and qk = hg_corner_coefficient
// formed once per corner (the one a MODE does not read is dead code).  MODE 0: w_k * grad;  MODE 1: coefficient * grad;
// MODE 2: w_k * grad + coefficient * grad2, both table gradients in one pass
template <int MODE>
__device__ __forceinline__ float hg_corner_value(const float wk, const float qk, const float g1, const float g2) {
  if (MODE == 0) return wk * g1;
  if (MODE == 1) return qk * g1;
  return wk * g1 + qk * g2;
}
// the operands of the three functions above for one cell; gg: the point's three gg_inputs, NULL where no second-order
// term is formed.  (hb2_place_k keeps them as plain locals: see there.)
struct HgCorners {
  float wx[2], wy[2], wz[2];
  float q0 = 0.f, q1 = 0.f, q2 = 0.f;
  __device__ __forceinline__ HgCorners(const HgCell& c, const float* __restrict__ gg)
      : wx{1.f - c.sx, c.sx}, wy{1.f - c.sy, c.sy}, wz{1.f - c.sz, c.sz} {
    if (gg != nullptr) {
      q0 = gg[0] * c.dx * c.scale;
      q1 = gg[1] * c.dy * c.scale;
      q2 = gg[2] * c.dz * c.scale;
    }
  }
  __device__ __forceinline__ float weight(const int k) const { return hg_corner_weight(wx, wy, wz, k); }
  __device__ __forceinline__ float coefficient(const int k) const {
    return hg_corner_coefficient(wx, wy, wz, q0, q1, q2, k);
  }
};

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
// one (point, level): the 8 corner reads feed the output and its three directional derivatives
template <int C>
__device__ __forceinline__ void hg_forward_cell(const HgCell& c, const float* __restrict__ grid,
                                                const int* __restrict__ offsets, float* __restrict__ out,
                                                const HgLevel& lv, const uint32_t level, const int calc_grad_inputs,
                                                float* __restrict__ dy) {
  if (c.oob) {
#pragma unroll
    for (int ch = 0; ch < C; ++ch) out[ch] = 0.f;
    if (calc_grad_inputs) {
#pragma unroll
      for (int k = 0; k < 3 * C; ++k) dy[k] = 0.f;
    }
    return;
  }
  const float* table = grid + (size_t)(uint32_t)offsets[level] * C;
  // gather the 8 corners once
  float v[8][C];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const uint32_t idx = hg_corner_index(lv, c, k);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) v[k][ch] = table[(size_t)idx * C + ch];
  }
  const float wx[2] = {1.f - c.sx, c.sx}, wy[2] = {1.f - c.sy, c.sy}, wz[2] = {1.f - c.sz, c.sz};
  float res[C];
#pragma unroll
  for (int ch = 0; ch < C; ++ch) res[ch] = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float w = hg_corner_weight(wx, wy, wz, k);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) res[ch] += w * v[k][ch];
  }
#pragma unroll
  for (int ch = 0; ch < C; ++ch) out[ch] = res[ch];
  if (calc_grad_inputs) {
    // d/dx: pairs differing in bit 0; weights of the other two axes; times scale * smoothstep'
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        const int a = m & 1, bq = (m >> 1) & 1;
        gx += (c.scale * wy[a] * wz[bq]) * (v[1 | (a << 1) | (bq << 2)][ch] - v[0 | (a << 1) | (bq << 2)][ch]) * c.dx;
        gy += (c.scale * wx[a] * wz[bq]) * (v[a | 2 | (bq << 2)][ch] - v[a | 0 | (bq << 2)][ch]) * c.dy;
        gz += (c.scale * wx[a] * wy[bq]) * (v[a | (bq << 1) | 4][ch] - v[a | (bq << 1) | 0][ch]) * c.dz;
      }
      dy[0 * C + ch] = gx;
      dy[1 * C + ch] = gy;
      dy[2 * C + ch] = gz;
    }
  }
}

template <int C>
__global__ void __launch_bounds__(HG_THREADS)
hg_forward_kernel(const float* __restrict__ inputs, const float* __restrict__ grid, const int* __restrict__ offsets,
                  float* __restrict__ outputs, const uint32_t B, const uint32_t L, const float S, const uint32_t H,
                  const int calc_grad_inputs, float* __restrict__ dy_dx) {
  const uint32_t b = blockIdx.x * HG_THREADS + threadIdx.x;
  if (b >= B) return;
  const uint32_t level = blockIdx.y;
  const HgLevel lv = hg_level(offsets, level, S, H);
  float* out = outputs + ((size_t)level * B + b) * C;
  // calc_grad_inputs == 2: dy_dx level-major [L, B, 3 C] (a wave writes 64 x 3 C contiguous floats) instead of the
  // reference's [B, L, 3 C] (3 C floats every L 3 C: partial lines written by 16 different launches' blocks)
  float* dy = (calc_grad_inputs == 2) ? dy_dx + ((size_t)level * B + b) * 3 * C
                                      : dy_dx + (size_t)b * 3 * L * C + (size_t)level * 3 * C;
  hg_forward_cell<C>(hg_locate(inputs, lv, b), grid, offsets, out, lv, level, calc_grad_inputs, dy);
}

// ---------------------------------------------------------------------------
// "Node" forms (ops.GridSdfFunction, the sampler's evaluations): the same arithmetic with the tensors laid out as
// the fused MLP kernels read and write them, and the elementwise steps around the encoder done here instead of as
// PyTorch launches:
//   * points arrive in world coordinates; x01 = (x * inv_divide + 1) * 0.5 is formed per lane exactly as the
//     module's tensor expression rounds it (a multiply by the reciprocal -- formed in double, rounded to fp32 --
//     an add, a multiply) and stored once;
//   * features, d sdf / d features and their gradients: pitch == 0 keeps the kernels' own level-major [L, B, C] layout
//     (coalesced: a wave touches 64 C contiguous floats); pitch > 0: point-major rows of `pitch` floats ([B, pitch],
//     level l channel c at column l C + c, columns >= L C zeroed), the layout of the fused SDF kernels' input tiles.
//     Point-major is free in the two small kernels (hg_node_input_gradient / hg_node_second_grad) and costly in the
//     two large ones (8-byte pieces at a 128-byte stride: forward 0.115 -> 0.148 ms per step, the scatter 0.120 ->
//     0.163), so ops.GridSdfFunction uses it for the former and msdf_hash_transpose (LDS tiles, both sides coalesced)
//     around the latter -- instead of five strided tensor copies of 11-48 us per training step.
// ---------------------------------------------------------------------------
template <int C>
__global__ void __launch_bounds__(HG_THREADS)
hg_node_forward_kernel(const float* __restrict__ x, const float inv_divide, float* __restrict__ x01_out,
                       const float* __restrict__ grid, const int* __restrict__ offsets, float* __restrict__ feat,
                       const uint32_t pitch, const uint32_t B, const uint32_t L, const float S, const uint32_t H,
                       float* __restrict__ dy_dx) {
  const uint32_t b = blockIdx.x * HG_THREADS + threadIdx.x;
  if (b >= B) return;
  const uint32_t level = blockIdx.y;
  const HgLevel lv = hg_level(offsets, level, S, H);
  const float u0 = (x[(size_t)b * 3 + 0] * inv_divide + 1.0f) * 0.5f;
  const float u1 = (x[(size_t)b * 3 + 1] * inv_divide + 1.0f) * 0.5f;
  const float u2 = (x[(size_t)b * 3 + 2] * inv_divide + 1.0f) * 0.5f;
  if (level == 0) {
    if (x01_out != nullptr) {
      x01_out[(size_t)b * 3 + 0] = u0; x01_out[(size_t)b * 3 + 1] = u1; x01_out[(size_t)b * 3 + 2] = u2;
    }
    for (uint32_t k = L * C; k < pitch; ++k) feat[(size_t)b * pitch + k] = 0.f;
  }
  float* dy = (dy_dx != nullptr) ? dy_dx + ((size_t)level * B + b) * 3 * C : nullptr;
  float* out = pitch ? feat + (size_t)b * pitch + level * C : feat + ((size_t)level * B + b) * C;
  hg_forward_cell<C>(hg_locate_xyz(u0, u1, u2, lv), grid, offsets, out, lv, level, dy != nullptr ? 2 : 0, dy);
}

// inout[b,d] += scale * sum_{l,c} g[b, l C + c] * dy_dx[l,b,d,c]   (the grid part of d sdf / d x, chain rule factor in)
// One thread per (point, input dimension) -- consecutive lanes read consecutive 8-byte (C = 2) pieces of dy_dx and write
// consecutive floats; the sum over (level, channel) runs in the reference's order (hashencoder.cu:347-372, also one thread per (b, d)).
template <int C>
__global__ void __launch_bounds__(HG_THREADS)
hg_node_input_gradient_kernel(const float* __restrict__ g, const uint32_t pitch, const float* __restrict__ dy_dx,
                              const uint32_t B, const uint32_t L, const float scale, float* __restrict__ inout) {
  const uint32_t t = blockIdx.x * HG_THREADS + threadIdx.x;
  if (t >= 3 * B) return;
  const uint32_t b = t / 3, d = t - 3 * b;
  float r = 0.f;
#pragma unroll 8
  for (uint32_t l = 0; l < L; ++l) {
    const float* dy = dy_dx + ((size_t)l * B + b) * 3 * C + d * C;
    const float* gp = pitch ? g + (size_t)b * pitch + l * C : g + ((size_t)l * B + b) * C;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) r += gp[ch] * dy[ch];
  }
  inout[t] += r * scale;      // the rounded product, then the sum (as the tensor expression nrm + through * k rounds them)
}

// gg[b] = scale * (b < n_split ? g_a[b] : g_b[b - n_split])  (a missing part is zero), stored once;
// grad_grad[b, l C + c] = sum_d gg[b,d] * dy_dx[l,b,d,c]
template <int C>
__global__ void __launch_bounds__(HG_THREADS)
hg_node_second_grad_kernel(const float* __restrict__ g_a, const float* __restrict__ g_b, const uint32_t n_split,
                           const float scale, float* __restrict__ gg_out, const float* __restrict__ dy_dx,
                           float* __restrict__ grad_grad, const uint32_t pitch, const uint32_t B, const uint32_t L) {
  const uint32_t b = blockIdx.x * HG_THREADS + threadIdx.x;
  if (b >= B) return;
  const uint32_t level = blockIdx.y;
  const float* src = (b < n_split) ? g_a : g_b;
  const size_t j = (b < n_split) ? b : b - n_split;
  float g0 = 0.f, g1 = 0.f, g2 = 0.f;
  if (src != nullptr) { g0 = src[j * 3 + 0] * scale; g1 = src[j * 3 + 1] * scale; g2 = src[j * 3 + 2] * scale; }
  if (level == 0) {
    gg_out[(size_t)b * 3 + 0] = g0; gg_out[(size_t)b * 3 + 1] = g1; gg_out[(size_t)b * 3 + 2] = g2;
    for (uint32_t k = L * C; k < pitch; ++k) grad_grad[(size_t)b * pitch + k] = 0.f;
  }
  const float* dy = dy_dx + ((size_t)level * B + b) * 3 * C;
  float* out = pitch ? grad_grad + (size_t)b * pitch + level * C : grad_grad + ((size_t)level * B + b) * C;
#pragma unroll
  for (int ch = 0; ch < C; ++ch) out[ch] = g0 * dy[0 * C + ch] + g1 * dy[1 * C + ch] + g2 * dy[2 * C + ch];
}

#include "hash_scatter.h"     // the table-gradient scatter: its kernels and hg_table_gradient

// grad_inputs[b,d] = sum_{l,c} grad[l,b,c] * dy_dx[b,l,d,c]
template <int C>
__global__ void __launch_bounds__(HG_THREADS)
hg_backward_input_kernel(const float* __restrict__ grad, const float* __restrict__ dy_dx,
                         float* __restrict__ grad_inputs, const uint32_t B, const uint32_t L, const int level_major) {
  const uint32_t b = blockIdx.x * HG_THREADS + threadIdx.x;
  if (b >= B) return;
  float r0 = 0.f, r1 = 0.f, r2 = 0.f;
  for (uint32_t l = 0; l < L; ++l) {
    const float* dy = level_major ? dy_dx + ((size_t)l * B + b) * 3 * C : dy_dx + (size_t)b * L * 3 * C + l * 3 * C;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
      const float g = grad[((size_t)l * B + b) * C + ch];
      r0 += g * dy[0 * C + ch];
      r1 += g * dy[1 * C + ch];
      r2 += g * dy[2 * C + ch];
    }
  }
  grad_inputs[(size_t)b * 3 + 0] = r0;
  grad_inputs[(size_t)b * 3 + 1] = r1;
  grad_inputs[(size_t)b * 3 + 2] = r2;
}

// grad_grad[l,b,c] = sum_d gg_inputs[b,d] * dy_dx[b,l,d,c]
template <int C>
__global__ void __launch_bounds__(HG_THREADS)
hg_second_backward_grad_kernel(const float* __restrict__ gg_inputs, const float* __restrict__ dy_dx,
                               float* __restrict__ grad_grad, const uint32_t B, const uint32_t L,
                               const int level_major) {
  const uint32_t b = blockIdx.x * HG_THREADS + threadIdx.x;
  if (b >= B) return;
  const uint32_t level = blockIdx.y;
  const float g0 = gg_inputs[(size_t)b * 3 + 0], g1 = gg_inputs[(size_t)b * 3 + 1], g2 = gg_inputs[(size_t)b * 3 + 2];
  const float* dy = level_major ? dy_dx + ((size_t)level * B + b) * 3 * C
                                : dy_dx + (size_t)b * L * 3 * C + (size_t)level * 3 * C;
#pragma unroll
  for (int ch = 0; ch < C; ++ch)
    grad_grad[((size_t)level * B + b) * C + ch] = g0 * dy[0 * C + ch] + g1 * dy[1 * C + ch] + g2 * dy[2 * C + ch];
}

// ---------------------------------------------------------------------------
// C-ABI (mirrors hash_encode_forward / _backward / _second_backward of
// code/hashencoder/src/hashencoder.h:13-15, same argument order, raw device pointers).  Return codes of the entry
// points that read the table or its Jacobian: the second table of the hash-grid block of include/monosdf_hip.h.
// ---------------------------------------------------------------------------
#define HG_DISPATCH_C(C, ...)                                    \
  switch (C) {                                                   \
    case 1: { constexpr int CC = 1; __VA_ARGS__; } break;        \
    case 2: { constexpr int CC = 2; __VA_ARGS__; } break;        \
    case 4: { constexpr int CC = 4; __VA_ARGS__; } break;        \
    case 8: { constexpr int CC = 8; __VA_ARGS__; } break;        \
    default: return MSDF_ERR_UNSUPPORTED;                        \
  }

extern "C" int msdf_hash_encode_forward(const float* inputs, const float* embeddings, const int* offsets,
                                        float* outputs, uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S,
                                        uint32_t H, int calc_grad_inputs, float* dy_dx, void* stream) {
  if (D != 3) return MSDF_ERR_UNSUPPORTED;   // the reference also accepts D=2; this path only uses 3
  if (B == 0) return MSDF_OK;
  if (inputs == nullptr || embeddings == nullptr || offsets == nullptr || outputs == nullptr ||
      (calc_grad_inputs && dy_dx == nullptr))
    return MSDF_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((B + HG_THREADS - 1) / HG_THREADS, L);
  HG_DISPATCH_C(C, (hg_forward_kernel<CC><<<grid, HG_THREADS, 0, st>>>(inputs, embeddings, offsets, outputs, B, L, S,
                                                                       H, calc_grad_inputs, dy_dx)));
  return msdf_check_launch();
}

// ---------------------------------------------------------------------------
// The seven table-gradient entry points: each its own argument contract, one HG_DISPATCH_C around hg_table_gradient
// (hash_scatter.h), then its small companion kernel.  Return codes and the order in which they are tested: the table
// above the hash-grid block of include/monosdf_hip.h.  A refusal launches nothing.
// ---------------------------------------------------------------------------
static bool hg_channels_ok(const uint32_t C, const bool second_order) {
  // the reference has no C=1 second backward either (cu:678-684)
  return (C == 1 && !second_order) || C == 2 || C == 4 || C == 8;
}

// msdf_hash_encode_backward / _ws: t says atomic or binned; a NULL grad_embeddings skips the table gradient
static int hg_backward(HgTableGrad t, const float* grad, const float* inputs, const int* offsets, float* grad_embeddings,
                       uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, int calc_grad_inputs,
                       const float* dy_dx, float* grad_inputs, hipStream_t st) {
  if (D != 3 || !hg_channels_ok(C, false)) return MSDF_ERR_UNSUPPORTED;
  if (B == 0) return MSDF_OK;
  if (calc_grad_inputs && (grad == nullptr || dy_dx == nullptr || grad_inputs == nullptr)) return MSDF_ERR_ARG;
  t.grad_first = grad;
  HG_DISPATCH_C(C, {
    const int rc = grad_embeddings ? hg_table_gradient<CC>(t, inputs, offsets, grad_embeddings, B, L, S, H, st) : MSDF_OK;
    if (rc != MSDF_OK) return rc;
    if (calc_grad_inputs)
      hg_backward_input_kernel<CC><<<(B + HG_THREADS - 1) / HG_THREADS, HG_THREADS, 0, st>>>(grad, dy_dx, grad_inputs, B, L,
                                                                                             calc_grad_inputs == 2);
  });
  return msdf_check_launch();
}

// msdf_hash_encode_second_backward / _ws: a NULL grad_grad or grad2_embeddings skips that output
static int hg_second_backward(HgTableGrad t, const float* grad, const float* inputs, const int* offsets, uint32_t B,
                              uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, int calc_grad_inputs,
                              const float* dy_dx, const float* grad_grad_inputs, float* grad_grad,
                              float* grad2_embeddings, hipStream_t st) {
  if (D != 3 || !hg_channels_ok(C, true)) return MSDF_ERR_UNSUPPORTED;
  if (B == 0) return MSDF_OK;
  if (grad_grad != nullptr && (grad_grad_inputs == nullptr || dy_dx == nullptr)) return MSDF_ERR_ARG;
  t.grad_second = grad;
  t.gg_inputs = grad_grad_inputs;
  HG_DISPATCH_C(C, {
    const int rc = grad2_embeddings ? hg_table_gradient<CC>(t, inputs, offsets, grad2_embeddings, B, L, S, H, st) : MSDF_OK;
    if (rc != MSDF_OK) return rc;
    if (grad_grad != nullptr)
      hg_second_backward_grad_kernel<CC><<<dim3((B + HG_THREADS - 1) / HG_THREADS, L), HG_THREADS, 0, st>>>(
          grad_grad_inputs, dy_dx, grad_grad, B, L, calc_grad_inputs == 2);
  });
  return msdf_check_launch();
}

// msdf_hash_encode_backward_fused / _fused_out / msdf_hash_node_scatter: both terms in ONE binned scatter,
//   grad_embeddings (+)= sum_k [ w_k * grad_first[l,b,c] + coef_k(grad_grad_inputs[b]) * grad_second[l,b,c] ]
// (the sum of what msdf_hash_encode_backward and msdf_hash_encode_second_backward add for the same points).
// empty_null: the operands of an empty point set may be NULL (empty tensors have no storage)
static int hg_fused(const HgTableGrad& t, const float* inputs, const int* offsets, float* grad_embeddings, uint32_t B,
                    uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H, bool empty_null, hipStream_t st) {
  if (D != 3 || !hg_channels_ok(C, true)) return MSDF_ERR_UNSUPPORTED;
  const bool operands = t.grad_first != nullptr && t.grad_second != nullptr && t.gg_inputs != nullptr;
  if (grad_embeddings == nullptr || (!operands && !(empty_null && B == 0))) return MSDF_ERR_ARG;
  HG_DISPATCH_C(C, {
    const int rc = hg_table_gradient<CC>(t, inputs, offsets, grad_embeddings, B, L, S, H, st);
    if (rc != MSDF_OK) return rc;
  });
  return msdf_check_launch();
}

extern "C" int msdf_hash_encode_backward(const float* grad, const float* inputs, const float* embeddings,
                                         const int* offsets, float* grad_embeddings, uint32_t B, uint32_t D,
                                         uint32_t C, uint32_t L, float S, uint32_t H, int calc_grad_inputs,
                                         const float* dy_dx, float* grad_inputs, void* stream) {
  (void)embeddings;
  return hg_backward(HgTableGrad{}, grad, inputs, offsets, grad_embeddings, B, D, C, L, S, H, calc_grad_inputs, dy_dx,
                     grad_inputs, (hipStream_t)stream);
}

extern "C" int msdf_hash_encode_second_backward(const float* grad, const float* inputs, const float* embeddings,
                                                const int* offsets, uint32_t B, uint32_t D, uint32_t C, uint32_t L,
                                                float S, uint32_t H, int calc_grad_inputs, const float* dy_dx,
                                                const float* grad_grad_inputs, float* grad_grad,
                                                float* grad2_embeddings, void* stream) {
  (void)embeddings;
  return hg_second_backward(HgTableGrad{}, grad, inputs, offsets, B, D, C, L, S, H, calc_grad_inputs, dy_dx,
                            grad_grad_inputs, grad_grad, grad2_embeddings, (hipStream_t)stream);
}

extern "C" int64_t msdf_hash_scatter_workspace_bytes(uint32_t B, uint32_t C, uint32_t L, uint64_t n_entries) {
  const size_t a = hb_layout(B, C, L, n_entries).total_bytes, b = hb2_layout(B, C, L, n_entries).total_bytes;
  return (int64_t)(a > b ? a : b);
}

// a binned request; the reference-order entries fill in their one operand themselves
static HgTableGrad hg_binned(const float* grad_first, const float* grad_second, const float* gg_inputs, uint32_t pitch,
                             bool overwrite, uint64_t n_entries, void* workspace, uint64_t workspace_bytes) {
  return HgTableGrad{grad_first, grad_second, gg_inputs, pitch, overwrite, true, n_entries, workspace, (size_t)workspace_bytes};
}

extern "C" int msdf_hash_encode_backward_ws(const float* grad, const float* inputs, const float* embeddings,
                                            const int* offsets, float* grad_embeddings, uint32_t B, uint32_t D,
                                            uint32_t C, uint32_t L, float S, uint32_t H, int calc_grad_inputs,
                                            const float* dy_dx, float* grad_inputs, uint64_t n_entries,
                                            void* workspace, uint64_t workspace_bytes, void* stream) {
  (void)embeddings;
  return hg_backward(hg_binned(nullptr, nullptr, nullptr, 0, false, n_entries, workspace, workspace_bytes), grad, inputs, offsets,
                     grad_embeddings, B, D, C, L, S, H, calc_grad_inputs, dy_dx, grad_inputs, (hipStream_t)stream);
}

extern "C" int msdf_hash_encode_second_backward_ws(const float* grad, const float* inputs, const float* embeddings,
                                                   const int* offsets, uint32_t B, uint32_t D, uint32_t C,
                                                   uint32_t L, float S, uint32_t H, int calc_grad_inputs,
                                                   const float* dy_dx, const float* grad_grad_inputs,
                                                   float* grad_grad, float* grad2_embeddings, uint64_t n_entries,
                                                   void* workspace, uint64_t workspace_bytes, void* stream) {
  (void)embeddings;
  return hg_second_backward(hg_binned(nullptr, nullptr, nullptr, 0, false, n_entries, workspace, workspace_bytes), grad, inputs,
                            offsets, B, D, C, L, S, H, calc_grad_inputs, dy_dx, grad_grad_inputs, grad_grad,
                            grad2_embeddings, (hipStream_t)stream);
}

extern "C" int msdf_hash_encode_backward_fused(const float* grad_first, const float* grad_second, const float* inputs,
                                               const int* offsets, float* grad_embeddings, uint32_t B, uint32_t D,
                                               uint32_t C, uint32_t L, float S, uint32_t H,
                                               const float* grad_grad_inputs, uint64_t n_entries, void* workspace,
                                               uint64_t workspace_bytes, void* stream) {
  return hg_fused(hg_binned(grad_first, grad_second, grad_grad_inputs, 0, false, n_entries, workspace, workspace_bytes), inputs,
                  offsets, grad_embeddings, B, D, C, L, S, H, false, (hipStream_t)stream);
}

// the same with "=" instead of "+=": grad_embeddings need not be initialised (no 48.8 MB fill before the call, no
// read of the table inside it)
extern "C" int msdf_hash_encode_backward_fused_out(const float* grad_first, const float* grad_second,
                                                   const float* inputs, const int* offsets, float* grad_embeddings,
                                                   uint32_t B, uint32_t D, uint32_t C, uint32_t L, float S, uint32_t H,
                                                   const float* grad_grad_inputs, uint64_t n_entries, void* workspace,
                                                   uint64_t workspace_bytes, void* stream) {
  return hg_fused(hg_binned(grad_first, grad_second, grad_grad_inputs, 0, true, n_entries, workspace, workspace_bytes), inputs,
                  offsets, grad_embeddings, B, D, C, L, S, H, false, (hipStream_t)stream);
}

// [L, B, C] <-> [B, pitch] (level l, channel c of a point at column l C + c; columns >= L C zero) through an LDS tile
// of 64 points: both the level-major side (64 C contiguous floats per level) and the point-major side (whole rows)
// move as contiguous runs.  Up to two tensors of the same shape per launch.
#define HT_PTS 64
template <bool TO_PM>
__global__ void __launch_bounds__(256)
hg_transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, const float* __restrict__ src2,
                    float* __restrict__ dst2, const uint32_t L, const uint32_t B, const uint32_t C,
                    const uint32_t pitch) {
  extern __shared__ float ht_tile[];                 // [HT_PTS][LC + 1]
  const uint32_t LC = L * C, ld = LC + 1;
  const uint32_t b0 = blockIdx.x * HT_PTS;
  const float* in = blockIdx.y ? src2 : src;
  float* out = blockIdx.y ? dst2 : dst;
  const uint32_t n_pts = min((uint32_t)HT_PTS, B - b0);
  if (TO_PM) {
    for (uint32_t i = threadIdx.x; i < L * n_pts * C; i += 256) {          // level-major reads: runs of n_pts * C floats
      const uint32_t l = i / (n_pts * C), r = i - l * (n_pts * C);
      ht_tile[(r / C) * ld + l * C + (r % C)] = in[((size_t)l * B + b0) * C + r];
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n_pts * pitch; i += 256) {          // rows out
      const uint32_t p = i / pitch, k = i - p * pitch;
      out[(size_t)(b0 + p) * pitch + k] = (k < LC) ? ht_tile[p * ld + k] : 0.f;
    }
  } else {
    for (uint32_t i = threadIdx.x; i < n_pts * LC; i += 256) {             // rows in
      const uint32_t p = i / LC, k = i - p * LC;
      ht_tile[p * ld + k] = in[(size_t)(b0 + p) * pitch + k];
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < L * n_pts * C; i += 256) {
      const uint32_t l = i / (n_pts * C), r = i - l * (n_pts * C);
      out[((size_t)l * B + b0) * C + r] = ht_tile[(r / C) * ld + l * C + (r % C)];
    }
  }
}

extern "C" int msdf_hash_transpose(const float* src, float* dst, const float* src2, float* dst2, uint32_t L,
                                   uint32_t B, uint32_t C, uint32_t pitch, int to_point_major, void* stream) {
  if (B == 0) return MSDF_OK;          // an empty point set has NULL tensors (empty CUDA tensors have no storage)
  if (src == nullptr || dst == nullptr || (src2 == nullptr) != (dst2 == nullptr) || pitch < L * C || L * C == 0)
    return MSDF_ERR_ARG;
  const size_t lds = (size_t)HT_PTS * (L * C + 1) * sizeof(float);
  if (lds > 64 * 1024) return MSDF_ERR_UNSUPPORTED;
  const dim3 grid((B + HT_PTS - 1) / HT_PTS, src2 != nullptr ? 2 : 1);
  if (to_point_major) hg_transpose_kernel<true><<<grid, 256, lds, (hipStream_t)stream>>>(src, dst, src2, dst2, L, B, C, pitch);
  else hg_transpose_kernel<false><<<grid, 256, lds, (hipStream_t)stream>>>(src, dst, src2, dst2, L, B, C, pitch);
  return msdf_check_launch();
}

// ---- node forms (see hg_node_forward_kernel) ----
extern "C" int msdf_hash_node_forward(const float* x, double divide_factor, float* x01_out, const float* embeddings,
                                      const int* offsets, float* feat, uint32_t pitch, uint32_t B, uint32_t C,
                                      uint32_t L, float S, uint32_t H, float* dy_dx, void* stream) {
  if (B == 0) return MSDF_OK;          // as msdf_hash_encode_forward: nothing to do, NULL tensors allowed
  if ((pitch != 0 && pitch < L * C) || x == nullptr || feat == nullptr || embeddings == nullptr || offsets == nullptr)
    return MSDF_ERR_ARG;
  // what the module's `x / divide_factor` multiplies by on the device: the reciprocal formed in double, rounded to
  // fp32 (scripts/dbg/x01_rounding.py: bit-identical on 196,608 values; 1.0f / 1.1f differs in 41 % of them)
  const float inv = (float)(1.0 / divide_factor);
  const dim3 grid((B + HG_THREADS - 1) / HG_THREADS, L);
  HG_DISPATCH_C(C, (hg_node_forward_kernel<CC><<<grid, HG_THREADS, 0, (hipStream_t)stream>>>(
                       x, inv, x01_out, embeddings, offsets, feat, pitch, B, L, S, H, dy_dx)));
  return msdf_check_launch();
}

extern "C" int msdf_hash_node_input_gradient(const float* g, uint32_t pitch, const float* dy_dx, uint32_t B,
                                             uint32_t C, uint32_t L, float scale, float* inout, void* stream) {
  if (B == 0) return MSDF_OK;
  if ((pitch != 0 && pitch < L * C) || g == nullptr || dy_dx == nullptr || inout == nullptr) return MSDF_ERR_ARG;
  if ((uint64_t)B * 3 >= (1ull << 32)) return MSDF_ERR_UNSUPPORTED;
  HG_DISPATCH_C(C, (hg_node_input_gradient_kernel<CC><<<(3 * B + HG_THREADS - 1) / HG_THREADS, HG_THREADS, 0,
                                                        (hipStream_t)stream>>>(g, pitch, dy_dx, B, L, scale, inout)));
  return msdf_check_launch();
}

extern "C" int msdf_hash_node_second_grad(const float* g_a, const float* g_b, uint32_t n_split, float scale,
                                          float* gg_out, const float* dy_dx, float* grad_grad, uint32_t pitch,
                                          uint32_t B, uint32_t C, uint32_t L, void* stream) {
  if (B == 0) return MSDF_OK;
  if ((pitch != 0 && pitch < L * C) || gg_out == nullptr || dy_dx == nullptr || grad_grad == nullptr || n_split > B)
    return MSDF_ERR_ARG;
  const dim3 grid((B + HG_THREADS - 1) / HG_THREADS, L);
  HG_DISPATCH_C(C, (hg_node_second_grad_kernel<CC><<<grid, HG_THREADS, 0, (hipStream_t)stream>>>(
                       g_a, g_b, n_split, scale, gg_out, dy_dx, grad_grad, pitch, B, L)));
  return msdf_check_launch();
}

// msdf_hash_encode_backward_fused_out with grad_first / grad_second as point-major rows of `pitch` floats (0: level-major)
extern "C" int msdf_hash_node_scatter(const float* grad_first, const float* grad_second, uint32_t pitch,
                                      const float* inputs, const int* offsets, float* grad_embeddings, uint32_t B,
                                      uint32_t C, uint32_t L, float S, uint32_t H, const float* grad_grad_inputs,
                                      uint64_t n_entries, void* workspace, uint64_t workspace_bytes, void* stream) {
  return hg_fused(hg_binned(grad_first, grad_second, grad_grad_inputs, pitch, true, n_entries, workspace, workspace_bytes), inputs,
                  offsets, grad_embeddings, B, 3, C, L, S, H, true, (hipStream_t)stream);
}
