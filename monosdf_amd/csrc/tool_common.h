// What the mesh tools share beyond common.h: mcubes, nnsearch, refuse, dtueval, gridnn, meshcc, obb, highres, icp and
// meshrender include this, the training-path sources do not.  The host half is the checks and launch arithmetic every
// entry point repeats; the device half is the expressions whose rounding two or more tools promise bit for bit.  Everything is inline: each translation unit compiles these with its own flags (csrc/Makefile), and no
// fp-contract pragma stands here for the same reason as in common.h.
#pragma once
#include "common.h"

// ---------------------------------------------------------------- host: sizes, launches, arguments

constexpr int64_t MSDF_COUNT_MAX = 0x7fffffffll;   // 2^31 - 1

// A count stored in int32, 0 <= n <= 2^31 - 1 (nnsearch, gridnn, dtueval, refuse, meshrender, mcubes): their kernels
// index in int64 and only store an index, at most n - 1, or the count itself in an int32.
static inline bool fits_int32(int64_t n) { return n >= 0 && n <= MSDF_COUNT_MAX; }
// A count whose every index AND the count itself stay below the int32 maximum, 0 <= n < 2^31 - 1 (meshcc, obb, icp).
// No reason for the stricter form is known: these three refuse 2^31 - 1 since they were written, and still do.
static inline bool below_int32_max(int64_t n) { return n >= 0 && n < MSDF_COUNT_MAX; }

// workgroups (slices, tiles) of per_block items that cover n items
static inline int64_t blocks_for(int64_t n, int per_block) { return (n + per_block - 1) / per_block; }

static inline bool positive_finite(float x) { return x > 0.0f && x < __builtin_inff(); }   // NaN fails
static inline bool positive_finite(double x) { return x > 0.0 && x < __builtin_inf(); }

// pinhole intrinsics: finite positive focal lengths, a principal point that is a number
static inline bool intrinsics_ok(float fx, float fy, float cx, float cy) {
  return positive_finite(fx) && positive_finite(fy) && cx == cx && cy == cy;
}

// a workspace is never smaller than 256 bytes, so that a caller always has something to allocate
static inline int64_t workspace_floor(int64_t bytes) { return bytes > 256 ? bytes : 256; }

// ---------------------------------------------------------------- device: pinned expressions

// Row ROW, `a b c d`, of the row-major 3x4 matrix m applied to a point: ((a x + b y) + c z) + d, left to right, every
// operation rounded on its own -- the users (tsdf_integrate_k, dt_mask_vertices_k, icp_transform_k) are built with
// -ffp-contract=off and this adds no fmaf.  cull_vertices_k and rnd_views_see_k spell the same rule out themselves:
// through this function the compiler orders their bound comparisons differently.
template <int ROW, typename T>
__device__ __forceinline__ T affine_row(const T* m, T x, T y, T z) {
  return m[4 * ROW] * x + m[4 * ROW + 1] * y + m[4 * ROW + 2] * z + m[4 * ROW + 3];
}

// The nearest-neighbour searches (nnsearch.hip, gridnn.hip) return the same bits because both use these: the squared
// distance from the three differences with two of the products fused, and the word (bits of d2 << 32) | index, whose
// unsigned minimum is the smallest d2 (non-negative floats order as unsigned integers) and, among equal d2, the
// smallest index.  nn_word_d2 and nn_word_index take the word apart again.
__device__ __forceinline__ float nn_d2(float dx, float dy, float dz) { return fmaf(dz, dz, fmaf(dy, dy, dx * dx)); }
__device__ __forceinline__ uint64_t nn_word(float d2, uint32_t index) {
  return ((uint64_t)__float_as_uint(d2) << 32) | index;
}
__device__ __forceinline__ float nn_word_d2(uint64_t word) { return __uint_as_float((uint32_t)(word >> 32)); }
__device__ __forceinline__ int32_t nn_word_index(uint64_t word) { return (int32_t)(uint32_t)word; }
