/* C ABI of the high-resolution cue merge of libmonosdf_hip.so (csrc/highres.hip): the device half of
 * utils/highres_cues.py, which stitches the overlapping monocular depth and normal patches of one training image into
 * one mosaic (preprocess/generate_high_res_map.py --mode merge_patches, lines 44-174 and 297-383).
 * Same conventions as monosdf_hip.h, whose status codes these functions return: raw DEVICE pointers, an explicit
 * hipStream_t passed as void*, callers own every buffer, nothing allocates, frees or synchronises, and nothing is
 * copied to the host between the first and the last launch of a merge.  These entry points are additive:
 * monosdf_hip.h and MSDF_ABI_VERSION are unchanged.  Arguments are checked on the host and refused with MSDF_ERR_ARG
 * before any launch.  No atomics, no workgroup waits on another: the same input gives bitwise the same output every
 * call, and the output of one image does not depend on the other images of the batch.  Inputs must be finite.
 *
 * Geometry.  n images, each a grid of rows x cols square patches of side `patch`, neighbours `stride` apart:
 *   overlap O = patch - stride, mosaic H = patch + stride (rows - 1) by W = patch + stride (cols - 1).
 *   Required: 1 <= n <= 65536, 1 <= rows, cols <= 1024, 1 <= stride < patch <= 16384, O >= 2, 3 H W < 2^31,
 *   3 n rows cols patch^2 < 2^40, and fewer than 2^31 workgroups in every launch.
 *
 * One step merges a patch Q into the running mosaic M along one axis.  Over the overlap (the last O lines of M, the
 * first O lines of Q) sums are taken in fp64: every lane adds its elements e = tile * 2048 + k * 256 + lane,
 * k = 0 .. 7, in ascending order (e counts the overlap in memory order), the 64 lanes of a wave by the xor tree
 * 32, 16, .. 1, the four waves in ascending order, the tiles by lane t of one wave taking tiles t, t + 64, ..
 * ascending and the same xor tree.  One lane solves; all lanes then store, every stored value formed in fp64 and
 * rounded once:
 *   before the overlap M is unchanged; in the overlap, line i of O,   M w + Q' (1 - w),
 *   w = i * (-1 / (O - 1)) + 1 and exactly 0 on the last line (numpy's linspace(1, 0, O)); behind it the remaining
 *   `stride` lines of Q'.
 * The steps of an image: for every row the patches left to right (cols - 1 steps), then the rows - 1 row strips top to
 * bottom, then the centre patch `mid` if given.  `steps` receives the solved coefficients as [n, n_steps, K] fp64 in
 * that order, n_steps = rows (cols - 1) + (rows - 1) + (mid ? 1 : 0); it may be null when n_steps == 0.
 *
 * msdf_hrc_merge_depth: patches [n, rows, cols, patch, patch] fp32, mid [n, patch, patch] fp32 or null ->
 *   out [n, H, W] fp32; K = 2 (scale, shift).  With p from Q and t from M (fp32 values converted to fp64, so every
 *   product is exact):  a00 = sum p p, a01 = sum p, a11 = the element count, b0 = sum p t, b1 = sum t,
 *   det = a00 a11 - a01 a01;  det != 0: scale = (a11 b0 - a01 b1) / det, shift = (-a01 b0 + a00 b1) / det, each
 *   product, difference and quotient rounded once; det == 0: scale = shift = 0 exactly.  Q' = scale Q + shift.
 *   The running mosaic is stored in fp32.  mid: the same fit with p = the mosaic's patch x patch crop whose first line
 *   and column are H / 2 - patch / 2 and W / 2 - patch / 2 (integer division) and t = mid; the whole mosaic becomes
 *   scale M + shift.  normalize != 0: at the end out = (out - min) / (max - min) per image, min and max over the
 *   stored fp32 values, the quotient formed in fp64 (max == min gives NaN, as the division does).
 *
 * msdf_hrc_merge_normals: patches [n, rows, cols, 3, patch, patch] fp64 unit normals (already decoded), mid
 *   [n, 3, patch, patch] fp64 or null -> out [n, 3, H, W] fp64; K = 9, the rotation row-major.  With A = the patch's
 *   normals and B = the mosaic's, Hm = A^T B (9 sums, Hm[a][b] = sum A_a B_b).  Its singular vectors come from a
 *   one-sided Jacobi iteration in fp64 on one lane: column pairs of Hm V are rotated until
 *   |g_p . g_q| <= 1e-15 |g_p| |g_q| (at most 30 sweeps); the columns ordered by descending length s_k give
 *   u_k = g_k / s_k and v_k.  The rotation is  R = v1 u1^T + v2 u2^T + (v1 x v2) (u1 x u2)^T,  which is V U^T where
 *   that is proper and V diag(1, 1, -1) U^T where it is a reflection: numpy's svd followed by the reference's sign
 *   change of the last row of V^T.  Hm == 0 gives the identity; s2 <= 1e-300 or s2 <= 1e-14 s1 (a rank-one Hm, whose
 *   rotation is not unique) completes u2, v2 by the cross product with the coordinate axis of the smallest component,
 *   which is NOT LAPACK's choice.  Q' = R Q per pixel, as ((r0 x + r1 y) + r2 z); blended as for depth; every pixel
 *   written by a step is divided by (its length + 1e-15), the length sqrt((x x + y y) + z z).  The reference divides
 *   the whole mosaic at every step; that matters once per pixel (the input is unit in fp32 only), so the first step
 *   of a chain also divides the lines of the chain's first patch in front of the overlap, after the sums of that step
 *   have read the overlap as it came.  A 1 x 1 grid has no step; its one patch is divided once on its own, so that
 *   the output is unit in fp64 for every grid (the reference, which never runs such a grid, would save it as it
 *   came: a difference of 2^-24 relative).  mid: R from
 *   A = the mosaic's centre crop, B = mid; the whole mosaic is rotated and not renormalised.  At the end
 *   out = (out + 1) / 2, what the reference saves.  The running mosaic is fp64.
 *
 * workspace: msdf_hrc_workspace_bytes(n, rows, cols, patch, stride, channels) bytes, channels = 1 for depth and 3 for
 *   normals; -1 for sizes out of range.  It holds the row strips 1 .. rows - 1 (strip 0 is built in `out`), the
 *   per-tile partial sums and the per-image minimum and maximum. */
#ifndef MONOSDF_HIGHRES_H
#define MONOSDF_HIGHRES_H

#include <stdint.h>
#include "monosdf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t msdf_hrc_workspace_bytes(int64_t n, int64_t rows, int64_t cols, int64_t patch, int64_t stride,
                                 int64_t channels);
int msdf_hrc_merge_depth(const float* patches, const float* mid, int64_t n, int64_t rows, int64_t cols, int64_t patch,
                         int64_t stride, int normalize, void* workspace, float* out, double* steps, void* stream);
int msdf_hrc_merge_normals(const double* patches, const double* mid, int64_t n, int64_t rows, int64_t cols,
                           int64_t patch, int64_t stride, void* workspace, double* out, double* steps, void* stream);

#ifdef __cplusplus
}
#endif

#endif
