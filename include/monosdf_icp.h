/* C ABI of the point-to-point ICP kernels of libmonosdf_hip.so (csrc/icp.hip): the device half of
 * utils/mesh_align.py, the alignment that replica_eval/eval_recon.py:51-65 (get_align_transformation) runs before it
 * scores a mesh.  Same conventions as monosdf_hip.h, whose status codes these functions return: raw DEVICE pointers, an
 * explicit hipStream_t passed as void*, callers own every buffer, nothing allocates, frees or synchronises.  These entry
 * points are additive: monosdf_hip.h and MSDF_ABI_VERSION are unchanged.  Every size lies in [0, 2^31): a size outside
 * it returns MSDF_ERR_ARG, a null pointer with every size > 0 returns MSDF_ERR_ARG, `state` and `pivots` are never
 * null.  Inputs must be finite.  No atomics: the same input gives bitwise the same output every call.
 *
 * The rule is open3d's registration_icp with TransformationEstimationPointToPoint() and the default criteria
 * (max_iteration 30, relative_fitness 1e-6, relative_rmse 1e-6), on source [n, 3] and target [m, 3] fp32 with the
 * correspondence distance max_dist and a start T_0.  Evaluation k = 0, 1, .. with the current transform T_k:
 *   1. y_i = fl32(((r0 x + r1 y) + r2 z) + t) per row (r0 r1 r2 t) of T_k: fp64 arithmetic on the fp32 coordinates,
 *      each operation rounded on its own, the result rounded once to fp32.
 *   2. The correspondence of i is the target point nearest to y_i if its fp32 distance is <= (float) max_dist: bit for
 *      bit the answer of msdf_gnn_query (monosdf_gridnn.h), the smallest index on ties, idx = -1 where there is none.
 *   3. With n_k correspondences: fitness_k = n_k / n, rmse_k = sqrt(sum r^2 / n_k), r^2 = (dx dx + dy dy) + dz dz in
 *      fp64 from (double) y - (double) q; both 0 when n_k = 0.
 *   4. Stop if k >= 1 and |fitness_k - fitness_{k-1}| < relative_fitness and |rmse_k - rmse_{k-1}| < relative_rmse, and
 *      stop if k = max_iteration: at most max_iteration updates and one evaluation more than updates.
 *   5. Otherwise T_{k+1} is the rigid transform that best maps the ORIGINAL source points p of the correspondences onto
 *      their target points q.  All sums are taken about two fixed pivots c_s and c_t (the centres of the two clouds'
 *      bounding boxes, so that the covariance does not cancel):  mp = sum (p - c_s) / n_k,  mq = sum (q - c_t) / n_k,
 *      H[a][b] = sum (p_a - c_s,a)(q_b - c_t,b) / n_k - mp_a mq_b;  R = the rotation of monosdf_highres.h's one-sided
 *      Jacobi solver for Hm = H (always proper: Umeyama's S(2,2) = -1 case where V U^T would reflect; H == 0 gives the
 *      identity);  t_a = (c_t,a + mq_a) - ((R_a0 P_0 + R_a1 P_1) + R_a2 P_2) with P = c_s + mp.  n_k = 0 leaves T
 *      unchanged.
 * The result is the last evaluated T with its fitness and rmse.  Two deliberate differences from open3d: it composes
 * update * T on a cloud it transforms in place, here T is solved from the original points every time (the same optimum
 * in exact arithmetic, no drift); it holds points in fp64, here the searched point y is fp32.  Parity with open3d is
 * UNVERIFIED: there is no open3d where this is built and no recorded output of it.
 *
 * state: msdf_icp_state_bytes(max_iteration) bytes of device memory that the caller fills before the first launch
 *   (-1 for max_iteration outside [0, 2^20]):
 *     double T[16]                       row-major 4 x 4, last row 0 0 0 1
 *     double prev_fitness, prev_rmse     of evaluation iteration - 1
 *     int32  iteration, done             the evaluation the next msdf_icp_solve performs; set once ICP has stopped
 *     double log[max_iteration + 1][3]   (fitness, rmse, count) per evaluation
 *   After the run `iteration` is the last evaluation, iteration + 1 log rows are filled and T belongs to log row
 *   `iteration`.  EVERY msdf_icp_* launch returns at once when `done` is set and changes nothing, so a caller may
 *   enqueue any number of iterations and look at `done` whenever it likes: the result does not depend on when.
 * pivots: [6] fp64, c_s then c_t.
 *
 * msdf_icp_transform: y[n, 3] (fp32) = step 1 with T of the state.
 * msdf_icp_accumulate: over (source, y, target, idx[n] int32) one partial of 17 fp64 per slice of 2048 consecutive
 *   points: the count, sum (p - c_s) [3], sum (q - c_t) [3], sum (p - c_s)(q - c_t)^T [9, row-major], sum r^2.  Entries
 *   with idx outside [0, m) add nothing.  Order: a lane adds its 8 consecutive points in ascending order, the 64 lanes
 *   of a wave by the xor tree 32, 16, .. 1, the four waves in ascending order.  workspace:
 *   msdf_icp_workspace_bytes(n) bytes (-1 for n out of range).
 * msdf_icp_solve: one wave.  Adds the slices in ascending order (component c on lane c), then one lane does steps 3 to
 *   5 for evaluation k = state.iteration: writes log row k; sets `done`, or stores prev_fitness, prev_rmse,
 *   iteration = k + 1 and T_{k+1}.  An `iteration` outside [0, max_iteration] sets `done` and writes nothing else. */
#ifndef MONOSDF_ICP_H
#define MONOSDF_ICP_H

#include <stdint.h>
#include "monosdf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t msdf_icp_state_bytes(int64_t max_iteration);
int64_t msdf_icp_workspace_bytes(int64_t n);
int msdf_icp_transform(const float* source, int64_t n, const void* state, float* y, void* stream);
int msdf_icp_accumulate(const float* source, const float* y, const float* target, const int32_t* idx, int64_t n,
                        int64_t m, const double* pivots, const void* state, void* workspace, void* stream);
int msdf_icp_solve(const void* workspace, int64_t n, const double* pivots, int64_t max_iteration,
                   double relative_fitness, double relative_rmse, void* state, void* stream);

#ifdef __cplusplus
}
#endif

#endif
