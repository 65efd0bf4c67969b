/* C ABI of the oriented-bounding-box kernels of libmonosdf_hip.so (csrc/obb.hip): the device half of
 * utils/mesh_bounds.py (convex hull, trimesh's oriented_bounds search, the crop of replica_eval/eval_recon.py:121-136).
 * Same conventions as monosdf_hip.h, whose status codes these functions return: raw DEVICE pointers, an explicit
 * hipStream_t passed as void*, callers own every buffer, nothing allocates, frees or synchronises.  These entry points
 * are additive: monosdf_hip.h and MSDF_ABI_VERSION are unchanged.  Every size lies in [0, 2^31): a size outside it
 * returns MSDF_ERR_ARG, a null pointer with every size > 0 returns MSDF_ERR_ARG.  Inputs must be finite.  No atomics:
 * the same input gives bitwise the same output every call.
 *
 * msdf_obb_support: planes [n_planes, 4] fp64 (a, b, c, w), points [n_points, 3] fp32 ->
 *     value[d] = max over the points of   fma(c, z, fma(b, y, a * x)) + w   in fp64,
 *   (x, y, z) being the point's coordinates converted to fp64 (exact), a * x and the final sum rounded once each, the
 *   two fma fused; index[d] (int32) = the point that attains value[d], the SMALLEST index among points of equal fp64
 *   value.  n_planes == 0 launches nothing and returns MSDF_OK; n_points == 0 with n_planes > 0 is MSDF_ERR_ARG (a
 *   maximum over nothing).  The cloud is cut into slices of 2048 consecutive points and the planes into tiles of 128,
 *   one workgroup per slice and tile; a lane holds 8 consecutive points in registers, the tile's planes are read from
 *   LDS as broadcasts, the lanes of a wave are reduced by an xor tree on the value and a ballot for the lowest tied
 *   lane, the four waves and then the slices in ascending order with a strict `>`.  workspace:
 *   msdf_obb_support_workspace_bytes(n_points, n_planes) bytes (-1 for sizes out of range), one (value, index) per
 *   slice and plane.
 *
 * msdf_obb_candidates: the boxes of one search of trimesh.bounds.oriented_bounds.  vertices [n_vertices, 3] fp64: the
 *   hull's vertices; normals [n_normals, 3] fp64: unit vectors; edges [n_edges, 2] int32: the hull's edges as rows of
 *   `vertices`; edge_normals [n_edges, 6] fp64: the unit normals (n1, n2) of an edge's two faces.  For normal n, edge e
 *   is a silhouette edge when the products s1 = n . n1, s2 = n . n2 do not have one strict sign: (s1 <= eps and
 *   s2 >= -eps) or (s1 >= -eps and s2 <= eps), eps = 1e-12; its direction u = d - (d . n) n, d = v1 - v0, normalised,
 *   is used when |u|^2 > 1e-24 |d|^2; the third axis is n x u.  The box of (n, e) has as extents max - min over the
 *   vertices of p . n, p . u and p . (n x u), each dot product fma(pz, az, fma(py, ay, px * ax)), and their product as
 *   volume.  Per normal: volume[k] = the smallest volume over its silhouette edges, edge[k] (int32) the edge that
 *   gives it (smallest edge index on ties), extents[k] = (along n, along u, along n x u).  A normal without a usable
 *   silhouette edge gets volume +inf and edge -1.  One workgroup per normal; a lane takes edges t, t + 256, ... in
 *   ascending order, lane 0 takes the minimum over the lanes in ascending lane order. */
#ifndef MONOSDF_OBB_H
#define MONOSDF_OBB_H

#include <stdint.h>
#include "monosdf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t msdf_obb_support_workspace_bytes(int64_t n_points, int64_t n_planes);
int msdf_obb_support(const float* points, int64_t n_points, const double* planes, int64_t n_planes, void* workspace,
                     double* value, int32_t* index, void* stream);
int msdf_obb_candidates(const double* vertices, int64_t n_vertices, const double* normals, int64_t n_normals,
                        const int32_t* edges, const double* edge_normals, int64_t n_edges, double* volume,
                        int32_t* edge, double* extents, void* stream);

#ifdef __cplusplus
}
#endif

#endif
