/* C ABI of the grid-bounded nearest-neighbour search of libmonosdf_hip.so (csrc/gridnn.hip), the search behind the two
 * closing queries of the DTU protocol (dtu_eval/eval.py:120-134 uses only the distances below max_dist).  Same
 * conventions as monosdf_hip.h, whose status codes these functions return: raw DEVICE pointers, an explicit hipStream_t
 * passed as void*, callers own every buffer, nothing allocates, frees or synchronises.  These entry points are additive:
 * monosdf_hip.h and MSDF_ABI_VERSION are unchanged.
 *
 * The grid.  n_x n_y n_z cells of side h over the box that starts at lo; the cell of a point is
 * clamp(floor((p - lo) / h), 0, n - 1) per axis in fp64 on the fp32 coordinate, the linear cell index
 * (c_x n_y + c_y) n_z + c_z (z fastest).  h > 0 and finite, every n >= 1, n_x n_y n_z < 2^31 - 1.  The caller chooses lo,
 * h and n so that every reference point falls inside without the clamp; a query may lie anywhere.
 *
 * msdf_gnn_cells: cells[i] (int32) = the linear cell index of points[i] ([n, 3] fp32).
 * msdf_gnn_records: with order[n_ref] (int64) the permutation of a STABLE sort of the reference cloud's cell indices,
 *   records[i] = x y z of ref[order[i]] and, in the fourth word, the bits of (int32) order[i]: 16 bytes a point, in
 *   cell order and in ascending original index inside a cell.  msdf_gnn_workspace_bytes(n_ref): the size of `records`
 *   (-1 for n_ref outside [1, 2^31)).
 * msdf_gnn_query: starts[n_x n_y n_z + 1] (int32) = for every cell the position in `records` of its first point (the
 *   number of reference points in cells of smaller index), n_ref last.  query_order[n_query] (int64): a permutation;
 *   lane t of the launch answers query query_order[t] (sorted by cell, so that neighbouring lanes walk the same runs)
 *   and writes position query_order[t] of the outputs.  With (d, i) the fp32 distance
 *   sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx dx))) and the index of the nearest reference point, the smallest index among
 *   equal fp32 squared distances -- bit for bit what msdf_nn_search returns -- dist[q] = d and idx[q] = i if
 *   d <= (float) max_dist, else dist[q] = +inf and idx[q] = -1.  The result does not depend on lo, h or n.  No atomics:
 *   the same inputs give bitwise the same outputs every call.  max_dist > 0 and finite; all coordinates must be finite.
 *   n_query == 0 launches nothing. */
#ifndef MONOSDF_GRIDNN_H
#define MONOSDF_GRIDNN_H

#include <stdint.h>
#include "monosdf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t msdf_gnn_workspace_bytes(int64_t n_ref);
int msdf_gnn_cells(const float* points, int64_t n, double lo_x, double lo_y, double lo_z, double h, int n_x, int n_y,
                   int n_z, int32_t* cells, void* stream);
int msdf_gnn_records(const float* ref, const int64_t* order, int64_t n_ref, void* records, void* stream);
int msdf_gnn_query(const float* query, const int64_t* query_order, int64_t n_query, const void* records,
                   int64_t n_ref, const int32_t* starts, double lo_x, double lo_y, double lo_z, double h, int n_x,
                   int n_y, int n_z, double max_dist, float* dist, int32_t* idx, void* stream);

#ifdef __cplusplus
}
#endif

#endif
