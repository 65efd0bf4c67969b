/* C ABI of the mesh connected-components kernels of libmonosdf_hip.so (csrc/meshcc.hip): the graph half of
 * utils/mesh_clean.py (trimesh's Trimesh.split and its face_adjacency rule, plots.py:330-336).  Same conventions as
 * monosdf_hip.h, whose status codes these functions return: raw DEVICE pointers, an explicit hipStream_t passed as
 * void*, callers own every buffer, nothing allocates, frees or synchronises.  These entry points are additive:
 * monosdf_hip.h and MSDF_ABI_VERSION are unchanged.  Every size lies in [0, 2^31): a size outside it returns
 * MSDF_ERR_ARG, a size of 0 launches nothing and returns MSDF_OK, a null pointer with a size > 0 returns MSDF_ERR_ARG.
 *
 * The forest.  parent[n] (int32) holds a union-find forest with parent[i] <= i at all times: a root points at itself,
 * a union hooks the LARGER root under the smaller one, and every write lowers a value.  msdf_mcc_link_* may be called
 * any number of times on one forest; after msdf_mcc_flatten, in a launch of its own, parent[i] is the smallest id of
 * i's component, whatever order the atomics of the link launches landed in.  Face and vertex ids must lie inside the
 * forest (the caller has checked the mesh); the kernels check none.
 *
 * msdf_mcc_edge_keys: faces [F, 3] int32 -> keys[3f + e] = (min(a, b) << 32) | max(a, b) for edge e of face f, the
 *   edges being (v0, v1), (v1, v2), (v2, v0).  n_faces < 2^31 / 3, so that 3F is a size.
 * msdf_mcc_init: parent[i] = i.
 * msdf_mcc_link_edges: sorted_keys[n_keys] are the keys above after a STABLE ascending sort, order[n_keys] (int64) the
 *   sort's permutation: the face at sorted position i is order[i] / 3.  Position i looks at its neighbours only, so the
 *   runs of equal keys are found in the kernel and no pair list exists.
 *     rule 0: the two faces of every run of length exactly two are united (trimesh's face_adjacency: an edge with one
 *             face, or with three or more, connects nothing);
 *     rule 1: positions i and i + 1 of every run are united, so all faces on an edge are connected.
 *   Any other rule returns MSDF_ERR_ARG.  parent is a forest over the faces.
 * msdf_mcc_link_vertices: unites (v0, v1) and (v0, v2) of every face; parent is a forest over the vertices.
 * msdf_mcc_flatten: parent[i] = the root of i.  Its own launch, after the links.
 * msdf_mcc_segment_sum: out[s] = the fp64 sum of values[seg_start[s] : seg_start[s + 1]] for s in [0, m); seg_start
 *   [m + 1] (int64) is ascending.  One workgroup per segment: lane t adds elements t, t + 512, ... in ascending order,
 *   the lanes of a wave are added by the xor tree 32, 16, .., 1, the eight waves in ascending order.  No atomics: the
 *   same input gives bitwise the same output every call.  An empty segment gives 0. */
#ifndef MONOSDF_MESHCC_H
#define MONOSDF_MESHCC_H

#include <stdint.h>
#include "monosdf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int msdf_mcc_edge_keys(const int32_t* faces, int64_t n_faces, int64_t* keys, void* stream);
int msdf_mcc_init(int32_t* parent, int64_t n, void* stream);
int msdf_mcc_link_edges(const int64_t* sorted_keys, const int64_t* order, int64_t n_keys, int rule, int32_t* parent,
                        void* stream);
int msdf_mcc_link_vertices(const int32_t* faces, int64_t n_faces, int32_t* parent, void* stream);
int msdf_mcc_flatten(int32_t* parent, int64_t n, void* stream);
int msdf_mcc_segment_sum(const double* values, const int64_t* seg_start, int64_t m, double* out, void* stream);

#ifdef __cplusplus
}
#endif

#endif
