// Connected components of a triangle mesh by a lock-free union-find (ABI: include/monosdf_meshcc.h), the graph half of
// utils/mesh_clean.py.  The caller sorts one 64-bit key per face edge; the faces that share an edge are then neighbours
// in the sorted list, and one lane per sorted position unites them directly.
//
// The forest.  parent[i] <= i at all times.  A root points at itself; the only write to a root is the hook
//     atomicCAS(&parent[larger_root], larger_root, smaller_root),
// and the only write to a node that is no root is path halving, atomicMin(&parent[x], grandparent).  Both lower the
// value they touch, so a node that has stopped being a root never becomes one again, and whatever parent[x] has held at
// any time is a node of x's tree with an id below x.
//
// Termination.  find() walks strictly down the ids, so it takes at most x steps from x.  unite() runs find on both
// ends and hooks; a CAS that fails returns the new parent of the larger root, an id below it, and the loop goes on from
// there: the sum of the two ids falls with every round.  Nothing here waits for another lane, wave or workgroup -- no
// spin, no lock, no barrier between workgroups -- so every lane ends whatever the others do.
//
// Uniqueness.  When a link launch has ended, every unite(a, b) has seen a and b under one root or has hooked one root
// under the other, and trees only ever merge; so the trees are the components.  A hook goes from a larger id to a
// smaller one, so the root of a tree is its smallest id.  msdf_mcc_flatten, in a launch of its own, writes that id to
// every node: the result does not depend on the order the atomics landed in.
//
// Memory scope.  A CU's vector L1 is not refreshed by another CU's stores, so find() reads parent with relaxed
// agent-scope atomic loads (served by L2, where the atomics land).  Correctness does not rest on that: a stale parent
// is still a node of the same tree with a smaller id, and the walk from it reaches the same root.  The scope only keeps
// the chains short.  Integer vector atomics only; no floating-point atomics, no inline assembly.
#include "tool_common.h"
#include "../../include/monosdf_meshcc.h"

namespace {

constexpr int MCC_THREADS = 256;
constexpr int MCC_SUM_THREADS = 512;                 // 8 waves per segment
constexpr int64_t MCC_SUM_MAX_BLOCKS = 1 << 20;      // more segments than this: a workgroup takes several

__device__ __forceinline__ int32_t mcc_load(const int32_t* parent, int32_t i) {
  return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x's tree, halving the path on the way: x's parent becomes its grandparent (never a larger id)
__device__ __forceinline__ int32_t mcc_find(int32_t* parent, int32_t x) {
  int32_t p = mcc_load(parent, x);
  while (p != x) {                                   // p < x
    const int32_t g = mcc_load(parent, p);           // g <= p
    if (g == p) return p;
    atomicMin(parent + x, g);
    x = p;
    p = g;
  }
  return x;
}

__device__ __forceinline__ void mcc_unite(int32_t* parent, int32_t a, int32_t b) {
  for (;;) {
    a = mcc_find(parent, a);
    b = mcc_find(parent, b);
    if (a == b) return;
    const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const int32_t was = atomicCAS(parent + hi, hi, lo);
    if (was == hi) return;
    a = was;                                         // hi has a parent by now, below hi: go on from it
    b = lo;
  }
}

__global__ void __launch_bounds__(MCC_THREADS)
mcc_edge_keys_k(const int32_t* __restrict__ faces, int64_t n_keys, int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * MCC_THREADS + threadIdx.x;
  if (i >= n_keys) return;
  const int64_t f = i / 3;
  const int e = (int)(i - 3 * f);
  const int32_t a = faces[3 * f + e], b = faces[3 * f + (e == 2 ? 0 : e + 1)];
  const uint64_t lo = (uint32_t)(a < b ? a : b), hi = (uint32_t)(a < b ? b : a);
  keys[i] = (int64_t)((lo << 32) | hi);
}

__global__ void __launch_bounds__(MCC_THREADS)
mcc_init_k(int32_t* __restrict__ parent, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * MCC_THREADS + threadIdx.x;
  if (i < n) parent[i] = (int32_t)i;
}

// position i unites itself with position i + 1 when both hold one key; under rule 0 only when the run is those two
__global__ void __launch_bounds__(MCC_THREADS)
mcc_link_edges_k(const int64_t* __restrict__ keys, const int64_t* __restrict__ order, int64_t n, int rule,
                 int32_t* parent) {
  const int64_t i = (int64_t)blockIdx.x * MCC_THREADS + threadIdx.x;
  if (i + 1 >= n) return;
  const int64_t k = keys[i];
  if (keys[i + 1] != k) return;
  if (rule == 0 && ((i > 0 && keys[i - 1] == k) || (i + 2 < n && keys[i + 2] == k))) return;
  mcc_unite(parent, (int32_t)(order[i] / 3), (int32_t)(order[i + 1] / 3));
}

__global__ void __launch_bounds__(MCC_THREADS)
mcc_link_vertices_k(const int32_t* __restrict__ faces, int64_t n_faces, int32_t* parent) {
  const int64_t f = (int64_t)blockIdx.x * MCC_THREADS + threadIdx.x;
  if (f >= n_faces) return;
  const int32_t v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
  mcc_unite(parent, v0, v1);
  mcc_unite(parent, v0, v2);
}

// no hook runs in this launch, so the roots are fixed; other lanes only write roots over ancestors meanwhile
__global__ void __launch_bounds__(MCC_THREADS)
mcc_flatten_k(int32_t* parent, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * MCC_THREADS + threadIdx.x;
  if (i >= n) return;
  int32_t x = (int32_t)i, p = mcc_load(parent, x);
  while (p != x) {
    x = p;
    p = mcc_load(parent, x);
  }
  parent[i] = x;
}

__global__ void __launch_bounds__(MCC_SUM_THREADS)
mcc_segment_sum_k(const double* __restrict__ values, const int64_t* __restrict__ seg_start, int64_t m,
                  double* __restrict__ out) {
  __shared__ double part[MCC_SUM_THREADS / MSDF_WAVE];
  for (int64_t s = blockIdx.x; s < m; s += gridDim.x) {          // uniform over the workgroup
    const int64_t a = seg_start[s], b = seg_start[s + 1];
    double acc = 0.0;
#pragma unroll 4
    for (int64_t i = a + threadIdx.x; i < b; i += MCC_SUM_THREADS) acc += values[i];
    acc = wave_sum(acc);
    if (lane_id() == 0) part[threadIdx.x / MSDF_WAVE] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      double total = part[0];
      for (int w = 1; w < MCC_SUM_THREADS / MSDF_WAVE; ++w) total += part[w];
      out[s] = total;
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int msdf_mcc_edge_keys(const int32_t* faces, int64_t n_faces, int64_t* keys, void* stream) {
  if (!below_int32_max(n_faces) || !below_int32_max(3 * n_faces)) return MSDF_ERR_ARG;
  if (n_faces == 0) return MSDF_OK;
  if (!faces || !keys) return MSDF_ERR_ARG;
  mcc_edge_keys_k<<<blocks_for(3 * n_faces, MCC_THREADS), MCC_THREADS, 0, (hipStream_t)stream>>>(faces, 3 * n_faces,
                                                                                                 keys);
  return msdf_check_launch();
}

extern "C" int msdf_mcc_init(int32_t* parent, int64_t n, void* stream) {
  if (!below_int32_max(n)) return MSDF_ERR_ARG;
  if (n == 0) return MSDF_OK;
  if (!parent) return MSDF_ERR_ARG;
  mcc_init_k<<<blocks_for(n, MCC_THREADS), MCC_THREADS, 0, (hipStream_t)stream>>>(parent, n);
  return msdf_check_launch();
}

extern "C" int msdf_mcc_link_edges(const int64_t* sorted_keys, const int64_t* order, int64_t n_keys, int rule,
                                   int32_t* parent, void* stream) {
  if (!below_int32_max(n_keys) || (rule != 0 && rule != 1)) return MSDF_ERR_ARG;
  if (n_keys == 0) return MSDF_OK;
  if (!sorted_keys || !order || !parent) return MSDF_ERR_ARG;
  mcc_link_edges_k<<<blocks_for(n_keys, MCC_THREADS), MCC_THREADS, 0, (hipStream_t)stream>>>(sorted_keys, order, n_keys,
                                                                                             rule, parent);
  return msdf_check_launch();
}

extern "C" int msdf_mcc_link_vertices(const int32_t* faces, int64_t n_faces, int32_t* parent, void* stream) {
  if (!below_int32_max(n_faces)) return MSDF_ERR_ARG;
  if (n_faces == 0) return MSDF_OK;
  if (!faces || !parent) return MSDF_ERR_ARG;
  mcc_link_vertices_k<<<blocks_for(n_faces, MCC_THREADS), MCC_THREADS, 0, (hipStream_t)stream>>>(faces, n_faces,
                                                                                                 parent);
  return msdf_check_launch();
}

extern "C" int msdf_mcc_flatten(int32_t* parent, int64_t n, void* stream) {
  if (!below_int32_max(n)) return MSDF_ERR_ARG;
  if (n == 0) return MSDF_OK;
  if (!parent) return MSDF_ERR_ARG;
  mcc_flatten_k<<<blocks_for(n, MCC_THREADS), MCC_THREADS, 0, (hipStream_t)stream>>>(parent, n);
  return msdf_check_launch();
}

extern "C" int msdf_mcc_segment_sum(const double* values, const int64_t* seg_start, int64_t m, double* out,
                                    void* stream) {
  if (!below_int32_max(m)) return MSDF_ERR_ARG;
  if (m == 0) return MSDF_OK;
  if (!values || !seg_start || !out) return MSDF_ERR_ARG;
  const unsigned blocks = (unsigned)(m < MCC_SUM_MAX_BLOCKS ? m : MCC_SUM_MAX_BLOCKS);
  mcc_segment_sum_k<<<blocks, MCC_SUM_THREADS, 0, (hipStream_t)stream>>>(values, seg_start, m, out);
  return msdf_check_launch();
}
