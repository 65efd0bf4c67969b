// Mesh evaluation on the device: exact brute-force 1-nearest-neighbour search and the voxel down-sample, the two
// steps the reference's evaluation scripts do on CPU threads (scannet_eval/evaluate.py:16-56 with sklearn's KDTree
// and open3d's voxel_down_sample; replica_eval/eval_recon.py:25-43, 96-179 with scipy's cKDTree).
//
// Search.  For every query the reference point with the smallest squared distance, formed from the three
// DIFFERENCES (dx = q.x - r.x, ..., d2 = dx dx + dy dy + dz dz; two of the products fused) in fp32 on the vector ALU.
// Not the expanded form |q|^2 + |r|^2 - 2 q.r and so not an MFMA GEMM: at scene coordinates of several metres the
// expanded form loses ~1e-7 |p|^2 absolutely in d2, which is millimetres in d for close pairs, against thresholds of
// 5 cm and means of 2-5 cm.  The differences are exact to 1 ulp each, so d is good to ~2.4e-7 relative wherever the
// clouds lie.
//   * every lane keeps NN_QPL queries in registers (independent chains); a workgroup of 256 lanes covers
//     NN_QBLOCK = 1024 queries (grid.x) and one slice of the reference cloud (grid.y = split)
//   * the slice streams through LDS in tiles of NN_TILE records `x y z pad` (16 bytes); every lane reads the same
//     record in the same ds_read_b128 (a broadcast: no bank conflict), the next tile's records wait in registers
//   * per pair and query 8 vector instructions: 3 subtract, 1 multiply, 2 fma, 1 compare, 2 select (minimum, index)
//   * the running minimum and its index stay in registers; a split writes one 64-bit word per query,
//     (bits of d2 << 32) | index -- non-negative floats order as unsigned integers -- and nn_finish_k takes the
//     minimum of the words over the splits.  Inside a split the scan is in ascending index with a strict `<`.
//     Both give the tie rule: of several points at the same fp32 d2 the SMALLEST INDEX wins, whatever the split
//     count, and no atomics: the same inputs give bitwise the same outputs every call.
// Inputs must be finite: the packed minimum is defined for non-negative, non-NaN d2 only (+inf, from a difference that
// overflows, still orders).  The pad records of a slice's last tile are NaN, which no `<` ever selects.
//
// Voxel down-sample (the rule of open3d's PointCloud.voxel_down_sample): voxel of a point = floor((p - o) / v) per
// axis, o = min_bound - v / 2, every operation rounded separately in fp32 (this object is built with
// -ffp-contract=off); one output per occupied voxel, the fp64 sum of its points in ascending original index over their
// count, rounded once to fp32.  The keys are sorted by the caller (a stable sort); no floating-point atomics.
#include "tool_common.h"

namespace {

constexpr int NN_THREADS = 256;                    // 4 waves
constexpr int NN_QPL = 4;                          // queries per lane
constexpr int NN_QBLOCK = NN_THREADS * NN_QPL;     // queries per workgroup
constexpr int NN_TILE = 1024;                      // reference records per LDS tile (16 KiB)
constexpr int NN_RPT = NN_TILE / NN_THREADS;       // records a thread stages per tile
constexpr int64_t NN_TARGET_BLOCKS = 4096;         // automatic split: about this many workgroups ...
constexpr int64_t NN_MIN_TILES = 4;                // ... of at least this many tiles each
constexpr int64_t NN_MAX_SPLITS = 65535;           // grid.y

struct NnSplit {
  int64_t tiles_per_split;
  int n_splits;
};

// n_splits <= 0: chosen from the sizes; > 0: the caller's, clamped to what the tile count allows
NnSplit nn_split(int64_t R, int64_t Q, int n_splits) {
  const int64_t tiles = blocks_for(R, NN_TILE);
  int64_t s = n_splits;
  if (s <= 0) {
    const int64_t qb = Q > 0 ? blocks_for(Q, NN_QBLOCK) : 1;
    s = (NN_TARGET_BLOCKS + qb - 1) / qb;
    const int64_t s_max = (tiles + NN_MIN_TILES - 1) / NN_MIN_TILES;
    if (s > s_max) s = s_max;
  }
  if (s > tiles) s = tiles;
  if (s > NN_MAX_SPLITS) s = NN_MAX_SPLITS;
  if (s < 1) s = 1;
  NnSplit p;
  p.tiles_per_split = (tiles + s - 1) / s;
  p.n_splits = (int)((tiles + p.tiles_per_split - 1) / p.tiles_per_split);
  return p;
}

bool nn_sizes_ok(int64_t R, int64_t Q) { return R >= 1 && fits_int32(R) && fits_int32(Q); }

__global__ void __launch_bounds__(NN_THREADS)
nn_search_k(const float* __restrict__ ref, int64_t R, const float* __restrict__ query, int64_t Q,
            int64_t tiles_per_split, uint64_t* __restrict__ partial) {
  __shared__ v4f tile[NN_TILE];
  const int t = (int)threadIdx.x;
  const int64_t r_begin = (int64_t)blockIdx.y * tiles_per_split * NN_TILE;
  const int64_t r_stop = r_begin + tiles_per_split * NN_TILE;
  const int64_t r_end = r_stop < R ? r_stop : R;                       // r_begin < R by the split's construction
  const int n_tiles = (int)((r_end - r_begin + NN_TILE - 1) / NN_TILE);

  // query k of this lane: block base + k * 256 + t (coalesced); lanes past Q repeat the last query and store nothing
  const int64_t q0 = (int64_t)blockIdx.x * NN_QBLOCK + t;
  float qx[NN_QPL], qy[NN_QPL], qz[NN_QPL], best[NN_QPL];
  int32_t best_i[NN_QPL];
#pragma unroll
  for (int k = 0; k < NN_QPL; ++k) {
    int64_t q = q0 + (int64_t)k * NN_THREADS;
    if (q >= Q) q = Q - 1;
    qx[k] = query[3 * q];
    qy[k] = query[3 * q + 1];
    qz[k] = query[3 * q + 2];
    best[k] = __builtin_inff();
    best_i[k] = (int32_t)r_begin;                                      // every d2 = +inf: the slice's first point
  }

  // the tile after the current one waits in registers while the current one is scanned
  float nx[NN_RPT], ny[NN_RPT], nz[NN_RPT];
  auto fetch = [&](int64_t base) {
#pragma unroll
    for (int u = 0; u < NN_RPT; ++u) {
      const int64_t r = base + u * NN_THREADS + t;
      const bool in = r < r_end;
      nx[u] = in ? ref[3 * r] : __builtin_nanf("");
      ny[u] = in ? ref[3 * r + 1] : __builtin_nanf("");
      nz[u] = in ? ref[3 * r + 2] : __builtin_nanf("");
    }
  };
  fetch(r_begin);
  for (int it = 0; it < n_tiles; ++it) {
    const int64_t base = r_begin + (int64_t)it * NN_TILE;
    __syncthreads();                                                   // the previous tile has been read by all
#pragma unroll
    for (int u = 0; u < NN_RPT; ++u) tile[u * NN_THREADS + t] = v4f{nx[u], ny[u], nz[u], 0.0f};
    __syncthreads();
    if (it + 1 < n_tiles) fetch(base + NN_TILE);
    const int32_t jb = (int32_t)base;
#pragma unroll 8
    for (int j = 0; j < NN_TILE; ++j) {
      const v4f r = tile[j];                                           // same address in every lane: broadcast
#pragma unroll
      for (int k = 0; k < NN_QPL; ++k) {
        const float dx = qx[k] - r.x, dy = qy[k] - r.y, dz = qz[k] - r.z;
        const float d2 = nn_d2(dx, dy, dz);
        const bool lt = d2 < best[k];                                  // strict: the earlier index keeps a tie
        best[k] = lt ? d2 : best[k];
        best_i[k] = lt ? jb + j : best_i[k];
      }
    }
  }
  uint64_t* out = partial + (size_t)blockIdx.y * (size_t)Q;
#pragma unroll
  for (int k = 0; k < NN_QPL; ++k) {
    const int64_t q = q0 + (int64_t)k * NN_THREADS;
    if (q < Q) out[q] = nn_word(best[k], (uint32_t)best_i[k]);
  }
}

__global__ void __launch_bounds__(NN_THREADS)
nn_finish_k(const uint64_t* __restrict__ partial, int64_t Q, int n_splits, float* __restrict__ dist,
            int32_t* __restrict__ idx) {
  const int64_t q = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x;
  if (q >= Q) return;
  uint64_t m = partial[q];
  for (int s = 1; s < n_splits; ++s) {
    const uint64_t v = partial[(size_t)s * (size_t)Q + q];
    m = v < m ? v : m;
  }
  dist[q] = sqrtf(nn_word_d2(m));
  idx[q] = nn_word_index(m);
}

constexpr int VOX_BITS = 21;                       // per axis in the 63-bit key

__global__ void __launch_bounds__(NN_THREADS)
voxel_keys_k(const float* __restrict__ pts, int64_t n, const float* __restrict__ min_bound, float v,
             int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x;
  if (i >= n) return;
  const float h = v * 0.5f;
  int64_t key = 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const float o = min_bound[d] - h;
    const float c = floorf((pts[3 * i + d] - o) / v);                  // >= 0: p >= min_bound > o
    int64_t ci = (int64_t)c;
    ci = ci < 0 ? 0 : (ci > ((1ll << VOX_BITS) - 1) ? ((1ll << VOX_BITS) - 1) : ci);
    key = (key << VOX_BITS) | ci;
  }
  keys[i] = key;
}

// one thread per voxel: its points are order[seg_start[s] .. seg_start[s + 1]) (ascending original index)
__global__ void __launch_bounds__(NN_THREADS)
voxel_mean_k(const float* __restrict__ pts, const int64_t* __restrict__ order, const int64_t* __restrict__ seg_start,
             int64_t n, int64_t m, float* __restrict__ out) {
  const int64_t s = (int64_t)blockIdx.x * NN_THREADS + threadIdx.x;
  if (s >= m) return;
  const int64_t a = seg_start[s], b = s + 1 < m ? seg_start[s + 1] : n;
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int64_t e = a; e < b; ++e) {
    const int64_t p = order[e];
    sx += (double)pts[3 * p];
    sy += (double)pts[3 * p + 1];
    sz += (double)pts[3 * p + 2];
  }
  const double c = (double)(b - a);
  out[3 * s] = (float)(sx / c);
  out[3 * s + 1] = (float)(sy / c);
  out[3 * s + 2] = (float)(sz / c);
}

}  // namespace

extern "C" int msdf_nn_split_count(int64_t n_ref, int64_t n_query, int n_splits) {
  if (!nn_sizes_ok(n_ref, n_query)) return -1;
  return nn_split(n_ref, n_query, n_splits).n_splits;
}

extern "C" int64_t msdf_nn_workspace_bytes(int64_t n_ref, int64_t n_query, int n_splits) {
  if (!nn_sizes_ok(n_ref, n_query)) return -1;
  return workspace_floor((int64_t)nn_split(n_ref, n_query, n_splits).n_splits * n_query * 8);
}

extern "C" int msdf_nn_search(const float* ref, int64_t n_ref, const float* query, int64_t n_query, int n_splits,
                              void* workspace, float* dist, int32_t* idx, void* stream) {
  if (!nn_sizes_ok(n_ref, n_query) || !ref) return MSDF_ERR_ARG;
  if (n_query == 0) return MSDF_OK;
  if (!query || !workspace || !dist || !idx) return MSDF_ERR_ARG;
  const NnSplit p = nn_split(n_ref, n_query, n_splits);
  const hipStream_t s = (hipStream_t)stream;
  uint64_t* partial = (uint64_t*)workspace;
  const dim3 grid((unsigned)blocks_for(n_query, NN_QBLOCK), (unsigned)p.n_splits);
  nn_search_k<<<grid, NN_THREADS, 0, s>>>(ref, n_ref, query, n_query, p.tiles_per_split, partial);
  nn_finish_k<<<blocks_for(n_query, NN_THREADS), NN_THREADS, 0, s>>>(partial, n_query, p.n_splits, dist, idx);
  return msdf_check_launch();
}

extern "C" int msdf_voxel_keys(const float* points, int64_t n, const float* min_bound, float voxel_size,
                               int64_t* keys, void* stream) {
  if (!fits_int32(n) || !(voxel_size > 0.0f)) return MSDF_ERR_ARG;
  if (n == 0) return MSDF_OK;
  if (!points || !min_bound || !keys) return MSDF_ERR_ARG;
  voxel_keys_k<<<blocks_for(n, NN_THREADS), NN_THREADS, 0, (hipStream_t)stream>>>(points, n, min_bound, voxel_size,
                                                                                   keys);
  return msdf_check_launch();
}

extern "C" int msdf_voxel_mean(const float* points, const int64_t* order, const int64_t* seg_start, int64_t n,
                               int64_t m, float* out, void* stream) {
  if (!fits_int32(n) || m < 0 || m > n) return MSDF_ERR_ARG;
  if (m == 0) return MSDF_OK;
  if (!points || !order || !seg_start || !out) return MSDF_ERR_ARG;
  voxel_mean_k<<<blocks_for(m, NN_THREADS), NN_THREADS, 0, (hipStream_t)stream>>>(points, order, seg_start, n, m, out);
  return msdf_check_launch();
}
