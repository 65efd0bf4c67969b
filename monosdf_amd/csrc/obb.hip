// Oriented bounding box of a cloud on the device (ABI: include/monosdf_obb.h), the device half of
// utils/mesh_bounds.py: the support function of a point cloud, which a convex hull by rounds and the final measurement
// of the box are built from, and the candidate boxes of trimesh's oriented_bounds search.
//
// Support.  For every plane (a, b, c, w) the maximum over the cloud of fma(c, z, fma(b, y, a * x)) + w in fp64 and the
// smallest index that attains it.  The shape of nnsearch.hip with the roles swapped: the POINTS stay in registers, the
// planes stream through LDS.
//   * a lane holds OBB_PPL = 8 CONSECUTIVE points as fp64 (48 registers); a workgroup of 256 lanes covers one slice of
//     OBB_SLICE = 2048 consecutive points (grid.x), so a lower lane, and in a lane a lower k, is a lower index
//   * the planes go through LDS in tiles of OBB_TILE = 128 records of 32 bytes, one tile per workgroup (grid.y: the
//     launch has enough waves to hide the reductions' latency at a few hundred planes); every lane reads the same
//     record (two broadcast ds_read_b128, no bank conflict)
//   * per plane a lane scans its 8 points in ascending index with a strict `>`: 3 fp64 multiply-adds, 1 add, 1 compare
//     and 3 selects each, the 8 chains independent
//   * the wave's maximum by the xor tree 32, 16, .., 1 on the value alone (fmax is exact and order-free), then a ballot
//     of the lanes that hold it: the lowest such lane holds the smallest index; OBB_GROUP = 4 planes are reduced side
//     by side, four independent chains of cross-lane moves
//   * the four waves in ascending order with a strict `>` (one lane per plane, through LDS), then obb_finish_k the
//     slices in ascending order with a strict `>`
// Positions of the last slice past the cloud repeat the last point WITH its own index: a copy ties with the original
// and names the same point.  No atomics anywhere.
//
// Candidates.  One workgroup per face normal; see the header for the rule.  min and max are exact, so the extent along
// the normal may be reduced in any order; the minimum over the edges is taken with the edge index as tie-break.
//
// Built with -ffp-contract=off: a * x is rounded before the first fma, as the header says.
#include "tool_common.h"
#include "../../include/monosdf_obb.h"

namespace {

constexpr int OBB_THREADS = 256;                        // 4 waves
constexpr int OBB_WAVES = OBB_THREADS / MSDF_WAVE;
constexpr int OBB_PPL = 8;                              // points per lane
constexpr int OBB_SLICE = OBB_THREADS * OBB_PPL;        // points per workgroup
constexpr int OBB_TILE = 128;                           // planes per workgroup, in LDS (4 KiB)
constexpr int OBB_GROUP = 4;                            // planes reduced side by side
constexpr int64_t OBB_MAX_TILES = 65535;                // grid.y
constexpr double OBB_SIL_EPS = 1e-12;                   // |n . n_face| up to this counts as zero
constexpr double OBB_DIR_EPS = 1e-24;                   // an edge whose projection keeps less of |d|^2 has no direction

inline int64_t obb_slices(int64_t n) { return blocks_for(n, OBB_SLICE); }

__device__ __forceinline__ double obb_dot(double px, double py, double pz, double ax, double ay, double az) {
  return fma(pz, az, fma(py, ay, px * ax));
}

__global__ void __launch_bounds__(OBB_THREADS)
obb_support_k(const float* __restrict__ points, int64_t N, const double* __restrict__ planes, int64_t D,
              int64_t tile0, double* __restrict__ pval, int32_t* __restrict__ pidx) {
  __shared__ double tile[OBB_TILE * 4];
  __shared__ double wval[OBB_WAVES][OBB_TILE];
  __shared__ int32_t widx[OBB_WAVES][OBB_TILE];
  const int t = (int)threadIdx.x, lane = lane_id(), wave = t / MSDF_WAVE;
  const int64_t first = (int64_t)blockIdx.x * OBB_SLICE + (int64_t)t * OBB_PPL;
  const int64_t jb = (tile0 + blockIdx.y) * OBB_TILE;                  // < D by the grid's construction
  const int count = (int)(D - jb < OBB_TILE ? D - jb : OBB_TILE);

  double x[OBB_PPL], y[OBB_PPL], z[OBB_PPL];
  int32_t id[OBB_PPL];
#pragma unroll
  for (int k = 0; k < OBB_PPL; ++k) {
    int64_t p = first + k;
    if (p >= N) p = N - 1;                                             // N >= 1: the host has checked
    x[k] = (double)points[3 * p];
    y[k] = (double)points[3 * p + 1];
    z[k] = (double)points[3 * p + 2];
    id[k] = (int32_t)p;
  }
#pragma unroll
  for (int u = 0; u < 4 * OBB_TILE / OBB_THREADS; ++u) {
    const int e = u * OBB_THREADS + t;                                 // element of the tile, coalesced
    tile[e] = e < 4 * count ? planes[4 * jb + e] : 0.0;                // past the last plane: zeros, never stored
  }
  __syncthreads();

  // OBB_GROUP planes at a time: their reductions are independent chains of cross-lane moves that overlap
  for (int j0 = 0; j0 < count; j0 += OBB_GROUP) {                      // uniform over the workgroup
    double best[OBB_GROUP];
    int32_t best_i[OBB_GROUP];
#pragma unroll
    for (int g = 0; g < OBB_GROUP; ++g) {
      const int j = j0 + g;                                            // < OBB_TILE: the tile is a multiple of the group
      const double a = tile[4 * j], b = tile[4 * j + 1], c = tile[4 * j + 2], w = tile[4 * j + 3];
      best[g] = fma(c, z[0], fma(b, y[0], a * x[0])) + w;
      best_i[g] = id[0];
#pragma unroll
      for (int k = 1; k < OBB_PPL; ++k) {
        const double v = fma(c, z[k], fma(b, y[k], a * x[k])) + w;
        const bool gt = v > best[g];                                   // strict: the earlier index keeps a tie
        best[g] = gt ? v : best[g];
        best_i[g] = gt ? id[k] : best_i[g];
      }
    }
    double m[OBB_GROUP];
#pragma unroll
    for (int g = 0; g < OBB_GROUP; ++g) m[g] = best[g];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
      for (int g = 0; g < OBB_GROUP; ++g) m[g] = fmax(m[g], __shfl_xor(m[g], d, 64));
    }
#pragma unroll
    for (int g = 0; g < OBB_GROUP; ++g) {
      const unsigned long long tie = __ballot(best[g] == m[g]);        // never empty: finite inputs, no NaN
      const int32_t win = __shfl(best_i[g], __ffsll(tie) - 1, 64);     // the lowest lane holds the smallest index
      if (lane == 0) {
        wval[wave][j0 + g] = m[g];
        widx[wave][j0 + g] = win;
      }
    }
  }
  __syncthreads();
  if (t < count) {
    double best = wval[0][t];
    int32_t best_i = widx[0][t];
#pragma unroll
    for (int s = 1; s < OBB_WAVES; ++s) {
      const double v = wval[s][t];
      const bool gt = v > best;
      best = gt ? v : best;
      best_i = gt ? widx[s][t] : best_i;
    }
    const size_t o = (size_t)blockIdx.x * (size_t)D + (size_t)(jb + t);
    pval[o] = best;
    pidx[o] = best_i;
  }
}

__global__ void __launch_bounds__(OBB_THREADS)
obb_finish_k(const double* __restrict__ pval, const int32_t* __restrict__ pidx, int64_t D, int64_t n_slices,
             double* __restrict__ value, int32_t* __restrict__ index) {
  const int64_t d = (int64_t)blockIdx.x * OBB_THREADS + threadIdx.x;
  if (d >= D) return;
  double best = pval[d];
  int32_t best_i = pidx[d];
#pragma unroll 8
  for (int64_t s = 1; s < n_slices; ++s) {                             // selects, no branch: the loads run ahead
    const size_t o = (size_t)s * (size_t)D + (size_t)d;
    const double v = pval[o];
    const int32_t i = pidx[o];
    const bool gt = v > best;                                          // strict: the earlier slice keeps a tie
    best = gt ? v : best;
    best_i = gt ? i : best_i;
  }
  value[d] = best;
  index[d] = best_i;
}

__global__ void __launch_bounds__(OBB_THREADS)
obb_candidates_k(const double* __restrict__ verts, int h, const double* __restrict__ normals,
                 const int32_t* __restrict__ edges, const double* __restrict__ edge_normals, int E,
                 double* __restrict__ volume, int32_t* __restrict__ edge_out, double* __restrict__ extents) {
  __shared__ double s_lo[OBB_THREADS], s_hi[OBB_THREADS], s_eu[OBB_THREADS], s_ev[OBB_THREADS];
  __shared__ int32_t s_edge[OBB_THREADS];
  const int t = (int)threadIdx.x;
  const int64_t k = blockIdx.x;
  const double nx = normals[3 * k], ny = normals[3 * k + 1], nz = normals[3 * k + 2];

  // the extent along the normal, once per workgroup
  double lo = __builtin_inf(), hi = -__builtin_inf();
  for (int i = t; i < h; i += OBB_THREADS) {
    const double s = obb_dot(verts[3 * i], verts[3 * i + 1], verts[3 * i + 2], nx, ny, nz);
    lo = fmin(lo, s);
    hi = fmax(hi, s);
  }
  s_lo[t] = lo;
  s_hi[t] = hi;
  __syncthreads();
  for (int w = OBB_THREADS / 2; w >= 1; w >>= 1) {
    if (t < w) {
      s_lo[t] = fmin(s_lo[t], s_lo[t + w]);
      s_hi[t] = fmax(s_hi[t], s_hi[t + w]);
    }
    __syncthreads();
  }
  const double en = s_hi[0] - s_lo[0];
  __syncthreads();                                                     // s_lo is written again below

  double best = __builtin_inf(), best_eu = 0.0, best_ev = 0.0;
  int32_t best_e = -1;
  for (int e = t; e < E; e += OBB_THREADS) {
    const double* q = edge_normals + 6 * (size_t)e;
    const double s1 = obb_dot(q[0], q[1], q[2], nx, ny, nz), s2 = obb_dot(q[3], q[4], q[5], nx, ny, nz);
    if (!((s1 <= OBB_SIL_EPS && s2 >= -OBB_SIL_EPS) || (s1 >= -OBB_SIL_EPS && s2 <= OBB_SIL_EPS))) continue;
    const int32_t i0 = edges[2 * e], i1 = edges[2 * e + 1];
    const double dx = verts[3 * i1] - verts[3 * i0], dy = verts[3 * i1 + 1] - verts[3 * i0 + 1],
                 dz = verts[3 * i1 + 2] - verts[3 * i0 + 2];
    const double dn = obb_dot(dx, dy, dz, nx, ny, nz);
    double ux = dx - dn * nx, uy = dy - dn * ny, uz = dz - dn * nz;
    const double uu = obb_dot(ux, uy, uz, ux, uy, uz), dd = obb_dot(dx, dy, dz, dx, dy, dz);
    if (!(uu > OBB_DIR_EPS * dd)) continue;
    const double len = sqrt(uu);
    ux /= len;
    uy /= len;
    uz /= len;
    const double vx = ny * uz - nz * uy, vy = nz * ux - nx * uz, vz = nx * uy - ny * ux;
    double ulo = __builtin_inf(), uhi = -__builtin_inf(), vlo = __builtin_inf(), vhi = -__builtin_inf();
    for (int i = 0; i < h; ++i) {
      const double px = verts[3 * i], py = verts[3 * i + 1], pz = verts[3 * i + 2];
      const double su = obb_dot(px, py, pz, ux, uy, uz), sv = obb_dot(px, py, pz, vx, vy, vz);
      ulo = fmin(ulo, su);
      uhi = fmax(uhi, su);
      vlo = fmin(vlo, sv);
      vhi = fmax(vhi, sv);
    }
    const double eu = uhi - ulo, ev = vhi - vlo, vol = en * eu * ev;
    if (vol < best) {                                                  // strict: the earlier edge keeps a tie
      best = vol;
      best_e = e;
      best_eu = eu;
      best_ev = ev;
    }
  }
  s_lo[t] = best;
  s_eu[t] = best_eu;
  s_ev[t] = best_ev;
  s_edge[t] = best_e;
  __syncthreads();
  if (t == 0) {
    int w = 0;
    for (int l = 1; l < OBB_THREADS; ++l) {
      if (s_edge[l] < 0) continue;
      if (s_edge[w] < 0 || s_lo[l] < s_lo[w] || (s_lo[l] == s_lo[w] && s_edge[l] < s_edge[w])) w = l;
    }
    volume[k] = s_lo[w];
    edge_out[k] = s_edge[w];
    extents[3 * k] = en;
    extents[3 * k + 1] = s_eu[w];
    extents[3 * k + 2] = s_ev[w];
  }
}

}  // namespace

extern "C" int64_t msdf_obb_support_workspace_bytes(int64_t n_points, int64_t n_planes) {
  if (!below_int32_max(n_points) || !below_int32_max(n_planes)) return -1;
  return workspace_floor(obb_slices(n_points) * n_planes * 12);        // < 2^20 * 2^31 * 12
}

extern "C" int msdf_obb_support(const float* points, int64_t n_points, const double* planes, int64_t n_planes,
                                void* workspace, double* value, int32_t* index, void* stream) {
  if (!below_int32_max(n_points) || !below_int32_max(n_planes)) return MSDF_ERR_ARG;
  if (n_planes == 0) return MSDF_OK;
  if (n_points == 0 || !points || !planes || !workspace || !value || !index) return MSDF_ERR_ARG;
  const int64_t n_slices = obb_slices(n_points);
  double* pval = (double*)workspace;
  int32_t* pidx = (int32_t*)(pval + (size_t)n_slices * (size_t)n_planes);
  const hipStream_t s = (hipStream_t)stream;
  const int64_t n_tiles = blocks_for(n_planes, OBB_TILE);
  for (int64_t tile0 = 0; tile0 < n_tiles; tile0 += OBB_MAX_TILES) {
    const int64_t tiles = n_tiles - tile0 < OBB_MAX_TILES ? n_tiles - tile0 : OBB_MAX_TILES;
    obb_support_k<<<dim3((unsigned)n_slices, (unsigned)tiles), OBB_THREADS, 0, s>>>(points, n_points, planes, n_planes,
                                                                                     tile0, pval, pidx);
  }
  obb_finish_k<<<blocks_for(n_planes, OBB_THREADS), OBB_THREADS, 0, s>>>(pval, pidx, n_planes, n_slices, value, index);
  return msdf_check_launch();
}

extern "C" int msdf_obb_candidates(const double* vertices, int64_t n_vertices, const double* normals,
                                   int64_t n_normals, const int32_t* edges, const double* edge_normals,
                                   int64_t n_edges, double* volume, int32_t* edge, double* extents, void* stream) {
  if (!below_int32_max(n_vertices) || !below_int32_max(n_normals) || !below_int32_max(n_edges)) return MSDF_ERR_ARG;
  if (n_normals == 0) return MSDF_OK;
  if (n_vertices == 0 || !vertices || !normals || !volume || !edge || !extents) return MSDF_ERR_ARG;
  if (n_edges > 0 && (!edges || !edge_normals)) return MSDF_ERR_ARG;
  obb_candidates_k<<<(unsigned)n_normals, OBB_THREADS, 0, (hipStream_t)stream>>>(
      vertices, (int)n_vertices, normals, edges, edge_normals, (int)n_edges, volume, edge, extents);
  return msdf_check_launch();
}
