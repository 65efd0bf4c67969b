// Exact nearest neighbour within a bound, through a uniform grid (ABI: include/monosdf_gridnn.h).  The DTU protocol uses
// only the distances below max_dist (dtu_eval/eval.py:120-134), so "the nearest reference point, if one lies within
// max_dist" is enough, and on thinned clouds it looks at a few hundred candidates per query where the brute-force
// search of nnsearch.hip looks at all of them.  What is reported is bit for bit what that search returns: both form the
// distance with nn_d2 and take the minimum over nn_word (tool_common.h, which states them; this object is built with
// the flags of nnsearch.o), and both take the same sqrtf.  No atomics: the same inputs give the same bits every call.
//
// Grid.  Cells of side h over the reference cloud's box; cell = floor((p - lo) / h) per axis in fp64 on the fp32
// coordinate, clamped to the grid (in fp64, before the conversion: a query may lie anywhere), linear index with z
// fastest.  The reference points are gathered into records `x y z index` (16 bytes) in cell order by the caller's
// stable sort; starts[c] is the first record of cell c, so the cells z0..z1 of one (x, y) column are the records
// starts[col + z0] .. starts[col + z1 + 1]: two table loads a column.
//
// Query: one lane per query, the queries visited in cell order so that the lanes of a wave walk nearly the same runs
// (records and table lines are then shared through L1 / L2); results go back to the queries' own positions.  A lane
// scans the cube of cells within Chebyshev radius k of its cell, k = 1, 2, 4, ... (the whole cube again each time:
// about 1.14 times the last cube in all, and no shell bookkeeping), and stops when
//     best_d2 <= (k h / SLACK)^2     or     k >= kmax = ceil(max_dist SLACK / h),          SLACK = 1 + 2^-10.
// Why that is exact.  A reference point outside cube k has a cell coordinate that differs from the query's by at least
// k + 1 on some axis, so its true coordinate differs by more than k h there (for a query whose cell was clamped the
// query is farther still); the fp64 cell arithmetic moves that by ~1e-16 and the fp32 rounding of d2 by ~3e-7
// relative, both far inside SLACK^2 - 1 = 2e-3.  So every point outside has an fp32 d2 > (k h / SLACK)^2: once best_d2
// is at or below that, no point outside ties or beats it.  At k = kmax every point outside has fp32 distance >
// (float) max_dist, so a best that passes the final test sqrtf(best_d2) <= (float) max_dist beats all of them (sqrtf is
// monotone), and a best that does not pass is not reported.  h, and so the grid, only ever changes the speed.
#include "tool_common.h"
#include "../../include/monosdf_gridnn.h"

namespace {

constexpr int GN_THREADS = 256;
constexpr int64_t GN_MAX_CELLS = MSDF_COUNT_MAX - 1;   // starts holds cells + 1 int32 entries
constexpr double GN_SLACK = 1.0 + 1.0 / 1024.0;
constexpr uint64_t GN_NONE = 0x7f800000ffffffffull;   // d2 = +inf, index -1: any point orders before it

struct GnGrid {
  double lo[3];
  double h;
  int n[3];
};

bool gn_grid_ok(double lx, double ly, double lz, double h, int nx, int ny, int nz) {
  const double inf = __builtin_inf();
  if (!positive_finite(h) || !(lx > -inf && lx < inf) || !(ly > -inf && ly < inf) || !(lz > -inf && lz < inf))
    return false;
  if (nx < 1 || ny < 1 || nz < 1) return false;
  return (int64_t)nx * ny <= GN_MAX_CELLS && (int64_t)nx * ny * nz <= GN_MAX_CELLS;
}

__device__ __forceinline__ int gn_cell(float p, double lo, double h, int n) {
  double c = floor(((double)p - lo) / h);
  const double top = (double)(n - 1);
  c = c < 0.0 ? 0.0 : c;
  c = c > top ? top : c;                                               // finite input: c is no NaN
  return (int)c;
}

__global__ void __launch_bounds__(GN_THREADS)
gn_cells_k(const float* __restrict__ pts, int64_t n, GnGrid g, int32_t* __restrict__ cells) {
  const int64_t i = (int64_t)blockIdx.x * GN_THREADS + threadIdx.x;
  if (i >= n) return;
  const int cx = gn_cell(pts[3 * i], g.lo[0], g.h, g.n[0]);
  const int cy = gn_cell(pts[3 * i + 1], g.lo[1], g.h, g.n[1]);
  const int cz = gn_cell(pts[3 * i + 2], g.lo[2], g.h, g.n[2]);
  cells[i] = (int32_t)(((int64_t)cx * g.n[1] + cy) * g.n[2] + cz);
}

__global__ void __launch_bounds__(GN_THREADS)
gn_records_k(const float* __restrict__ ref, const int64_t* __restrict__ order, int64_t n, v4f* __restrict__ rec) {
  const int64_t i = (int64_t)blockIdx.x * GN_THREADS + threadIdx.x;
  if (i >= n) return;
  const int64_t p = order[i];
  rec[i] = v4f{ref[3 * p], ref[3 * p + 1], ref[3 * p + 2], __uint_as_float((uint32_t)p)};
}

__global__ void __launch_bounds__(GN_THREADS)
gn_query_k(const float* __restrict__ query, const int64_t* __restrict__ qorder, int64_t Q,
           const v4f* __restrict__ rec, const int32_t* __restrict__ starts, GnGrid g, int kmax, float max_dist,
           float* __restrict__ dist, int32_t* __restrict__ idx) {
  const int64_t t = (int64_t)blockIdx.x * GN_THREADS + threadIdx.x;
  if (t >= Q) return;
  const int64_t q = qorder[t];
  const float qx = query[3 * q], qy = query[3 * q + 1], qz = query[3 * q + 2];
  const int64_t nx = g.n[0], ny = g.n[1], nz = g.n[2];
  const int64_t cx = gn_cell(qx, g.lo[0], g.h, g.n[0]);
  const int64_t cy = gn_cell(qy, g.lo[1], g.h, g.n[1]);
  const int64_t cz = gn_cell(qz, g.lo[2], g.h, g.n[2]);
  uint64_t best = GN_NONE;
  for (int64_t k = 1;;) {
    const int64_t x0 = cx - k > 0 ? cx - k : 0, x1 = cx + k < nx - 1 ? cx + k : nx - 1;
    const int64_t y0 = cy - k > 0 ? cy - k : 0, y1 = cy + k < ny - 1 ? cy + k : ny - 1;
    const int64_t z0 = cz - k > 0 ? cz - k : 0, z1 = cz + k < nz - 1 ? cz + k : nz - 1;
    for (int64_t x = x0; x <= x1; ++x) {
      for (int64_t y = y0; y <= y1; ++y) {
        const int64_t col = (x * ny + y) * nz;
        const int32_t a = starts[col + z0], b = starts[col + z1 + 1];
        for (int32_t r = a; r < b; ++r) {
          const v4f p = rec[r];
          const float dx = qx - p.x, dy = qy - p.y, dz = qz - p.z;
          const uint64_t key = nn_word(nn_d2(dx, dy, dz), __float_as_uint(p.w));
          best = key < best ? key : best;
        }
      }
    }
    const double bound = (double)k * g.h / GN_SLACK;
    if ((double)nn_word_d2(best) <= bound * bound || k >= kmax) break;
    k = 2 * k < kmax ? 2 * k : kmax;
  }
  const float d = sqrtf(nn_word_d2(best));
  const bool within = d <= max_dist;
  dist[q] = within ? d : __builtin_inff();
  idx[q] = within ? nn_word_index(best) : -1;
}

}  // namespace

extern "C" int64_t msdf_gnn_workspace_bytes(int64_t n_ref) {
  if (n_ref < 1 || !fits_int32(n_ref)) return -1;
  return workspace_floor(16 * n_ref);
}

extern "C" int msdf_gnn_cells(const float* points, int64_t n, double lo_x, double lo_y, double lo_z, double h, int n_x,
                              int n_y, int n_z, int32_t* cells, void* stream) {
  if (!fits_int32(n) || !gn_grid_ok(lo_x, lo_y, lo_z, h, n_x, n_y, n_z)) return MSDF_ERR_ARG;
  if (n == 0) return MSDF_OK;
  if (!points || !cells) return MSDF_ERR_ARG;
  const GnGrid g = {{lo_x, lo_y, lo_z}, h, {n_x, n_y, n_z}};
  gn_cells_k<<<blocks_for(n, GN_THREADS), GN_THREADS, 0, (hipStream_t)stream>>>(points, n, g, cells);
  return msdf_check_launch();
}

extern "C" int msdf_gnn_records(const float* ref, const int64_t* order, int64_t n_ref, void* records, void* stream) {
  if (n_ref < 1 || !fits_int32(n_ref) || !ref || !order || !records) return MSDF_ERR_ARG;
  gn_records_k<<<blocks_for(n_ref, GN_THREADS), GN_THREADS, 0, (hipStream_t)stream>>>(ref, order, n_ref, (v4f*)records);
  return msdf_check_launch();
}

extern "C" int msdf_gnn_query(const float* query, const int64_t* query_order, int64_t n_query, const void* records,
                              int64_t n_ref, const int32_t* starts, double lo_x, double lo_y, double lo_z, double h,
                              int n_x, int n_y, int n_z, double max_dist, float* dist, int32_t* idx, void* stream) {
  if (n_ref < 1 || !fits_int32(n_ref) || !fits_int32(n_query)) return MSDF_ERR_ARG;
  if (!gn_grid_ok(lo_x, lo_y, lo_z, h, n_x, n_y, n_z) || !positive_finite(max_dist)) return MSDF_ERR_ARG;
  if (n_query == 0) return MSDF_OK;
  if (!query || !query_order || !records || !starts || !dist || !idx) return MSDF_ERR_ARG;
  const GnGrid g = {{lo_x, lo_y, lo_z}, h, {n_x, n_y, n_z}};
  // a cube of radius max(n) around a cell of the grid is the whole grid: nothing lies outside it
  const int widest = n_x > n_y ? (n_x > n_z ? n_x : n_z) : (n_y > n_z ? n_y : n_z);
  const double rings = ceil(max_dist * GN_SLACK / h);
  const int kmax = rings < (double)widest ? (rings < 1.0 ? 1 : (int)rings) : widest;
  gn_query_k<<<blocks_for(n_query, GN_THREADS), GN_THREADS, 0, (hipStream_t)stream>>>(
      query, query_order, n_query, (const v4f*)records, starts, g, kmax, (float)max_dist, dist, idx);
  return msdf_check_launch();
}
