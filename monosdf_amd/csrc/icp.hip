// Point-to-point ICP on the device (ABI: include/monosdf_icp.h, which states the rule), the device half of
// utils/mesh_align.py.  One iteration is a chain of launches on the caller's stream with nothing read back:
//   * icp_transform_k:   y = T x, fp64 arithmetic rounded once to fp32, one point per lane
//   * (msdf_gnn_cells, a sort, msdf_gnn_query of gridnn.hip: the nearest target point within max_dist)
//   * icp_accumulate_k:  the shape of obb.hip's support kernel: a lane takes ICP_PPL = 8 CONSECUTIVE points, a workgroup
//                        of 256 lanes one slice of ICP_SLICE = 2048; 17 fp64 sums per lane, added over the lanes of a
//                        wave by the xor tree and over the four waves in ascending order -> one partial per slice
//   * icp_solve_k:       one wave: lane c adds component c of the slices in ascending order, lane 0 forms fitness and
//                        rmse, writes the log row, tests convergence and either sets `done` or solves T_{k+1}
// The state lives in device memory; every kernel first reads its `done` flag and returns if it is set, so the host may
// enqueue iterations blindly and look at the flag now and then.  No atomics, no workgroup waits on another.
//
// Built with -ffp-contract=off: every product and sum is rounded on its own, as the header states and the float64
// restatement of the tests (tests/icp_numpy.py) computes.
#include "tool_common.h"
#include "rotation_solve.h"
#include "../../include/monosdf_icp.h"

namespace {

constexpr int ICP_THREADS = 256;                        // 4 waves
constexpr int ICP_WAVES = ICP_THREADS / MSDF_WAVE;
constexpr int ICP_PPL = 8;                              // points per lane
constexpr int ICP_SLICE = ICP_THREADS * ICP_PPL;        // points per workgroup
constexpr int ICP_NS = 17;                              // sums per slice
constexpr int64_t ICP_MAX_ITERATION = 1 << 20;

struct IcpState {                                       // the header's layout; the log rows follow
  double T[16];
  double prev_fitness, prev_rmse;
  int32_t iteration, done;
};
static_assert(sizeof(IcpState) == 152, "the layout that include/monosdf_icp.h states");

inline int64_t icp_slices(int64_t n) { return blocks_for(n, ICP_SLICE); }

__global__ void __launch_bounds__(ICP_THREADS)
icp_transform_k(const float* __restrict__ src, int64_t n, const IcpState* __restrict__ st, float* __restrict__ out) {
  if (st->done) return;
  const int64_t i = (int64_t)blockIdx.x * ICP_THREADS + threadIdx.x;
  if (i >= n) return;
  const double x = (double)src[3 * i], y = (double)src[3 * i + 1], z = (double)src[3 * i + 2];
  out[3 * i] = (float)affine_row<0>(st->T, x, y, z);
  out[3 * i + 1] = (float)affine_row<1>(st->T, x, y, z);
  out[3 * i + 2] = (float)affine_row<2>(st->T, x, y, z);
}

__global__ void __launch_bounds__(ICP_THREADS)
icp_accumulate_k(const float* __restrict__ src, const float* __restrict__ moved, const float* __restrict__ tgt,
                 const int32_t* __restrict__ idx, int64_t n, int64_t m, const double* __restrict__ pivots,
                 const IcpState* __restrict__ st, double* __restrict__ part) {
  __shared__ double red[ICP_WAVES][ICP_NS];
  if (st->done) return;                                                // uniform over the launch
  const int t = (int)threadIdx.x, lane = lane_id(), wave = t / MSDF_WAVE;
  const int64_t first = (int64_t)blockIdx.x * ICP_SLICE + (int64_t)t * ICP_PPL;
  double cs[3], ct[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    cs[a] = pivots[a];
    ct[a] = pivots[3 + a];
  }
  double acc[ICP_NS];
#pragma unroll
  for (int k = 0; k < ICP_NS; ++k) acc[k] = 0.0;
#pragma unroll
  for (int k = 0; k < ICP_PPL; ++k) {
    const int64_t i = first + k;
    if (i >= n) continue;
    const int64_t j = idx[i];
    if (j < 0 || j >= m) continue;                                     // no correspondence
    double p[3], q[3], d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double qa = (double)tgt[3 * j + a];
      p[a] = (double)src[3 * i + a] - cs[a];
      q[a] = qa - ct[a];
      d[a] = (double)moved[3 * i + a] - qa;
    }
    acc[0] += 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      acc[1 + a] += p[a];
      acc[4 + a] += q[a];
#pragma unroll
      for (int b = 0; b < 3; ++b) acc[7 + 3 * a + b] += p[a] * q[b];
    }
    acc[16] += (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
  }
#pragma unroll
  for (int k = 0; k < ICP_NS; ++k) {
    const double v = wave_sum(acc[k]);
    if (lane == 0) red[wave][k] = v;
  }
  __syncthreads();
  if (t < ICP_NS) part[(size_t)blockIdx.x * ICP_NS + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

__global__ void __launch_bounds__(MSDF_WAVE)
icp_solve_k(const double* __restrict__ part, int64_t n_slices, int64_t n, const double* __restrict__ pivots,
            int max_iteration, double relative_fitness, double relative_rmse, IcpState* __restrict__ st) {
  if (st->done) return;
  const int lane = lane_id();
  double v = 0.0;
  if (lane < ICP_NS) {
#pragma unroll 8
    for (int64_t s = 0; s < n_slices; ++s) v += part[(size_t)s * ICP_NS + lane];   // ascending slices
  }
  double sum[ICP_NS];
#pragma unroll
  for (int k = 0; k < ICP_NS; ++k) sum[k] = __shfl(v, k, 64);
  if (lane != 0) return;

  const int k = st->iteration;
  if (k < 0 || k > max_iteration) {                                    // not a state of this run: touch no log row
    st->done = 1;
    return;
  }
  const double count = sum[0];
  const double fitness = count > 0.0 ? count / (double)n : 0.0;
  const double rmse = count > 0.0 ? sqrt(sum[16] / count) : 0.0;
  double* log = (double*)(st + 1) + 3 * (size_t)k;
  log[0] = fitness;
  log[1] = rmse;
  log[2] = count;
  const bool converged = k >= 1 && fabs(fitness - st->prev_fitness) < relative_fitness &&
                         fabs(rmse - st->prev_rmse) < relative_rmse;
  if (converged || k >= max_iteration) {
    st->done = 1;
    return;
  }
  st->prev_fitness = fitness;
  st->prev_rmse = rmse;
  st->iteration = k + 1;
  if (!(count > 0.0)) return;                                          // no correspondence: T stays

  double mp[3], mq[3], h[9], r[9];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    mp[a] = sum[1 + a] / count;
    mq[a] = sum[4 + a] / count;
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) h[3 * a + b] = sum[7 + 3 * a + b] / count - mp[a] * mq[b];
  }
  solve_rotation(h, r);
  double P[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) P[a] = pivots[a] + mp[a];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    st->T[4 * a] = r[3 * a];
    st->T[4 * a + 1] = r[3 * a + 1];
    st->T[4 * a + 2] = r[3 * a + 2];
    st->T[4 * a + 3] = (pivots[3 + a] + mq[a]) - ((r[3 * a] * P[0] + r[3 * a + 1] * P[1]) + r[3 * a + 2] * P[2]);
  }
  st->T[12] = 0.0;
  st->T[13] = 0.0;
  st->T[14] = 0.0;
  st->T[15] = 1.0;
}

}  // namespace

extern "C" int64_t msdf_icp_state_bytes(int64_t max_iteration) {
  if (max_iteration < 0 || max_iteration > ICP_MAX_ITERATION) return -1;
  return (int64_t)sizeof(IcpState) + (max_iteration + 1) * 24;
}

extern "C" int64_t msdf_icp_workspace_bytes(int64_t n) {
  if (!below_int32_max(n)) return -1;
  return workspace_floor(icp_slices(n) * ICP_NS * 8);                  // < 2^20 * 136
}

extern "C" int msdf_icp_transform(const float* source, int64_t n, const void* state, float* y, void* stream) {
  if (!below_int32_max(n) || !state) return MSDF_ERR_ARG;
  if (n == 0) return MSDF_OK;
  if (!source || !y) return MSDF_ERR_ARG;
  icp_transform_k<<<blocks_for(n, ICP_THREADS), ICP_THREADS, 0, (hipStream_t)stream>>>(source, n,
                                                                                       (const IcpState*)state, y);
  return msdf_check_launch();
}

extern "C" int msdf_icp_accumulate(const float* source, const float* y, const float* target, const int32_t* idx,
                                   int64_t n, int64_t m, const double* pivots, const void* state, void* workspace,
                                   void* stream) {
  if (!below_int32_max(n) || !below_int32_max(m) || !state || !pivots) return MSDF_ERR_ARG;
  if (n == 0) return MSDF_OK;
  if (!source || !y || !idx || !workspace || (m > 0 && !target)) return MSDF_ERR_ARG;
  icp_accumulate_k<<<(unsigned)icp_slices(n), ICP_THREADS, 0, (hipStream_t)stream>>>(
      source, y, target, idx, n, m, pivots, (const IcpState*)state, (double*)workspace);
  return msdf_check_launch();
}

extern "C" int msdf_icp_solve(const void* workspace, int64_t n, const double* pivots, int64_t max_iteration,
                              double relative_fitness, double relative_rmse, void* state, void* stream) {
  if (!below_int32_max(n) || max_iteration < 0 || max_iteration > ICP_MAX_ITERATION || !state || !pivots)
    return MSDF_ERR_ARG;
  if (n > 0 && !workspace) return MSDF_ERR_ARG;
  icp_solve_k<<<1, MSDF_WAVE, 0, (hipStream_t)stream>>>((const double*)workspace, icp_slices(n), n, pivots,
                                                        (int)max_iteration, relative_fitness, relative_rmse,
                                                        (IcpState*)state);
  return msdf_check_launch();
}
