// The DTU evaluation protocol on the device: what the reference's dtu_eval/evaluate_single_scene.py (cull_scan) and
// dtu_eval/eval.py do on the CPU before the two closing nearest-neighbour queries (those reuse csrc/nnsearch.hip).
// Every rule here is integer, boolean, separately rounded fp32 or fp64 (this object is built with -ffp-contract=off),
// so the numpy restatements of tests/dtu_numpy.py are matched exactly.  No floating-point atomics anywhere.
//
// Mask dilation (skimage binary_dilation with disk(r); evaluate_single_scene.py:80-82).  The disk is 2r+1 row runs of
// half-width w(dy) = floor(sqrt(r^2 - dy^2)) (integers, from the host).  The views are packed to one bit per pixel
// (32-bit words, bit b of word k = pixel 32 k + b); an output word ORs, over the 2r+1 source rows, the source row
// dilated horizontally by w(dy): the word with its two neighbours as one 128-bit value, OR-ed with itself shifted by
// 1, 2, 4, ... until a run of 2 w + 1 is covered (log steps), shifted back by w.  About 25 x 5 shift-ORs per 32 pixels
// in place of 441 taps per pixel.  Pixels outside the image are unset.
//
// Vertex rule (evaluate_single_scene.py:69-93): per vertex and view (u, v, z) = P (x, 1) with
// ((P0 x + P1 y) + P2 z) + P3 per row, px = u / (z + 1e-6), py likewise, valid iff 0 < px < W-1 and 0 < py < H-1,
// pixel = (rint(px), rint(py)) half to even; kept iff in every view not valid or the dilated mask is set there.
//
// Lattice sampler (eval.py:54-71) in fp64: one wave per face.  Row i of the lattice keeps the candidates j with
// a_i + b_j < 1; b_j and so the sum are non-decreasing in j, so they are a prefix [0, c_i), found from an estimate
// corrected by the exact test.  Count: rows spread over the lanes, summed by shuffles.  Emit: 64 rows at a time, their
// counts scanned across the wave, the points of those rows spread evenly over the lanes (a six-step search through
// the scanned counts by shuffles gives each point its row), written at the face's offset: the order is face, i, j
// whatever the scheduling, and neither an empty face nor one of thousands of points runs a long loop on one lane.
//
// Radius thinning (eval.py:86-94): the lexicographically first maximal independent set of the graph {d^2 <= r^2}
// under the visiting order.  Points are sorted by the key of their grid cell (side >= r (1 + 2^-10), so two points
// within r are at most one cell apart); per point the nine runs of three z-adjacent cells (consecutive keys) are
// looked up once.  A round: every undecided point scans its earlier-ranked neighbours; one kept -> removed, else one
// undecided -> stays, else kept.  States only move from undecided to their final value, so the update is in place and
// the result does not depend on what a racing read sees, only the number of rounds does.
#include "tool_common.h"

namespace {

constexpr int DT_THREADS = 256;
constexpr int DT_MAX_RADIUS = 32;                  // half-width <= one word: a word and its two neighbours suffice
constexpr int64_t DT_MAX_PIXELS = 1ll << 37;
constexpr int DT_CELL_BITS = 21;
constexpr int64_t DT_CELL_MAX = (1ll << DT_CELL_BITS) - 2;   // cells of points lie in [1, DT_CELL_MAX]
constexpr double LAT_MAX_CANDIDATES = 17179869184.0;         // 2^34: such a face alone has >= 2^31 points
constexpr int64_t LAT_TOO_MANY = 1ll << 40;

typedef unsigned __int128 u128;

struct DtDisk {
  int r;
  int8_t hw[2 * DT_MAX_RADIUS + 1];                // hw[dy + r]
};

// ---------------------------------------------------------------- dilation

__global__ void __launch_bounds__(DT_THREADS)
dt_pack_k(const uint8_t* __restrict__ masks, int64_t rows, int W, int Wd, uint32_t* __restrict__ packed) {
  const int64_t idx = (int64_t)blockIdx.x * DT_THREADS + threadIdx.x;
  if (idx >= rows * Wd) return;
  const int64_t row = idx / Wd;
  const int w = (int)(idx - row * Wd);
  const uint8_t* src = masks + row * W;
  uint32_t word = 0;
  for (int b = 0; b < 32; ++b) {
    const int x = w * 32 + b;
    if (x < W && src[x] != 0) word |= 1u << b;
  }
  packed[idx] = word;
}

__global__ void __launch_bounds__(DT_THREADS)
dt_dilate_k(const uint32_t* __restrict__ packed, int64_t rows, int H, int Wd, DtDisk disk,
            uint32_t* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * DT_THREADS + threadIdx.x;
  if (idx >= rows * Wd) return;
  const int64_t row = idx / Wd;
  const int w = (int)(idx - row * Wd);
  const int y = (int)(row % H);
  uint32_t acc = 0;
  for (int dy = -disk.r; dy <= disk.r; ++dy) {
    const int yy = y + dy;
    if (yy < 0 || yy >= H) continue;
    const uint32_t* src = packed + (row + dy) * Wd;
    const uint32_t lo = w > 0 ? src[w - 1] : 0u, mid = src[w], hi = w + 1 < Wd ? src[w + 1] : 0u;
    if ((lo | mid | hi) == 0u) continue;
    const int hw = disk.hw[dy + disk.r];
    u128 v = ((u128)hi << 64) | ((u128)mid << 32) | (u128)lo;
    const int run = 2 * hw + 1;
    for (int have = 1; have < run;) {                                  // v covers `have` consecutive shifts
      const int s = have < run - have ? have : run - have;
      v |= v << s;
      have += s;
    }
    acc |= (uint32_t)(v >> (32 + hw));
  }
  out[idx] = acc;
}

__global__ void __launch_bounds__(DT_THREADS)
dt_unpack_k(const uint32_t* __restrict__ packed, int64_t pixels, int W, int Wd, uint8_t* __restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * DT_THREADS + threadIdx.x;
  if (idx >= pixels) return;
  const int64_t row = idx / W;
  const int x = (int)(idx - row * W);
  out[idx] = (uint8_t)((packed[row * Wd + (x >> 5)] >> (x & 31)) & 1u);
}

// ---------------------------------------------------------------- vertex rule

__global__ void __launch_bounds__(DT_THREADS)
dt_mask_vertices_k(const float* __restrict__ verts, int64_t n, const float* __restrict__ proj, int n_views,
                   const uint8_t* __restrict__ dilated, int H, int W, uint8_t* __restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * DT_THREADS + threadIdx.x;
  if (i >= n) return;
  const float x = verts[3 * i], y = verts[3 * i + 1], z = verts[3 * i + 2];
  const float wmax = (float)(W - 1), hmax = (float)(H - 1);
  uint8_t kept = 1;
  for (int v = 0; v < n_views; ++v) {
    const float* P = proj + 12 * v;                                    // same address in every lane
    const float pu = affine_row<0>(P, x, y, z), pv = affine_row<1>(P, x, y, z), pz = affine_row<2>(P, x, y, z);
    const float den = pz + 1e-6f;
    const float px = pu / den, py = pv / den;
    const bool valid = px > 0.0f && px < wmax && py > 0.0f && py < hmax;    // false for NaN
    if (!valid) continue;
    const int ix = (int)rintf(px), iy = (int)rintf(py);                // in [0, W-1] x [0, H-1] by the test above
    if (dilated[((int64_t)v * H + iy) * W + ix] == 0) {
      kept = 0;
      break;
    }
  }
  keep[i] = kept;
}

// ---------------------------------------------------------------- lattice sampler

struct LatFace {
  double p0[3], v1[3], v2[3];
  double m1, m2;                                   // max(n, 1e-7)
  int64_t rows, cols;                              // n1 + 1, n2 + 1; rows = 0: the face gives nothing
  bool too_many;
};

__device__ __forceinline__ double lat_norm(const double* v) {
  return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
}

__device__ LatFace lat_face(const float* __restrict__ verts, int64_t n_verts, const int32_t* __restrict__ faces,
                            int64_t f, double density) {
  LatFace L;
  L.rows = 0;
  L.cols = 0;
  L.too_many = false;
  L.m1 = L.m2 = 1.0;
  const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  if (i0 < 0 || i0 >= n_verts || i1 < 0 || i1 >= n_verts || i2 < 0 || i2 >= n_verts) return L;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    L.p0[d] = (double)verts[3 * i0 + d];
    L.v1[d] = (double)verts[3 * i1 + d] - L.p0[d];
    L.v2[d] = (double)verts[3 * i2 + d] - L.p0[d];
  }
  const double l1 = lat_norm(L.v1), l2 = lat_norm(L.v2);
  double c[3];
  c[0] = L.v1[1] * L.v2[2] - L.v1[2] * L.v2[1];
  c[1] = L.v1[2] * L.v2[0] - L.v1[0] * L.v2[2];
  c[2] = L.v1[0] * L.v2[1] - L.v1[1] * L.v2[0];
  const double area2 = lat_norm(c);
  if (!(area2 > 0.0)) return L;
  const double thr = density * sqrt(l1 * l2 / area2);
  const double n1 = floor(l1 / thr), n2 = floor(l2 / thr);
  if (!(n1 >= 1.0 && n2 >= 1.0)) return L;         // n = 0: every candidate is 0.5 / 1e-7, none below 1; NaN: nothing
  if ((n1 + 1.0) * (n2 + 1.0) >= LAT_MAX_CANDIDATES) {
    L.too_many = true;
    return L;
  }
  L.m1 = fmax(n1, 1e-7);
  L.m2 = fmax(n2, 1e-7);
  L.rows = (int64_t)n1 + 1;
  L.cols = (int64_t)n2 + 1;
  return L;
}

__device__ __forceinline__ bool lat_keep(double a, int64_t j, double m2) {
  return a + ((double)j + 0.5) / m2 < 1.0;
}

// how many j in [0, cols) pass lat_keep: they are a prefix, since the test is monotone in j
__device__ int64_t lat_row_count(double a, double m2, int64_t cols) {
  const double t = ceil((1.0 - a) * m2 - 0.5);
  int64_t c = !(t > 0.0) ? 0 : (t >= (double)cols ? cols : (int64_t)t);
  while (c > 0 && !lat_keep(a, c - 1, m2)) --c;
  while (c < cols && lat_keep(a, c, m2)) ++c;
  return c;
}

__device__ __forceinline__ int64_t lat_row(const LatFace& L, int64_t i) {
  return i < L.rows ? lat_row_count(((double)i + 0.5) / L.m1, L.m2, L.cols) : 0;
}

__global__ void __launch_bounds__(DT_THREADS)
dt_lattice_count_k(const float* __restrict__ verts, int64_t n_verts, const int32_t* __restrict__ faces,
                   int64_t n_faces, double density, int64_t* __restrict__ counts) {
  const int64_t f = (int64_t)blockIdx.x * (DT_THREADS / MSDF_WAVE) + (threadIdx.x >> 6);   // wave-uniform
  if (f >= n_faces) return;
  const int lane = lane_id();
  const LatFace L = lat_face(verts, n_verts, faces, f, density);
  long long sum = 0;
  for (int64_t i = lane; i < L.rows; i += MSDF_WAVE) sum += lat_row(L, i);
  sum = wave_sum(sum);
  if (lane == 0) counts[f] = L.too_many ? LAT_TOO_MANY : (int64_t)sum;
}

__global__ void __launch_bounds__(DT_THREADS)
dt_lattice_emit_k(const float* __restrict__ verts, int64_t n_verts, const int32_t* __restrict__ faces,
                  int64_t n_faces, double density, const int64_t* __restrict__ offsets, int64_t n_points,
                  float* __restrict__ out) {
  const int64_t f = (int64_t)blockIdx.x * (DT_THREADS / MSDF_WAVE) + (threadIdx.x >> 6);   // wave-uniform
  if (f >= n_faces) return;
  const int64_t base = offsets[f];
  if (offsets[f + 1] <= base) return;
  const int lane = lane_id();
  const LatFace L = lat_face(verts, n_verts, faces, f, density);
  int64_t done = 0;
  for (int64_t i0 = 0; i0 < L.rows; i0 += MSDF_WAVE) {                  // every lane runs every shuffle below
    const long long c = lat_row(L, i0 + lane);
    const long long incl = wave_incl_scan(c);
    const long long total = __shfl(incl, MSDF_WAVE - 1, MSDF_WAVE);
    for (long long pb = 0; pb < total; pb += MSDF_WAVE) {
      const long long p = pb + lane;
      int row = 0;                                                     // rows of this pass with incl <= p
#pragma unroll
      for (int step = 32; step >= 1; step >>= 1) {
        const long long v = __shfl(incl, row + step - 1, MSDF_WAVE);
        if (v <= p) row += step;
      }
      const int src = row < MSDF_WAVE ? row : MSDF_WAVE - 1;
      const long long before = __shfl(incl - c, src, MSDF_WAVE);
      const int64_t at = base + done + p;
      if (p < total && at < n_points && at < offsets[f + 1]) {
        const double a = ((double)(i0 + row) + 0.5) / L.m1;
        const double b = ((double)(p - before) + 0.5) / L.m2;
#pragma unroll
        for (int d = 0; d < 3; ++d) out[3 * at + d] = (float)((L.v1[d] * a + L.v2[d] * b) + L.p0[d]);
      }
    }
    done += total;
  }
}

// ---------------------------------------------------------------- radius thinning

struct ThinWs {
  v4f* rec;                                        // [n] x y z and the visiting rank (as bits), in cell order
  int32_t* range;                                  // [18][n]: begin / end of the nine cell runs
  uint8_t* state;                                  // [n] 0 undecided, 1 kept, 2 removed
};

__host__ __device__ inline ThinWs thin_ws(void* workspace, int64_t n) {
  ThinWs w;
  char* p = (char*)workspace;
  w.rec = (v4f*)p;
  w.range = (int32_t*)(p + 16 * n);
  w.state = (uint8_t*)(p + 16 * n + 72 * n);
  return w;
}

__global__ void __launch_bounds__(DT_THREADS)
dt_thin_keys_k(const float* __restrict__ pts, int64_t n, double lx, double ly, double lz, double cell,
               int64_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * DT_THREADS + threadIdx.x;
  if (i >= n) return;
  const double lo[3] = {lx, ly, lz};
  int64_t key = 0;
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    int64_t c = (int64_t)floor(((double)pts[3 * i + d] - lo[d]) / cell) + 1;
    c = c < 1 ? 1 : (c > DT_CELL_MAX ? DT_CELL_MAX : c);
    key = (key << DT_CELL_BITS) | c;
  }
  keys[i] = key;
}

__device__ int32_t thin_lower_bound(const int64_t* __restrict__ keys, int32_t lo, int32_t hi, int64_t k) {
  while (lo < hi) {                                                    // first position in [lo, hi) with keys >= k
    const int32_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(DT_THREADS)
dt_thin_prepare_k(const float* __restrict__ pts, const int64_t* __restrict__ perm, const int64_t* __restrict__ rank,
                  const int64_t* __restrict__ keys, int64_t n, ThinWs w) {
  const int64_t s = (int64_t)blockIdx.x * DT_THREADS + threadIdx.x;
  if (s >= n) return;
  int64_t p = perm[s];
  p = p < 0 ? 0 : (p >= n ? n - 1 : p);
  const int64_t rk = rank ? rank[p] : p;
  w.rec[s] = v4f{pts[3 * p], pts[3 * p + 1], pts[3 * p + 2], __int_as_float((int32_t)rk)};
  w.state[s] = 0;
  const int64_t key = keys[s];
  int k = 0;
  for (int dx = -1; dx <= 1; ++dx)
    for (int dy = -1; dy <= 1; ++dy, ++k) {
      // cells lie in [1, 2^21 - 2] per axis, so a neighbour's key has no carry and z - 1, z, z + 1 are consecutive
      const int64_t first = key + dx * (1ll << (2 * DT_CELL_BITS)) + dy * (1ll << DT_CELL_BITS) - 1;
      const int32_t b = thin_lower_bound(keys, 0, (int32_t)n, first);
      const int32_t e = thin_lower_bound(keys, b, (int32_t)n, first + 3);
      w.range[(int64_t)(2 * k) * n + s] = b;
      w.range[(int64_t)(2 * k + 1) * n + s] = e;
    }
}

__global__ void __launch_bounds__(DT_THREADS)
dt_thin_round_k(ThinWs w, int64_t n, double r2, uint32_t* __restrict__ undecided) {
  const int64_t s = (int64_t)blockIdx.x * DT_THREADS + threadIdx.x;
  bool waits = false;
  if (s < n && w.state[s] == 0) {
    const v4f me = w.rec[s];
    const int32_t rk = __float_as_int(me.w);
    const double x = (double)me.x, y = (double)me.y, z = (double)me.z;
    bool removed = false;
    for (int k = 0; k < 9 && !removed; ++k) {
      const int32_t b = w.range[(int64_t)(2 * k) * n + s], e = w.range[(int64_t)(2 * k + 1) * n + s];
      for (int32_t q = b; q < e; ++q) {
        const v4f o = w.rec[q];
        if (__float_as_int(o.w) >= rk) continue;                       // later in the order, or this point itself
        const double dx = x - (double)o.x, dy = y - (double)o.y, dz = z - (double)o.z;
        if (!(((dx * dx + dy * dy) + dz * dz) <= r2)) continue;
        const uint8_t st = __atomic_load_n(&w.state[q], __ATOMIC_RELAXED);
        if (st == 1) {
          removed = true;
          break;
        }
        waits = waits || st == 0;
      }
    }
    if (removed) {
      w.state[s] = 2;
      waits = false;
    } else if (!waits) {
      w.state[s] = 1;
    }
  }
  const unsigned long long m = __ballot(waits);
  if (lane_id() == 0 && m != 0) atomicAdd(undecided, (uint32_t)__popcll(m));
}

__global__ void __launch_bounds__(DT_THREADS)
dt_thin_finish_k(ThinWs w, const int64_t* __restrict__ perm, int64_t n, uint8_t* __restrict__ keep) {
  const int64_t s = (int64_t)blockIdx.x * DT_THREADS + threadIdx.x;
  if (s >= n) return;
  const int64_t p = perm[s];
  if (p >= 0 && p < n) keep[p] = w.state[s] == 1 ? 1 : 0;
}

bool dilate_sizes_ok(int n, int H, int W, int radius) {
  return n >= 0 && H >= 1 && W >= 1 && radius >= 0 && radius <= DT_MAX_RADIUS &&
         (int64_t)n * H * (int64_t)W <= DT_MAX_PIXELS;
}

int64_t dilate_words(int n, int H, int W) { return (int64_t)n * H * ((W + 31) / 32); }

}  // namespace

extern "C" int64_t msdf_dtu_dilate_workspace_bytes(int n_views, int height, int width) {
  if (!dilate_sizes_ok(n_views, height, width, 0)) return -1;
  return workspace_floor(2 * 4 * dilate_words(n_views, height, width));
}

extern "C" int msdf_dtu_dilate(const uint8_t* masks, int n_views, int height, int width, int radius, void* workspace,
                               uint8_t* out, void* stream) {
  if (!dilate_sizes_ok(n_views, height, width, radius)) return MSDF_ERR_ARG;
  if (n_views == 0) return MSDF_OK;
  if (!masks || !workspace || !out) return MSDF_ERR_ARG;
  DtDisk disk;
  disk.r = radius;
  for (int dy = -radius; dy <= radius; ++dy) {
    int w = 0;
    while ((w + 1) * (w + 1) + dy * dy <= radius * radius) ++w;        // floor(sqrt(r^2 - dy^2)) in integers
    disk.hw[dy + radius] = (int8_t)w;
  }
  const hipStream_t s = (hipStream_t)stream;
  const int Wd = (width + 31) / 32;
  const int64_t rows = (int64_t)n_views * height, words = rows * Wd, pixels = rows * width;
  uint32_t* packed = (uint32_t*)workspace;
  uint32_t* grown = packed + words;
  dt_pack_k<<<blocks_for(words, DT_THREADS), DT_THREADS, 0, s>>>(masks, rows, width, Wd, packed);
  dt_dilate_k<<<blocks_for(words, DT_THREADS), DT_THREADS, 0, s>>>(packed, rows, height, Wd, disk, grown);
  dt_unpack_k<<<blocks_for(pixels, DT_THREADS), DT_THREADS, 0, s>>>(grown, pixels, width, Wd, out);
  return msdf_check_launch();
}

extern "C" int msdf_dtu_mask_vertices(const float* verts, int64_t n_verts, const float* proj, int n_views,
                                      const uint8_t* dilated, int height, int width, uint8_t* keep, void* stream) {
  if (!fits_int32(n_verts) || !dilate_sizes_ok(n_views, height, width, 0)) return MSDF_ERR_ARG;
  if (n_verts == 0) return MSDF_OK;
  if (!verts || !keep || (n_views > 0 && (!proj || !dilated))) return MSDF_ERR_ARG;
  dt_mask_vertices_k<<<blocks_for(n_verts, DT_THREADS), DT_THREADS, 0, (hipStream_t)stream>>>(verts, n_verts, proj,
                                                                                              n_views, dilated, height,
                                                                                              width, keep);
  return msdf_check_launch();
}

static bool lattice_args_ok(int64_t n_verts, int64_t n_faces, double density) {
  return fits_int32(n_verts) && fits_int32(n_faces) && positive_finite(density);
}

extern "C" int msdf_dtu_lattice_count(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                      double density, int64_t* counts, void* stream) {
  if (!lattice_args_ok(n_verts, n_faces, density)) return MSDF_ERR_ARG;
  if (n_faces == 0) return MSDF_OK;
  if (!verts || !faces || !counts) return MSDF_ERR_ARG;
  const unsigned blocks = (unsigned)blocks_for(n_faces, DT_THREADS / MSDF_WAVE);   // a wave per face
  dt_lattice_count_k<<<blocks, DT_THREADS, 0, (hipStream_t)stream>>>(verts, n_verts, faces, n_faces, density, counts);
  return msdf_check_launch();
}

extern "C" int msdf_dtu_lattice_emit(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                     double density, const int64_t* offsets, int64_t n_points, float* out,
                                     void* stream) {
  if (!lattice_args_ok(n_verts, n_faces, density) || !fits_int32(n_points)) return MSDF_ERR_ARG;
  if (n_faces == 0 || n_points == 0) return MSDF_OK;
  if (!verts || !faces || !offsets || !out) return MSDF_ERR_ARG;
  const unsigned blocks = (unsigned)blocks_for(n_faces, DT_THREADS / MSDF_WAVE);   // a wave per face
  dt_lattice_emit_k<<<blocks, DT_THREADS, 0, (hipStream_t)stream>>>(verts, n_verts, faces, n_faces, density, offsets,
                                                                    n_points, out);
  return msdf_check_launch();
}

extern "C" int64_t msdf_dtu_thin_workspace_bytes(int64_t n) {
  if (!fits_int32(n)) return -1;
  return workspace_floor(16 * n + 72 * n + n);
}

extern "C" int msdf_dtu_thin_keys(const float* points, int64_t n, double lo_x, double lo_y, double lo_z, double cell,
                                  int64_t* keys, void* stream) {
  if (!fits_int32(n) || !positive_finite(cell)) return MSDF_ERR_ARG;
  if (n == 0) return MSDF_OK;
  if (!points || !keys) return MSDF_ERR_ARG;
  dt_thin_keys_k<<<blocks_for(n, DT_THREADS), DT_THREADS, 0, (hipStream_t)stream>>>(points, n, lo_x, lo_y, lo_z, cell,
                                                                                    keys);
  return msdf_check_launch();
}

extern "C" int msdf_dtu_thin_prepare(const float* points, const int64_t* perm, const int64_t* rank,
                                     const int64_t* sorted_keys, int64_t n, void* workspace, void* stream) {
  if (!fits_int32(n)) return MSDF_ERR_ARG;
  if (n == 0) return MSDF_OK;
  if (!points || !perm || !sorted_keys || !workspace) return MSDF_ERR_ARG;
  dt_thin_prepare_k<<<blocks_for(n, DT_THREADS), DT_THREADS, 0, (hipStream_t)stream>>>(points, perm, rank, sorted_keys,
                                                                                       n, thin_ws(workspace, n));
  return msdf_check_launch();
}

extern "C" int msdf_dtu_thin_round(void* workspace, int64_t n, double radius, uint32_t* undecided, void* stream) {
  if (!fits_int32(n) || !positive_finite(radius)) return MSDF_ERR_ARG;
  if (!undecided) return MSDF_ERR_ARG;
  const hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(undecided, 0, sizeof(uint32_t), s) != hipSuccess) return MSDF_ERR_LAUNCH;
  if (n == 0) return MSDF_OK;
  if (!workspace) return MSDF_ERR_ARG;
  dt_thin_round_k<<<blocks_for(n, DT_THREADS), DT_THREADS, 0, s>>>(thin_ws(workspace, n), n, radius * radius,
                                                                   undecided);
  return msdf_check_launch();
}

extern "C" int msdf_dtu_thin_finish(const void* workspace, const int64_t* perm, int64_t n, uint8_t* keep,
                                    void* stream) {
  if (!fits_int32(n)) return MSDF_ERR_ARG;
  if (n == 0) return MSDF_OK;
  if (!workspace || !perm || !keep) return MSDF_ERR_ARG;
  dt_thin_finish_k<<<blocks_for(n, DT_THREADS), DT_THREADS, 0, (hipStream_t)stream>>>(thin_ws((void*)workspace, n),
                                                                                      perm, n, keep);
  return msdf_check_launch();
}
