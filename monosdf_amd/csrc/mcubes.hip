// Marching cubes on a fp32 volume [nx, ny, nz] (C order, axis 0 = x): the mesh extraction of
// plots.get_surface_sliding (skimage.measure.marching_cubes, utils/plots.py:199-205) on the device.
//
// Wave64-native layout: word w covers the linear voxel indices [64 w, 64 w + 64), one lane per voxel.  Voxel p owns
// the grid edges p -> p + e_a (a = x, y, z, when inside the volume) and, when it is a cell (i < nx-1, j < ny-1,
// k < nz-1), the cube with p as corner 0.  Four passes:
//   classify   every lane reads its 8 corners; three ballots give the word's ownership masks (edges that cross the
//              level), a wave sum its triangle count (table mc_tables.h)
//   scan       exclusive scans of the per-word vertex / triangle counts: block scans of 1024 words, one workgroup over
//              the block sums (which also writes the two totals), add-back
//   vertices   words with crossing edges: vertex id = word base + popcount of the masks below the lane (order: linear
//              voxel index, then axis); position and gradient-normal interpolated along the edge
//   faces      words with triangles: every cell recomputes its code; a cell edge maps to (owner voxel, axis) and so to
//              its vertex id through the owner word's base and masks (order: linear cell index, then table order)
// Every output position follows from the scans: no atomics, so results are bitwise identical run to run.
#include "tool_common.h"
#define MC_TABLE static __constant__ const
#include "mc_tables.h"

namespace {

constexpr int MC_THREADS = 256;             // 4 waves
constexpr int MC_SCAN_WORDS = 1024;         // words per block of the first scan level (256 threads x 4)
constexpr int MC_CLASSIFY_WORDS = 4;        // words per wave of the classify pass, their loads in flight together
constexpr int MC_EMIT_WORDS = 8;            // words per wave of the emit passes (active ones are visited in turn)

// per word: ownership masks of the x / y / z edges, then (after the scan) the word's first vertex and triangle id
struct McWord {
  uint64_t m[3];
  uint32_t vbase, tbase;
};
static_assert(sizeof(McWord) == 32, "McWord layout");

struct McLayout {
  int64_t n_words, n_blocks;
  size_t words_off, counts_off, bsum_off, total;
};

McLayout mc_layout(int nx, int ny, int nz) {
  McLayout L;
  const int64_t n = (int64_t)nx * ny * nz;
  L.n_words = blocks_for(n, 64);
  L.n_blocks = blocks_for(L.n_words, MC_SCAN_WORDS);
  L.words_off = 0;
  L.counts_off = (size_t)L.n_words * sizeof(McWord);                     // uint32 [n_words][2]: vertices, triangles
  L.bsum_off = L.counts_off + (size_t)L.n_words * 8;                     // int64 [n_blocks][2]
  L.total = (L.bsum_off + (size_t)L.n_blocks * 16 + 255) & ~(size_t)255;
  return L;
}

bool mc_dims_ok(int nx, int ny, int nz) {
  return nx >= 2 && ny >= 2 && nz >= 2 && (int64_t)nx * ny * nz <= MSDF_COUNT_MAX;
}

struct Grid {
  int nx, ny, nz;
  uint32_t sx, sy;                          // strides of axes 0 and 1 (axis 2: 1)
  __device__ void decode(uint32_t lin, int& i, int& j, int& k) const {
    k = (int)(lin % (uint32_t)nz);
    const uint32_t r = lin / (uint32_t)nz;
    j = (int)(r % (uint32_t)ny);
    i = (int)(r / (uint32_t)ny);
  }
};

// 8-corner cube code of the cell at lin (bit c = corner c below the level)
__device__ __forceinline__ int cube_code(const float* __restrict__ vol, const Grid& g, uint32_t lin, float level) {
  int code = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const uint32_t p = lin + ((c & 1) ? g.sx : 0u) + ((c & 2) ? g.sy : 0u) + ((c & 4) ? 1u : 0u);
    code |= (vol[p] < level ? 1 : 0) << c;
  }
  return code;
}

__global__ void __launch_bounds__(MC_THREADS)
mc_classify_k(const float* __restrict__ vol, Grid g, uint32_t n, int64_t n_words, float level,
              McWord* __restrict__ words, uint32_t* __restrict__ counts) {
  constexpr int Q = MC_CLASSIFY_WORDS;
  const int64_t w0 = ((int64_t)blockIdx.x * (MC_THREADS / 64) + (threadIdx.x >> 6)) * Q;
  if (w0 >= n_words) return;                                   // wave-uniform
  const int lane = lane_id();
  // all 8 Q corner loads first (one word per wave leaves the kernel latency-bound), then the classification
  float v[Q][8];
  bool in[Q], hx[Q], hy[Q], hz[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const uint32_t lin = (uint32_t)(w0 + q) * 64u + (uint32_t)lane;
    in[q] = w0 + q < n_words && lin < n;
    int i = 0, j = 0, k = 0;
    if (in[q]) g.decode(lin, i, j, k);
    hx[q] = in[q] && i + 1 < g.nx;
    hy[q] = in[q] && j + 1 < g.ny;
    hz[q] = in[q] && k + 1 < g.nz;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const bool inside = in[q] && (!(c & 1) || hx[q]) && (!(c & 2) || hy[q]) && (!(c & 4) || hz[q]);
      const uint32_t p = lin + ((c & 1) ? g.sx : 0u) + ((c & 2) ? g.sy : 0u) + ((c & 4) ? 1u : 0u);
      v[q][c] = inside ? vol[p] : 0.0f;
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    int code = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) code |= (v[q][c] < level ? 1 : 0) << c;
    const bool b0 = code & 1;
    const bool ex = hx[q] && b0 != (bool)(code & 2);           // edges leaving the volume do not exist
    const bool ey = hy[q] && b0 != (bool)(code & 4);
    const bool ez = hz[q] && b0 != (bool)(code & 16);
    const int ntri = (hx[q] && hy[q] && hz[q]) ? (int)MC_TRI_COUNT[code] : 0;
    const uint64_t mx = __ballot(ex), my = __ballot(ey), mz = __ballot(ez);
    const int tcount = wave_sum(ntri);
    if (lane == 0 && w0 + q < n_words) {
      const int64_t w = w0 + q;
      McWord r;
      r.m[0] = mx;
      r.m[1] = my;
      r.m[2] = mz;
      r.vbase = 0;
      r.tbase = 0;
      words[w] = r;
      counts[2 * w] = (uint32_t)(__popcll(mx) + __popcll(my) + __popcll(mz));
      counts[2 * w + 1] = (uint32_t)tcount;
    }
  }
}

// first scan level: exclusive offsets of the words inside their block of 1024, block totals to bsum
__global__ void __launch_bounds__(MC_THREADS)
mc_scan_blocks_k(const uint32_t* __restrict__ counts, int64_t n_words, McWord* __restrict__ words,
                 int64_t* __restrict__ bsum) {
  __shared__ uint32_t wv[MC_THREADS / 64], wt[MC_THREADS / 64];
  const int wave = threadIdx.x >> 6;
  const int64_t w0 = (int64_t)blockIdx.x * MC_SCAN_WORDS + threadIdx.x * 4;
  uint32_t cv[4], ct[4], sv = 0, st = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const bool in = w0 + q < n_words;
    cv[q] = in ? counts[2 * (w0 + q)] : 0u;
    ct[q] = in ? counts[2 * (w0 + q) + 1] : 0u;
    sv += cv[q];
    st += ct[q];
  }
  const uint32_t iv = wave_incl_scan(sv), it = wave_incl_scan(st);
  if (lane_id() == 63) {
    wv[wave] = iv;
    wt[wave] = it;
  }
  __syncthreads();
  uint32_t pv = 0, pt = 0;
  for (int q = 0; q < wave; ++q) {
    pv += wv[q];
    pt += wt[q];
  }
  uint32_t ev = pv + iv - sv, et = pt + it - st;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (w0 + q < n_words) {
      words[w0 + q].vbase = ev;
      words[w0 + q].tbase = et;
    }
    ev += cv[q];
    et += ct[q];
  }
  if (threadIdx.x == MC_THREADS - 1) {
    bsum[2 * blockIdx.x] = (int64_t)(pv + iv);
    bsum[2 * blockIdx.x + 1] = (int64_t)(pt + it);
  }
}

// second level: one workgroup scans the block totals in place (exclusive, int64) and writes the two totals
__global__ void __launch_bounds__(1024)
mc_scan_top_k(int64_t* __restrict__ bsum, int64_t n_blocks, int64_t* __restrict__ totals) {
  __shared__ int64_t wv[16], wt[16], carry[2];
  const int wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) {
    carry[0] = 0;
    carry[1] = 0;
  }
  for (int64_t base = 0; base < n_blocks; base += 1024) {
    const int64_t b = base + threadIdx.x;
    const int64_t x = b < n_blocks ? bsum[2 * b] : 0, y = b < n_blocks ? bsum[2 * b + 1] : 0;
    const int64_t ix = wave_incl_scan(x), iy = wave_incl_scan(y);
    if (lane_id() == 63) {
      wv[wave] = ix;
      wt[wave] = iy;
    }
    __syncthreads();                                           // wave totals and the carry are visible
    int64_t px = carry[0], py = carry[1], chunk_x = 0, chunk_y = 0;
    for (int q = 0; q < 16; ++q) {
      if (q < wave) {
        px += wv[q];
        py += wt[q];
      }
      chunk_x += wv[q];
      chunk_y += wt[q];
    }
    if (b < n_blocks) {
      bsum[2 * b] = px + ix - x;
      bsum[2 * b + 1] = py + iy - y;
    }
    __syncthreads();                                           // every read of wv / wt / carry is done
    if (threadIdx.x == 0) {
      carry[0] += chunk_x;
      carry[1] += chunk_y;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    totals[0] = carry[0];
    totals[1] = carry[1];
  }
}

__global__ void __launch_bounds__(MC_THREADS)
mc_add_back_k(const int64_t* __restrict__ bsum, int64_t n_words, McWord* __restrict__ words) {
  const int64_t w = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x;
  if (w >= n_words) return;
  const int64_t blk = w / MC_SCAN_WORDS;
  // ids are < 2^31 whenever the caller goes on to emit (the totals are checked first): 32 bits hold them
  words[w].vbase += (uint32_t)bsum[2 * blk];
  words[w].tbase += (uint32_t)bsum[2 * blk + 1];
}

// d v / d axis at node p (index idx of n along the axis), central inside, one-sided on the border
__device__ __forceinline__ float grad1(const float* __restrict__ vol, uint32_t p, int idx, int n, uint32_t stride,
                                       float s) {
  if (idx == 0) return (vol[p + stride] - vol[p]) / s;
  if (idx == n - 1) return (vol[p] - vol[p - stride]) / s;
  return (vol[p + stride] - vol[p - stride]) / (2.0f * s);
}

// Both emit passes: wave `gw` looks at the MC_EMIT_WORDS words from MC_EMIT_WORDS * gw with one load of their counts
// and visits only the words whose count (field `which`) is non-zero, one after another.
__device__ __forceinline__ uint64_t active_words(const uint32_t* __restrict__ counts, int64_t n_words, int which,
                                                 int64_t& w_first) {
  const int64_t gw = (int64_t)blockIdx.x * (MC_THREADS / 64) + (threadIdx.x >> 6);
  w_first = gw * MC_EMIT_WORDS;
  const int64_t w = w_first + lane_id();
  return __ballot(lane_id() < MC_EMIT_WORDS && w < n_words && counts[2 * w + which] != 0u);
}

__global__ void __launch_bounds__(MC_THREADS)
mc_emit_vertices_k(const float* __restrict__ vol, Grid g, float level, float spx, float spy, float spz,
                   const McWord* __restrict__ words, const uint32_t* __restrict__ counts, int64_t n_words,
                   float* __restrict__ verts, float* __restrict__ normals) {
  int64_t w_first;
  uint64_t act = active_words(counts, n_words, 0, w_first);
  const int lane = lane_id();
  const uint64_t below_lane = (1ull << lane) - 1ull;
  const float sp[3] = {spx, spy, spz};
  while (act) {
    const int64_t w = w_first + __builtin_ctzll(act);
    act &= act - 1ull;
    const McWord r = words[w];
    const uint32_t lin = (uint32_t)w * 64u + (uint32_t)lane;
    uint32_t id = r.vbase + (uint32_t)(__popcll(r.m[0] & below_lane) + __popcll(r.m[1] & below_lane) +
                                       __popcll(r.m[2] & below_lane));
    int idx[3];
    g.decode(lin, idx[0], idx[1], idx[2]);
    const int dims[3] = {g.nx, g.ny, g.nz};
    const uint32_t stride[3] = {g.sx, g.sy, 1u};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!((r.m[a] >> lane) & 1ull)) continue;
      const uint32_t p1 = lin + stride[a];
      const float v0 = vol[lin], v1 = vol[p1];
      const float t = (level - v0) / (v1 - v0);
      int idx1[3] = {idx[0], idx[1], idx[2]};
      idx1[a] += 1;
      float pos[3], n[3];
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        pos[d] = (d == a ? (float)idx[d] + t : (float)idx[d]) * sp[d];
        const float g0 = grad1(vol, lin, idx[d], dims[d], stride[d], sp[d]);
        const float g1 = grad1(vol, p1, idx1[d], dims[d], stride[d], sp[d]);
        n[d] = g0 + t * (g1 - g0);
      }
      const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
      const size_t o = (size_t)id * 3;
#pragma unroll
      for (int d = 0; d < 3; ++d) {
        verts[o + d] = pos[d];
        normals[o + d] = len > 0.0f ? n[d] / len : 0.0f;
      }
      ++id;
    }
  }
}

// vertex id of the edge along `axis` owned by voxel `owner`
__device__ __forceinline__ uint32_t vertex_id(const McWord* __restrict__ words, uint32_t owner, int axis) {
  const McWord r = words[owner >> 6];
  const int l = (int)(owner & 63u);
  const uint64_t below = (1ull << l) - 1ull;
  uint32_t id = r.vbase + (uint32_t)(__popcll(r.m[0] & below) + __popcll(r.m[1] & below) + __popcll(r.m[2] & below));
  if (axis > 0) id += (uint32_t)((r.m[0] >> l) & 1ull);
  if (axis > 1) id += (uint32_t)((r.m[1] >> l) & 1ull);
  return id;
}

__global__ void __launch_bounds__(MC_THREADS)
mc_emit_faces_k(const float* __restrict__ vol, Grid g, uint32_t n, float level, const McWord* __restrict__ words,
                const uint32_t* __restrict__ counts, int64_t n_words, int32_t* __restrict__ faces) {
  int64_t w_first;
  uint64_t act = active_words(counts, n_words, 1, w_first);
  const int lane = lane_id();
  while (act) {
    const int64_t w = w_first + __builtin_ctzll(act);
    act &= act - 1ull;
    const uint32_t lin = (uint32_t)w * 64u + (uint32_t)lane;
    int code = 0, ntri = 0;
    if (lin < n) {
      int i, j, k;
      g.decode(lin, i, j, k);
      if (i + 1 < g.nx && j + 1 < g.ny && k + 1 < g.nz) {
        code = cube_code(vol, g, lin, level);
        ntri = MC_TRI_COUNT[code];
      }
    }
    const int incl = wave_incl_scan(ntri);
    size_t f = (size_t)(words[w].tbase + (uint32_t)(incl - ntri)) * 3;
    for (int t = 0; t < ntri; ++t) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int e = MC_TRIS[code][3 * t + c];
        const int c0 = MC_EDGE_C0[e];
        const uint32_t owner = lin + ((c0 & 1) ? g.sx : 0u) + ((c0 & 2) ? g.sy : 0u) + ((c0 & 4) ? 1u : 0u);
        faces[f + c] = (int32_t)vertex_id(words, owner, e >> 2);
      }
      f += 3;
    }
  }
}

Grid make_grid(int nx, int ny, int nz) {
  Grid g;
  g.nx = nx;
  g.ny = ny;
  g.nz = nz;
  g.sx = (uint32_t)ny * (uint32_t)nz;
  g.sy = (uint32_t)nz;
  return g;
}

}  // namespace

extern "C" int64_t msdf_mc_workspace_bytes(int nx, int ny, int nz) {
  if (!mc_dims_ok(nx, ny, nz)) return -1;
  return (int64_t)mc_layout(nx, ny, nz).total;
}

extern "C" int msdf_mc_count(const float* vol, int nx, int ny, int nz, float level, void* workspace, int64_t* totals,
                             void* stream) {
  if (!vol || !workspace || !totals || !mc_dims_ok(nx, ny, nz)) return MSDF_ERR_ARG;
  const McLayout L = mc_layout(nx, ny, nz);
  char* ws = (char*)workspace;
  McWord* words = (McWord*)(ws + L.words_off);
  uint32_t* counts = (uint32_t*)(ws + L.counts_off);
  int64_t* bsum = (int64_t*)(ws + L.bsum_off);
  const hipStream_t s = (hipStream_t)stream;
  const uint32_t n = (uint32_t)((int64_t)nx * ny * nz);
  mc_classify_k<<<blocks_for(L.n_words, (MC_THREADS / 64) * MC_CLASSIFY_WORDS), MC_THREADS, 0, s>>>(
      vol, make_grid(nx, ny, nz), n, L.n_words, level, words, counts);
  mc_scan_blocks_k<<<(unsigned)L.n_blocks, MC_THREADS, 0, s>>>(counts, L.n_words, words, bsum);
  mc_scan_top_k<<<1, 1024, 0, s>>>(bsum, L.n_blocks, totals);
  mc_add_back_k<<<blocks_for(L.n_words, MC_THREADS), MC_THREADS, 0, s>>>(bsum, L.n_words, words);
  return msdf_check_launch();
}

extern "C" int msdf_mc_emit(const float* vol, int nx, int ny, int nz, float level, float sx, float sy, float sz,
                            const void* workspace, float* verts, float* normals, int32_t* faces, void* stream) {
  if (!vol || !workspace || !verts || !normals || !faces || !mc_dims_ok(nx, ny, nz)) return MSDF_ERR_ARG;
  const McLayout L = mc_layout(nx, ny, nz);
  const char* ws = (const char*)workspace;
  const McWord* words = (const McWord*)(ws + L.words_off);
  const uint32_t* counts = (const uint32_t*)(ws + L.counts_off);
  const hipStream_t s = (hipStream_t)stream;
  const Grid g = make_grid(nx, ny, nz);
  const unsigned blocks = (unsigned)blocks_for(L.n_words, MC_EMIT_WORDS * (MC_THREADS / 64));
  mc_emit_vertices_k<<<blocks, MC_THREADS, 0, s>>>(vol, g, level, sx, sy, sz, words, counts, L.n_words, verts,
                                                   normals);
  mc_emit_faces_k<<<blocks, MC_THREADS, 0, s>>>(vol, g, (uint32_t)((int64_t)nx * ny * nz), level, words, counts,
                                                L.n_words, faces);
  return msdf_check_launch();
}
