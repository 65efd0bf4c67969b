// Mesh re-fusion on the device: what the reference's evaluation does to a mesh before it scores it
// (scannet_eval/evaluate.py:111-137 and postprocess/refuse.py with pyrender + open3d's ScalableTSDFVolume;
// replica_eval/cull_mesh.py:58-87).  Four groups of kernels, none with a floating-point atomic: the same inputs give
// bitwise the same outputs every call.  Cameras are OpenCV-style (x right, y down, z forward); every kernel gets the
// WORLD-TO-CAMERA rows `r00 r01 r02 tx | r10 r11 r12 ty | r20 r21 r22 tz` (12 floats per view), inverted by the caller.
// This object is built with -ffp-contract=off: the TSDF and culling rules are the separately rounded fp32 operations
// the numpy restatement (tests/refuse_numpy.py) performs, and the rasteriser's edge tests rely on a * b - c * d
// changing sign exactly when its operands are swapped.
//
// Depth rasteriser (raster_*_k).  Parallel over triangles, one lane each, grid.y = view:
//   * the three vertices go to the camera frame; the two edge vectors are formed in WORLD coordinates (exact to an ulp
//     of the edge, not of the distance to the camera) and rotated
//   * per pixel the ray is d = ((j + c - cx) / fx, (i + c - cy) / fy, 1); the side test of edge (p, q) is
//     d . (p x (q - p)) with p the endpoint of the SMALLER vertex index, negated when the triangle runs the edge the
//     other way: two triangles that share an edge evaluate the same expression with opposite sign, and `>= 0` (or,
//     for the other winding, `<= 0`) on all three edges accepts the ray on both sides -- no cracks
//   * depth z = (n . a) / (n . d) with n the plane normal (from the vertices in ascending index, a the first): ray against plane per pixel, nothing interpolated from
//     projected vertices, so a triangle that crosses the near plane covers what its visible part covers
//   * a triangle whose vertices all lie at z >= znear is bounded by the box of its projection (one pixel of slack); one
//     that crosses z = znear takes the whole image
//   * a box of at most RASTER_COOP_AREA pixels is scanned by the lane itself (marching-cubes meshes: millions of
//     triangles of a few pixels); larger boxes are handed round the wave: their set-up is broadcast lane by lane and
//     all 64 lanes stride over the box, so an image-spanning triangle does not serialise on one lane
//   * the minimum is kept with a 32-bit unsigned atomicMin on the bits of z (positive floats order as unsigned
//     integers, as in nn_finish_k); a minimum does not depend on order.  raster_clear_k writes +inf before,
//     raster_finish_k turns +inf into 0 (background) after.
// Degenerate faces (a repeated vertex, n . d = 0, an index outside [0, V)) touch no pixel.
//
// TSDF integration (tsdf_integrate_k): one lane owns one voxel of a dense block and loops over the views in the order
// given; the camera rows are wave-uniform reads, the running mean stays in registers and each voxel is written once.
// Face rule (tsdf_face_keep_k) and frustum culling (cull_vertices_k): one lane per face / vertex.
#include "common.h"

namespace {

constexpr int RF_THREADS = 256;
constexpr int RASTER_COOP_AREA = 256;              // boxes of more pixels than this are scanned by the whole wave
constexpr unsigned RASTER_INF = 0x7f800000u;       // bits of +inf
constexpr int64_t RF_MAX = 0x7fffffffll;

struct RasterCam {
  float fx, fy, cx, cy, pc, znear, zfar;
  int height, width;
};

// what the pixel loop needs of one triangle: the three (signed) edge vectors, the plane, the pixel box
struct TriSetup {
  float e0x, e0y, e0z, e1x, e1y, e1z, e2x, e2y, e2z;
  float nx, ny, nz, na;
  int j0, i0, bw, bh;                               // box: columns j0 .. j0 + bw - 1, rows i0 .. i0 + bh - 1; bw = 0: none
};

struct V3 {
  float x, y, z;
};

__device__ __forceinline__ V3 cross3(V3 a, V3 b) {
  return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

__device__ __forceinline__ V3 rotate(const float* __restrict__ m, V3 v) {
  return V3{m[0] * v.x + m[1] * v.y + m[2] * v.z, m[4] * v.x + m[5] * v.y + m[6] * v.z,
            m[8] * v.x + m[9] * v.y + m[10] * v.z};
}

// edge (p -> q) of the triangle, p / q given as world and camera positions with their vertex indices: the vector
// lo x (hi - lo) of the endpoint pair in ascending index, negated when the triangle runs from hi to lo
__device__ __forceinline__ V3 edge_vector(const float* __restrict__ m, int ip, V3 wp, V3 cp, int iq, V3 wq, V3 cq) {
  if (ip == iq) return V3{0.0f, 0.0f, 0.0f};
  const bool fwd = ip < iq;
  const V3 wl = fwd ? wp : wq, wh = fwd ? wq : wp, cl = fwd ? cp : cq;
  const V3 e = cross3(cl, rotate(m, V3{wh.x - wl.x, wh.y - wl.y, wh.z - wl.z}));
  return fwd ? e : V3{-e.x, -e.y, -e.z};
}

__device__ __forceinline__ int clamp_to_int(float v, int lo, int hi) {   // NaN -> lo
  const float c = fminf(fmaxf(v, (float)lo), (float)hi);
  return (int)c;
}

__device__ __forceinline__ void raster_pixel(const TriSetup& t, const RasterCam& cam, int i, int j,
                                             unsigned* __restrict__ img) {
  const float dx = ((float)j + cam.pc - cam.cx) / cam.fx;
  const float dy = ((float)i + cam.pc - cam.cy) / cam.fy;
  const float w0 = dx * t.e0x + dy * t.e0y + t.e0z;
  const float w1 = dx * t.e1x + dy * t.e1y + t.e1z;
  const float w2 = dx * t.e2x + dy * t.e2y + t.e2z;
  const bool in = (w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f) || (w0 <= 0.0f && w1 <= 0.0f && w2 <= 0.0f);
  if (!in) return;
  const float nd = dx * t.nx + dy * t.ny + t.nz;
  if (nd == 0.0f) return;
  const float z = t.na / nd;
  if (!(z >= cam.znear && z <= cam.zfar)) return;                      // NaN fails
  unsigned* p = img + (size_t)i * (size_t)cam.width + (size_t)j;
  const unsigned bits = __float_as_uint(z);                             // z > 0: ordered as unsigned
  if (bits < *p) atomicMin(p, bits);                                    // values only fall: a stale read costs an atomic
}

__global__ void __launch_bounds__(RF_THREADS)
raster_clear_k(unsigned* __restrict__ img, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * RF_THREADS + threadIdx.x;
  if (i < n) img[i] = RASTER_INF;
}

__global__ void __launch_bounds__(RF_THREADS)
raster_finish_k(unsigned* __restrict__ img, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * RF_THREADS + threadIdx.x;
  if (i < n && img[i] == RASTER_INF) img[i] = 0u;
}

__global__ void __launch_bounds__(RF_THREADS)
raster_tri_k(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t F,
             const float* __restrict__ w2c, RasterCam cam, unsigned* __restrict__ depth) {
  const int view = (int)blockIdx.y;
  const float* __restrict__ m = w2c + 12 * (size_t)view;
  unsigned* __restrict__ img = depth + (size_t)view * (size_t)cam.height * (size_t)cam.width;
  const int64_t f = (int64_t)blockIdx.x * RF_THREADS + threadIdx.x;

  TriSetup t;
  t.bw = 0;
  t.bh = 0;
  if (f < F) {
    const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
    if (ia >= 0 && ib >= 0 && ic >= 0 && ia < V && ib < V && ic < V) {
      const V3 wa{verts[3 * (size_t)ia], verts[3 * (size_t)ia + 1], verts[3 * (size_t)ia + 2]};
      const V3 wb{verts[3 * (size_t)ib], verts[3 * (size_t)ib + 1], verts[3 * (size_t)ib + 2]};
      const V3 wc{verts[3 * (size_t)ic], verts[3 * (size_t)ic + 1], verts[3 * (size_t)ic + 2]};
      V3 a = rotate(m, wa), b = rotate(m, wb), c = rotate(m, wc);
      a = V3{a.x + m[3], a.y + m[7], a.z + m[11]};
      b = V3{b.x + m[3], b.y + m[7], b.z + m[11]};
      c = V3{c.x + m[3], c.y + m[7], c.z + m[11]};
      const float zmin = fminf(a.z, fminf(b.z, c.z)), zmax = fmaxf(a.z, fmaxf(b.z, c.z));
      // every intersection lies between the vertices' depths
      if (zmax >= cam.znear && zmin <= cam.zfar) {
        const V3 e0 = edge_vector(m, ia, wa, a, ib, wb, b);
        const V3 e1 = edge_vector(m, ib, wb, b, ic, wc, c);
        const V3 e2 = edge_vector(m, ic, wc, c, ia, wa, a);
        // the plane from the vertices in ascending index, so that every rotation and winding of the face gives the
        // same bits of z
        int s0 = ia, s1 = ib, s2 = ic;
        V3 p0 = wa, p1 = wb, p2 = wc, q0 = a;
        if (s1 < s0) {
          const int ti = s0; s0 = s1; s1 = ti;
          const V3 tp = p0; p0 = p1; p1 = tp;
          q0 = b;
        }
        if (s2 < s1) {
          const int ti = s1; s1 = s2; s2 = ti;
          const V3 tp = p1; p1 = p2; p2 = tp;
          if (s1 < s0) {
            const int tj = s0; s0 = s1; s1 = tj;
            const V3 tq = p0; p0 = p1; p1 = tq;
            q0 = c;
          }
        }
        const V3 n = cross3(rotate(m, V3{p1.x - p0.x, p1.y - p0.y, p1.z - p0.z}),
                            rotate(m, V3{p2.x - p0.x, p2.y - p0.y, p2.z - p0.z}));
        t.e0x = e0.x, t.e0y = e0.y, t.e0z = e0.z;
        t.e1x = e1.x, t.e1y = e1.y, t.e1z = e1.z;
        t.e2x = e2.x, t.e2y = e2.y, t.e2z = e2.z;
        t.nx = n.x, t.ny = n.y, t.nz = n.z;
        t.na = n.x * q0.x + n.y * q0.y + n.z * q0.z;
        int j0 = 0, j1 = cam.width - 1, i0 = 0, i1 = cam.height - 1;
        if (zmin >= cam.znear) {                                        // znear > 0: the projections exist
          const float ua = cam.fx * a.x / a.z, ub = cam.fx * b.x / b.z, uc = cam.fx * c.x / c.z;
          const float va = cam.fy * a.y / a.z, vb = cam.fy * b.y / b.z, vc = cam.fy * c.y / c.z;
          const float off_u = cam.cx - cam.pc, off_v = cam.cy - cam.pc;  // pixel j has its centre at u = j - off_u
          j0 = clamp_to_int(floorf(fminf(ua, fminf(ub, uc)) + off_u) - 1.0f, 0, cam.width);
          j1 = clamp_to_int(ceilf(fmaxf(ua, fmaxf(ub, uc)) + off_u) + 1.0f, -1, cam.width - 1);
          i0 = clamp_to_int(floorf(fminf(va, fminf(vb, vc)) + off_v) - 1.0f, 0, cam.height);
          i1 = clamp_to_int(ceilf(fmaxf(va, fmaxf(vb, vc)) + off_v) + 1.0f, -1, cam.height - 1);
        }
        if (j1 >= j0 && i1 >= i0 && !(n.x == 0.0f && n.y == 0.0f && n.z == 0.0f)) {
          t.j0 = j0, t.i0 = i0, t.bw = j1 - j0 + 1, t.bh = i1 - i0 + 1;
        }
      }
    }
  }

  const int area = t.bw * t.bh;                                         // <= height * width < 2^31 (checked by the host)
  const bool large = area > RASTER_COOP_AREA;
  if (area > 0 && !large) {
    for (int i = t.i0; i < t.i0 + t.bh; ++i)
      for (int j = t.j0; j < t.j0 + t.bw; ++j) raster_pixel(t, cam, i, j, img);
  }
  // the large boxes of this wave, one after the other, by all its lanes
  unsigned long long todo = __ballot(large);
  const int lane = lane_id();
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    TriSetup s;
    s.e0x = __shfl(t.e0x, src, 64), s.e0y = __shfl(t.e0y, src, 64), s.e0z = __shfl(t.e0z, src, 64);
    s.e1x = __shfl(t.e1x, src, 64), s.e1y = __shfl(t.e1y, src, 64), s.e1z = __shfl(t.e1z, src, 64);
    s.e2x = __shfl(t.e2x, src, 64), s.e2y = __shfl(t.e2y, src, 64), s.e2z = __shfl(t.e2z, src, 64);
    s.nx = __shfl(t.nx, src, 64), s.ny = __shfl(t.ny, src, 64), s.nz = __shfl(t.nz, src, 64);
    s.na = __shfl(t.na, src, 64);
    s.j0 = __shfl(t.j0, src, 64), s.i0 = __shfl(t.i0, src, 64);
    s.bw = __shfl(t.bw, src, 64), s.bh = __shfl(t.bh, src, 64);
    const unsigned n_px = (unsigned)(s.bw * s.bh), bw = (unsigned)s.bw;
    for (unsigned k = (unsigned)lane; k < n_px; k += 64u)
      raster_pixel(s, cam, s.i0 + (int)(k / bw), s.j0 + (int)(k % bw), img);
  }
}

struct TsdfArgs {
  float fx, fy, cx, cy, ox, oy, oz, voxel_length, sdf_trunc, depth_trunc;
  int height, width, nx, ny, nz, n_views, i0, j0, k0, resume;
};

__global__ void __launch_bounds__(RF_THREADS)
tsdf_integrate_k(const float* __restrict__ depth, const float* __restrict__ w2c, TsdfArgs p,
                 float* __restrict__ tsdf, float* __restrict__ weight) {
  const int64_t n = (int64_t)p.nx * p.ny * p.nz;
  const int64_t idx = (int64_t)blockIdx.x * RF_THREADS + threadIdx.x;
  if (idx >= n) return;
  const int k = (int)(idx % p.nz), j = (int)((idx / p.nz) % p.ny), i = (int)(idx / ((int64_t)p.nz * p.ny));
  // the centre is formed from the voxel's index in the WHOLE volume: a voxel two blocks share gets the same bits in both
  const float x = p.ox + p.voxel_length * ((float)(i + p.i0) + 0.5f);
  const float y = p.oy + p.voxel_length * ((float)(j + p.j0) + 0.5f);
  const float z = p.oz + p.voxel_length * ((float)(k + p.k0) + 0.5f);
  const size_t hw = (size_t)p.height * (size_t)p.width;
  float t = 0.0f, w = 0.0f;
  if (p.resume) {                                                       // a later chunk of the same list of views
    t = tsdf[idx];
    w = weight[idx];
  }
  for (int v = 0; v < p.n_views; ++v) {
    const float* __restrict__ m = w2c + 12 * (size_t)v;                 // the same address in every lane
    const float pz = m[8] * x + m[9] * y + m[10] * z + m[11];
    if (!(pz > 0.0f)) continue;
    const float px = m[0] * x + m[1] * y + m[2] * z + m[3];
    const float py = m[4] * x + m[5] * y + m[6] * z + m[7];
    const float uf = p.fx * px / pz + p.cx + 0.5f;
    const float vf = p.fy * py / pz + p.cy + 0.5f;
    if (!(uf >= 0.0f && uf < (float)p.width && vf >= 0.0f && vf < (float)p.height)) continue;   // NaN fails
    const int u = (int)uf, r = (int)vf;
    const float d = depth[(size_t)v * hw + (size_t)r * (size_t)p.width + (size_t)u];
    if (!(d > 0.0f) || d > p.depth_trunc) continue;
    const float rx = ((float)u - p.cx) / p.fx, ry = ((float)r - p.cy) / p.fy;
    const float len = sqrtf(rx * rx + ry * ry + 1.0f);
    const float s = (d - pz) * len;
    if (s <= -p.sdf_trunc) continue;
    const float tau = fminf(1.0f, s / p.sdf_trunc);
    t = (t * w + tau) / (w + 1.0f);
    w = w + 1.0f;
  }
  tsdf[idx] = t;
  weight[idx] = w;
}

__global__ void __launch_bounds__(RF_THREADS)
tsdf_face_keep_k(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t F,
                 const float* __restrict__ weight, int nx, int ny, int nz, uint8_t* __restrict__ keep) {
  const int64_t f = (int64_t)blockIdx.x * RF_THREADS + threadIdx.x;
  if (f >= F) return;
  const int dims[3] = {nx, ny, nz};
  int lo[3], hi[3];
  bool ok = true;
  float vmin[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
  float vmax[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int iv = faces[3 * f + c];
    if (iv < 0 || iv >= V) {
      ok = false;
      continue;
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const float x = verts[3 * (size_t)iv + d];
      vmin[d] = fminf(vmin[d], x);
      vmax[d] = fmaxf(vmax[d], x);
    }
  }
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    // a vertex outside the lattice (or not a number) is not kept
    if (!(vmin[d] >= 0.0f && vmax[d] <= (float)(dims[d] - 1))) ok = false;
    lo[d] = clamp_to_int(floorf(vmin[d]), 0, dims[d] - 1);
    hi[d] = clamp_to_int(ceilf(vmax[d]), 0, dims[d] - 1);
  }
  if (ok) {
    for (int i = lo[0]; i <= hi[0] && ok; ++i)
      for (int j = lo[1]; j <= hi[1] && ok; ++j)
        for (int k = lo[2]; k <= hi[2]; ++k)
          if (!(weight[((size_t)i * (size_t)ny + (size_t)j) * (size_t)nz + (size_t)k] > 0.0f)) {
            ok = false;
            break;
          }
  }
  keep[f] = ok ? 1 : 0;
}

__global__ void __launch_bounds__(RF_THREADS)
cull_vertices_k(const float* __restrict__ verts, int64_t V, const float* __restrict__ w2c, int n_views, float fx,
                float fy, float cx, float cy, float width, float height, uint8_t* __restrict__ seen) {
  const int64_t i = (int64_t)blockIdx.x * RF_THREADS + threadIdx.x;
  if (i >= V) return;
  const float x = verts[3 * i], y = verts[3 * i + 1], z = verts[3 * i + 2];
  uint8_t s = 0;
  for (int v = 0; v < n_views; ++v) {
    const float* __restrict__ m = w2c + 12 * (size_t)v;
    const float pz = m[8] * x + m[9] * y + m[10] * z + m[11];
    if (!(pz >= 1e-5f)) continue;
    const float px = m[0] * x + m[1] * y + m[2] * z + m[3];
    const float py = m[4] * x + m[5] * y + m[6] * z + m[7];
    const float zz = pz - 1e-5f;
    const float u = fx * px / zz + cx, r = fy * py / zz + cy;
    if (u > 0.0f && u < width && r > 0.0f && r < height) {              // NaN (zz = 0, px = 0) fails
      s = 1;
      break;
    }
  }
  seen[i] = s;
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + RF_THREADS - 1) / RF_THREADS); }

bool intrinsics_ok(float fx, float fy, float cx, float cy) {
  return fx > 0.0f && fy > 0.0f && cx == cx && cy == cy && fx < __builtin_inff() && fy < __builtin_inff();
}

}  // namespace

extern "C" int msdf_raster_depth(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                 const float* w2c, int n_views, float fx, float fy, float cx, float cy, int height,
                                 int width, float znear, float zfar, float pixel_center, float* depth, void* stream) {
  if (n_verts < 0 || n_verts > RF_MAX || n_faces < 0 || n_faces > RF_MAX || n_views < 0 || n_views > 65535 ||
      height < 1 || width < 1 || (int64_t)height * width > RF_MAX || !intrinsics_ok(fx, fy, cx, cy) ||
      !(znear > 0.0f) || !(zfar >= znear) || !(pixel_center == pixel_center))
    return MSDF_ERR_ARG;
  if (n_views == 0) return MSDF_OK;
  if (!depth || !w2c || (n_faces > 0 && (!verts || !faces))) return MSDF_ERR_ARG;
  const hipStream_t s = (hipStream_t)stream;
  const int64_t n_px = (int64_t)n_views * height * width;
  unsigned* img = (unsigned*)depth;
  raster_clear_k<<<blocks_for(n_px), RF_THREADS, 0, s>>>(img, n_px);
  if (n_faces > 0 && n_verts > 0) {
    const RasterCam cam{fx, fy, cx, cy, pixel_center, znear, zfar, height, width};
    raster_tri_k<<<dim3(blocks_for(n_faces), (unsigned)n_views), RF_THREADS, 0, s>>>(verts, n_verts, faces, n_faces,
                                                                                     w2c, cam, img);
  }
  raster_finish_k<<<blocks_for(n_px), RF_THREADS, 0, s>>>(img, n_px);
  return msdf_check_launch();
}

extern "C" int msdf_tsdf_integrate(const float* depth, const float* w2c, int n_views, float fx, float fy, float cx,
                                   float cy, int height, int width, float ox, float oy, float oz, int i0, int j0, int k0, int nx, int ny,
                                   int nz, float voxel_length, float sdf_trunc, float depth_trunc, int resume,
                                   float* tsdf, float* weight, void* stream) {
  if (n_views < 0 || height < 1 || width < 1 || (int64_t)height * width > RF_MAX || nx < 1 || ny < 1 || nz < 1 ||
      (int64_t)nx * ny * nz > RF_MAX || i0 < 0 || j0 < 0 || k0 < 0 || (int64_t)i0 + nx > (1 << 24) ||
      (int64_t)j0 + ny > (1 << 24) || (int64_t)k0 + nz > (1 << 24) || !intrinsics_ok(fx, fy, cx, cy) ||
      !(voxel_length > 0.0f) || !(sdf_trunc > 0.0f) || !(depth_trunc == depth_trunc) || !(ox - ox == 0.0f) || !(oy - oy == 0.0f) || !(oz - oz == 0.0f) || !tsdf || !weight ||
      (n_views > 0 && (!depth || !w2c)))
    return MSDF_ERR_ARG;
  const TsdfArgs p{fx, fy, cx, cy, ox, oy, oz, voxel_length, sdf_trunc, depth_trunc,
                   height, width, nx, ny, nz, n_views, i0, j0, k0, resume ? 1 : 0};
  tsdf_integrate_k<<<blocks_for((int64_t)nx * ny * nz), RF_THREADS, 0, (hipStream_t)stream>>>(depth, w2c, p, tsdf,
                                                                                             weight);
  return msdf_check_launch();
}

extern "C" int msdf_tsdf_face_keep(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                   const float* weight, int nx, int ny, int nz, uint8_t* keep, void* stream) {
  if (n_verts < 0 || n_verts > RF_MAX || n_faces < 0 || n_faces > RF_MAX || nx < 1 || ny < 1 || nz < 1 ||
      (int64_t)nx * ny * nz > RF_MAX)
    return MSDF_ERR_ARG;
  if (n_faces == 0) return MSDF_OK;
  if (!verts || !faces || !weight || !keep) return MSDF_ERR_ARG;
  tsdf_face_keep_k<<<blocks_for(n_faces), RF_THREADS, 0, (hipStream_t)stream>>>(verts, n_verts, faces, n_faces,
                                                                               weight, nx, ny, nz, keep);
  return msdf_check_launch();
}

extern "C" int msdf_cull_vertices(const float* verts, int64_t n_verts, const float* w2c, int n_views, float fx,
                                  float fy, float cx, float cy, int height, int width, uint8_t* seen, void* stream) {
  if (n_verts < 0 || n_verts > RF_MAX || n_views < 0 || height < 1 || width < 1 || !intrinsics_ok(fx, fy, cx, cy))
    return MSDF_ERR_ARG;
  if (n_verts == 0) return MSDF_OK;
  if (!verts || !seen || (n_views > 0 && !w2c)) return MSDF_ERR_ARG;
  cull_vertices_k<<<blocks_for(n_verts), RF_THREADS, 0, (hipStream_t)stream>>>(verts, n_verts, w2c, n_views, fx, fy,
                                                                              cx, cy, (float)width, (float)height,
                                                                              seen);
  return msdf_check_launch();
}
