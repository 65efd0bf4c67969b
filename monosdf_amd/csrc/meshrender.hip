// Mesh renderer on the device (ABI: include/monosdf_render.h, which states every rule): what the reference shows
// its results with (render/render_trajectory_open3d.py: open3d's Phong shader and the four lights of render.json) and
// the depth L1 of replica_eval/eval_recon.py:196-285.  Five groups of kernels, none with a floating-point atomic: the
// same inputs give bitwise the same outputs every call.  Built with -ffp-contract=off: the rasteriser of raster_core.h
// needs it, and the other rules are stated as separately rounded operations that tests/render_numpy.py restates.
//
// Visibility (rnd_vis_*_k): the rasteriser of raster_core.h, grid.y = view, with the action
//   key = (bits of z << 32) | face, 64-bit unsigned atomicMin into a workspace cleared to all ones
// z > 0, so its bits order as unsigned integers and the key orders by depth first, face index second: the minimum is
// the nearest depth and, among the faces that reach exactly those bits, the smallest index -- whatever the order the
// lanes arrive in.  Culling drops a (face, pixel) pair before the atomic by the sign of the plane term nd the hit test
// already has, corrected by the parity of the sort that produced the plane.  rnd_vis_finish_k splits the keys.
// Vertex normals (rnd_vertex_normals_k): one lane owns one vertex and walks its incidence list in ascending face index.
// Shading (rnd_shade_k): one lane per pixel; the set-up of the winning face is formed again by raster_face_plane.
// Depth L1 (rnd_depth_l1_k): one workgroup per view, a fixed summation order.  View rejection (rnd_views_see_k): point
// chunks x views, a plain store of 1.
#include "tool_common.h"
#include "raster_core.h"
#include "../../include/monosdf_render.h"

namespace {

constexpr int RN_THREADS = 256;
constexpr unsigned long long RN_EMPTY = ~0ull;
constexpr int RN_VIEWS_PER_LAUNCH = 65535;         // grid.y
constexpr int RN_CHUNK = 2048;                     // points of one workgroup of rnd_views_see_k

bool image_ok(int64_t n_views, int64_t height, int64_t width) {
  if (!fits_int32(n_views) || !fits_int32(height) || !fits_int32(width)) return false;
  if (height == 0 || width == 0 || n_views == 0) return true;
  if (height > MSDF_COUNT_MAX / width) return false;
  return n_views <= MSDF_COUNT_MAX / (height * width);
}

// ---- visibility

struct VisibilityMin {
  unsigned long long* __restrict__ img;
  int cull;
  __device__ __forceinline__ void operator()(const TriSetup& t, const RasterCam& cam, int i, int j, float z,
                                             float nd) const {
    // the face's own normal is n or -n (t.odd): front-facing iff it points against the ray
    const bool front = (nd < 0.0f) != (t.odd != 0);
    if ((cull == 1 && !front) || (cull == 2 && front)) return;
    unsigned long long* p = img + (size_t)i * (size_t)cam.width + (size_t)j;
    const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)t.face;
    if (key < *p) atomicMin(p, key);                                    // values only fall: a stale read costs an atomic
  }
};

__global__ void __launch_bounds__(RN_THREADS)
rnd_vis_clear_k(unsigned long long* __restrict__ ws, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * RN_THREADS + threadIdx.x;
  if (i < n) ws[i] = RN_EMPTY;
}

__global__ void __launch_bounds__(RN_THREADS)
rnd_vis_tri_k(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t F,
              const float* __restrict__ w2c, RasterCam cam, int cull, unsigned long long* __restrict__ ws) {
  const int view = (int)blockIdx.y;
  const float* __restrict__ m = w2c + 12 * (size_t)view;
  unsigned long long* __restrict__ img = ws + (size_t)view * (size_t)cam.height * (size_t)cam.width;
  const int64_t f = (int64_t)blockIdx.x * RN_THREADS + threadIdx.x;
  raster_triangle(verts, V, faces, F, f, m, cam, VisibilityMin{img, cull});
}

__global__ void __launch_bounds__(RN_THREADS)
rnd_vis_finish_k(const unsigned long long* __restrict__ ws, int64_t n, float* __restrict__ depth,
                 int32_t* __restrict__ face) {
  const int64_t i = (int64_t)blockIdx.x * RN_THREADS + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = ws[i];
  const bool hit = key != RN_EMPTY;
  depth[i] = hit ? __uint_as_float((unsigned)(key >> 32)) : 0.0f;
  face[i] = hit ? (int32_t)(unsigned)(key & 0xffffffffull) : -1;
}

// ---- vertex normals

__global__ void __launch_bounds__(RN_THREADS)
rnd_vertex_normals_k(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t F,
                     const int32_t* __restrict__ inc_start, const int32_t* __restrict__ inc_face,
                     float* __restrict__ normals) {
  const int64_t v = (int64_t)blockIdx.x * RN_THREADS + threadIdx.x;
  if (v >= V) return;
  const int64_t n_inc = 3 * F;
  int64_t lo = inc_start[v], hi = inc_start[v + 1];
  lo = lo < 0 ? 0 : (lo > n_inc ? n_inc : lo);
  hi = hi < 0 ? 0 : (hi > n_inc ? n_inc : hi);
  double sx = 0.0, sy = 0.0, sz = 0.0;
  for (int64_t k = lo; k < hi; ++k) {
    const int64_t f = inc_face[k];
    if (f < 0 || f >= F) continue;
    const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
    if (ia < 0 || ib < 0 || ic < 0 || ia >= V || ib >= V || ic >= V || ia == ib || ib == ic || ia == ic) continue;
    const double ax = verts[3 * (size_t)ia], ay = verts[3 * (size_t)ia + 1], az = verts[3 * (size_t)ia + 2];
    const double ux = (double)verts[3 * (size_t)ib] - ax, uy = (double)verts[3 * (size_t)ib + 1] - ay,
                 uz = (double)verts[3 * (size_t)ib + 2] - az;
    const double wx = (double)verts[3 * (size_t)ic] - ax, wy = (double)verts[3 * (size_t)ic + 1] - ay,
                 wz = (double)verts[3 * (size_t)ic + 2] - az;
    sx += uy * wz - uz * wy;
    sy += uz * wx - ux * wz;
    sz += ux * wy - uy * wx;
  }
  const double len = sqrt((sx * sx + sy * sy) + sz * sz);
  const bool ok = len > 0.0 && len < (double)__builtin_inff();          // NaN fails
  normals[3 * v] = ok ? (float)(sx / len) : 0.0f;
  normals[3 * v + 1] = ok ? (float)(sy / len) : 0.0f;
  normals[3 * v + 2] = ok ? (float)(sz / len) : 1.0f;
}

// ---- shading

struct ShadeArgs {
  float fx, fy, cx, cy, pc;
  float base_r, base_g, base_b;
  float centre_x, centre_y, centre_z, extent;
  int height, width, flat, two_sided;
};

__device__ __forceinline__ float dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }

__device__ __forceinline__ V3 unit3(V3 v) {
  const float len = sqrtf(dot3(v, v));
  if (!(len > 0.0f)) return V3{0.0f, 0.0f, 0.0f};
  return V3{v.x / len, v.y / len, v.z / len};
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

__device__ __forceinline__ V3 load3(const float* __restrict__ p, int i) {
  return V3{p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]};
}

__global__ void __launch_bounds__(RN_THREADS)
rnd_shade_k(const int32_t* __restrict__ face, const float* __restrict__ depth, int64_t n_px,
            const float* __restrict__ w2c, ShadeArgs p, const float* __restrict__ verts, int64_t V,
            const int32_t* __restrict__ faces, int64_t F, const float* __restrict__ normals,
            const float* __restrict__ colors, const float* __restrict__ lights, float* __restrict__ rgb) {
  const int64_t idx = (int64_t)blockIdx.x * RN_THREADS + threadIdx.x;
  if (idx >= n_px) return;
  const int64_t hw = (int64_t)p.height * p.width;
  const int view = (int)(idx / hw);
  const int rem = (int)(idx % hw);
  const int i = rem / p.width, j = rem % p.width;
  const float* __restrict__ m = w2c + 12 * (size_t)view;
  float* __restrict__ out = rgb + 3 * (size_t)idx;
  const int64_t f = face[idx];
  FaceVerts q;
  if (f < 0 || f >= F || !raster_face_vertices(verts, V, faces, f, m, q)) {
    out[0] = lights[39], out[1] = lights[40], out[2] = lights[41];
    return;
  }
  TriSetup t;
  raster_face_plane(m, q, f, t);
  RasterCam cam{p.fx, p.fy, p.cx, p.cy, p.pc, 0.0f, 0.0f, p.height, p.width};
  float dx, dy, w0, w1, w2;
  raster_ray(cam, i, j, dx, dy);
  raster_edge_terms(t, dx, dy, w0, w1, w2);
  const float s = (w0 + w1) + w2;
  const float ba = w1 / s, bb = w2 / s, bc = w0 / s;                    // the edge opposite a vertex carries its weight
  const float z = depth[idx];
  const V3 P{z * dx, z * dy, z};
  const int ia = q.ia, ib = q.ib, ic = q.ic;

  V3 N;
  if (p.flat) {
    N = t.odd ? V3{-t.nx, -t.ny, -t.nz} : V3{t.nx, t.ny, t.nz};             // the face's own normal
  } else {
    const V3 na = rotate(m, load3(normals, ia)), nb = rotate(m, load3(normals, ib)), nc = rotate(m, load3(normals, ic));
    N = V3{(ba * na.x + bb * nb.x) + bc * nc.x, (ba * na.y + bb * nb.y) + bc * nc.y,
           (ba * na.z + bb * nb.z) + bc * nc.z};
  }
  N = unit3(N);
  const V3 toeye{-P.x, -P.y, -P.z};
  if (p.two_sided && dot3(N, toeye) < 0.0f) N = V3{-N.x, -N.y, -N.z};
  const V3 e = unit3(toeye);

  V3 base{p.base_r, p.base_g, p.base_b};
  if (colors) {
    const V3 ca = load3(colors, ia), cb = load3(colors, ib), cc = load3(colors, ic);
    base = V3{(ba * ca.x + bb * cb.x) + bc * cc.x, (ba * ca.y + bb * cb.y) + bc * cc.y,
              (ba * ca.z + bb * cb.z) + bc * cc.z};
  }
  float dr = lights[36], dg = lights[37], db = lights[38];               // ambient + diffuse
  float sr = 0.0f, sg = 0.0f, sb = 0.0f;                                 // specular
  const V3 r{m[0], m[1], m[2]}, u{-m[4], -m[5], -m[6]}, fw{-m[8], -m[9], -m[10]};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float* __restrict__ L = lights + 9 * k;
    const V3 world{p.centre_x + p.extent * ((L[0] * r.x + L[1] * u.x) + L[2] * fw.x),
                   p.centre_y + p.extent * ((L[0] * r.y + L[1] * u.y) + L[2] * fw.y),
                   p.centre_z + p.extent * ((L[0] * r.z + L[1] * u.z) + L[2] * fw.z)};
    V3 lc = rotate(m, world);
    lc = V3{lc.x + m[3], lc.y + m[7], lc.z + m[11]};
    const V3 l = unit3(V3{lc.x - P.x, lc.y - P.y, lc.z - P.z});
    const float nl = dot3(N, l);
    const float cos_t = clamp01(nl);
    const float two_nl = 2.0f * nl;
    const V3 R{two_nl * N.x - l.x, two_nl * N.y - l.y, two_nl * N.z - l.z};
    const float cos_a = clamp01(dot3(e, R));
    const float spec = cos_a > 0.0f ? powf(cos_a, L[8]) : 0.0f;
    const float kd = L[6] * cos_t, ks = L[7] * spec;
    dr += kd * L[3], dg += kd * L[4], db += kd * L[5];
    sr += ks * L[3], sg += ks * L[4], sb += ks * L[5];
  }
  out[0] = clamp01(base.x * dr + sr);
  out[1] = clamp01(base.y * dg + sg);
  out[2] = clamp01(base.z * db + sb);
}

// ---- depth L1

__global__ void __launch_bounds__(RN_THREADS)
rnd_depth_l1_k(const float* __restrict__ a, const float* __restrict__ b, int64_t hw, double* __restrict__ out) {
  __shared__ double part[RN_THREADS / 64];
  const size_t base = (size_t)blockIdx.x * (size_t)hw;
  double s = 0.0;
  for (int64_t k = threadIdx.x; k < hw; k += RN_THREADS) s += (double)fabsf(a[base + k] - b[base + k]);
  s = wave_sum(s);
  if (lane_id() == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = part[0];
#pragma unroll
    for (int w = 1; w < RN_THREADS / 64; ++w) total += part[w];
    out[blockIdx.x] = total / (double)hw;
  }
}

// ---- view rejection

__global__ void __launch_bounds__(RN_THREADS)
rnd_flags_clear_k(int32_t* __restrict__ flags, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * RN_THREADS + threadIdx.x;
  if (i < n) flags[i] = 0;
}

__global__ void __launch_bounds__(RN_THREADS)
rnd_views_see_k(const float* __restrict__ pts, int64_t N, const float* __restrict__ w2c, float fx, float fy, float cx,
                float cy, float width, float height, int32_t* __restrict__ flags) {
  const float* __restrict__ m = w2c + 12 * (size_t)blockIdx.y;
  const int64_t first = (int64_t)blockIdx.x * RN_CHUNK;
  bool found = false;
  for (int k = threadIdx.x; k < RN_CHUNK && !found; k += RN_THREADS) {
    const int64_t i = first + k;
    if (i >= N) break;
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    const float pz = m[8] * x + m[9] * y + m[10] * z + m[11];
    const float q = pz - 1e-5f;
    if (!(q >= 0.0f)) continue;
    const float px = m[0] * x + m[1] * y + m[2] * z + m[3];
    const float py = m[4] * x + m[5] * y + m[6] * z + m[7];
    const float u = (fx * px + cx * pz) / q, r = (fy * py + cy * pz) / q;
    found = u > 0.0f && u < width && r > 0.0f && r < height;            // NaN (q = 0, numerator 0) fails
  }
  if (found) flags[blockIdx.y] = 1;                                     // every writer stores the same value
}

}  // namespace

extern "C" int64_t msdf_rnd_visibility_workspace_bytes(int64_t n_views, int64_t height, int64_t width) {
  if (!image_ok(n_views, height, width)) return -1;
  return 8 * n_views * height * width;
}

extern "C" int msdf_rnd_visibility(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                   const float* w2c, int64_t n_views, float fx, float fy, float cx, float cy,
                                   int64_t height, int64_t width, float znear, float zfar, float pixel_center, int cull,
                                   void* workspace, float* depth, int32_t* face, void* stream) {
  if (!fits_int32(n_verts) || !fits_int32(n_faces) || !image_ok(n_views, height, width) ||
      !intrinsics_ok(fx, fy, cx, cy) || !(znear > 0.0f) || !(zfar >= znear) || !(pixel_center == pixel_center) ||
      cull < 0 || cull > 2)
    return MSDF_ERR_ARG;
  const int64_t n_px = n_views * height * width;
  if (n_px == 0) return MSDF_OK;
  if (!depth || !face || !workspace || !w2c || (n_faces > 0 && (!verts || !faces))) return MSDF_ERR_ARG;
  const hipStream_t s = (hipStream_t)stream;
  unsigned long long* ws = (unsigned long long*)workspace;
  rnd_vis_clear_k<<<blocks_for(n_px, RN_THREADS), RN_THREADS, 0, s>>>(ws, n_px);
  if (n_faces > 0 && n_verts > 0) {
    const RasterCam cam{fx, fy, cx, cy, pixel_center, znear, zfar, (int)height, (int)width};
    for (int64_t v0 = 0; v0 < n_views; v0 += RN_VIEWS_PER_LAUNCH) {
      const int64_t nv = n_views - v0 < RN_VIEWS_PER_LAUNCH ? n_views - v0 : RN_VIEWS_PER_LAUNCH;
      rnd_vis_tri_k<<<dim3((unsigned)blocks_for(n_faces, RN_THREADS), (unsigned)nv), RN_THREADS, 0, s>>>(
          verts, n_verts, faces, n_faces, w2c + 12 * v0, cam, cull, ws + v0 * height * width);
    }
  }
  rnd_vis_finish_k<<<blocks_for(n_px, RN_THREADS), RN_THREADS, 0, s>>>(ws, n_px, depth, face);
  return msdf_check_launch();
}

extern "C" int msdf_rnd_vertex_normals(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                       const int32_t* inc_start, const int32_t* inc_face, float* normals,
                                       void* stream) {
  if (!fits_int32(n_verts) || n_faces < 0 || n_faces > MSDF_COUNT_MAX / 3) return MSDF_ERR_ARG;
  if (n_verts == 0) return MSDF_OK;
  if (!verts || !normals || !inc_start || (n_faces > 0 && (!faces || !inc_face))) return MSDF_ERR_ARG;
  rnd_vertex_normals_k<<<blocks_for(n_verts, RN_THREADS), RN_THREADS, 0, (hipStream_t)stream>>>(verts, n_verts, faces,
                                                                                                n_faces, inc_start,
                                                                                                inc_face, normals);
  return msdf_check_launch();
}

extern "C" int msdf_rnd_shade(const int32_t* face, const float* depth, int64_t n_views, int64_t height, int64_t width,
                              const float* w2c, float fx, float fy, float cx, float cy, float pixel_center,
                              const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                              const float* normals, const float* colors, float base_r, float base_g, float base_b,
                              const float* lights, float centre_x, float centre_y, float centre_z, float extent,
                              int flat, int two_sided, float* rgb, void* stream) {
  if (!fits_int32(n_verts) || !fits_int32(n_faces) || !image_ok(n_views, height, width) ||
      !intrinsics_ok(fx, fy, cx, cy) || !(pixel_center == pixel_center))
    return MSDF_ERR_ARG;
  const int64_t n_px = n_views * height * width;
  if (n_px == 0) return MSDF_OK;
  if (!face || !depth || !w2c || !lights || !rgb ||
      (n_faces > 0 && (!verts || !faces || n_verts == 0 || (!flat && !normals))))
    return MSDF_ERR_ARG;
  const ShadeArgs p{fx, fy, cx, cy, pixel_center, base_r, base_g, base_b, centre_x, centre_y, centre_z, extent,
                    (int)height, (int)width, flat ? 1 : 0, two_sided ? 1 : 0};
  rnd_shade_k<<<blocks_for(n_px, RN_THREADS), RN_THREADS, 0, (hipStream_t)stream>>>(face, depth, n_px, w2c, p, verts,
                                                                                    n_verts, faces, n_faces, normals,
                                                                                    colors, lights, rgb);
  return msdf_check_launch();
}

extern "C" int msdf_rnd_depth_l1(const float* a, const float* b, int64_t n_views, int64_t height, int64_t width,
                                 double* out, void* stream) {
  if (!image_ok(n_views, height, width)) return MSDF_ERR_ARG;
  if (n_views * height * width == 0) return MSDF_OK;
  if (!a || !b || !out) return MSDF_ERR_ARG;
  rnd_depth_l1_k<<<(unsigned)n_views, RN_THREADS, 0, (hipStream_t)stream>>>(a, b, height * width, out);
  return msdf_check_launch();
}

extern "C" int msdf_rnd_views_see(const float* points, int64_t n_points, const float* w2c, int64_t n_views, float fx,
                                  float fy, float cx, float cy, int64_t height, int64_t width, int32_t* flags,
                                  void* stream) {
  if (n_points < 0 || n_points > MSDF_COUNT_MAX / 3 || !fits_int32(n_views) || !fits_int32(height) ||
      !fits_int32(width) || !intrinsics_ok(fx, fy, cx, cy))
    return MSDF_ERR_ARG;
  if (n_views == 0) return MSDF_OK;
  if (!flags || !w2c || (n_points > 0 && !points)) return MSDF_ERR_ARG;
  const hipStream_t s = (hipStream_t)stream;
  rnd_flags_clear_k<<<blocks_for(n_views, RN_THREADS), RN_THREADS, 0, s>>>(flags, n_views);
  if (n_points > 0) {
    for (int64_t v0 = 0; v0 < n_views; v0 += RN_VIEWS_PER_LAUNCH) {
      const int64_t nv = n_views - v0 < RN_VIEWS_PER_LAUNCH ? n_views - v0 : RN_VIEWS_PER_LAUNCH;
      rnd_views_see_k<<<dim3((unsigned)blocks_for(n_points, RN_CHUNK), (unsigned)nv), RN_THREADS, 0, s>>>(
          points, n_points, w2c + 12 * v0, fx, fy, cx, cy, (float)width, (float)height, flags + v0);
    }
  }
  return msdf_check_launch();
}
