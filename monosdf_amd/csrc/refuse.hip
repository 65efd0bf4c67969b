// Mesh re-fusion on the device: what the reference's evaluation does to a mesh before it scores it
// (scannet_eval/evaluate.py:111-137 and postprocess/refuse.py with pyrender + open3d's ScalableTSDFVolume;
// replica_eval/cull_mesh.py:58-87).  Four groups of kernels, none with a floating-point atomic: the same inputs give
// bitwise the same outputs every call.  Cameras are OpenCV-style (x right, y down, z forward); every kernel gets the
// WORLD-TO-CAMERA rows `r00 r01 r02 tx | r10 r11 r12 ty | r20 r21 r22 tz` (12 floats per view), inverted by the caller.
// This object is built with -ffp-contract=off: the TSDF and culling rules are the separately rounded fp32 operations
// the numpy restatement (tests/refuse_numpy.py) performs, and the rasteriser's edge tests rely on a * b - c * d
// changing sign exactly when its operands are swapped.
//
// Depth rasteriser (raster_*_k): the shared triangle rasteriser of raster_core.h (set-up, box walk, wave hand-round,
// hit test; grid.y = view) with this file's action at an accepted pixel:
//   * the minimum is kept with a 32-bit unsigned atomicMin on the bits of z (positive floats order as unsigned
//     integers, as in nn_finish_k); a minimum does not depend on order.  raster_clear_k writes +inf before,
//     raster_finish_k turns +inf into 0 (background) after.
// Degenerate faces (a repeated vertex, n . d = 0, an index outside [0, V)) touch no pixel.
//
// TSDF integration (tsdf_integrate_k): one lane owns one voxel of a dense block and loops over the views in the order
// given; the camera rows are wave-uniform reads, the running mean stays in registers and each voxel is written once.
// Face rule (tsdf_face_keep_k) and frustum culling (cull_vertices_k): one lane per face / vertex.
#include "tool_common.h"
#include "raster_core.h"

namespace {

constexpr int RF_THREADS = 256;
constexpr unsigned RASTER_INF = 0x7f800000u;       // bits of +inf

// the action of the depth image at an accepted pixel: the minimum of the bits of z
struct DepthMin {
  unsigned* __restrict__ img;
  __device__ __forceinline__ void operator()(const TriSetup&, const RasterCam& cam, int i, int j, float z,
                                             float) const {
    unsigned* p = img + (size_t)i * (size_t)cam.width + (size_t)j;
    const unsigned bits = __float_as_uint(z);                           // z > 0: ordered as unsigned
    if (bits < *p) atomicMin(p, bits);                                  // values only fall: a stale read costs an atomic
  }
};

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
  raster_triangle(verts, V, faces, F, f, m, cam, DepthMin{img});
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
    const float pz = affine_row<2>(m, x, y, z);
    if (!(pz > 0.0f)) continue;
    const float px = affine_row<0>(m, x, y, z);
    const float py = affine_row<1>(m, x, y, z);
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

}  // namespace

extern "C" int msdf_raster_depth(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                 const float* w2c, int n_views, float fx, float fy, float cx, float cy, int height,
                                 int width, float znear, float zfar, float pixel_center, float* depth, void* stream) {
  if (!fits_int32(n_verts) || !fits_int32(n_faces) || n_views < 0 || n_views > 65535 ||
      height < 1 || width < 1 || (int64_t)height * width > MSDF_COUNT_MAX || !intrinsics_ok(fx, fy, cx, cy) ||
      !(znear > 0.0f) || !(zfar >= znear) || !(pixel_center == pixel_center))
    return MSDF_ERR_ARG;
  if (n_views == 0) return MSDF_OK;
  if (!depth || !w2c || (n_faces > 0 && (!verts || !faces))) return MSDF_ERR_ARG;
  const hipStream_t s = (hipStream_t)stream;
  const int64_t n_px = (int64_t)n_views * height * width;
  unsigned* img = (unsigned*)depth;
  raster_clear_k<<<blocks_for(n_px, RF_THREADS), RF_THREADS, 0, s>>>(img, n_px);
  if (n_faces > 0 && n_verts > 0) {
    const RasterCam cam{fx, fy, cx, cy, pixel_center, znear, zfar, height, width};
    raster_tri_k<<<dim3((unsigned)blocks_for(n_faces, RF_THREADS), (unsigned)n_views), RF_THREADS, 0, s>>>(
        verts, n_verts, faces, n_faces, w2c, cam, img);
  }
  raster_finish_k<<<blocks_for(n_px, RF_THREADS), RF_THREADS, 0, s>>>(img, n_px);
  return msdf_check_launch();
}

extern "C" int msdf_tsdf_integrate(const float* depth, const float* w2c, int n_views, float fx, float fy, float cx,
                                   float cy, int height, int width, float ox, float oy, float oz, int i0, int j0, int k0, int nx, int ny,
                                   int nz, float voxel_length, float sdf_trunc, float depth_trunc, int resume,
                                   float* tsdf, float* weight, void* stream) {
  if (n_views < 0 || height < 1 || width < 1 || (int64_t)height * width > MSDF_COUNT_MAX || nx < 1 || ny < 1 ||
      nz < 1 || (int64_t)nx * ny * nz > MSDF_COUNT_MAX || i0 < 0 || j0 < 0 || k0 < 0 || (int64_t)i0 + nx > (1 << 24) ||
      (int64_t)j0 + ny > (1 << 24) || (int64_t)k0 + nz > (1 << 24) || !intrinsics_ok(fx, fy, cx, cy) ||
      !(voxel_length > 0.0f) || !(sdf_trunc > 0.0f) || !(depth_trunc == depth_trunc) || !(ox - ox == 0.0f) || !(oy - oy == 0.0f) || !(oz - oz == 0.0f) || !tsdf || !weight ||
      (n_views > 0 && (!depth || !w2c)))
    return MSDF_ERR_ARG;
  const TsdfArgs p{fx, fy, cx, cy, ox, oy, oz, voxel_length, sdf_trunc, depth_trunc,
                   height, width, nx, ny, nz, n_views, i0, j0, k0, resume ? 1 : 0};
  tsdf_integrate_k<<<blocks_for((int64_t)nx * ny * nz, RF_THREADS), RF_THREADS, 0, (hipStream_t)stream>>>(
      depth, w2c, p, tsdf, weight);
  return msdf_check_launch();
}

extern "C" int msdf_tsdf_face_keep(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                   const float* weight, int nx, int ny, int nz, uint8_t* keep, void* stream) {
  if (!fits_int32(n_verts) || !fits_int32(n_faces) || nx < 1 || ny < 1 || nz < 1 ||
      (int64_t)nx * ny * nz > MSDF_COUNT_MAX)
    return MSDF_ERR_ARG;
  if (n_faces == 0) return MSDF_OK;
  if (!verts || !faces || !weight || !keep) return MSDF_ERR_ARG;
  tsdf_face_keep_k<<<blocks_for(n_faces, RF_THREADS), RF_THREADS, 0, (hipStream_t)stream>>>(verts, n_verts, faces,
                                                                                            n_faces, weight, nx, ny, nz,
                                                                                            keep);
  return msdf_check_launch();
}

extern "C" int msdf_cull_vertices(const float* verts, int64_t n_verts, const float* w2c, int n_views, float fx,
                                  float fy, float cx, float cy, int height, int width, uint8_t* seen, void* stream) {
  if (!fits_int32(n_verts) || n_views < 0 || height < 1 || width < 1 || !intrinsics_ok(fx, fy, cx, cy))
    return MSDF_ERR_ARG;
  if (n_verts == 0) return MSDF_OK;
  if (!verts || !seen || (n_views > 0 && !w2c)) return MSDF_ERR_ARG;
  cull_vertices_k<<<blocks_for(n_verts, RF_THREADS), RF_THREADS, 0, (hipStream_t)stream>>>(verts, n_verts, w2c, n_views,
                                                                                           fx, fy, cx, cy, (float)width,
                                                                                           (float)height, seen);
  return msdf_check_launch();
}
