/* C ABI of the mesh renderer of libmonosdf_hip.so (csrc/meshrender.hip): the device half of utils/mesh_render.py,
 * which stands in for the reference's open3d renderings (render/render_trajectory_open3d.py, render_tntvideos_open3d.py
 * with render/render.json; replica_eval/eval_recon.py:196-285, calc_2d_metric).  Same conventions as monosdf_hip.h, whose
 * status codes these functions return: raw DEVICE pointers, an explicit hipStream_t passed as void*, callers own every
 * buffer, nothing allocates, frees or synchronises.  These entry points are additive: monosdf_hip.h and
 * MSDF_ABI_VERSION are unchanged.
 * Every size lies in [0, 2^31), n_views * height * width among them: a size outside it returns MSDF_ERR_ARG, and so do a
 * null pointer where the sizes leave work to do, znear <= 0, zfar < znear and a cull mode outside 0..2.  Zero work
 * returns MSDF_OK and launches nothing.  No floating-point atomics: the same input gives bitwise the same output
 * every call.
 *
 * Cameras are OpenCV-style (x right, y down, z forward); w2c holds the WORLD-TO-CAMERA rows
 * `r00 r01 r02 tx | r10 r11 r12 ty | r20 r21 r22 tz` (12 floats per view).  The ray of pixel (row i, column j) is
 * d = ((j + pixel_center - cx) / fx, (i + pixel_center - cy) / fy, 1).  fp32 with separately rounded operations unless
 * a line says otherwise.
 *
 * msdf_rnd_visibility: depth[n, H, W] fp32 (0 = background) and face[n, H, W] int32 (-1 = background).  The triangle
 *   set-up and the per-pixel hit test are those of msdf_raster_depth (one definition, csrc/raster_core.h): with
 *   cull = 0 depth is bit for bit msdf_raster_depth's image.  face is the smallest index among the faces that reach
 *   exactly the bits of depth at the pixel.  cull: 0 none, 1 back faces, 2 front faces; a face (a, b, c) is front-facing
 *   at a pixel iff ((b - a) x (c - a)) . d < 0.  Degenerate faces and faces with an index outside [0, V) touch nothing.
 *   One pass of a 64-bit unsigned atomicMin on (bits of z << 32) | face into the workspace, which this entry clears
 *   itself: msdf_rnd_visibility_workspace_bytes(n_views, height, width) = 8 n H W bytes (-1 out of range).
 * msdf_rnd_vertex_normals: normals[V, 3] fp32 = per vertex the sum over its incident faces, in ascending face index, of
 *   (b - a) x (c - a) in fp64 (fp32 coordinates widened; each operation rounded on its own), divided by its fp64
 *   length ((x x + y y) + z z) and rounded once to fp32; (0, 0, 1) where that length is zero or not finite.  Faces with
 *   a repeated index or one outside [0, V) add nothing.  inc_start[V + 1] int32 and inc_face[3 F] int32: the faces of
 *   vertex v are inc_face[inc_start[v] .. inc_start[v + 1]), ascending (entries outside [0, F) are skipped; positions
 *   are clamped to [0, 3 F]).  One lane owns one vertex.
 * msdf_rnd_shade: rgb[n, H, W, 3] fp32 from face and depth, in the camera frame of each view.  Background (face < 0 or
 *   >= F, or a face that msdf_rnd_visibility would not touch) gets lights[39..41].  Otherwise with the ray d:
 *     P = depth d.  (w0, w1, w2) = the three edge terms of csrc/raster_core.h for the face (a, b, c): d . (a x (b - a)),
 *     d . (b x (c - b)), d . (c x (a - c)); s = (w0 + w1) + w2; the weights of a, b, c are w1 / s, w2 / s, w0 / s.
 *     N = unit(wa Na + wb Nb + wc Nc) of the vertex normals rotated into the camera frame; flat != 0: N = unit of the
 *     face's own normal.  A zero N: the pixel is shaded with N = 0.  two_sided != 0: N = -N when N . (-P) < 0.
 *     base = (base_r, base_g, base_b), or with colors != NULL the vertex colours colors[V, 3] interpolated by the weights.
 *     Light i = 0..3 at L_i = w2c (C + E (p_i.x r + p_i.y u + p_i.z f)): C = (centre_x, centre_y, centre_z), E = extent,
 *     r = row 0, u = -row 1, f = -row 2 of w2c's rotation (for a rigid pose: column 0, -column 1, -column 2 of the
 *     camera-to-world rotation).  l = unit(L_i - P), e = unit(-P), nl = N . l, cos_t = clamp(nl, 0, 1),
 *     R = 2 nl N - l, cos_a = clamp(e . R, 0, 1), spec = cos_a > 0 ? powf(cos_a, s_i) : 0.
 *     rgb = clamp(base (ambient + sum kd_i cos_t c_i) + sum ks_i spec c_i, 0, 1) per channel, sums in ascending i.
 *   lights: 42 floats: per light 9 (position x y z, colour r g b, diffuse power kd, specular power ks, shininess s),
 *   then ambient r g b, then background r g b.  unit(v) = v / sqrtf((x x + y y) + z z); unit(0) = 0.
 * msdf_rnd_depth_l1: out[n] fp64 = per view the mean over its H W pixels of |a - b|, the difference and its absolute
 *   value in fp32, the sum in fp64: one workgroup of 256 lanes per view; lane t adds pixels t, t + 256, .. in ascending
 *   order, the 64 lanes of a wave by the xor tree 32, 16, .. 1, the four waves in ascending order; / (double)(H W).
 * msdf_rnd_views_see: flags[n] int32 = 1 iff some point of points[N, 3] projects into view v's frame (check_proj of
 *   eval_recon.py:68-94 in the OpenCV frame), else 0: with (x, y, z) = w2c p as msdf_cull_vertices forms it and
 *   q = z - 1e-5f:  q >= 0 and 0 < (fx x + cx z) / q < width and 0 < (fy y + cy z) / q < height (NaN fails).
 *   Grid: chunks of 2048 points x views; a chunk that finds a point stores 1 with a plain store.  Clears flags itself. */
#ifndef MONOSDF_RENDER_H
#define MONOSDF_RENDER_H

#include <stdint.h>
#include "monosdf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t msdf_rnd_visibility_workspace_bytes(int64_t n_views, int64_t height, int64_t width);
int msdf_rnd_visibility(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* w2c,
                        int64_t n_views, float fx, float fy, float cx, float cy, int64_t height, int64_t width,
                        float znear, float zfar, float pixel_center, int cull, void* workspace, float* depth,
                        int32_t* face, void* stream);
int msdf_rnd_vertex_normals(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                            const int32_t* inc_start, const int32_t* inc_face, float* normals, void* stream);
int msdf_rnd_shade(const int32_t* face, const float* depth, int64_t n_views, int64_t height, int64_t width,
                   const float* w2c, float fx, float fy, float cx, float cy, float pixel_center, const float* verts,
                   int64_t n_verts, const int32_t* faces, int64_t n_faces, const float* normals, const float* colors,
                   float base_r, float base_g, float base_b, const float* lights, float centre_x, float centre_y,
                   float centre_z, float extent, int flat, int two_sided, float* rgb, void* stream);
int msdf_rnd_depth_l1(const float* a, const float* b, int64_t n_views, int64_t height, int64_t width, double* out,
                      void* stream);
int msdf_rnd_views_see(const float* points, int64_t n_points, const float* w2c, int64_t n_views, float fx, float fy,
                       float cx, float cy, int64_t height, int64_t width, int32_t* flags, void* stream);

#ifdef __cplusplus
}
#endif

#endif
