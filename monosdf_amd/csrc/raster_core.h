// The triangle rasteriser that csrc/refuse.hip (depth) and csrc/meshrender.hip (visibility, shading) share: camera,
// triangle set-up, box walk, the wave hand-round of large boxes and the per-pixel hit test.  What happens at an accepted
// pixel is the template parameter `Action`; everything before it is one definition, so every user accepts exactly the
// same pixels with exactly the same bits of z.  Both users are built with -ffp-contract=off (csrc/Makefile): the edge
// tests rely on a * b - c * d changing sign exactly when its operands are swapped.
//
// Parallel over triangles, one lane each; the caller picks the view (its 12 world-to-camera floats `m`):
//   * the three vertices go to the camera frame; the two edge vectors are formed in WORLD coordinates (exact to an ulp
//     of the edge, not of the distance to the camera) and rotated
//   * per pixel the ray is d = ((j + c - cx) / fx, (i + c - cy) / fy, 1); the side test of edge (p, q) is
//     d . (p x (q - p)) with p the endpoint of the SMALLER vertex index, negated when the triangle runs the edge the
//     other way: two triangles that share an edge evaluate the same expression with opposite sign, and `>= 0` (or,
//     for the other winding, `<= 0`) on all three edges accepts the ray on both sides -- no cracks
//   * depth z = (n . a) / (n . d) with n the plane normal (from the vertices in ascending index, a the first): ray
//     against plane per pixel, nothing interpolated from projected vertices, so a triangle that crosses the near plane
//     covers what its visible part covers.  `odd` records whether that ascending sort was an odd permutation of the
//     face's own order: the face's own normal is n when it is 0 and -n when it is 1
//   * a triangle whose vertices all lie at z >= znear is bounded by the box of its projection (one pixel of slack); one
//     that crosses z = znear takes the whole image
//   * a box of at most RASTER_COOP_AREA pixels is scanned by the lane itself (marching-cubes meshes: millions of
//     triangles of a few pixels); larger boxes are handed round the wave: their set-up is broadcast lane by lane and
//     all 64 lanes stride over the box, so an image-spanning triangle does not serialise on one lane
// Degenerate faces (a repeated vertex, n . d = 0, an index outside [0, V)) touch no pixel.
//
// Action: `void operator()(const TriSetup& t, const RasterCam& cam, int i, int j, float z, float nd) const`, called
// once per accepted (triangle, pixel) with znear <= z <= zfar and nd = n . d != 0.
#pragma once
#include "common.h"

constexpr int RASTER_COOP_AREA = 256;              // boxes of more pixels than this are scanned by the whole wave

struct RasterCam {
  float fx, fy, cx, cy, pc, znear, zfar;
  int height, width;
};

// what the pixel loop needs of one triangle: the three (signed) edge vectors, the plane, the pixel box
struct TriSetup {
  float e0x, e0y, e0z, e1x, e1y, e1z, e2x, e2y, e2z;
  float nx, ny, nz, na;
  int j0, i0, bw, bh;                               // box: columns j0 .. j0 + bw - 1, rows i0 .. i0 + bh - 1; bw = 0: none
  int face, odd;                                    // the face's index; parity of the sort behind (nx, ny, nz)
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

// the ray of pixel (row i, column j) without its z = 1
__device__ __forceinline__ void raster_ray(const RasterCam& cam, int i, int j, float& dx, float& dy) {
  dx = ((float)j + cam.pc - cam.cx) / cam.fx;
  dy = ((float)i + cam.pc - cam.cy) / cam.fy;
}

// the three edge terms of a ray: all >= 0 or all <= 0 inside the triangle; w0 belongs to edge (a, b) and so on
__device__ __forceinline__ void raster_edge_terms(const TriSetup& t, float dx, float dy, float& w0, float& w1,
                                                  float& w2) {
  w0 = dx * t.e0x + dy * t.e0y + t.e0z;
  w1 = dx * t.e1x + dy * t.e1y + t.e1z;
  w2 = dx * t.e2x + dy * t.e2y + t.e2z;
}

template <typename Action>
__device__ __forceinline__ void raster_pixel(const TriSetup& t, const RasterCam& cam, int i, int j,
                                             const Action& action) {
  float dx, dy, w0, w1, w2;
  raster_ray(cam, i, j, dx, dy);
  raster_edge_terms(t, dx, dy, w0, w1, w2);
  const bool in = (w0 >= 0.0f && w1 >= 0.0f && w2 >= 0.0f) || (w0 <= 0.0f && w1 <= 0.0f && w2 <= 0.0f);
  if (!in) return;
  const float nd = dx * t.nx + dy * t.ny + t.nz;
  if (nd == 0.0f) return;
  const float z = t.na / nd;
  if (!(z >= cam.znear && z <= cam.zfar)) return;                      // NaN fails
  action(t, cam, i, j, z, nd);
}

// the three vertices of a face: their indices, world and camera positions
struct FaceVerts {
  int ia, ib, ic;
  V3 wa, wb, wc, a, b, c;
};

// Loads face f and takes its vertices to the camera frame of m.  false for an index outside [0, V).
__device__ __forceinline__ bool raster_face_vertices(const float* __restrict__ verts, int64_t V,
                                                     const int32_t* __restrict__ faces, int64_t f,
                                                     const float* __restrict__ m, FaceVerts& q) {
  const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
  if (!(ia >= 0 && ib >= 0 && ic >= 0 && ia < V && ib < V && ic < V)) return false;
  q.ia = ia, q.ib = ib, q.ic = ic;
  q.wa = V3{verts[3 * (size_t)ia], verts[3 * (size_t)ia + 1], verts[3 * (size_t)ia + 2]};
  q.wb = V3{verts[3 * (size_t)ib], verts[3 * (size_t)ib + 1], verts[3 * (size_t)ib + 2]};
  q.wc = V3{verts[3 * (size_t)ic], verts[3 * (size_t)ic + 1], verts[3 * (size_t)ic + 2]};
  V3 a = rotate(m, q.wa), b = rotate(m, q.wb), c = rotate(m, q.wc);
  q.a = V3{a.x + m[3], a.y + m[7], a.z + m[11]};
  q.b = V3{b.x + m[3], b.y + m[7], b.z + m[11]};
  q.c = V3{c.x + m[3], c.y + m[7], c.z + m[11]};
  return true;
}

// Edge vectors, plane and sort parity of face f from its vertices.  The box is left alone.
__device__ __forceinline__ void raster_face_plane(const float* __restrict__ m, const FaceVerts& q, int64_t f,
                                                  TriSetup& t) {
  const int ia = q.ia, ib = q.ib, ic = q.ic;
  const V3 wa = q.wa, wb = q.wb, wc = q.wc, a = q.a, b = q.b, c = q.c;
  const V3 e0 = edge_vector(m, ia, wa, a, ib, wb, b);
  const V3 e1 = edge_vector(m, ib, wb, b, ic, wc, c);
  const V3 e2 = edge_vector(m, ic, wc, c, ia, wa, a);
  // the plane from the vertices in ascending index, so that every rotation and winding of the face gives the
  // same bits of z
  int s0 = ia, s1 = ib, s2 = ic, odd = 0;
  V3 p0 = wa, p1 = wb, p2 = wc, q0 = a;
  if (s1 < s0) {
    const int ti = s0; s0 = s1; s1 = ti;
    const V3 tp = p0; p0 = p1; p1 = tp;
    q0 = b;
    odd ^= 1;
  }
  if (s2 < s1) {
    const int ti = s1; s1 = s2; s2 = ti;
    const V3 tp = p1; p1 = p2; p2 = tp;
    odd ^= 1;
    if (s1 < s0) {
      const int tj = s0; s0 = s1; s1 = tj;
      const V3 tq = p0; p0 = p1; p1 = tq;
      q0 = c;
      odd ^= 1;
    }
  }
  const V3 n = cross3(rotate(m, V3{p1.x - p0.x, p1.y - p0.y, p1.z - p0.z}),
                      rotate(m, V3{p2.x - p0.x, p2.y - p0.y, p2.z - p0.z}));
  t.e0x = e0.x, t.e0y = e0.y, t.e0z = e0.z;
  t.e1x = e1.x, t.e1y = e1.y, t.e1z = e1.z;
  t.e2x = e2.x, t.e2y = e2.y, t.e2z = e2.z;
  t.nx = n.x, t.ny = n.y, t.nz = n.z;
  t.na = n.x * q0.x + n.y * q0.y + n.z * q0.z;
  t.face = (int)f, t.odd = odd;
}

// One lane's triangle f (any f: a lane past F takes part in the hand-round only) of the view with rows m.  Every lane
// of the wave must call this: the large boxes are scanned by all 64 lanes together.
template <typename Action>
__device__ __forceinline__ void raster_triangle(const float* __restrict__ verts, int64_t V,
                                                const int32_t* __restrict__ faces, int64_t F, int64_t f,
                                                const float* __restrict__ m, const RasterCam& cam,
                                                const Action& action) {
  TriSetup t = {};                                                      // bw = bh = 0: no box
  if (f < F) {
    FaceVerts q;
    if (raster_face_vertices(verts, V, faces, f, m, q)) {
      const V3 a = q.a, b = q.b, c = q.c;
      const float zmin = fminf(a.z, fminf(b.z, c.z)), zmax = fmaxf(a.z, fmaxf(b.z, c.z));
      // every intersection lies between the vertices' depths
      if (zmax >= cam.znear && zmin <= cam.zfar) {
        raster_face_plane(m, q, f, t);
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
        if (j1 >= j0 && i1 >= i0 && !(t.nx == 0.0f && t.ny == 0.0f && t.nz == 0.0f)) {
          t.j0 = j0, t.i0 = i0, t.bw = j1 - j0 + 1, t.bh = i1 - i0 + 1;
        }
      }
    }
  }

  const int area = t.bw * t.bh;                                         // <= height * width < 2^31 (checked by the host)
  const bool large = area > RASTER_COOP_AREA;
  if (area > 0 && !large) {
    for (int i = t.i0; i < t.i0 + t.bh; ++i)
      for (int j = t.j0; j < t.j0 + t.bw; ++j) raster_pixel(t, cam, i, j, action);
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
    s.face = __shfl(t.face, src, 64), s.odd = __shfl(t.odd, src, 64);
    const unsigned n_px = (unsigned)(s.bw * s.bh), bw = (unsigned)s.bw;
    for (unsigned k = (unsigned)lane; k < n_px; k += 64u)
      raster_pixel(s, cam, s.i0 + (int)(k / bw), s.j0 + (int)(k % bw), action);
  }
}
