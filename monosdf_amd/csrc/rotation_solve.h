// The rotation that best maps one set of vectors onto another, from their 3 x 3 cross-covariance: the one definition
// behind the normal-patch fit of highres.hip and the point-to-point update of icp.hip.  include/monosdf_highres.h
// states the rule.  Runs on one lane in fp64.  No fp-contract pragma here: both translation units are built with
// -ffp-contract=off (csrc/Makefile), so every product and sum is rounded on its own in both.
#pragma once

__device__ __forceinline__ double rot_dot3(const double* a, const double* b) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
__device__ __forceinline__ void rot_cross3(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}
// a unit vector perpendicular to the unit vector a: the cross product with the axis of a's smallest component
static __device__ void rot_perpendicular(const double* a, double* c) {
  int m = 0;
  if (fabs(a[1]) < fabs(a[m])) m = 1;
  if (fabs(a[2]) < fabs(a[m])) m = 2;
  double axis[3] = {0.0, 0.0, 0.0};
  axis[m] = 1.0;
  rot_cross3(a, axis, c);
  const double len = sqrt(rot_dot3(c, c));
  c[0] /= len;
  c[1] /= len;
  c[2] /= len;
}

// h: Hm row-major, Hm[a][b] = sum A_a B_b -> r: the rotation row-major, B ~ R A.  One-sided Jacobi on the columns of
// Hm V; always a proper rotation (V diag(1, 1, -1) U^T where V U^T is a reflection); Hm == 0 gives the identity.
static __device__ void solve_rotation(const double* h, double* r) {
  double g[3][3], v[3][3];                               // g[k]: column k of Hm V; v[k]: column k of V
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      g[k][a] = h[3 * a + k];
      v[k][a] = a == k ? 1.0 : 0.0;
    }
  }
  for (int sweep = 0; sweep < 30; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int pair = 0; pair < 3; ++pair) {
      const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2;
      const double alpha = rot_dot3(g[p], g[p]), beta = rot_dot3(g[q], g[q]), gamma = rot_dot3(g[p], g[q]);
      if (gamma == 0.0 || fabs(gamma) <= 1e-15 * sqrt(alpha * beta)) continue;
      rotated = true;
      const double zeta = (beta - alpha) / (2.0 * gamma);
      const double tn = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      const double c = 1.0 / sqrt(1.0 + tn * tn), sn = c * tn;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const double gp = g[p][a], gq = g[q][a], vp = v[p][a], vq = v[q][a];
        g[p][a] = c * gp - sn * gq;
        g[q][a] = sn * gp + c * gq;
        v[p][a] = c * vp - sn * vq;
        v[q][a] = sn * vp + c * vq;
      }
    }
    if (!rotated) break;
  }
  double len[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) len[k] = sqrt(rot_dot3(g[k], g[k]));
  int k1 = 0;                                            // the two longest columns, the earlier one on a tie
  if (len[1] > len[k1]) k1 = 1;
  if (len[2] > len[k1]) k1 = 2;
  int k2 = k1 == 0 ? 1 : 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k != k1 && len[k] > len[k2]) k2 = k;
  }
#pragma unroll
  for (int a = 0; a < 9; ++a) r[a] = (a % 4 == 0) ? 1.0 : 0.0;
  if (!(len[k1] > 0.0)) return;                          // Hm == 0: the identity
  double u1[3], u2[3], v1[3], v2[3], u3[3], v3[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    u1[a] = g[k1][a] / len[k1];
    v1[a] = v[k1][a];
  }
  if (len[k2] <= 1e-300 || len[k2] <= 1e-14 * len[k1]) {
    rot_perpendicular(u1, u2);
    rot_perpendicular(v1, v2);
  } else {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      u2[a] = g[k2][a] / len[k2];
      v2[a] = v[k2][a];
    }
  }
  rot_cross3(u1, u2, u3);
  rot_cross3(v1, v2, v3);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) r[3 * a + b] = (v1[a] * u1[b] + v2[a] * u2[b]) + v3[a] * u3[b];
  }
}
