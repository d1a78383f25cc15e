// graphik_amd/csrc/gik_anch_pairs.h -- the pair geometry of the fixed-anchor solve, once: a link against a sphere, a link
// against a link, and the two functions of the sweep.  The clearance kernels (gik_anch_seed.hip.h) and the hinges of the
// solve kernels (WaveCtx<.., LINKS> and <.., SELF>, gik_wave.hip.h) call the same functions, so the restart rule, which reads
// a clearance, and the cost, which acts on a hinge, agree bit for bit on what "inside" is.  No kernels and no argument
// structs: all __host__ __device__ inline, so that a host program can walk them (tests/host/anch_*_walk.cpp), and every
// product and sum rounded on its own (contraction off), so that numpy can restate them (AnchoredProblem's *_host mirrors).
#pragma once

#include <hip/hip_runtime.h>

namespace gik {

// ---- a link against a sphere ----
// The (link, sphere) pair as the solve kernel's link hinge reads it: a, b the link's ends, s the sphere's centre;
// d = b - a, L2 = d.d, u = s - a and the foot parameter t = u.d / L2 clamped to [0, 1] -- the nearest point of the segment is
// a + t d, and a zero-length link is its point (t = 0) -- the vector m = (1 - t) a + t b - c from the centre to the foot, and
// d = m.m.  The hinge is  res = (r + rho)^2 - d > 0  (AnchoredProblem.link_hinge_terms_host is the same operations in
// numpy); t = 0 gives m = a - c and t = 1 gives m = b - c exactly, so a link that clamps to an end carries that end's node
// residual.  This text runs inside the solve kernels: it stays as it is.
__host__ __device__ inline void anch_link_foot(const double *a, const double *b, const double *s, double &t, double (&m)[3],
                                               double &d) {
#pragma clang fp contract(off)
  const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
  const double L2 = dx * dx + dy * dy + dz * dz;
  const double ux = s[0] - a[0], uy = s[1] - a[1], uz = s[2] - a[2];
  t = 0.0;
  if (L2 > 0.0) {
    t = (ux * dx + uy * dy + uz * dz) / L2;
    t = t > 0.0 ? t : 0.0;
    t = t < 1.0 ? t : 1.0;
  }
  const double w = 1.0 - t;
  m[0] = (w * a[0] + t * b[0]) - s[0];
  m[1] = (w * a[1] + t * b[1]) - s[1];
  m[2] = (w * a[2] + t * b[2]) - s[2];
  d = m[0] * m[0] + m[1] * m[1] + m[2] * m[2];
}

// clearance of one (link, sphere) pair: s = (centre, r^2), rho the link's radius (AnchoredProblem.link_clearance is the
// same operations in numpy).  The foot parameter t, with its clamps and its zero-length case, is the hinge's, by calling
// it (m and d.m fall away unused); the vector is NOT, on purpose: the clearance takes v = u - t d and the hinge
// m = ((1 - t) a + t b) - c, which round differently, and both sets of bits are pinned by tests.  Do not unify the two
// vectors.  (d, L2 and u are spelled again here, not handed back by a helper under both: every helper tried changed the
// operand order of one addition per hinge in the LINKS solve kernels -- docs/NOTEBOOK.md 40.)  A NaN in either end comes out
// as NaN: one in b alone would otherwise be lost where L2 > 0 is false.
__host__ __device__ inline double anch_link_pair(const double *a, const double *b, const double *s, double rho) {
#pragma clang fp contract(off)
  const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
  const double L2 = dx * dx + dy * dy + dz * dz;
  const double ux = s[0] - a[0], uy = s[1] - a[1], uz = s[2] - a[2];
  double t, m[3], dm;
  anch_link_foot(a, b, s, t, m, dm);
  const double vx = ux - t * dx, vy = uy - t * dy, vz = uz - t * dz;
  const double v = sqrt(vx * vx + vy * vy + vz * vz) - sqrt(s[3]) - rho;
  return L2 != L2 ? __builtin_nan("") : v;
}

// ---- a link against a link ----
// The closest points of the segments a1 -> b1 and a2 -> b2, as the solve kernel's self hinge reads them: a1 + s d1 and
// a2 + t d2, the vector v between them and d = v.v.  s from the unconstrained minimum clamped to [0, 1], t from s, and where
// t leaves [0, 1] it is clamped and s taken again for that end.  A zero-length link is its point (a == 0: s = 0 and t is
// the foot of that point; e == 0: it has no t to solve for and takes the t = 0 branch, whose s is the foot of its point;
// both: the two points); parallel links (den == 0) take s = 0 and the clamps: exactly parallel overlapping links get the
// foot pair of that branch, finite, a kink of measure zero; crossing links give d = 0.
// (AnchoredProblem.self_feet_host is the same operations in numpy.)
__host__ __device__ inline void anch_self_feet(const double *a1, const double *b1, const double *a2, const double *b2, double &s,
                                               double &t, double (&v)[3], double &d) {
#pragma clang fp contract(off)
  const double d1x = b1[0] - a1[0], d1y = b1[1] - a1[1], d1z = b1[2] - a1[2];
  const double d2x = b2[0] - a2[0], d2y = b2[1] - a2[1], d2z = b2[2] - a2[2];
  const double rx = a1[0] - a2[0], ry = a1[1] - a2[1], rz = a1[2] - a2[2];
  const double a = d1x * d1x + d1y * d1y + d1z * d1z;
  const double e = d2x * d2x + d2y * d2y + d2z * d2z;
  const double f = d2x * rx + d2y * ry + d2z * rz;
  const double c = d1x * rx + d1y * ry + d1z * rz;
  const double b = d1x * d2x + d1y * d2y + d1z * d2z;
  const double den = a * e - b * b;
  s = 0.0;
  if (a > 0.0 && den > 0.0) {
    s = (b * f - c * e) / den;
    s = s > 0.0 ? s : 0.0;
    s = s < 1.0 ? s : 1.0;
  }
  t = e > 0.0 ? (b * s + f) / e : -1.0;
  if (t < 0.0) {
    t = 0.0;
    s = 0.0;
    if (a > 0.0) {
      s = -c / a;
      s = s > 0.0 ? s : 0.0;
      s = s < 1.0 ? s : 1.0;
    }
  } else if (t > 1.0) {
    t = 1.0;
    s = 0.0;
    if (a > 0.0) {
      s = (b - c) / a;
      s = s > 0.0 ? s : 0.0;
      s = s < 1.0 ? s : 1.0;
    }
  }
  v[0] = (a1[0] + s * d1x) - (a2[0] + t * d2x);
  v[1] = (a1[1] + s * d1y) - (a2[1] + t * d2y);
  v[2] = (a1[2] + s * d1z) - (a2[2] + t * d2z);
  d = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
}
// the residual of a self hinge, R = rho1 + rho2 and d of anch_self_feet: R^2 - d in two rounded operations.  Active where
// it is positive; R = 0 gives -d <= 0, never active.
__host__ __device__ inline double anch_self_res(double R, double d) {
#pragma clang fp contract(off)
  const double R2 = R * R;
  return R2 - d;
}

// clearance of one (link, link) pair: the distance of anch_self_feet less the two radii; crossing links give -rho1 - rho2
// (AnchoredProblem.self_clearance is the same operations in numpy).  A NaN in any end comes out as NaN with no guard of
// its own: every coordinate enters v through a sum -- a1 and a2 directly, b1 and b2 through s * d1 and t * d2, which are
// NaN for a NaN d1 or d2 even where s or t is 0 -- and s and t can only be NaN where a coordinate is.
__host__ __device__ inline double anch_self_pair(const double *a1, const double *b1, const double *a2, const double *b2,
                                                 double rho1, double rho2) {
#pragma clang fp contract(off)
  double s, t, v[3], d;
  anch_self_feet(a1, b1, a2, b2, s, t, v, d);
  return sqrt(d) - rho1 - rho2;
}

// ---- the sweep ----
// sample s of 0 .. S between two joint angles: two rounded products and one rounded sum, as the retry seeds are
// written; s = 0 gives qa and s = S gives qb (finite angles; the sign of a zero aside)
__host__ __device__ inline double anch_sweep_interp(double qa, double qb, int s, int S) {
#pragma clang fp contract(off)
  const double w = (double)s / (double)S;
  const double pa = (1.0 - w) * qa;
  const double pb = w * qb;
  return pa + pb;
}

// min of n values `stride` apart; a NaN among them gives NaN (fmin would drop it)
__host__ __device__ inline double anch_sweep_min(const double *c, int n, size_t stride) {
  double m = __builtin_huge_val();
  bool nan = false;
  for (int s = 0; s < n; ++s) {
    const double v = c[(size_t)s * stride];
    nan |= v != v;
    m = v < m ? v : m;
  }
  return nan ? __builtin_nan("") : m;
}

}  // namespace gik
