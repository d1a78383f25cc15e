// tests/host/anch_self_walk.cpp -- the pair function of the self clearance (anch_self_pair, gik_anch_pairs.h) as a
// program of its own: walked over hand-made cells and over 400 random point matrices x every pair of 12 links, with
// planted parallel, crossing, zero-length and nanometre-long links, on exactly sized heap arrays, against a long-double
// restatement.  tests/test_anchored_self_host.py compiles it (host only, with the address and undefined-behaviour
// sanitizers) and runs it; it prints "ok ..." with the worst difference, one pinned value, and the digest of every
// pair value of the random cells (walk_digest.h).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gik_anch_pairs.h"
#include "walk_digest.h"

using namespace gik;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static double uniform(double lo, double hi) { return lo + (hi - lo) * (double)(next_u64() >> 11) * 0x1p-53; }

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// distance from the point p to the segment a -> b in long double, by its three cases
static long double point_segment(const long double *p, const long double *a, const long double *b) {
  long double d[3], u[3], L2 = 0, ud = 0;
  for (int c = 0; c < 3; ++c) {
    d[c] = b[c] - a[c];
    u[c] = p[c] - a[c];
    L2 += d[c] * d[c];
    ud += u[c] * d[c];
  }
  long double t = 0;
  if (L2 > 0) t = ud <= 0 ? 0 : (ud >= L2 ? 1 : ud / L2);
  long double v2 = 0;
  for (int c = 0; c < 3; ++c) v2 += (u[c] - t * d[c]) * (u[c] - t * d[c]);
  return sqrtl(v2);
}

// The same geometry from the definition: the squared distance is convex in (s, t) over the unit square, so its minimum is
// at the critical point of the two lines where that lies inside, or on an edge of the square -- and an edge is an end of
// one link against the whole of the other.  Every candidate is the distance of two points of the links, so a candidate
// computed from an ill-conditioned critical point (nearly parallel lines) can only be too long, never too short.
static long double pair_ref(const double *a1, const double *b1, const double *a2, const double *b2, double rho1, double rho2) {
  long double A1[3], B1[3], A2[3], B2[3];
  for (int c = 0; c < 3; ++c) A1[c] = a1[c], B1[c] = b1[c], A2[c] = a2[c], B2[c] = b2[c];
  long double best = point_segment(A1, A2, B2);
  const long double e1 = point_segment(B1, A2, B2), e2 = point_segment(A2, A1, B1), e3 = point_segment(B2, A1, B1);
  best = e1 < best ? e1 : best;
  best = e2 < best ? e2 : best;
  best = e3 < best ? e3 : best;
  long double d1[3], d2[3], r[3], a = 0, e = 0, f = 0, cc = 0, b = 0;
  for (int c = 0; c < 3; ++c) {
    d1[c] = B1[c] - A1[c];
    d2[c] = B2[c] - A2[c];
    r[c] = A1[c] - A2[c];
    a += d1[c] * d1[c], e += d2[c] * d2[c], f += d2[c] * r[c], cc += d1[c] * r[c], b += d1[c] * d2[c];
  }
  const long double den = a * e - b * b;
  if (den > 0) {
    const long double s = (b * f - cc * e) / den, t = (a * f - b * cc) / den;
    if (s > 0 && s < 1 && t > 0 && t < 1) {
      long double v2 = 0;
      for (int c = 0; c < 3; ++c) {
        const long double v = (A1[c] + s * d1[c]) - (A2[c] + t * d2[c]);
        v2 += v * v;
      }
      const long double in = sqrtl(v2);
      best = in < best ? in : best;
    }
  }
  return best - rho1 - rho2;
}

// which of the nine clamp cells a pair ends in: 3 (s: 0, interior, 1) + (t: 0, interior, 1); the steps of anch_self_pair
static int clamp_cell(const double *a1, const double *b1, const double *a2, const double *b2) {
  double d1[3], d2[3], r[3], a = 0, e = 0, f = 0, c = 0, b = 0;
  for (int k = 0; k < 3; ++k) {
    d1[k] = b1[k] - a1[k], d2[k] = b2[k] - a2[k], r[k] = a1[k] - a2[k];
    a += d1[k] * d1[k], e += d2[k] * d2[k], f += d2[k] * r[k], c += d1[k] * r[k], b += d1[k] * d2[k];
  }
  const double den = a * e - b * b;
  auto clamp = [](double x) { return x > 0.0 ? (x < 1.0 ? x : 1.0) : 0.0; };
  double s = (a > 0.0 && den > 0.0) ? clamp((b * f - c * e) / den) : 0.0;
  double t = e > 0.0 ? (b * s + f) / e : -1.0;
  if (t < 0.0) t = 0.0, s = a > 0.0 ? clamp(-c / a) : 0.0;
  else if (t > 1.0) t = 1.0, s = a > 0.0 ? clamp((b - c) / a) : 0.0;
  return 3 * (s == 0.0 ? 0 : (s == 1.0 ? 2 : 1)) + (t == 0.0 ? 0 : (t == 1.0 ? 2 : 1));
}

int main() {
  const double nan = std::nan("");
  // ---- hand-made cells: link 1 along x from 0 to 1, link 2 of length 1 along y from (x0, y0, z0), in eighths (exact):
  //      s = clamp(x0), t = clamp(-y0), and every clamped cell is a 3-4-5 triangle of hypotenuse 0.625
  {
    const double a1[3] = {0, 0, 0}, b1[3] = {1, 0, 0};
    const double cells[9][3] = {{-0.375, 0.5, 0}, {-0.375, -0.5, 0.5}, {-0.375, -1.5, 0},     // s = 0: t = 0, interior, 1
                                {0.25, 0.5, 0.375}, {0.5, -0.5, 0.25}, {0.25, -1.5, 0.375},   // s interior
                                {1.375, 0.5, 0}, {1.375, -0.5, 0.5}, {1.375, -1.5, 0}};       // s = 1
    for (int k = 0; k < 9; ++k) {
      const double a2[3] = {cells[k][0], cells[k][1], cells[k][2]}, b2[3] = {cells[k][0], cells[k][1] + 1.0, cells[k][2]};
      CHECK(clamp_cell(a1, b1, a2, b2) == k);
      CHECK(anch_self_pair(a1, b1, a2, b2, 0.0, 0.0) == (k == 4 ? 0.25 : 0.625));
      CHECK(anch_self_pair(a2, b2, a1, b1, 0.0, 0.0) == (k == 4 ? 0.25 : 0.625));
    }
    const double po[2][3] = {{0.5, 0.25, 0}, {1.5, 0.25, 0}}, pd[2][3] = {{1.375, 0.5, 0}, {2.375, 0.5, 0}};
    CHECK(anch_self_pair(a1, b1, po[0], po[1], 0.0, 0.0) == 0.25);       // parallel, overlapping
    CHECK(anch_self_pair(a1, b1, pd[0], pd[1], 0.0, 0.0) == 0.625);      // parallel, disjoint: end against end
    const double x[2][3] = {{0.5, -0.5, 0}, {0.5, 0.5, 0}};
    CHECK(anch_self_pair(a1, b1, x[0], x[1], 0.03, 0.02) == -0.03 - 0.02);      // crossing
    const double pt[3] = {0.5, 0.25, 0}, far[3] = {-0.375, 0.5, 0};
    CHECK(anch_self_pair(a1, b1, pt, pt, 0.0, 0.0) == 0.25 && anch_self_pair(pt, pt, a1, b1, 0.0, 0.0) == 0.25);   // one zero-length link
    CHECK(anch_self_pair(a1, a1, far, far, 0.0, 0.0) == 0.625);          // two: point against point
    CHECK(anch_self_pair(a1, b1, po[0], po[1], 0.125, 0.0625) == 0.0625);      // radii subtract exactly
    for (int k = 0; k < 4; ++k) {                                         // a NaN in any of the four ends
      double e[4][3] = {{0, 0, 0}, {1, 0, 0}, {0.5, -0.5, 0.25}, {0.5, 0.5, 0.25}};
      e[k][k % 3] = nan;
      CHECK(std::isnan(anch_self_pair(e[0], e[1], e[2], e[3], 0.0, 0.0)));
    }
  }
  // ---- random and planted cells on exactly sized heap arrays, indexed as the kernel indexes them
  const int CELLS = 400, full_N = 22, n_link = 12;
  std::vector<double> Y((size_t)CELLS * full_N * 3), rho(n_link);
  std::vector<int> la(n_link), lb(n_link), pl, pm;
  for (int l = 0; l < 10; ++l) la[l] = 2 * l, lb[l] = 2 * l + 1;      // ten links with ends of their own ...
  la[10] = 19, lb[10] = 20, la[11] = 20, lb[11] = 21;                 // ... and two that share a row with their neighbour
  for (int l = 0; l < n_link; ++l) rho[l] = l % 2 ? 0.03 : 0.0;
  for (int l = 0; l < n_link; ++l)
    for (int m = l + 1; m < n_link; ++m) pl.push_back(l), pm.push_back(m);
  const int n_pair = (int)pl.size();
  CHECK(n_pair == 66);
  double worst = 0.0;
  WalkDigest dg;
  int cell[9] = {0}, negative = 0, den0 = 0;
  for (int b = 0; b < CELLS; ++b) {
    double *y = Y.data() + (size_t)b * full_N * 3;
    for (int e = 0; e < full_N * 3; ++e) y[e] = uniform(-0.6, 0.6);
    auto row = [&](int i) { return y + i * 3; };
    if (b % 5 == 1)       // link 1 has length zero; every other time link 2 as well
      for (int c = 0; c < 3; ++c) {
        row(3)[c] = row(2)[c];
        if (b % 10 == 6) row(5)[c] = row(4)[c];
      }
    if (b % 5 == 2)       // link 3 passes through a point of link 2
      for (int c = 0; c < 3; ++c) {
        const double p = row(4)[c] + 0.3 * (row(5)[c] - row(4)[c]), w = uniform(-0.5, 0.5);
        row(6)[c] = p - 0.4 * w;
        row(7)[c] = p + 0.6 * w;
      }
    if (b % 5 == 3)       // link 0 is about a nanometre long
      for (int c = 0; c < 3; ++c) row(1)[c] = row(0)[c] + 1e-9 * (c + 1);
    if (b % 5 == 4) {     // link 5 is parallel to link 4: beside it, or every other time beyond its end; b % 20 == 19: twice its vector
      const double along = b % 10 == 9 ? 1.5 : 0.25, len = b % 20 == 19 ? 2.0 : 0.7;
      for (int c = 0; c < 3; ++c) {
        const double d = row(9)[c] - row(8)[c];
        row(10)[c] = row(8)[c] + along * d + (c == 0 ? 0.05 : 0.0);
        row(11)[c] = row(10)[c] + len * d;
      }
    }
    double m = HUGE_VAL;
    for (int p = 0; p < n_pair; ++p) {      // the kernel's pair loop, all lanes
      const int l = pl[p], k = pm[p];
      const double *a1 = y + la[l] * 3, *b1 = y + lb[l] * 3, *a2 = y + la[k] * 3, *b2 = y + lb[k] * 3;
      const double v = anch_self_pair(a1, b1, a2, b2, rho[l], rho[k]);
      dg.add(v);
      CHECK(v == v);
      const double err = (double)fabsl((long double)v - pair_ref(a1, b1, a2, b2, rho[l], rho[k]));
      worst = err > worst ? err : worst;
      const double sw = anch_self_pair(a2, b2, a1, b1, rho[k], rho[l]);      // the links swapped: another branch order
      CHECK(std::fabs(sw - v) <= 1e-13);
      ++cell[clamp_cell(a1, b1, a2, b2)];
      m = v < m ? v : m;
    }
    negative += m < 0;
    den0 += b % 20 == 19;
  }
  for (int k = 0; k < 9; ++k) CHECK(cell[k] > 20);
  CHECK(negative > 10 && den0 > 0);
  CHECK(worst < 1e-12);
  std::printf("ok cells %d pairs %d clamp", CELLS, CELLS * n_pair);
  for (int k = 0; k < 9; ++k) std::printf(" %d", cell[k]);
  std::printf(" colliding %d worst %.3g\n", negative, worst);
  const double a1[3] = {0.1, -0.2, 0.3}, b1[3] = {0.7, 0.4, -0.1}, a2[3] = {0.35, 0.2, 0.25}, b2[3] = {-0.15, 0.6, 0.45};
  std::printf("pinned pair %a\n", anch_self_pair(a1, b1, a2, b2, 0.03, 0.02));
  std::printf("digest %016llx\n", (unsigned long long)dg.h);
  return 0;
}
