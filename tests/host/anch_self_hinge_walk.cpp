// tests/host/anch_self_hinge_walk.cpp -- the pair function of the self hinges (anch_self_feet, gik_anch_pairs.h) as a
// program of its own: walked over the hand-made and planted cells of anch_self_walk.cpp (zero-length, crossing, nanometre,
// parallel overlapping / disjoint / exact-multiple links) and over 400 random point matrices x every pair of 12 links, on
// exactly sized heap arrays.  Checked: sqrt(d) - rho - rho' is anch_self_pair's value in all 64 bits (true by
// construction since anch_self_pair calls anch_self_feet; what the bits were before is the digest's to say); (s, t) lie in [0, 1],
// v is the vector between the points they name and d its square, and |v| is the distance of the two segments, each
// against a long-double restatement; the residual is finite, and never positive with R = 0.
// tests/test_anchored_self_hinges_host.py compiles it (host only, with the address and undefined-behaviour sanitizers) and
// runs it; it prints "ok ..." with the worst differences, one pinned pair, and the digest of (s, t, v, d) of every random
// cell (walk_digest.h).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static bool same_bits(double x, double y) { return std::memcmp(&x, &y, sizeof(double)) == 0; }

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

// the distance of two segments from the definition: the squared distance is convex in (s, t) over the unit square, so the
// minimum is at the critical point of the two lines where that lies inside, or on an edge of the square -- an end of one
// link against the whole of the other
static long double dist_ref(const double *a1, const double *b1, const double *a2, const double *b2) {
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
  return best;
}

struct Worst {
  double dist = 0.0, vec = 0.0, sq = 0.0;
};

// one pair: every check of the header comment; cell: 3 (s: 0, inside, 1) + (t: 0, inside, 1)
static int walk_pair(const double *a1, const double *b1, const double *a2, const double *b2, double rho1, double rho2, Worst &w,
                     int &cell) {
  double s, t, v[3], d;
  anch_self_feet(a1, b1, a2, b2, s, t, v, d);
  CHECK(s >= 0.0 && s <= 1.0 && t >= 0.0 && t <= 1.0);
  CHECK(d == d && d >= 0.0);
  CHECK(same_bits(std::sqrt(d) - rho1 - rho2, anch_self_pair(a1, b1, a2, b2, rho1, rho2)));
  long double v2 = 0;
  for (int c = 0; c < 3; ++c) {
    const long double vc = ((long double)a1[c] + (long double)s * ((long double)b1[c] - a1[c])) -
                           ((long double)a2[c] + (long double)t * ((long double)b2[c] - a2[c]));
    const double err = (double)fabsl(vc - v[c]);
    w.vec = err > w.vec ? err : w.vec;
    v2 += vc * vc;
  }
  const double esq = (double)fabsl(v2 - d);
  w.sq = esq > w.sq ? esq : w.sq;
  const double ed = (double)fabsl((long double)std::sqrt(d) - dist_ref(a1, b1, a2, b2));
  w.dist = ed > w.dist ? ed : w.dist;
  const double R = rho1 + rho2, res = anch_self_res(R, d);
  CHECK(res == res && res <= R * R);
  CHECK(!(anch_self_res(0.0, d) > 0.0));
  CHECK((res > 0.0) == (R * R > d));
  cell = 3 * (s == 0.0 ? 0 : (s == 1.0 ? 2 : 1)) + (t == 0.0 ? 0 : (t == 1.0 ? 2 : 1));
  return 0;
}

int main() {
  Worst w;
  int cell = 0;
  // ---- hand-made cells: link 1 along x from 0 to 1, link 2 of length 1 along y from (x0, y0, z0), in eighths (exact)
  {
    const double a1[3] = {0, 0, 0}, b1[3] = {1, 0, 0};
    const double cells[9][3] = {{-0.375, 0.5, 0}, {-0.375, -0.5, 0.5}, {-0.375, -1.5, 0},
                                {0.25, 0.5, 0.375}, {0.5, -0.5, 0.25}, {0.25, -1.5, 0.375},
                                {1.375, 0.5, 0}, {1.375, -0.5, 0.5}, {1.375, -1.5, 0}};
    for (int k = 0; k < 9; ++k) {
      const double a2[3] = {cells[k][0], cells[k][1], cells[k][2]}, b2[3] = {cells[k][0], cells[k][1] + 1.0, cells[k][2]};
      CHECK(walk_pair(a1, b1, a2, b2, 0.03, 0.02, w, cell) == 0 && cell == k);
      double s, t, v[3], d;
      anch_self_feet(a1, b1, a2, b2, s, t, v, d);
      CHECK(d == (k == 4 ? 0.0625 : 0.390625));      // 0.25^2, 0.625^2
      CHECK(walk_pair(a2, b2, a1, b1, 0.0, 0.0, w, cell) == 0);
    }
    const double po[2][3] = {{0.5, 0.25, 0}, {1.5, 0.25, 0}}, pd[2][3] = {{1.375, 0.5, 0}, {2.375, 0.5, 0}};
    double s, t, v[3], d;
    anch_self_feet(a1, b1, po[0], po[1], s, t, v, d);      // parallel, overlapping: the foot pair of the s = 0 branch, finite
    CHECK(d == 0.0625 && v[0] == 0.0 && v[1] == -0.25 && v[2] == 0.0 && s == 0.5 && t == 0.0);
    CHECK(walk_pair(a1, b1, po[0], po[1], 0.125, 0.0625, w, cell) == 0);
    CHECK(walk_pair(a1, b1, pd[0], pd[1], 0.0, 0.0, w, cell) == 0);      // parallel, disjoint
    const double x[2][3] = {{0.5, -0.5, 0}, {0.5, 0.5, 0}};
    anch_self_feet(a1, b1, x[0], x[1], s, t, v, d);         // crossing
    CHECK(d == 0.0 && s == 0.5 && t == 0.5 && anch_self_res(0.05, d) == 0.05 * 0.05);
    CHECK(walk_pair(a1, b1, x[0], x[1], 0.03, 0.02, w, cell) == 0 && cell == 4);
    const double pt[3] = {0.5, 0.25, 0}, far[3] = {-0.375, 0.5, 0};
    CHECK(walk_pair(a1, b1, pt, pt, 0.0, 0.0, w, cell) == 0 && walk_pair(pt, pt, a1, b1, 0.0, 0.0, w, cell) == 0);   // one zero-length link
    CHECK(walk_pair(a1, a1, far, far, 0.01, 0.0, w, cell) == 0 && cell == 0);      // two: point against point
    CHECK(walk_pair(a1, a1, a1, a1, 0.03, 0.03, w, cell) == 0 && cell == 0);       // ... the same point: d = 0, finite
    const double nan = std::nan("");      // a NaN end: d is NaN, the hinge inactive
    const double bad[3] = {nan, 0, 0};
    anch_self_feet(a1, b1, bad, x[1], s, t, v, d);
    CHECK(d != d && !(anch_self_res(0.06, d) > 0.0));
  }
  // ---- random and planted cells on exactly sized heap arrays, indexed as the kernel indexes them
  const int CELLS = 400, full_N = 22, n_link = 12;
  std::vector<double> Y((size_t)CELLS * full_N * 3), rho(n_link);
  std::vector<int> la(n_link), lb(n_link), pl, pm;
  for (int l = 0; l < 10; ++l) la[l] = 2 * l, lb[l] = 2 * l + 1;
  la[10] = 19, lb[10] = 20, la[11] = 20, lb[11] = 21;
  for (int l = 0; l < n_link; ++l) rho[l] = l % 2 ? 0.03 : 0.0;
  for (int l = 0; l < n_link; ++l)
    for (int m = l + 1; m < n_link; ++m) pl.push_back(l), pm.push_back(m);
  const int n_pair = (int)pl.size();
  CHECK(n_pair == 66);
  int cells[9] = {0}, active = 0;
  WalkDigest dg;
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
        const double p = row(4)[c] + 0.3 * (row(5)[c] - row(4)[c]), u = uniform(-0.5, 0.5);
        row(6)[c] = p - 0.4 * u;
        row(7)[c] = p + 0.6 * u;
      }
    if (b % 5 == 3)       // link 0 is about a nanometre long
      for (int c = 0; c < 3; ++c) row(1)[c] = row(0)[c] + 1e-9 * (c + 1);
    if (b % 5 == 4) {     // link 5 is parallel to link 4: beside it, or beyond its end; b % 20 == 19: twice its vector
      const double along = b % 10 == 9 ? 1.5 : 0.25, len = b % 20 == 19 ? 2.0 : 0.7;
      for (int c = 0; c < 3; ++c) {
        const double d = row(9)[c] - row(8)[c];
        row(10)[c] = row(8)[c] + along * d + (c == 0 ? 0.05 : 0.0);
        row(11)[c] = row(10)[c] + len * d;
      }
    }
    for (int p = 0; p < n_pair; ++p) {
      const int l = pl[p], k = pm[p];
      const double *a1 = y + la[l] * 3, *b1 = y + lb[l] * 3, *a2 = y + la[k] * 3, *b2 = y + lb[k] * 3;
      CHECK(walk_pair(a1, b1, a2, b2, rho[l], rho[k], w, cell) == 0);
      ++cells[cell];
      double s, t, v[3], d;
      anch_self_feet(a1, b1, a2, b2, s, t, v, d);
      dg.add(s), dg.add(t), dg.add(v[0]), dg.add(v[1]), dg.add(v[2]), dg.add(d);
      active += anch_self_res(0.03 + 0.03, d) > 0.0;
    }
  }
  for (int k = 0; k < 9; ++k) CHECK(cells[k] > 20);
  CHECK(active > 10);
  CHECK(w.dist < 1e-12 && w.vec < 1e-12 && w.sq < 1e-12);
  std::printf("ok cells %d pairs %d clamp", CELLS, CELLS * n_pair);
  for (int k = 0; k < 9; ++k) std::printf(" %d", cells[k]);
  std::printf(" active %d worst distance %.3g vector %.3g square %.3g\n", active, w.dist, w.vec, w.sq);
  const double a1[3] = {0.1, -0.2, 0.3}, b1[3] = {0.7, 0.4, -0.1}, a2[3] = {0.35, 0.2, 0.25}, b2[3] = {-0.15, 0.6, 0.45};
  double s, t, v[3], d;
  anch_self_feet(a1, b1, a2, b2, s, t, v, d);
  std::printf("pinned s %a t %a v %a %a %a d %a value %a\n", s, t, v[0], v[1], v[2], d, std::sqrt(d) - 0.03 - 0.02);
  std::printf("digest %016llx\n", (unsigned long long)dg.h);
  return 0;
}
