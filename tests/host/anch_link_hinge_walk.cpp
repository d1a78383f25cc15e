// tests/host/anch_link_hinge_walk.cpp -- the pair function of the link hinges (anch_link_foot, gik_anch_pairs.h) as a
// program of its own: walked over random point matrices x the chain's skeleton x spheres on exactly sized heap arrays,
// zero-length links, links through a centre and nanometre links among them, against a long-double restatement.
// tests/test_anchored_link_hinges_host.py compiles it (host only, with the address and undefined-behaviour sanitizers)
// and runs it; it prints "ok ...", one pinned pair, which must be the numpy mirror's, and the digest of (t, m, d) of every random
// cell (walk_digest.h).
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

// the same geometry in long double, written from the definition: the nearest point of the segment by its three cases
static void foot_ref(const double *a, const double *b, const double *s, long double &t, long double (&m)[3], long double &d) {
  long double u[3], L2 = 0, cu = 0;
  for (int c = 0; c < 3; ++c) {
    u[c] = (long double)b[c] - a[c];
    L2 += u[c] * u[c];
    cu += ((long double)s[c] - a[c]) * u[c];
  }
  t = 0;
  if (L2 > 0) t = cu <= 0 ? 0 : (cu >= L2 ? 1 : cu / L2);
  d = 0;
  for (int c = 0; c < 3; ++c) {
    m[c] = (long double)a[c] + t * u[c] - s[c];
    d += m[c] * m[c];
  }
}

int main() {
  const int CELLS = 400;
  // ---- hand-made cells: a link along x from 0 to 1
  {
    const double a[3] = {0, 0, 0}, b[3] = {1, 0, 0};
    const double mid[3] = {0.5, 0.3, 0}, before[3] = {-0.3, 0.4, 0}, after[3] = {1.3, 0, 0.4}, on[3] = {0.25, 0, 0};
    double t, m[3], d;
    anch_link_foot(a, b, mid, t, m, d);
    CHECK(t == 0.5 && m[0] == 0.0 && m[1] == -0.3 && m[2] == 0.0 && d == 0.3 * 0.3);      // interior
    anch_link_foot(a, b, before, t, m, d);
    CHECK(t == 0.0 && m[0] == 0.3 && m[1] == -0.4 && d == 0.3 * 0.3 + 0.4 * 0.4);          // end a: m = a - c, exactly
    anch_link_foot(a, b, after, t, m, d);
    CHECK(t == 1.0 && m[0] == 1.0 - 1.3 && m[2] == -0.4);                                  // end b: m = b - c, exactly
    anch_link_foot(a, b, on, t, m, d);
    CHECK(t == 0.25 && d == 0.0);                                                          // the centre on the segment
    anch_link_foot(a, a, before, t, m, d);
    CHECK(t == 0.0 && d == 0.3 * 0.3 + 0.4 * 0.4);                                         // a zero-length link is its point
  }
  // ---- random and degenerate cells on exactly sized heap arrays, indexed as the kernels index them
  const int full_N = 7, n_link = 6, n_obs = 11;
  std::vector<double> Y((size_t)CELLS * full_N * 3), obs((size_t)n_obs * 4), rho(n_link);
  std::vector<int> la(n_link), lb(n_link);
  for (int l = 0; l < n_link; ++l) la[l] = l, lb[l] = l + 1, rho[l] = l % 2 ? 0.03 : 0.0;
  for (int o = 0; o < n_obs; ++o) {
    for (int c = 0; c < 3; ++c) obs[o * 4 + c] = uniform(-1.0, 1.0);
    const double r = uniform(0.05, 0.15);
    obs[o * 4 + 3] = r * r;
  }
  double worst_t = 0.0, worst_m = 0.0, worst_d = 0.0;
  WalkDigest dg;
  int clamp0 = 0, clamp1 = 0, inner = 0, zero = 0, active = 0;
  for (int b = 0; b < CELLS; ++b) {
    double *y = Y.data() + (size_t)b * full_N * 3;
    for (int e = 0; e < full_N * 3; ++e) y[e] = uniform(-1.2, 1.2);
    if (b % 5 == 1)      // a zero-length link
      for (int c = 0; c < 3; ++c) y[3 * 3 + c] = y[2 * 3 + c];
    if (b % 5 == 2)      // a link through a centre
      for (int c = 0; c < 3; ++c) y[5 * 3 + c] = 2.0 * obs[(b % n_obs) * 4 + c] - y[4 * 3 + c];
    if (b % 5 == 3)      // a link of about a nanometre: t is the quotient of two tiny numbers
      for (int c = 0; c < 3; ++c) y[1 * 3 + c] = y[0 * 3 + c] + 1e-9 * (c + 1);
    for (int p = 0; p < n_link * n_obs; ++p) {
      const int l = p / n_obs, o = p - l * n_obs;
      const double *pa = y + la[l] * 3, *pb = y + lb[l] * 3, *s = obs.data() + o * 4;
      double t, m[3], d;
      anch_link_foot(pa, pb, s, t, m, d);
      dg.add(t), dg.add(m[0]), dg.add(m[1]), dg.add(m[2]), dg.add(d);
      long double tr, mr[3], dr;
      foot_ref(pa, pb, s, tr, mr, dr);
      CHECK(t >= 0.0 && t <= 1.0 && d >= 0.0);
      const double dx = pb[0] - pa[0], dy = pb[1] - pa[1], dz = pb[2] - pa[2], L2 = dx * dx + dy * dy + dz * dz;
      // t itself is ill-conditioned on a nanometre link (the quotient of two rounded tiny numbers); the foot is not: an
      // error e in t moves it by e |b - a|
      const double len = std::sqrt(L2);
      const double et = (double)fabsl((long double)t - tr) * len;
      worst_t = et > worst_t ? et : worst_t;
      for (int c = 0; c < 3; ++c) {
        const double em = (double)fabsl((long double)m[c] - mr[c]);
        worst_m = em > worst_m ? em : worst_m;
      }
      // d is a minimum over t: first-order insensitive to the error of t
      const double ed = (double)fabsl((long double)d - dr);
      worst_d = ed > worst_d ? ed : worst_d;
      // a segment holds its ends: never farther from the centre than the nearer end
      const double ea = (s[0] - pa[0]) * (s[0] - pa[0]) + (s[1] - pa[1]) * (s[1] - pa[1]) + (s[2] - pa[2]) * (s[2] - pa[2]);
      const double eb = (s[0] - pb[0]) * (s[0] - pb[0]) + (s[1] - pb[1]) * (s[1] - pb[1]) + (s[2] - pb[2]) * (s[2] - pb[2]);
      CHECK(d <= (ea < eb ? ea : eb) + 1e-14);
      // t = 0 and t = 1 give the end's own offset, bit for bit
      if (t == 0.0) CHECK(m[0] == pa[0] - s[0] && m[1] == pa[1] - s[1] && m[2] == pa[2] - s[2]);
      if (t == 1.0) CHECK(m[0] == pb[0] - s[0] && m[1] == pb[1] - s[1] && m[2] == pb[2] - s[2]);
      const double R = std::sqrt(s[3]) + rho[l];
      zero += L2 == 0.0, clamp0 += L2 > 0 && t == 0.0, clamp1 += t == 1.0, inner += t > 0.0 && t < 1.0;
      active += R * R - d > 0.0;
    }
  }
  CHECK(zero > 0 && clamp0 > 100 && clamp1 > 100 && inner > 100 && active > 10);
  CHECK(worst_t < 1e-14 && worst_m < 1e-14 && worst_d < 1e-14);
  const double a[3] = {0.1, -0.2, 0.3}, b[3] = {0.7, 0.4, -0.1}, s[3] = {0.35, 0.2, 0.25};
  double t, m[3], d;
  anch_link_foot(a, b, s, t, m, d);
  std::printf("ok cells %d pairs %d zero %d end_a %d end_b %d interior %d active %d worst %.3g %.3g %.3g\n", CELLS,
              CELLS * n_link * n_obs, zero, clamp0, clamp1, inner, active, worst_t, worst_m, worst_d);
  std::printf("pinned t %a m %a %a %a d %a\n", t, m[0], m[1], m[2], d);
  std::printf("digest %016llx\n", (unsigned long long)dg.h);
  return 0;
}
