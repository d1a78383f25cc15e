// tests/host/anch_link_walk.cpp -- the host side of the link clearance and its sweep (gik_anch_pairs.h) as a program
// of its own: anch_link_pair, anch_sweep_interp and anch_sweep_min walked over a few hundred random and degenerate cells
// on exactly sized heap arrays, against a long-double restatement.  tests/test_anchored_links_host.py compiles it (host
// only, with the address and undefined-behaviour sanitizers) and runs it; it prints "ok ...", two pinned values and the digest of every pair value of the random cells (walk_digest.h).
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
static long double pair_ref(const double *a, const double *b, const double *s, double rho) {
  long double d[3], u[3], L2 = 0, ud = 0;
  for (int c = 0; c < 3; ++c) {
    d[c] = (long double)b[c] - a[c];
    u[c] = (long double)s[c] - a[c];
    L2 += d[c] * d[c];
    ud += u[c] * d[c];
  }
  long double t = 0;
  if (L2 > 0) t = ud <= 0 ? 0 : (ud >= L2 ? 1 : ud / L2);
  long double v2 = 0;
  for (int c = 0; c < 3; ++c) v2 += (u[c] - t * d[c]) * (u[c] - t * d[c]);
  return sqrtl(v2) - sqrtl((long double)s[3]) - rho;
}

int main() {
  const double inf = HUGE_VAL, nan = std::nan("");
  const int CELLS = 400;
  // ---- hand-made cells: a link along x from 0 to 1, a sphere of radius 0.1 (s[3] = r^2)
  {
    const double a[3] = {0, 0, 0}, b[3] = {1, 0, 0}, r2 = 0.1 * 0.1, r = std::sqrt(r2);
    const double mid[4] = {0.5, 0.3, 0, r2}, before[4] = {-0.3, 0.4, 0, r2}, after[4] = {1.3, 0, 0.4, r2}, on[4] = {0.25, 0, 0, r2};
    CHECK(anch_link_pair(a, b, mid, 0.0) == 0.3 - r);            // interior
    CHECK(anch_link_pair(a, b, before, 0.0) == 0.5 - r);         // end a (a 3-4-5 triangle)
    CHECK(anch_link_pair(a, b, after, 0.0) == std::sqrt((1.3 - 1.0) * (1.3 - 1.0) + 0.4 * 0.4) - r);   // end b
    CHECK(anch_link_pair(a, b, on, 0.0) == -r);                  // the centre on the segment
    CHECK(anch_link_pair(a, a, before, 0.0) == 0.5 - r);         // a zero-length link is its point
    CHECK(anch_link_pair(a, b, mid, 0.03) == 0.3 - r - 0.03);    // the capsule radius subtracts
    const double bn[3] = {1, nan, 0}, an[3] = {nan, 0, 0};
    CHECK(std::isnan(anch_link_pair(a, bn, before, 0.0)));       // a NaN in b alone (t would be 0, v = u finite)
    CHECK(std::isnan(anch_link_pair(an, b, mid, 0.0)) && std::isnan(anch_link_pair(bn, bn, mid, 0.0)));
  }
  // ---- random and degenerate cells on exactly sized heap arrays, indexed as the kernel indexes them
  const int full_N = 7, n_link = 6, n_obs = 11;
  std::vector<double> Y((size_t)CELLS * full_N * 3), obs((size_t)n_obs * 4), rho(n_link), cl(CELLS);
  std::vector<int> la(n_link), lb(n_link);
  for (int l = 0; l < n_link; ++l) la[l] = l, lb[l] = l + 1, rho[l] = l % 2 ? 0.03 : 0.0;
  for (int o = 0; o < n_obs; ++o) {
    for (int c = 0; c < 3; ++c) obs[o * 4 + c] = uniform(-1.0, 1.0);
    const double r = uniform(0.05, 0.15);
    obs[o * 4 + 3] = r * r;
  }
  double worst = 0.0;
  WalkDigest dg;
  int clamp0 = 0, clamp1 = 0, inner = 0, zero = 0, negative = 0;
  for (int b = 0; b < CELLS; ++b) {
    double *y = Y.data() + (size_t)b * full_N * 3;
    for (int e = 0; e < full_N * 3; ++e) y[e] = uniform(-1.2, 1.2);
    if (b % 5 == 1)      // a zero-length link
      for (int c = 0; c < 3; ++c) y[3 * 3 + c] = y[2 * 3 + c];
    if (b % 5 == 2)      // a link through a centre
      for (int c = 0; c < 3; ++c) y[5 * 3 + c] = 2.0 * obs[(b % n_obs) * 4 + c] - y[4 * 3 + c];
    if (b % 5 == 3)      // a link of about a nanometre: t is the quotient of two tiny numbers
      for (int c = 0; c < 3; ++c) y[1 * 3 + c] = y[0 * 3 + c] + 1e-9 * (c + 1);
    double m = inf;
    bool any_nan = false;
    for (int p = 0; p < n_link * n_obs; ++p) {      // the kernel's pair loop, all lanes
      const int l = p / n_obs, o = p - l * n_obs;
      const double *pa = y + la[l] * 3, *pb = y + lb[l] * 3, *s = obs.data() + o * 4;
      const double v = anch_link_pair(pa, pb, s, rho[l]);
      dg.add(v);
      const long double ref = pair_ref(pa, pb, s, rho[l]);
      const double err = (double)fabsl((long double)v - ref);
      worst = err > worst ? err : worst;
      // a segment holds its ends: never farther from the sphere than the nearer end
      const double ea = std::sqrt((s[0] - pa[0]) * (s[0] - pa[0]) + (s[1] - pa[1]) * (s[1] - pa[1]) + (s[2] - pa[2]) * (s[2] - pa[2]));
      const double eb = std::sqrt((s[0] - pb[0]) * (s[0] - pb[0]) + (s[1] - pb[1]) * (s[1] - pb[1]) + (s[2] - pb[2]) * (s[2] - pb[2]));
      CHECK(v <= (ea < eb ? ea : eb) - std::sqrt(s[3]) - rho[l] + 1e-14);
      const double dx = pb[0] - pa[0], dy = pb[1] - pa[1], dz = pb[2] - pa[2], L2 = dx * dx + dy * dy + dz * dz;
      const double ud = (s[0] - pa[0]) * dx + (s[1] - pa[1]) * dy + (s[2] - pa[2]) * dz;
      zero += L2 == 0.0, clamp0 += L2 > 0 && ud <= 0, clamp1 += L2 > 0 && ud >= L2, inner += L2 > 0 && ud > 0 && ud < L2;
      any_nan |= v != v;
      m = v < m ? v : m;
    }
    CHECK(!any_nan);
    cl[b] = m;
    negative += m < 0;
  }
  CHECK(zero > 0 && clamp0 > 100 && clamp1 > 100 && inner > 100 && negative > 10);
  CHECK(worst < 1e-14);
  // ---- the sweep: interpolation ends are the ends, bit for bit, and the min over s keeps a NaN
  for (int S : {1, 2, 7, 8, 1000}) {
    for (int k = 0; k < 50; ++k) {
      const double qa = uniform(-3.2, 3.2), qb = uniform(-3.2, 3.2);
      CHECK(anch_sweep_interp(qa, qb, 0, S) == qa && anch_sweep_interp(qa, qb, S, S) == qb);
      for (int s = 0; s <= S; s += (S > 8 ? 37 : 1)) {
        const double q = anch_sweep_interp(qa, qb, s, S), w = (double)s / S;
        CHECK(q == (1.0 - w) * qa + w * qb);
        CHECK(q >= (qa < qb ? qa : qb) - 1e-15 && q <= (qa < qb ? qb : qa) + 1e-15);
      }
    }
  }
  {
    const int B = 65, S = 7;
    std::vector<double> c((size_t)(S + 1) * B), out(B);      // [S+1][B], sample-major
    for (size_t i = 0; i < c.size(); ++i) c[i] = uniform(-0.2, 0.5);
    c[(size_t)3 * B + 17] = nan;
    c[(size_t)S * B + 64] = -7.0;      // the last sample of the last goal: the far corner of the array
    c[(size_t)2 * B + 5] = inf;
    for (int b = 0; b < B; ++b) out[b] = anch_sweep_min(c.data() + b, S + 1, (size_t)B);
    for (int b = 0; b < B; ++b) {
      if (b == 17) { CHECK(std::isnan(out[b])); continue; }
      double m = inf;
      for (int s = 0; s <= S; ++s) m = c[(size_t)s * B + b] < m ? c[(size_t)s * B + b] : m;
      CHECK(out[b] == m);
    }
    CHECK(out[64] == -7.0);
    const double all_inf[3] = {inf, inf, inf};
    CHECK(anch_sweep_min(all_inf, 3, 1) == inf);
  }
  const double a[3] = {0.1, -0.2, 0.3}, b[3] = {0.7, 0.4, -0.1}, s[4] = {0.35, 0.2, 0.25, 0.01};
  std::printf("ok cells %d pairs %d zero %d end_a %d end_b %d interior %d colliding %d worst %.3g\n", CELLS,
              CELLS * n_link * n_obs, zero, clamp0, clamp1, inner, negative, worst);
  std::printf("pinned pair %a interp %a\n", anch_link_pair(a, b, s, 0.03), anch_sweep_interp(0.3, -1.7, 3, 7));
  std::printf("digest %016llx\n", (unsigned long long)dg.h);
  return 0;
}
