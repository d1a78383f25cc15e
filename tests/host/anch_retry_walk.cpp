// tests/host/anch_retry_walk.cpp -- the host side of gik_retry.hip.h as a program of its own: select, seed and
// merge walked over a few hundred random slots on exactly sized heap arrays with the header's __host__ __device__
// helpers, the way the three kernels index them, with a clearance; then the same helpers without one (clearance = +inf)
// held to the plain rule, written out here, on every cell.  tests/test_anchored_retry_host.py compiles it (host only, with
// the address and undefined-behaviour sanitizers) and runs it; it prints "ok ...", the pinned local-mode seed value and
// the number of cells of the plain walk.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gik_retry.hip.h"

using namespace gik;

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t next_u64() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
template <typename T, size_t N>
static T pick(const T (&v)[N]) { return v[next_u64() % N]; }

// the rule of the restarts without a clearance, written out: what the unified helpers must give at clearance = +inf
static bool plain_failed(int stop, double p, double r, double pt, double rt) { return stop != 0 || !(p <= pt) || !(r <= rt); }
static double plain_score(double p, double r, double pt, double rt) {
  const double a = p / pt, b = r / rt;
  if (a != a || b != b) return HUGE_VAL;
  return a > b ? a : b;
}
static bool plain_better(int stop_r, double p_r, double r_r, int stop_i, double p_i, double r_i, double pt, double rt) {
  const bool ok_r = !plain_failed(stop_r, p_r, r_r, pt, rt), ok_i = !plain_failed(stop_i, p_i, r_i, pt, rt);
  return (ok_r && !ok_i) || (ok_r == ok_i && plain_score(p_r, r_r, pt, rt) < plain_score(p_i, r_i, pt, rt));
}

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main() {
  const double inf = HUGE_VAL, nan = std::nan("");
  const RetryTol tol = {0.01, 0.01, 1e-4};
  const int B = 389, n = 6, pose_w = 16, row = 7 * 3, attempt_no = 3;
  const uint64_t seed = 0xDEADBEEFCAFEF00Dull;
  const int stops[] = {0, 0, 0, 1, 2};
  const double errs[] = {0.002, 0.005, 0.01, 0.02, 0.05, nan};
  const double clears[] = {inf, 0.05, 0.0, -1e-4, std::nextafter(-1e-4, -1.0), -0.036, nan, -inf};

  // ---- the rule on hand-made cells
  CHECK(!retry_failed(0, 0.0, 0.0, -1e-4, tol));
  CHECK(retry_failed(0, 0.0, 0.0, std::nextafter(-1e-4, -1.0), tol));
  CHECK(retry_failed(0, 0.0, 0.0, nan, tol));
  CHECK(!retry_failed(0, 0.0, 0.0, inf, tol));
  CHECK(retry_failed(0, 1e-6, 1e-6, -0.036, tol));
  CHECK(retry_score(0.001, 0.001, -0.036, tol) == 0.036 / 1e-4);
  CHECK(retry_score(0.001, 0.002, inf, tol) == 0.002 / 0.01);
  CHECK(retry_score(0.001, 0.002, nan, tol) == inf);
  CHECK(!retry_better(0, 0.0, 0.0, nan, 1, 1.0, 1.0, -1.0, tol));          // a NaN never wins
  CHECK(!retry_better(1, 0.02, 0.0, 0.1, 1, 0.02, 0.0, 0.1, tol));         // a tie keeps the incumbent
  CHECK(retry_better(1, 0.02, 0.0, 0.1, 1, 0.03, 0.0, 0.1, tol));
  CHECK(retry_better(0, 0.009, 0.0, 0.1, 0, 0.001, 0.0, -0.036, tol));     // failure by clearance alone loses

  // ---- the batch: incumbents [B]
  std::vector<gik_stats> stats(B);
  std::vector<double> pos(B), rot(B), clr(B), Y((size_t)B * row), q((size_t)B * n), T((size_t)B * pose_w), center((size_t)B * n);
  std::vector<int> attempt(B, 0);
  std::memset(stats.data(), 0, sizeof(gik_stats) * B);
  for (int b = 0; b < B; ++b) {
    stats[b].stop = pick(stops);
    stats[b].iterations = b;
    pos[b] = pick(errs), rot[b] = pick(errs), clr[b] = pick(clears);
    for (int e = 0; e < row; ++e) Y[(size_t)b * row + e] = b + 0.001 * e;
    for (int j = 0; j < n; ++j) q[(size_t)b * n + j] = -b - j, center[(size_t)b * n + j] = -1.0 + 0.005 * b + 0.1 * j;
    for (int e = 0; e < pose_w; ++e) T[(size_t)b * pose_w + e] = 100.0 * b + e;
  }
  center[5 * n + 2] = nan;

  // ---- select (retry_select_kernel: wavefronts of 64 goals, each appends its failed ones)
  std::vector<int> idx;
  for (int w = (B + RETRY_WAVE - 1) / RETRY_WAVE - 1; w >= 0; --w)      // (the order of the list is unspecified: back to front)
    for (int lane = 0; lane < RETRY_WAVE; ++lane) {
      const int b = w * RETRY_WAVE + lane;
      if (b < B && retry_failed(stats[b].stop, pos[b], rot[b], clr[b], tol)) idx.push_back(b);
    }
  const int count = (int)idx.size();
  CHECK(count > B / 4 && count < B);
  idx.shrink_to_fit();

  // ---- seeds (retry_seed_kernel), uniform and local, into arrays of exactly count rows
  const double lo[n] = {-3.0, -1.5, 0.25, -2.0, -1e-3, -6.0}, hi[n] = {3.0, 1.5, 0.25, 2.0, 1e-3, 6.0};
  const double spread = 0.3;
  std::vector<double> T_out((size_t)count * pose_w), q_uni((size_t)count * n), q_loc((size_t)count * n);
  for (int r = 0; r < count; ++r) {
    const int g = idx[r];
    for (int e = 0; e < pose_w; ++e) T_out[(size_t)r * pose_w + e] = T[(size_t)g * pose_w + e];
    for (int j = 0; j < n; ++j) {
      const double u = retry_uniform(seed, (uint64_t)g, attempt_no, j);
      CHECK(u >= 0.0 && u < 1.0);
      const double c = center[(size_t)g * n + j];
      const double a = retry_seed_value(u, lo[j], hi[j], 0.0, 0.0), l = retry_seed_value(u, lo[j], hi[j], c, spread);
      CHECK(a == lo[j] + u * (hi[j] - lo[j]) && a >= lo[j] && a <= hi[j]);
      if (c != c) {
        CHECK(l != l);
      } else {
        CHECK(l >= lo[j] && l <= hi[j]);
        CHECK((l >= c - spread && l <= c + spread) || l == lo[j] || l == hi[j]);
      }
      q_uni[(size_t)r * n + j] = a, q_loc[(size_t)r * n + j] = l;
    }
    CHECK(T_out[(size_t)r * pose_w] == 100.0 * g);
  }

  // ---- merge (retry_merge_kernel): restart answers [count], better ones replace the incumbent's every part
  std::vector<gik_stats> stats_r(count);
  std::vector<double> pos_r(count), rot_r(count), clr_r(count), Y_r((size_t)count * row);
  std::memset(stats_r.data(), 0, sizeof(gik_stats) * count);
  for (int r = 0; r < count; ++r) {
    stats_r[r].stop = pick(stops);
    stats_r[r].iterations = 100000 + r;
    pos_r[r] = pick(errs), rot_r[r] = pick(errs), clr_r[r] = pick(clears);
    for (int e = 0; e < row; ++e) Y_r[(size_t)r * row + e] = -1000.0 - r;
  }
  const std::vector<gik_stats> stats0 = stats;
  const std::vector<double> pos0 = pos, rot0 = rot, clr0 = clr, Y0 = Y, q0 = q;
  int replaced = 0, rescued = 0;
  for (int r = 0; r < count; ++r) {
    const int g = idx[r];
    if (!retry_better(stats_r[r].stop, pos_r[r], rot_r[r], clr_r[r], stats[g].stop, pos[g], rot[g], clr[g], tol)) continue;
    for (int e = 0; e < row; ++e) Y[(size_t)g * row + e] = Y_r[(size_t)r * row + e];
    for (int j = 0; j < n; ++j) q[(size_t)g * n + j] = q_loc[(size_t)r * n + j];
    std::memcpy(&stats[g], &stats_r[r], sizeof(gik_stats));
    pos[g] = pos_r[r], rot[g] = rot_r[r], clr[g] = clr_r[r], attempt[g] = attempt_no;
    ++replaced;
  }
  for (int b = 0; b < B; ++b) {
    const bool was_ok = !retry_failed(stats0[b].stop, pos0[b], rot0[b], clr0[b], tol);
    const bool is_ok = !retry_failed(stats[b].stop, pos[b], rot[b], clr[b], tol);
    CHECK(!(was_ok && !is_ok));                        // no success is lost
    CHECK(!(was_ok && attempt[b] != 0));               // a goal that had succeeded was not in the list
    rescued += !was_ok && is_ok;
    if (attempt[b] == 0) {
      CHECK(std::memcmp(&stats[b], &stats0[b], sizeof(gik_stats)) == 0 && Y[(size_t)b * row] == Y0[(size_t)b * row] &&
            q[(size_t)b * n] == q0[(size_t)b * n]);
    } else {
      CHECK(stats[b].iterations >= 100000 && Y[(size_t)b * row + row - 1] <= -1000.0);
      CHECK(clr[b] == clr[b] && pos[b] == pos[b] && rot[b] == rot[b]);      // a NaN never wins
      CHECK(!retry_better(stats0[b].stop, pos0[b], rot0[b], clr0[b], stats[b].stop, pos[b], rot[b], clr[b], tol));
    }
  }
  CHECK(replaced > 0 && rescued > 0 && replaced < count);

  // ---- no clearance: at +inf the helpers are the plain rule, on the full cross product restart answer x incumbent,
  // and spread 0 is lo + u (hi - lo) on the limit table
  int cells = 0;
  for (int sr : stops)
    for (double pr : errs)
      for (double rr : errs) {
        CHECK(retry_failed(sr, pr, rr, inf, tol) == plain_failed(sr, pr, rr, tol.pos_tol, tol.rot_tol));
        const double want = plain_score(pr, rr, tol.pos_tol, tol.rot_tol);
        CHECK(want == want && retry_score(pr, rr, inf, tol) == want);
        for (int si : stops)
          for (double pi : errs)
            for (double ri : errs) {
              CHECK(retry_better(sr, pr, rr, inf, si, pi, ri, inf, tol) ==
                    plain_better(sr, pr, rr, si, pi, ri, tol.pos_tol, tol.rot_tol));
              ++cells;
            }
      }
  for (int j = 0; j < n; ++j)
    for (int g = 0; g < B; ++g) {
      const double uj = retry_uniform(seed, (uint64_t)g, attempt_no, j);
      CHECK(retry_seed_value(uj, lo[j], hi[j], 0.0, 0.0) == lo[j] + uj * (hi[j] - lo[j]));
    }

  // ---- the pinned local-mode value: seed 1, goal 0, attempt 1, joint 0; centre 0.5, spread 0.1 on [-1, 2]
  const double u = retry_uniform(1, 0, 1, 0);
  std::printf("ok slots %d failed %d replaced %d rescued %d\n", B, count, replaced, rescued);
  std::printf("pinned u %a local %a clipped %a\n", u, retry_seed_value(u, -1.0, 2.0, 0.5, 0.1),
              retry_seed_value(u, -1.0, 2.0, -1.0, 0.1));
  std::printf("plain cells %d\n", cells);
  return 0;
}
