// tests/host/anch_screen_walk.cpp -- the screened restart seeds of gik_retry.hip.h as a host program: the candidate seed
// formula and the pick walked over a few hundred random slots on exactly sized heap arrays, the way retry_candidate_kernel
// and retry_pick_kernel index them (candidate-major, [C][count]), with the header's __host__ __device__ helpers.
// tests/test_anchored_screen_host.py compiles it (host only, with the address and undefined-behaviour sanitizers) and runs
// it; it prints "ok ...", a pinned candidate value and the picks of a clearance table that the numpy mirror redraws.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gik_retry.hip.h"

using namespace gik;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// the pick rule written out a second time, in two passes: the first clear candidate; else the first of the largest
static int pick_by_hand(const std::vector<double> &v, double clear_tol) {
  for (size_t c = 0; c < v.size(); ++c)
    if (v[c] >= -clear_tol) return (int)c;
  int best = -1;
  for (size_t c = 0; c < v.size(); ++c)
    if (v[c] == v[c] && (best < 0 || v[c] > v[(size_t)best])) best = (int)c;
  return best < 0 ? 0 : best;
}

int main() {
  const double inf = HUGE_VAL, nan = std::nan(""), tol = 1e-4;
  const double clears[8] = {inf, 0.05, 0.0, -1e-4, std::nextafter(-1e-4, -1.0), -0.036, nan, -inf};

  // ---- the rule on hand-made rows (the rows of the numpy test)
  {
    const double first_clear[] = {-0.2, 0.01, 0.5}, with_inf[] = {inf, 0.3}, none[] = {-0.3, -0.1, -0.2}, tie[] = {-0.2, -0.1, -0.1};
    const double mixed[] = {nan, -0.3, nan, -0.2}, nan_then_clear[] = {nan, 0.0}, all_nan[] = {nan, nan, nan};
    const double at_tol[] = {std::nextafter(-1e-4, -1.0), -1e-4}, minus_inf[] = {nan, -inf};
    CHECK(retry_pick(first_clear, 3, 1, tol) == 1);
    CHECK(retry_pick(with_inf, 2, 1, tol) == 0);
    CHECK(retry_pick(none, 3, 1, tol) == 1);
    CHECK(retry_pick(tie, 3, 1, tol) == 1);
    CHECK(retry_pick(mixed, 4, 1, tol) == 3);
    CHECK(retry_pick(nan_then_clear, 2, 1, tol) == 1);
    CHECK(retry_pick(all_nan, 3, 1, tol) == 0);
    CHECK(retry_pick(at_tol, 2, 1, tol) == 1);
    CHECK(retry_pick(minus_inf, 2, 1, tol) == 1);
    CHECK(retry_pick(none, 1, 1, tol) == 0);
    // a stride: column 1 of a [3][2] table
    const double table[] = {0.5, -0.3, 0.5, -0.1, 0.5, -0.2};
    CHECK(retry_pick(table + 1, 3, 2, tol) == 1 && retry_pick(table, 3, 2, tol) == 0);
  }
  CHECK(retry_candidate_seed(7, 0) == 7);
  CHECK(retry_candidate_seed(7, 1) == 7 + 0xD1342543DE82EF95ull);
  CHECK(retry_candidate_seed(0xFFFFFFFFFFFFFFFFull, 2) == 0xA2684A87BD05DF29ull);      // (2 * step - 1) mod 2^64

  // ---- the batch: B goals, a shuffled subset of them in the compact list
  const int B = 389, n = 6, pose_w = 16, attempt = 3, C = 5;
  const uint64_t seed = 0xDEADBEEFCAFEF00Dull;
  std::vector<double> T((size_t)B * pose_w), center((size_t)B * n);
  std::vector<int> scene_id(B), order(B);
  for (int b = 0; b < B; ++b) {
    for (int e = 0; e < pose_w; ++e) T[(size_t)b * pose_w + e] = 100.0 * b + e;
    for (int j = 0; j < n; ++j) center[(size_t)b * n + j] = -1.0 + 0.005 * b + 0.1 * j;
    scene_id[b] = b % 3;
    order[b] = b;
  }
  center[5 * n + 2] = nan;
  for (int b = B - 1; b > 0; --b) std::swap(order[b], order[next_u64() % (uint64_t)(b + 1)]);
  const int count = 301;
  std::vector<int> idx(order.begin(), order.begin() + count);
  idx.shrink_to_fit();
  const double lo[n] = {-3.0, -1.5, 0.25, -2.0, -1e-3, -6.0}, hi[n] = {3.0, 1.5, 0.25, 2.0, 1e-3, 6.0};

  for (double spread : {0.0, 0.3}) {
    // ---- retry_candidate_kernel's indexing, into arrays of exactly C * count rows
    const size_t M = (size_t)C * count;
    std::vector<double> T_out((size_t)count * pose_w), T_c(M * pose_w), q_c(M * n);
    std::vector<int> ids_c(M);
    for (int r = 0; r < count; ++r) {
      const int g = idx[r];
      for (int e = 0; e < pose_w; ++e) T_out[(size_t)r * pose_w + e] = T[(size_t)g * pose_w + e];
      for (int c = 0; c < C; ++c) {
        const size_t m = (size_t)c * count + r;
        const uint64_t seed_c = retry_candidate_seed(seed, c);
        for (int e = 0; e < pose_w; ++e) T_c[m * pose_w + e] = T[(size_t)g * pose_w + e];
        for (int j = 0; j < n; ++j) {
          const double u = retry_uniform(seed_c, (uint64_t)g, attempt, j);
          CHECK(u >= 0.0 && u < 1.0);
          const double ctr = spread > 0.0 ? center[(size_t)g * n + j] : 0.0;
          q_c[m * n + j] = retry_seed_value(u, lo[j], hi[j], ctr, spread);
        }
        ids_c[m] = scene_id[g];
      }
    }
    int differ = 0;
    for (int r = 0; r < count; ++r) {
      const int g = idx[r];
      for (int j = 0; j < n; ++j) {
        // candidate 0 is the unscreened seed, bit for bit
        const double today = retry_seed_value(retry_uniform(seed, (uint64_t)g, attempt, j), lo[j], hi[j],
                                              spread > 0.0 ? center[(size_t)g * n + j] : 0.0, spread);
        const double c0 = q_c[(size_t)r * n + j];
        CHECK((c0 == today) || (c0 != c0 && today != today));
        for (int c = 0; c < C; ++c) {
          const double v = q_c[((size_t)c * count + r) * n + j];
          if (v != v) {
            CHECK(spread > 0.0 && g == 5 && j == 2);      // the NaN centre: every candidate of that joint, no other
          } else {
            CHECK(v >= lo[j] && v <= hi[j]);
            differ += c > 0 && v != c0;
          }
        }
      }
      for (int c = 0; c < C; ++c) CHECK(ids_c[(size_t)c * count + r] == g % 3 && T_c[((size_t)c * count + r) * pose_w] == 100.0 * g);
    }
    CHECK(differ > count * (C - 1) * 3);      // (the joints with lo < hi draw other angles under another seed)

    // ---- retry_pick_kernel's indexing: clearances [C][count], the chosen row into [count][n]
    std::vector<double> cl(M), q_out((size_t)count * n), pick_cl(count);
    std::vector<int> pick(count);
    for (size_t m = 0; m < M; ++m) cl[m] = clears[next_u64() % 8];
    int hist[C] = {0};
    for (int r = 0; r < count; ++r) {
      const int c = retry_pick(cl.data() + r, C, (size_t)count, tol);
      CHECK(c >= 0 && c < C);
      const size_t m = (size_t)c * count + r;
      for (int j = 0; j < n; ++j) q_out[(size_t)r * n + j] = q_c[m * n + j];
      pick[r] = c;
      pick_cl[r] = cl[m];
      ++hist[c];
    }
    for (int r = 0; r < count; ++r) {
      std::vector<double> col(C);
      for (int c = 0; c < C; ++c) col[c] = cl[(size_t)c * count + r];
      CHECK(pick[r] == pick_by_hand(col, tol));
      const double v = pick_cl[r];
      bool any_clear = false, all_nan = true;
      for (double w : col) any_clear |= w >= -tol, all_nan &= w != w;
      if (any_clear) CHECK(v >= -tol);
      if (!any_clear && !all_nan)
        for (double w : col) CHECK(!(w > v));
      if (all_nan) CHECK(pick[r] == 0 && v != v);
      for (int c = 0; c < pick[r]; ++c) CHECK(!(col[c] >= -tol));      // nothing clear stands before the pick
    }
    for (int c = 0; c < C; ++c) CHECK(hist[c] > 0);
  }

  // ---- pinned: candidates of (seed 1, goal 0, attempt 1, joint 0) on [-1, 2], and the picks of a table the mirror redraws:
  // clearance of (slot r, candidate c) = clears[floor(8 u(99, r, c, 0))], 16 candidates, 257 slots
  const int PC = 16, PR = 257;
  std::vector<double> pcl((size_t)PC * PR);
  for (int c = 0; c < PC; ++c)
    for (int r = 0; r < PR; ++r) pcl[(size_t)c * PR + r] = clears[(int)(8.0 * retry_uniform(99, (uint64_t)r, c, 0))];
  long checksum = 0;
  int phist[PC] = {0};
  for (int r = 0; r < PR; ++r) {
    const int c = retry_pick(pcl.data() + r, PC, (size_t)PR, tol);
    checksum += (long)(r + 1) * c;
    ++phist[c];
  }
  std::printf("ok slots %d candidates %d\n", count, C);
  std::printf("pinned c0 %a c1 %a c15 %a\n", retry_seed_value(retry_uniform(retry_candidate_seed(1, 0), 0, 1, 0), -1.0, 2.0, 0.0, 0.0),
              retry_seed_value(retry_uniform(retry_candidate_seed(1, 1), 0, 1, 0), -1.0, 2.0, 0.0, 0.0),
              retry_seed_value(retry_uniform(retry_candidate_seed(1, 15), 0, 1, 0), -1.0, 2.0, 0.5, 0.1));
  std::printf("picks checksum %ld hist", checksum);
  for (int c = 0; c < PC; ++c) std::printf(" %d", phist[c]);
  std::printf("\n");
  return 0;
}
