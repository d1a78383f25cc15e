// tests/host/claim_order_plan.cpp -- the claim-order part of the launch plan (graphik_amd/csrc/gik_plan.h), without a
// device: when a batch call orders its claims, where the key and order buffers sit in the leased workspace, that a
// template without a key is planned exactly as before, and which keys gik_template_set_claim_key refuses
// (claim_key_ok).  tests/test_claim_order_host.py builds it plain and with the address + undefined-behaviour sanitizers.
#include "gik_plan.h"

#include <cstdio>
#include <cstring>
#include <vector>

using gik::SolveFacts;
using gik::SolvePlan;

static int failures = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++failures;                                                       \
    }                                                                   \
  } while (0)

static SolveFacts arm(int n_cu, int wpc, bool spread, int claim_terms) {
  SolveFacts f;
  f.K = 3;
  f.n_cu = n_cu;
  f.waves_per_cu = wpc;
  f.has_spread = spread;
  f.maxiter = 3000;
  f.wave_slice_its = 256;
  f.claim_terms = claim_terms;
  return f;
}

// the byte ranges a plan hands out do not overlap and lie inside `bytes`
static void check_layout(const SolvePlan &p, int B) {
  CHECK(p.needs_ws);
  CHECK(p.off_key % 64 == 0 && p.off_order % 4 == 0);
  CHECK(p.off_order == p.off_key + 4 * (size_t)B);
  CHECK(p.bytes == p.off_order + 4 * (size_t)B);
  CHECK(p.off_key >= p.off_ctg + p.ctg_bytes);
  CHECK(p.off_key >= p.off_yids + 4 * p.ycap);
  CHECK(p.zero_head <= p.off_seq && p.off_seq <= p.off_key);
}

int main() {
  const int MAXB = gik::PLAN_CLAIM_ORDER_MAX_BATCH;
  // 1. the rule by batch size: more problems than resident waves, at most PLAN_CLAIM_ORDER_MAX_BATCH
  for (int n_cu : {8, 256})
    for (int wpc : {4, 8, 12})
      for (int spread : {0, 1}) {
        const SolveFacts on = arm(n_cu, wpc, spread, 1), off = arm(n_cu, wpc, spread, 0);
        std::vector<long long> bs = {1, 2, 63, 4LL * n_cu - 1, 4LL * n_cu, 4LL * n_cu + 1, 24LL * n_cu, 24LL * n_cu + 1,
                                     (long long)wpc * n_cu, (long long)wpc * n_cu + 1, 128LL * n_cu, MAXB - 1, MAXB, MAXB + 1,
                                     4LL * MAXB};
        for (long long b : bs) {
          const int B = (int)b;
          const SolvePlan p = gik::plan_solve(on, B), q = gik::plan_solve(off, B);
          CHECK(!q.order);
          CHECK(p.order == (B > p.grid && B <= MAXB));
          // the key changes nothing else of the plan
          CHECK(p.launch == q.launch && p.grid == q.grid && p.launch_grid == q.launch_grid && p.wpc == q.wpc);
          CHECK(p.slice_its == q.slice_its && p.slice_cycles == q.slice_cycles && p.mig == q.mig && p.cap == q.cap && p.ycap == q.ycap);
          if (q.needs_ws) {
            CHECK(p.off_simd == q.off_simd && p.off_seq == q.off_seq && p.off_ids == q.off_ids && p.off_state == q.off_state);
            CHECK(p.off_yseq == q.off_yseq && p.off_yids == q.off_yids && p.off_ctg == q.off_ctg && p.zero_head == q.zero_head);
            CHECK(p.seq_fill == q.seq_fill && p.state_zero == q.state_zero && p.yseq_zero == q.yseq_zero);
          }
          if (p.order) {
            check_layout(p, B);
            // lease sizing: what the queues need, padded to 64 bytes, plus B floats and B ints
            const size_t before = q.needs_ws ? q.bytes : p.off_ctg;
            CHECK(p.bytes == ((before + 63) & ~(size_t)63) + 8 * (size_t)B);
            if (!q.needs_ws) CHECK(p.zero_head == 0 && p.seq_fill == 0 && p.state_zero == 0 && p.yseq_zero == 0);
          } else {
            CHECK(p.needs_ws == q.needs_ws);
            if (p.needs_ws) CHECK(p.bytes == q.bytes);
          }
        }
      }
  // the headline: 4096 goals on 256 CUs run one wave per SIMD and order; 1024 goals have a wave each and do not
  CHECK(gik::plan_solve(arm(256, 8, true, 1), 4096).order && gik::plan_solve(arm(256, 8, true, 1), 4096).grid == 1024);
  CHECK(!gik::plan_solve(arm(256, 8, true, 1), 1024).order);
  // 2. only the 3-D trust-region wavefront kernels
  {
    SolveFacts f = arm(8, 8, true, 1);
    f.cg = true;
    CHECK(!gik::plan_solve(f, 4096).order);
    f = arm(8, 8, true, 1);
    f.is_block = true;
    CHECK(!gik::plan_solve(f, 4096).order);
    f.is_npt = true;
    f.ctg_doubles = 5050;
    CHECK(!gik::plan_solve(f, 4096).order);
    f = arm(8, 8, false, 1);
    f.K = 2;
    CHECK(!gik::plan_solve(f, 4096).order);
    f = arm(8, 8, true, 1);
    f.dbg = 1;      // the static block -> problem map goes through the table too
    CHECK(gik::plan_solve(f, 4096).order);
  }
  // 3. keys that are refused: more than 8 terms, a negative count, an index outside [0, T), no term list
  {
    const int T = 40;
    int ok[8] = {0, 39, 5, 5, 1, 2, 3, 4}, nine[9] = {0, 1, 2, 3, 4, 5, 6, 7, 8}, high[2] = {3, 40}, neg[1] = {-1};
    CHECK(gik::claim_key_ok(0, nullptr, T));
    CHECK(gik::claim_key_ok(1, ok, T) && gik::claim_key_ok(8, ok, T));
    CHECK(!gik::claim_key_ok(9, nine, T) && !gik::claim_key_ok(-1, ok, T));
    CHECK(!gik::claim_key_ok(2, high, T) && gik::claim_key_ok(1, high, T) && !gik::claim_key_ok(1, neg, T));
    CHECK(!gik::claim_key_ok(1, nullptr, T));
    CHECK(!gik::claim_key_ok(1, ok, 0));
    CHECK(gik::PLAN_CLAIM_KEY_MAX_TERMS == 8);
  }
  std::printf("claim_order_plan: %d failures\n", failures);
  return failures ? 1 : 0;
}
