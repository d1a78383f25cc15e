// tests/host/screen_ws_table.cpp -- anch_screen_ws and anch_screen_head (graphik_amd/csrc/gik_plan.h) tabulated: the byte
// offset of every array of the screened restart seeds' workspace over a null base (where a pointer is its offset), alone
// (head 0: gik_anchored_retry_seeds_screened) and behind the anchored restart workspace (gik_anchored_ik_batch_retry_screened),
// with the bytes of anch_retry_ws beside it.  Prints JSON; tests/test_anchored_screen_host.py compares it with the closed
// form of the layout comment.
#include "gik_plan.h"

#include <cstdio>

static size_t at(const void *p) { return (size_t) reinterpret_cast<uintptr_t>(p); }

int main() {
  // n_joints, pose_w, T_base, N_base, N_free, n_goal, full_N: UR10 + table, no goal anchors, odd everything
  const int sizes[][7] = {{6, 16, 78, 22, 14, 2, 22}, {6, 16, 78, 22, 14, 0, 22}, {7, 16, 101, 29, 23, 3, 29}};
  const int kB[] = {0, 1, 2, 3, 5, 64};
  const int kC[] = {1, 2, 3, 8, 16};
  std::printf("{\"fields\": [\"n\", \"pose_w\", \"base_T\", \"base_N\", \"free_N\", \"n_goal\", \"full_N\", \"B\", \"C\", \"loop\", "
              "\"head\", \"q\", \"poses\", \"targets\", \"Y\", \"clearance\", \"ids\", \"pick\", \"bytes\", \"retry_bytes\", \"retry_ids\"],\n"
              "\"rows\": [");
  const char *sep = "";
  for (const auto &s : sizes)
    for (int B : kB)
      for (int C : kC)
        for (int loop = 0; loop < 2; ++loop) {
          const gik::AnchRetryWs r = gik::anch_retry_ws(s[0], s[1], s[2], s[3], s[4], s[5], s[6], B, nullptr);
          const size_t head = loop ? gik::anch_screen_head(s[0], s[1], s[2], s[3], s[4], s[5], s[6], B) : 0;
          const gik::AnchScreenWs w = gik::anch_screen_ws(s[0], s[1], s[2], s[6], B, C, head, nullptr);
          std::printf("%s\n [", sep);
          for (int v : s) std::printf("%d, ", v);
          std::printf("%d, %d, %d, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu]", B, C, loop, head, at(w.q), at(w.T),
                      at(w.targets), at(w.Y), at(w.cl), at(w.ids), at(w.pick), w.bytes, r.bytes, at(r.ids));
          sep = ",";
        }
  std::printf("\n]}\n");
  return 0;
}
