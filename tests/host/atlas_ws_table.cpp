// tests/host/atlas_ws_table.cpp -- anch_atlas_ws (graphik_amd/csrc/gik_plan.h) tabulated: the byte offset of every array of
// the workspace of gik_anchored_ik_batch_atlas over a null base (where a pointer is its offset) -- the neighbour table, the
// attempt-0 seeds, the noted rows and the screened step's arrays behind them --, with the bytes of the anchored restart
// workspace it lies behind, without and with a scene entry's ids.  Prints JSON; tests/test_anchored_atlas_ws.py compares
// it with the closed form of the layout comment.
#include "gik_plan.h"

#include <cstdio>

static size_t at(const void *p) { return (size_t) reinterpret_cast<uintptr_t>(p); }

int main() {
  // n_joints, pose_w, T_base, N_base, N_free, n_goal, full_N: UR10 + table, KUKA-like odd everything
  const int sizes[][7] = {{6, 16, 78, 22, 14, 2, 22}, {7, 16, 101, 29, 23, 3, 29}};
  const int kB[] = {0, 1, 2, 3, 5, 64, 4096};
  const int kC[] = {1, 2, 3, 4, 16};
  const int kR[] = {0, 1, 3, 63};
  std::printf("{\"fields\": [\"n\", \"pose_w\", \"base_T\", \"base_N\", \"free_N\", \"n_goal\", \"full_N\", \"B\", \"C\", \"retries\", "
              "\"scenes\", \"head\", \"nbr\", \"q0\", \"rows\", \"screen_head\", \"q\", \"poses\", \"targets\", \"Y\", \"clearance\", "
              "\"ids\", \"pick\", \"bytes\", \"retry_bytes\", \"retry_ids\", \"screened_bytes\"],\n\"rows\": [");
  const char *sep = "";
  for (const auto &s : sizes)
    for (int B : kB)
      for (int C : kC)
        for (int R : kR) {
          if ((R + 1) * C > 64) continue;      // (K is refused beyond a wavefront's lanes)
          for (int scenes = 0; scenes < 2; ++scenes) {
            const gik::AnchRetryWs r = gik::anch_retry_ws(s[0], s[1], s[2], s[3], s[4], s[5], s[6], B, nullptr);
            const size_t head = gik::anch_screen_head(s[0], s[1], s[2], s[3], s[4], s[5], s[6], B);
            const gik::AnchAtlasWs a = gik::anch_atlas_ws(s[0], s[1], s[2], s[6], B, C, R, head, nullptr);
            const gik::AnchScreenWs w = gik::anch_screen_ws(s[0], s[1], s[2], s[6], B, C, a.screen_head, nullptr);
            const gik::AnchScreenWs old = gik::anch_screen_ws(s[0], s[1], s[2], s[6], B, C, head, nullptr);
            std::printf("%s\n [", sep);
            for (int v : s) std::printf("%d, ", v);
            std::printf("%d, %d, %d, %d, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu]", B, C, R, scenes,
                        head, at(a.nbr), at(a.q0), at(a.rows), a.screen_head, at(w.q), at(w.T), at(w.targets), at(w.Y), at(w.cl),
                        at(w.ids), at(w.pick), a.bytes, r.bytes, at(r.ids), old.bytes);
            sep = ",";
          }
        }
  std::printf("\n]}\n");
  return 0;
}
