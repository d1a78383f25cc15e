// tests/host/prep_plan_position.cpp -- plan_prepare (graphik_amd/csrc/gik_plan.h) on templates with inert goal slots: the
// four-goals-per-wavefront prepare kernel stays where every inert slot is the odd slot of a position goal
// (PrepFacts::position_goals), and prep_wave_kernel where a slot is inert for the old reason.  Prints JSON rows;
// tests/test_position_goals_host.py reads them.
#include "gik_plan.h"

#include <cstdio>

using gik::Prep;
using gik::PrepFacts;
using gik::PrepPlan;

int main() {
  static const char *name[] = {"quad13", "quad", "wave", "block_lds", "block", "block_big"};
  const char *sep = "";
  std::printf("[");
  for (int N : {13, 16, 17})
    for (int inert : {0, 1})
      for (int position : {0, 1})
        for (int no_quad : {0, 1}) {
          if (position && !inert) continue;      // (position_goals says something about the inert slots)
          PrepFacts f;
          f.N = N;
          f.K = N == 16 ? 3 : 2;      // planar-10 and a 17-node planar chain; UR10
          f.n_anchor = N == 16 ? 4 : 3;
          f.n_ee = 1;
          f.inert_goal_slot = inert != 0;
          f.position_goals = position != 0;
          f.env_no_quad = no_quad != 0;
          f.n_cu = 256;
          const PrepPlan p = gik::plan_prepare(f, [](Prep v, int, size_t) { return v == Prep::WAVE ? 12 : 8; });
          std::printf("%s\n {\"N\": %d, \"inert\": %d, \"position\": %d, \"no_quad\": %d, \"variant\": \"%s\", \"lds\": %zu, \"wpc\": %d, "
                      "\"wave_lds\": %zu, \"wave_wpc\": %d}",
                      sep, N, inert, position, no_quad, name[(int)p.variant], p.lds, p.wpc, p.wave_lds, p.wave_wpc);
          sep = ",";
        }
  std::printf("\n]\n");
  return 0;
}
