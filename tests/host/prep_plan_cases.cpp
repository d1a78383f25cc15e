// tests/host/prep_plan_cases.cpp -- plan_prepare (graphik_amd/csrc/gik_plan.h) on the facts of the boundary cases of
// tests/synth_prepare.py: which of the six prepare kernels each graph runs.  Arguments: the static LDS bytes of
// prep_block_kernel<true> (the test adds up the kernel's __shared__ arrays), then per case
//   id N K n_anchor env_no_quad env_no_compress env_a_global
// The stand-in occupancy answers 1 for the LDS variant exactly when its N x N work matrix fits next to those static
// bytes in the 160 KB of a CU.  Prints JSON rows; tests/test_prepare_boundaries_host.py reads them.
#include "gik_plan.h"

#include <cstdio>
#include <cstdlib>

using gik::Prep;
using gik::PrepFacts;
using gik::PrepPlan;

int main(int argc, char **argv) {
  static const char *name[] = {"quad13", "quad", "wave", "block_lds", "block", "block_big"};
  if (argc < 2 || (argc - 2) % 7) return 2;
  const size_t static_lds = (size_t)std::atol(argv[1]);
  const char *sep = "";
  std::printf("[");
  for (int at = 2; at < argc; at += 7) {
    PrepFacts f;
    f.N = std::atoi(argv[at + 1]);
    f.K = std::atoi(argv[at + 2]);
    f.n_anchor = std::atoi(argv[at + 3]);
    f.n_ee = 1;
    f.env_no_quad = std::atoi(argv[at + 4]) != 0;
    f.env_no_compress = std::atoi(argv[at + 5]) != 0;
    f.env_a_global = std::atoi(argv[at + 6]) != 0;
    f.n_cu = 256;
    const PrepPlan p = gik::plan_prepare(f, [&](Prep v, int, size_t lds) {
      if (v == Prep::BLOCK_LDS) return lds + static_lds <= (size_t)160 * 1024 ? 1 : 0;
      return v == Prep::WAVE ? 12 : (v <= Prep::QUAD ? 8 : 2);
    });
    std::printf("%s\n {\"id\": \"%s\", \"N\": %d, \"variant\": \"%s\", \"lds\": %zu, \"wpc\": %d, \"no_compress\": %d, \"slab_matrices\": %d, "
                "\"grid_b8\": %d}",
                sep, argv[at], f.N, name[(int)p.variant], p.lds, p.wpc, (int)p.no_compress,
                p.block() ? (int)(p.slab_bytes / (sizeof(double) * (size_t)f.N * f.N * f.n_cu * p.wpc)) : 0, p.launch_grid(8));
    sep = ",";
  }
  std::printf("\n]\n");
  return 0;
}
