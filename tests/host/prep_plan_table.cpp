// tests/host/prep_plan_table.cpp -- plan_prepare and anch_ws (graphik_amd/csrc/gik_plan.h) tabulated: the prepare variant of
// a template, its LDS bytes, waves per CU, slab and grids over the facts of every variant, stand-in occupancy answers and
// the batch sizes around every grid; then the layout of the anchored scratch.  Prints JSON; tests/test_prep_plan.py
// compares it field by field with tests/golden/prep_plan.json (docs/NOTEBOOK.md 27).
#include "gik_plan.h"

#include <cstdio>
#include <set>
#include <string>
#include <vector>

using gik::Prep;
using gik::PrepFacts;
using gik::PrepPlan;

static const char *kName[] = {"quad13", "quad", "wave", "block_lds", "block", "block_big"};

// occupancy answers by variant, -1 = the query failed; what attach would get from the device
struct Answers {
  int occ[6] = {8, 8, 12, 1, 2, 1};
};

static void emit_case(const std::string &name, const PrepFacts &f, const Answers &an) {
  static bool first = true;
  std::string queries;
  const PrepPlan p = gik::plan_prepare(f, [&](Prep v, int threads, size_t lds) {
    char s[96];
    std::snprintf(s, sizeof s, "%s[\"%s\", %d, %zu]", queries.empty() ? "" : ", ", kName[(int)v], threads, lds);
    queries += s;
    return an.occ[(int)v];
  });
  const PrepPlan d = p.diagnostics();
  std::printf("%s\n {\"case\": \"%s\", \"queries\": [%s], \"plan\": [\"%s\", %d, %zu, %d, %zu, %d, \"%s\", %d, %zu, %d], \"rows\": [",
              first ? "" : ",", name.c_str(), queries.c_str(), kName[(int)p.variant], p.threads(), p.lds, p.wpc, p.slab_bytes,
              (int)p.no_compress, kName[(int)d.variant], d.threads(), d.lds, d.wpc);
  first = false;
  // B = 1 and one below, at and one above every grid: the variant's (the quad kernel: four goals per wavefront) and
  // that of the launch with diagnostics
  std::set<long long> bs = {1};
  for (long long g : {(long long)f.n_cu * p.wpc, 4LL * f.n_cu * p.wpc, (long long)f.n_cu * d.wpc})
    for (long long b = g - 1; b <= g + 1; ++b)
      if (b >= 1) bs.insert(b);
  const char *sep = "";
  for (long long b : bs) {
    std::printf("%s[%lld, %d, %d]", sep, b, p.launch_grid((int)b), d.launch_grid((int)b));
    sep = ", ";
  }
  std::printf("]}");
}

static std::string tag(const PrepFacts &f, const Answers &an) {
  char s[320];
  std::snprintf(s, sizeof s, "N%d K%d na%d ee%d gg%d inert%d force%d envblock%d nocompress%d aglobal%d noquad%d waves%s%d cu%d occ %d %d %d %d %d %d",
                f.N, f.K, f.n_anchor, f.n_ee, f.n_gg, (int)f.inert_goal_slot, (int)f.force_block_prepare, (int)f.env_force_block,
                (int)f.env_no_compress, (int)f.env_a_global, (int)f.env_no_quad, f.env_waves_set ? "=" : "-", f.env_waves, f.n_cu,
                an.occ[0], an.occ[1], an.occ[2], an.occ[3], an.occ[4], an.occ[5]);
  return s;
}
static void emit(const PrepFacts &f, const Answers &an = Answers()) { emit_case(tag(f, an), f, an); }

static PrepFacts facts(int N, int K, int n_anchor, int n_ee, bool inert, int n_cu) {
  PrepFacts f;
  f.N = N;
  f.K = K;
  f.n_anchor = n_anchor;
  f.n_ee = n_ee;
  f.n_gg = n_ee > 1 ? 3 : 0;
  f.inert_goal_slot = inert;
  f.n_cu = n_cu;
  return f;
}

// every graph size against every anchor count: what gik_pipeline_attach accepts (at most 528 anchor-goal pairs, 2-D up to
// 128 nodes, an inert slot only among several end effectors)
static void sizes(int n_cu) {
  for (int N : {2, 13, 16, 17, 32, 33, 48, 123, 124, 128, 129, 255})
    for (int na : {1, 32, 33, 256})
      for (int K : {2, 3})
        for (int n_ee : {1, 8})
          for (int inert : {0, 1}) {
            const PrepFacts f = facts(N, K, na, n_ee, inert != 0, n_cu);
            if (2 * n_ee * na + f.n_gg > 528 || (N > 128 && K != 3) || (inert && n_ee == 1)) continue;
            emit(f);
          }
}

// one knob at a time on a graph of every variant
static void knobs(int n_cu) {
  const PrepFacts reps[] = {facts(13, 2, 1, 1, false, n_cu),  facts(16, 2, 2, 8, false, n_cu),  facts(17, 3, 1, 1, false, n_cu),
                            facts(32, 3, 32, 1, false, n_cu), facts(16, 2, 33, 1, false, n_cu), facts(48, 3, 4, 1, false, n_cu),
                            facts(124, 3, 4, 1, false, n_cu), facts(129, 3, 4, 1, false, n_cu)};
  const int answers[] = {-1, 0, 1, 2, 3, 8, 32, 33};
  for (const PrepFacts &rep : reps) {
    std::vector<PrepFacts> sw(5, rep);
    sw[0].force_block_prepare = true;
    sw[1].env_force_block = true;
    sw[2].env_no_compress = true;
    sw[3].env_a_global = true;
    sw[4].env_no_quad = true;
    for (const PrepFacts &f : sw) emit(f);
    // the answer to the first query, and to the second where the first one sends the plan on (failed, or no room)
    const Prep v1 = gik::plan_prepare(rep, [](Prep, int, size_t) { return 1; }).variant;
    const Prep v2 = gik::plan_prepare(rep, [v1](Prep v, int, size_t) { return v == v1 ? -1 : 1; }).variant;
    for (int a1 : answers) {
      Answers an;
      an.occ[(int)v1] = a1;
      emit(rep, an);
      if (v2 == v1 || a1 > 0) continue;
      for (int a2 : answers) {
        an.occ[(int)v2] = a2;
        emit(rep, an);
      }
    }
    // GIK_PREP_WAVES_PER_CU, over answers that work and over failed queries
    for (int waves : {0, 1, 40})
      for (int failed : {0, 1}) {
        PrepFacts f = rep;
        f.env_waves_set = true;
        f.env_waves = waves;
        Answers an;
        if (failed)
          for (int &o : an.occ) o = -1;
        emit(f, an);
      }
  }
  // the quad kernel's LDS: 360 anchor-goal distances are 40 KB to the byte at 16 nodes, 361 one step (two doubles) more
  for (int n_gg : {7, 8, 9}) {
    PrepFacts f = facts(16, 2, 22, 8, false, n_cu);
    f.n_gg = n_gg;
    emit(f);
  }
}

// the anchored scratch: offsets in doubles from the base, and the total
static void anchored_scratch() {
  const int shapes[][4] = {{22, 78, 14, 2}, {22, 78, 14, 0}, {63, 400, 61, 4}, {2, 1, 1, 1}};   // base N, base T, free N, n_goal
  const char *sep = "";
  for (const auto &s : shapes)
    for (int B : {0, 1, 2, 64, 4097}) {
      const gik::AnchWs w = gik::anch_ws(s[1], s[0], s[2], s[3], B, nullptr);      // (over a null base a pointer is its offset)
      auto at = [](const double *p) { return reinterpret_cast<uintptr_t>(p) / sizeof(double); };
      std::printf("%s\n [%d, %d, %d, %d, %d, %zu, %zu, %zu, %zu, %zu]", sep, s[0], s[1], s[2], s[3], B, (size_t)at(w.targets),
                  (size_t)at(w.Y_full0), (size_t)at(w.Y_free), (size_t)at(w.goal), w.doubles);
      sep = ",";
    }
}

int main() {
  std::printf("{\"plan_fields\": [\"variant\", \"threads\", \"lds\", \"wpc\", \"slab_bytes\", \"no_compress\", \"diag_variant\", "
              "\"diag_threads\", \"diag_lds\", \"diag_wpc\"],\n\"row_fields\": [\"B\", \"grid\", \"diag_grid\"],\n\"cases\": [");
  sizes(8);
  for (int n_cu : {8, 256}) knobs(n_cu);
  std::printf("\n],\n\"anch_ws_fields\": [\"base_N\", \"base_T\", \"free_N\", \"n_goal\", \"B\", \"targets\", \"Y_full0\", \"Y_free\", "
              "\"goal\", \"doubles\"],\n\"anch_ws\": [");
  anchored_scratch();
  std::printf("\n]}\n");
  return 0;
}
