// tests/host/solve_plan_table.cpp -- plan_solve (graphik_amd/csrc/gik_plan.h) tabulated over the facts of every path
// and, for each, the batch sizes around every threshold the plan has.  Prints JSON: the field names, then per case one row per batch size;
// tests/test_solve_plan.py compares it field by field with tests/golden/solve_plan.json (docs/NOTEBOOK.md 17).
#include "gik_plan.h"

#include <cstdio>
#include <set>
#include <string>
#include <vector>

using gik::SolveFacts;

#define FIELDS "\"B\", \"launch\", \"grid\", \"launch_grid\", \"wpc\", \"slice_its\", \"slice_cycles\", \"mig\", \"cap\", " \
               "\"ycap\", \"needs_ws\", \"off_simd\", \"off_seq\", \"off_ids\", \"off_state\", \"off_yseq\", \"off_yids\", " \
               "\"off_ctg\", \"ctg_bytes\", \"bytes\", \"zero_head\", \"seq_fill\", \"state_zero\", \"yseq_zero\""

static void emit(const SolveFacts &f, int B, const char *sep) {
  const gik::SolvePlan p = gik::plan_solve(f, B);
  static const char *kind[] = {"quad", "npt", "block", "wave", "wave_spread"};
  std::printf("%s\n  [%d, \"%s\", %d, %d, %d, %d, %d, %d, %zu, %zu, %d, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu, %zu]",
              sep, B, kind[(int)p.launch], p.grid, p.launch_grid, p.wpc, p.slice_its, p.slice_cycles, (int)p.mig, p.cap,
              p.ycap, (int)p.needs_ws, p.off_simd, p.off_seq, p.off_ids, p.off_state, p.off_yseq, p.off_yids, p.off_ctg,
              p.ctg_bytes, p.bytes, p.zero_head, p.seq_fill, p.state_zero, p.yseq_zero);
}

// one case: B = 1 and one below, at and one above every threshold
static void sweep(const std::string &name, const SolveFacts &f, const std::vector<long long> &thresholds) {
  static bool first = true;
  std::set<long long> bs = {1};
  for (long long t : thresholds)
    for (long long b = t - 1; b <= t + 1; ++b)
      if (b >= 1 && b < (1LL << 30)) bs.insert(b);
  std::printf("%s\n {\"case\": \"%s\", \"rows\": [", first ? "" : ",", name.c_str());
  first = false;
  const char *sep = "";
  for (long long b : bs) {
    emit(f, (int)b, sep);
    sep = ",";
  }
  std::printf("]}");
}

static std::string tag(const char *path, const SolveFacts &f) {
  char s[256];
  std::snprintf(s, sizeof s, "%s cu%d wpc%d nwpc%d ovr%d spread%d dbg%d slice%d nslice%d wslice%d auto%d maxiter%d cg%d quad%d qmin%d ctg%zu",
                path, f.n_cu, f.waves_per_cu, f.npt_waves_per_cu, f.wpc_override, (int)f.has_spread, f.dbg, f.slice_its,
                f.npt_slice_its, f.wave_slice_its, (int)f.wave_slice_auto, f.maxiter, (int)f.cg, (int)f.has_quad,
                f.quad_min_batch, f.ctg_doubles);
  return s;
}

// the thresholds of the one-unknown-per-lane path: the persistent grid (the small-batch one of 4 waves per CU too),
// the two caps on waves per CU, slice growth (8 problems per wave) and its 4 x cap (32 per wave)
static std::vector<long long> wave_thresholds(const SolveFacts &f) {
  const long long n = f.n_cu, grid = n * (f.wpc_override > 0 ? f.wpc_override : f.waves_per_cu);
  return {grid, 4 * n, 6 * 4 * n, 128 * n, 8 * grid, 32 * grid};
}

static void wave3d(int n_cu) {
  SolveFacts base;
  base.K = 3;
  base.n_cu = n_cu;
  base.maxiter = 3000;
  base.wave_slice_its = 256;
  for (int wpc : {4, 8, 12})
    for (int spread : {0, 1}) {
      SolveFacts f = base;
      f.waves_per_cu = wpc;
      f.has_spread = spread;
      sweep(tag("wave3", f), f, wave_thresholds(f));
    }
  // one knob at a time on the build that spreads its tail at three waves per SIMD
  base.waves_per_cu = 12;
  base.has_spread = true;
  std::vector<SolveFacts> variants;
  auto vary = [&](auto set) {
    SolveFacts f = base;
    set(f);
    variants.push_back(f);
  };
  vary([](SolveFacts &f) { f.wpc_override = 2; });
  vary([](SolveFacts &f) { f.wpc_override = 2; f.has_spread = false; });
  for (int dbg : {1, 512, 1024}) vary([dbg](SolveFacts &f) { f.dbg = dbg; });
  for (int w : {16, 1024}) vary([w](SolveFacts &f) { f.wave_slice_its = w; });
  vary([](SolveFacts &f) { f.wave_slice_auto = false; });
  vary([](SolveFacts &f) { f.wave_slice_its = 16; f.wave_slice_auto = false; });
  vary([](SolveFacts &f) { f.maxiter = 300; });
  vary([](SolveFacts &f) { f.maxiter = 300; f.wave_slice_its = 1024; });
  vary([](SolveFacts &f) { f.maxiter = 300; f.wave_slice_its = 16; f.wave_slice_auto = false; });
  for (const SolveFacts &f : variants) {
    std::vector<long long> th = wave_thresholds(f);
    // slice 16: from here on the 16 B + 8192 bound of the yield queue is the smaller one
    // (B (maxiter / slice + 2) > 16 B + 8192, with the slice at its 4 x cap or taken literally)
    const int yields = f.maxiter / (f.wave_slice_auto ? 64 : 16) + 2;
    if (f.wave_slice_its == 16 && yields > 16) th.push_back(8192 / (yields - 16) + 1);
    sweep(tag("wave3", f), f, th);
  }
}

static void planar(int n_cu) {
  SolveFacts base;
  base.K = 2;
  base.n_cu = n_cu;
  base.maxiter = 3000;
  base.waves_per_cu = 8;
  base.wave_slice_its = 256;
  sweep(tag("wave2", base), base, wave_thresholds(base));
  base.has_quad = true;
  for (int qmin : {0, 12 * n_cu})
    for (int dbg : {0, 8192, 16384}) {
      SolveFacts f = base;
      f.quad_min_batch = qmin;
      f.dbg = dbg;
      // 6: not a multiple of four problems per wavefront; 4 n_cu quad_waves_per_cu: the quad grid is full
      std::vector<long long> th = {6, n_cu * f.waves_per_cu, 4LL * n_cu * f.quad_waves_per_cu};
      if (qmin > 0) th.push_back(qmin);
      sweep(tag("wave2", f), f, th);
    }
  SolveFacts f = base;
  f.quad_min_batch = 12 * n_cu;
  f.wpc_override = 2;
  sweep(tag("wave2", f), f, {6, 2 * n_cu, 8 * n_cu, 12 * n_cu});
}

static void workgroup(int n_cu) {
  SolveFacts base;
  base.K = 3;
  base.is_block = true;
  base.n_cu = n_cu;
  base.maxiter = 3000;
  base.waves_per_cu = 2;
  for (int slice : {0, 24, 4000})
    for (int cg : {0, 1}) {
      SolveFacts f = base;
      f.slice_its = slice;
      f.cg = cg;
      sweep(tag("block", f), f, {2 * n_cu, 8 * 2 * n_cu});
    }
  SolveFacts f = base;
  f.slice_its = 24;
  f.dbg = 1;
  sweep(tag("block", f), f, {2 * n_cu});
}

static void node_per_lane(int n_cu) {
  SolveFacts base;
  base.K = 3;
  base.is_block = base.is_npt = true;
  base.n_cu = n_cu;
  base.maxiter = 3000;
  base.waves_per_cu = 1;
  base.npt_waves_per_cu = 2;
  base.slice_its = 256;
  for (int slice : {0, 24})
    for (size_t ctg : {(size_t)0, (size_t)5050}) {
      SolveFacts f = base;
      f.npt_slice_its = slice;
      f.ctg_doubles = ctg;
      sweep(tag("npt", f), f, {2 * n_cu, 8 * 2 * n_cu});
    }
}

int main() {
  std::printf("{\"fields\": [" FIELDS "],\n\"cases\": [");
  for (int n_cu : {8, 256}) {
    wave3d(n_cu);
    planar(n_cu);
    workgroup(n_cu);
    node_per_lane(n_cu);
  }
  std::printf("\n]}\n");
  return 0;
}
