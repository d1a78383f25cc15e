// tests/host/ws_layout_table.cpp -- retry_ws, anch_sweep_ws and anch_retry_ws (graphik_amd/csrc/gik_plan.h) tabulated: the
// byte offset of every array of the three caller-owned workspaces over a null base (where a pointer is its offset), and
// the totals, for a UR10-like, a planar and an odd set of sizes and batch sizes of both parities.  Prints JSON;
// tests/test_ws_layouts.py compares it field by field with the closed forms of the layout comments (docs/NOTEBOOK.md 30).
#include "gik_plan.h"

#include <cstdio>

static size_t at(const void *p) { return (size_t) reinterpret_cast<uintptr_t>(p); }

static const int kB[] = {0, 1, 2, 3, 5, 64};
static const char *sep = "";

static void row(const int *sizes, int n_sizes, const size_t *offsets, int n_offsets) {
  std::printf("%s\n [", sep);
  for (int i = 0; i < n_sizes; ++i) std::printf("%d, ", sizes[i]);
  for (int i = 0; i < n_offsets; ++i) std::printf("%zu%s", offsets[i], i + 1 < n_offsets ? ", " : "]");
  sep = ",";
}

int main() {
  // n_joints, pose_w, T, N, K: UR10, planar-10, odd everything
  const int retry[][5] = {{6, 16, 78, 22, 3}, {10, 9, 50, 21, 2}, {7, 16, 101, 29, 3}};
  std::printf("{\"retry_fields\": [\"n\", \"pose_w\", \"T\", \"N\", \"K\", \"B\", \"count\", \"idx\", \"poses\", \"q_seed\", \"targets\", "
              "\"Y\", \"stats\", \"q\", \"pos_err\", \"rot_err\", \"bytes\"],\n\"retry\": [");
  for (const auto &s : retry)
    for (int B : kB) {
      const gik::RetryWs w = gik::retry_ws(s[0], s[1], s[2], s[3], s[4], B, nullptr);
      const int sizes[] = {s[0], s[1], s[2], s[3], s[4], B};
      const size_t o[] = {at(w.count), at(w.idx),   at(w.T), at(w.q_seed),  at(w.targets), at(w.Y),
                          at(w.stats), at(w.q), at(w.pos_err), at(w.rot_err), w.bytes};
      row(sizes, 6, o, 11);
    }
  // n_joints, pose_w, T_base, full_N: UR10 + table, planar base, odd everything
  const int sweep[][4] = {{6, 16, 78, 22}, {10, 9, 50, 21}, {7, 16, 101, 29}};
  std::printf("\n],\n\"sweep_fields\": [\"n\", \"pose_w\", \"base_T\", \"full_N\", \"B\", \"S\", \"q\", \"poses\", \"targets\", \"Y\", "
              "\"clearance\", \"doubles\"],\n\"sweep\": [");
  sep = "";
  for (const auto &s : sweep)
    for (int S : {1, 4})
      for (int B : kB) {
        const gik::AnchSweepWs w = gik::anch_sweep_ws(s[0], s[1], s[2], s[3], B, S, nullptr);
        const int sizes[] = {s[0], s[1], s[2], s[3], B, S};
        const size_t o[] = {at(w.q), at(w.T), at(w.targets), at(w.Y), at(w.cl), w.doubles};
        row(sizes, 6, o, 6);
      }
  // n_joints, pose_w, T_base, N_base, N_free, n_goal, full_N: UR10 + table, no goal anchors, odd everything
  const int anch[][7] = {{6, 16, 78, 22, 14, 2, 22}, {6, 16, 78, 22, 14, 0, 22}, {7, 16, 101, 29, 23, 3, 29}};
  std::printf("\n],\n\"anch_retry_fields\": [\"n\", \"pose_w\", \"base_T\", \"base_N\", \"free_N\", \"n_goal\", \"full_N\", \"B\", "
              "\"scratch\", \"count\", \"idx\", \"poses\", \"q_seed\", \"q_center\", \"Y\", \"stats\", \"q\", \"pos_err\", \"rot_err\", "
              "\"clearance\", \"bytes\", \"ids\"],\n\"anch_retry\": [");
  sep = "";
  for (const auto &s : anch)
    for (int B : kB) {
      const gik::AnchRetryWs w = gik::anch_retry_ws(s[0], s[1], s[2], s[3], s[4], s[5], s[6], B, nullptr);
      const int sizes[] = {s[0], s[1], s[2], s[3], s[4], s[5], s[6], B};
      const size_t o[] = {at(w.scratch), at(w.count), at(w.idx), at(w.T),       at(w.q_seed),  at(w.q_center),  at(w.Y),
                          at(w.stats),   at(w.q),     at(w.pos_err), at(w.rot_err), at(w.clearance), w.bytes, at(w.ids)};
      row(sizes, 8, o, 14);
    }
  std::printf("\n]}\n");
  return 0;
}
