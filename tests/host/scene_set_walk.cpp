// tests/host/scene_set_walk.cpp -- graphik_amd/csrc/gik_scenes.h as a program of its own: the host-checkable validation
// of a scene set (gik_scene_set) walked over every combination of counts and null pointers, each held to the rule
// written out here, and the two clamps the kernels apply to what they read from the device, walked over ids and counts
// on exactly sized heap arrays the way a kernel indexes them.  tests/test_anchored_scenes_host.py compiles it plain and
// with the address and undefined-behaviour sanitizers and runs it; it prints "ok shapes <n> refused <n> clamped <n>".
#include <climits>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gik_scenes.h"

using namespace gik;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// the rule of include/graphik_amd.h, written out
static bool accepted(int n_scene, int stride, bool obs, bool n_obs, bool ids) {
  if (n_scene < 1) return false;
  if (stride < 0 || stride > 128) return false;
  if (!n_obs) return false;
  if (!obs && stride != 0) return false;
  if (!ids && n_scene != 1) return false;
  return true;
}

int main() {
  static double obs_mem[4];
  static int cnt_mem[1], id_mem[1];
  const int n_scenes[] = {INT_MIN, -1, 0, 1, 2, 3, 1000, INT_MAX};
  const int strides[] = {INT_MIN, -1, 0, 1, 64, 127, 128, 129, 4096, INT_MAX};
  int shapes = 0, refused = 0;
  for (int ns : n_scenes)
    for (int st : strides)
      for (int mask = 0; mask < 8; ++mask) {
        const bool obs = mask & 1, cnt = mask & 2, ids = mask & 4;
        const char *why = scene_set_fault(ns, st, obs ? obs_mem : nullptr, cnt ? cnt_mem : nullptr, ids ? id_mem : nullptr);
        CHECK((why == nullptr) == accepted(ns, st, obs, cnt, ids));
        CHECK(why == nullptr || std::strlen(why) > 10);
        ++shapes;
        refused += why != nullptr;
      }
  // the shapes the header names, one by one
  CHECK(!scene_set_fault(1, 0, nullptr, cnt_mem, nullptr));           // one scene without spheres, no ids, no rows
  CHECK(!scene_set_fault(1, 128, obs_mem, cnt_mem, nullptr));         // one scene, every goal uses it
  CHECK(!scene_set_fault(3, 128, obs_mem, cnt_mem, id_mem));
  CHECK(std::strstr(scene_set_fault(0, 4, obs_mem, cnt_mem, id_mem), "n_scene"));
  CHECK(std::strstr(scene_set_fault(2, 129, obs_mem, cnt_mem, id_mem), "stride"));
  CHECK(std::strstr(scene_set_fault(2, -1, obs_mem, cnt_mem, id_mem), "stride"));
  CHECK(std::strstr(scene_set_fault(2, 4, obs_mem, cnt_mem, nullptr), "d_scene_id"));
  CHECK(std::strstr(scene_set_fault(2, 4, nullptr, cnt_mem, id_mem), "d_obs"));
  CHECK(std::strstr(scene_set_fault(2, 4, obs_mem, nullptr, id_mem), "d_n_obs"));

  // the clamps: whatever the device arrays hold, the scene row and the sphere rows a kernel reads lie inside the set
  const int vals[] = {INT_MIN, -129, -1, 0, 1, 2, 3, 63, 64, 127, 128, 129, 1000, INT_MAX};
  int clamped = 0;
  for (int ns : {1, 2, 3, 17})
    for (int st : {0, 1, 5, 128}) {
      std::vector<double> rows((size_t)ns * st * 4, 1.0);      // exactly the set: an index past it is the sanitizer's to report
      std::vector<int> counts((size_t)ns, 0);
      double sum = 0.0;
      for (int id : vals)
        for (int count : vals) {
          const int s = scene_clamp_id(id, ns);
          CHECK(s >= 0 && s < ns);
          CHECK(s == id || id < 0 || id >= ns);
          counts[(size_t)s] = count;
          const int n = scene_clamp_count(counts[(size_t)s], st);
          CHECK(n >= 0 && n <= st && n <= SCENE_MAX_SPHERES);
          CHECK(n == count || count < 0 || count > st);
          const double *scene = rows.data() + (size_t)s * (size_t)st * 4;
          for (int t = 0; t < 4 * n; ++t) sum += scene[t];
          ++clamped;
        }
      CHECK(sum >= 0.0);
    }
  CHECK(scene_clamp_count(200, 4096) == SCENE_MAX_SPHERES);      // a stride the validation refuses still cannot pass 128 rows
  std::printf("ok shapes %d refused %d clamped %d\n", shapes, refused, clamped);
  return 0;
}
