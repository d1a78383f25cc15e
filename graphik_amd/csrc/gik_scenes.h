// graphik_amd/csrc/gik_scenes.h -- what the host can check of a per-goal scene set (gik_scene_set, include/graphik_amd.h)
// before a scene call queues anything: the counts and which of the device pointers may be null.  The contents of d_n_obs
// and d_scene_id live on the device and are the caller's precondition; the kernels clamp what they read from them
// (scene_clamp_id / scene_clamp_count below are those clamps, restated on the host), so a bad entry selects a wrong
// scene or fewer spheres, never memory outside the set.
// Plain C++17, no HIP, so that tests/host/scene_set_walk.cpp can walk it without a device.
#pragma once

namespace gik {

constexpr int SCENE_MAX_SPHERES = 128;   // rows of the obstacle table in LDS (ANCH_MAXOBS)

// what is wrong with a scene set, or null
inline const char *scene_set_fault(int n_scene, int stride, const void *d_obs, const void *d_n_obs, const void *d_scene_id) {
  if (n_scene < 1) return "n_scene must be at least 1";
  if (stride < 0 || stride > SCENE_MAX_SPHERES) return "stride must be within 0 .. 128 (spheres per scene)";
  if (!d_n_obs) return "null d_n_obs (the sphere count of every scene, [n_scene] on the device)";
  if (!d_obs && stride > 0) return "null d_obs (it may be null only with stride == 0: scenes without spheres)";
  if (!d_scene_id && n_scene != 1) return "null d_scene_id: every goal uses scene 0, which needs n_scene == 1";
  return nullptr;
}

// a scene set as the kernels take it: obstacle rows [n_scene][stride][4] come with the kernel's other arguments
struct SceneArgs {
  const int *scene_id = nullptr;   // [B] scene of each goal, or null: every goal uses scene 0
  const int *n_obs = nullptr;      // [n_scene] spheres of each scene
  int n_scene = 1, stride = 0;
};

// the scene a kernel reads for an id, and the rows it walks for a count (constexpr: host and device code alike)
constexpr int scene_clamp_id(int id, int n_scene) { return id < 0 ? 0 : (id > n_scene - 1 ? n_scene - 1 : id); }
constexpr int scene_clamp_count(int count, int stride) {
  const int cap = stride < SCENE_MAX_SPHERES ? stride : SCENE_MAX_SPHERES;
  return count < 0 ? 0 : (count > cap ? cap : count);
}

}  // namespace gik
