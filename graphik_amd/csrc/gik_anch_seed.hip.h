// graphik_amd/csrc/gik_anch_seed.hip.h -- fixed-anchor formulation from a joint-configuration seed, and the
// clearance of a point matrix from the template's obstacles: the device side.
//
//   anch_scatter_kernel   : the seeded twin of anch_init_kernel.  seed_kernel's realization of q_init on the robot
//                           graph is already in the world frame with the base anchors at their positions, so the
//                           anchored start point is a row gather of it -- Y_free[f] = Y_full_in[free_full[f]],
//                           copied, no arithmetic, no Procrustes fit -- and the goal anchors come from the goal pose
//                           (anchor_world), never from the seed: the goal nodes' seed rows are dropped.  One thread
//                           per double of the output, consecutive lanes on consecutive doubles.
//   anch_clearance_kernel : one wavefront per goal: min over (free node i with obs_node_mask[i], obstacle o) of
//                           |Y_i - c_o| - r_o on a full point matrix.  Lanes stride over the pairs, then a wave
//                           min-reduction by shuffles (no LDS, no atomics).  No pair: +inf.  A NaN coordinate of a
//                           masked node: NaN for that goal.
// Plain kernels, defined where GIK_DEFINE_ANCH_SEED_KERNELS is set (gik_k_anch_seed.hip); gik_host.hip sees prototypes.
#pragma once

#include <hip/hip_runtime.h>

#include "gik_prep.hip.h"

namespace gik {

constexpr int ANCH_SCATTER_NT = 256;

struct AnchClearArgs {
  const double *Y_full;      // [B][full_N*3]
  const double *obs;         // [n_obs][4] x, y, z, r^2
  const int *node_full;      // [n_node] the masked free nodes, as rows of the full point matrix
  double *clearance;         // [B]
  int B, full_N, n_node, n_obs;
};

// (AnchGlueArgs: Y_full_in = seed_kernel's output, Y_free / anchor_goal out; Y_full_out unused)
__global__ void __launch_bounds__(ANCH_SCATTER_NT) anch_scatter_kernel(AnchGlueArgs a)
#ifndef GIK_DEFINE_ANCH_SEED_KERNELS
    ;      // (defined in gik_k_anch_seed.hip)
#else
{
  const size_t rowF = (size_t)a.Nf * 3, rowG = (size_t)a.n_goal * 3;
  const size_t nF = (size_t)a.B * rowF, nG = (size_t)a.B * rowG;
  const size_t t = (size_t)blockIdx.x * ANCH_SCATTER_NT + threadIdx.x;
  if (t < nF) {
    const size_t b = t / rowF;
    const int e = (int)(t - b * rowF), f = e / 3, c = e - f * 3;
    a.Y_free[t] = a.Y_full_in[(b * a.full_N + a.free_full[f]) * 3 + c];
  } else if (t - nF < nG) {
    const size_t u = t - nF, b = u / rowG;
    const int e = (int)(u - b * rowG), r = e / 3, c = e - r * 3;
    double w[3];
    anchor_world(a, a.T_goal + b * 16, a.goal_row0 + r, w);
    a.anchor_goal[u] = c == 0 ? w[0] : (c == 1 ? w[1] : w[2]);
  }
}
#endif

__global__ void __launch_bounds__(WAVE) anch_clearance_kernel(AnchClearArgs a)
#ifndef GIK_DEFINE_ANCH_SEED_KERNELS
    ;
#else
{
  const int lane = threadIdx.x, pairs = a.n_node * a.n_obs;
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const double *Y = a.Y_full + (size_t)b * a.full_N * 3;
    double m = __builtin_huge_val();
    bool nan = false;
    for (int p = lane; p < pairs; p += WAVE) {
      const int i = p / a.n_obs, o = p - i * a.n_obs;
      const double *y = Y + a.node_full[i] * 3, *s = a.obs + o * 4;
      const double dx = y[0] - s[0], dy = y[1] - s[1], dz = y[2] - s[2];
      const double v = sqrt(dx * dx + dy * dy + dz * dz) - sqrt(s[3]);
      nan |= v != v;
      m = fmin(m, v);
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) m = fmin(m, __shfl_xor(m, off));
    if (__any(nan)) m = __builtin_nan("");
    if (lane == 0) a.clearance[b] = m;
  }
}
#endif

}  // namespace gik
