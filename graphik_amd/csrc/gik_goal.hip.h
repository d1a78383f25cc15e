// graphik_amd/csrc/gik_goal.hip.h -- goal assembly: the positions of a goal pose's nodes and the anchor <-> goal and
// goal <-> goal distances of one problem (PipeConst, gik_args.h).  What the prepare kernels (gik_prep.hip.h,
// gik_prep_quad.hip.h) and seed_kernel (gik_recover_seed.hip.h) have in common.
#pragma once

#include <hip/hip_runtime.h>

#include "gik_args.h"

namespace gik {

// position of goal node g = 2 e + s of problem `Tg` ([n_ee][(K+1)^2]): p_e, or q_e = p_e + len z_e
// (graph_revolute.py:243-249); k = 2: p_n, p_{n-1} = p_n - len x_n (graph_planar.py:136-145)
__device__ inline void goal_node_pos(const PipeConst &pc, const double *Tg, int g, double (&w)[3]) {
  const int K = pc.K, D = K + 1;
  const double *T = Tg + (size_t)(g >> 1) * D * D;
  for (int c = 0; c < K; ++c) {
    const double p = T[c * D + K];
    const double len = pc.ee_len[g >> 1];
    w[c] = !(g & 1) ? p : ((K == 3) ? p + T[c * D + 2] * len : p - T[c * D + 0] * len);
  }
}

// anchor <-> goal and goal <-> goal distances of one problem: entry idx of gd (see PipeConst)
__device__ inline double goal_distance(const PipeConst &pc, const double *Tg, int idx, int &na, int &nb) {
  const int K = pc.K, G = 2 * pc.n_ee;
  double a[3], b[3];
  if (idx < G * pc.n_anchor) {
    const int ai = idx / G, g = idx - ai * G;
    for (int c = 0; c < K; ++c) a[c] = pc.anchor_pos[ai * K + c];
    goal_node_pos(pc, Tg, g, b);
    na = pc.anchor_idx[ai];
    nb = pc.goal_node[g];
  } else {
    const int q = idx - G * pc.n_anchor;
    goal_node_pos(pc, Tg, pc.gg_a[q], a);
    goal_node_pos(pc, Tg, pc.gg_b[q], b);
    na = pc.goal_node[pc.gg_a[q]];
    nb = pc.goal_node[pc.gg_b[q]];
  }
  double d2 = 0.0;
  for (int c = 0; c < K; ++c) {
    const double df = a[c] - b[c];
    d2 += df * df;
  }
  return sqrt(d2);   // np.linalg.norm
}

}  // namespace gik
