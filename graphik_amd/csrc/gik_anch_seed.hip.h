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
//                           |Y_i - c_o| - r_o on a full point matrix (wave_pair_min: lanes stride over the pairs, then
//                           a wave min-reduction by shuffles, no LDS, no atomics).  No pair: +inf.  A NaN coordinate of
//                           a masked node: NaN for that goal.
//   anch_link_clearance_kernel : the same wave, over (link l, obstacle o): the distance from the sphere's centre to the
//                           SEGMENT between two rows of the point matrix, less the radius and the link's own
//                           thickness (anch_link_pair).  A link can cross a sphere with both ends outside it, which
//                           the node clearance does not see.  No pair: +inf.  A NaN coordinate of a link end: NaN.
//   anch_sweep_interp_kernel / anch_sweep_min_kernel : the ends of gik_anchored_sweep_clearance -- the S + 1 joint
//                           configurations between q_a and q_b (and the identity poses seed_kernel is handed with
//                           them), one thread per double; and the minimum over the samples, one thread per goal.
//   anch_clearance_scene_kernel / anch_link_clearance_scene_kernel / scene_gather_kernel : the two clearance kernels with
//                           the obstacle rows of a per-goal scene (gik_scene_set), and the scene ids of a compact batch.
//   anch_self_clearance_kernel : link against link: min over the attached pairs (l, m) of the distance between the two
//                           SEGMENTS less both radii (anch_self_pair), optionally merged into the value already there.
//                           Up to 16 pairs: four goals per wavefront, lane 16 g + p on pair p of goal slot g, the
//                           minimum and the NaN flag per 16-lane row.  More: one wavefront per goal, as the link kernel.
//   anch_half_clearance_kernel : against the template's half-spaces (gik_anchored_attach_halfspaces): one wavefront per goal,
//                           min over (item, end row P, half-space h) of s_h(P) - margin with s_h = ((nx x + ny y) + nz z) - d0,
//                           every product and sum rounded on its own.  The items are the masked free nodes with their
//                           margins, or the attached links -- both end rows, constants included -- with their radii.
//                           Optionally merged into the value already there, like the self kernel.  A NaN coordinate: NaN.
// The pair functions themselves (anch_link_pair, anch_self_pair, anch_sweep_interp, anch_sweep_min) are gik_anch_pairs.h's,
// shared with the hinges of the solve kernels.
// Plain kernels, defined where GIK_DEFINE_ANCH_SEED_KERNELS is set (gik_k_anch_seed.hip); every other unit that includes
// this header -- the two host units, which launch them -- sees prototypes.
#pragma once

#include <hip/hip_runtime.h>

#include "gik_anch_glue.hip.h"      // (anchor_world)
#include "gik_anch_pairs.h"
#include "gik_args.h"
#include "gik_scenes.h"

namespace gik {

constexpr int ANCH_SCATTER_NT = 256;
constexpr int ANCH_MAXLINK = 64;   // links of gik_anchored_attach_links
constexpr int ANCH_MAXSELF = ANCH_MAXLINK * (ANCH_MAXLINK - 1) / 2;   // pairs of gik_anchored_attach_self_pairs: 2016
constexpr int ANCH_SELF_ROW = 16;  // anch_self_clearance_kernel: up to this many pairs, a goal per 16-lane row

struct AnchClearArgs {
  const double *Y_full;      // [B][full_N*3]
  const double *obs;         // [n_obs][4] x, y, z, r^2
  const int *node_full;      // [n_node] the masked free nodes, as rows of the full point matrix
  double *clearance;         // [B]
  int B, full_N, n_node, n_obs;
};

struct AnchLinkArgs {
  const double *Y_full;      // [B][full_N*3]
  const double *obs;         // [n_obs][4] x, y, z, r^2
  const int *link_a, *link_b;   // [n_link] the ends of a link, as rows of the full point matrix
  const double *link_rho;    // [n_link] capsule radius of a link, >= 0
  double *clearance;         // [B]
  int B, full_N, n_link, n_obs;
};

struct AnchSelfArgs {
  const double *Y_full;      // [B][full_N*3]
  const int *link_a, *link_b;   // [n_link] as AnchLinkArgs
  const double *link_rho;    // [n_link]
  const int *pair_l, *pair_m;   // [n_pair] the two links of a pair, indices into the link arrays
  double *clearance;         // [B]
  int B, full_N, n_pair;
  int merge;                 // 0: clearance[b] = the minimum; 1: the NaN-propagating minimum of it and clearance[b]
};

struct AnchHalfArgs {
  const double *Y_full;      // [B][full_N*3]
  const double *half;        // [n_half][4] nx, ny, nz, d0
  const int *row_a, *row_b;  // [n_item] rows of the full point matrix: a node (row_b null), or the two ends of a link
  const double *margin;      // [n_item] the node's margin, or the link's radius
  double *clearance;         // [B]
  int B, full_N, n_item, n_half;
  int merge;                 // as AnchSelfArgs
};

struct AnchSweepInterpArgs {
  const double *q_a, *q_b;   // [B][n]
  double *q_s;               // [S+1][B][n]  sample-major
  double *T_id;              // [(S+1) B][pose_w] identity poses (seed_kernel's goal argument; nobody reads its targets)
  int B, n, S, pose_w, D;    // D = 4: a pose is n_ee blocks of D x D
};

struct AnchSweepMinArgs {
  const double *cl;          // [S+1][B]
  double *clearance;         // [B]
  int B, S;
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

#ifdef GIK_DEFINE_ANCH_SEED_KERNELS
// The minimum of value(p) over p = 0 .. pairs - 1 by one whole wavefront, handed back in every lane: lane l takes
// p = l, l + 64, ..., then a butterfly of shuffles.  No pair: +inf.  A NaN value in any lane: NaN (fmin would drop it).
template <class Value>
__device__ inline double wave_pair_min(int lane, int pairs, Value value) {
  double m = __builtin_huge_val();
  bool nan = false;
  for (int p = lane; p < pairs; p += WAVE) {
    const double v = value(p);
    nan |= v != v;
    m = fmin(m, v);
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) m = fmin(m, __shfl_xor(m, off));
  return __any(nan) ? __builtin_nan("") : m;
}

// goal b of the node clearance against the n_obs rows at obs: the template's own, or a scene's
__device__ inline double anch_node_min(const AnchClearArgs &a, int b, const double *obs, int n_obs) {
  const double *Y = a.Y_full + (size_t)b * a.full_N * 3;
  return wave_pair_min(threadIdx.x, a.n_node * n_obs, [&](int p) {
    const int i = p / n_obs, o = p - i * n_obs;
    const double *y = Y + a.node_full[i] * 3, *s = obs + o * 4;
    const double dx = y[0] - s[0], dy = y[1] - s[1], dz = y[2] - s[2];
    return sqrt(dx * dx + dy * dy + dz * dz) - sqrt(s[3]);
  });
}

// ... and of the link clearance
__device__ inline double anch_link_min(const AnchLinkArgs &a, int b, const double *obs, int n_obs) {
  const double *Y = a.Y_full + (size_t)b * a.full_N * 3;
  return wave_pair_min(threadIdx.x, a.n_link * n_obs, [&](int p) {
    const int l = p / n_obs, o = p - l * n_obs;
    return anch_link_pair(Y + a.link_a[l] * 3, Y + a.link_b[l] * 3, obs + o * 4, a.link_rho[l]);
  });
}

// pair p of one goal's point matrix (anch_self_clearance_kernel)
__device__ inline double anch_self_value(const AnchSelfArgs &a, const double *Y, int p) {
  const int l = a.pair_l[p], m = a.pair_m[p];
  return anch_self_pair(Y + a.link_a[l] * 3, Y + a.link_b[l] * 3, Y + a.link_a[m] * 3, Y + a.link_b[m] * 3, a.link_rho[l],
                        a.link_rho[m]);
}

// what anch_self_clearance_kernel stores for a goal: its minimum m, or with merge the NaN-propagating minimum of m and
// the value already there (the link clearance of the same point: clearance_mode = GIK_CLEARANCE_LINKS_SELF)
__device__ inline void anch_self_store(const AnchSelfArgs &a, int b, double m) {
  if (a.merge) {
    const double old = a.clearance[b];
    m = (old != old || m != m) ? __builtin_nan("") : (old < m ? old : m);
  }
  a.clearance[b] = m;
}

// The obstacle rows of goal b's scene (gik_scene_set): a.obs is [n_scene][stride][4] and a.n_obs is not read; the goal is
// measured against the first n_obs[s] rows of scene s = scene_id[b] (null: scene 0), id and count clamped as the solve
// kernel clamps them (SceneArgs, gik_scenes.h).
__device__ inline const double *anch_scene_rows(const SceneArgs &sc, const double *obs, int b, int &n) {
  const int s = scene_clamp_id(sc.scene_id ? sc.scene_id[b] : 0, sc.n_scene);
  n = scene_clamp_count(sc.n_obs[s], sc.stride);
  return obs + (size_t)s * (size_t)sc.stride * 4;
}
#endif

__global__ void __launch_bounds__(WAVE) anch_clearance_kernel(AnchClearArgs a)
#ifndef GIK_DEFINE_ANCH_SEED_KERNELS
    ;
#else
{
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const double m = anch_node_min(a, b, a.obs, a.n_obs);
    if (threadIdx.x == 0) a.clearance[b] = m;
  }
}
#endif

__global__ void __launch_bounds__(WAVE) anch_link_clearance_kernel(AnchLinkArgs a)
#ifndef GIK_DEFINE_ANCH_SEED_KERNELS
    ;
#else
{
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const double m = anch_link_min(a, b, a.obs, a.n_obs);
    if (threadIdx.x == 0) a.clearance[b] = m;
  }
}
#endif

__global__ void __launch_bounds__(WAVE) anch_self_clearance_kernel(AnchSelfArgs a)
#ifndef GIK_DEFINE_ANCH_SEED_KERNELS
    ;
#else
{
  const int lane = threadIdx.x;
  if (a.n_pair <= ANCH_SELF_ROW) {
    // four goals per wavefront: lane 16 g + p takes pair p of goal slot g; the trip count is the wavefront's, so every
    // lane reaches the exchanges; a slot beyond B computes and writes nothing
    const int g = lane / ANCH_SELF_ROW, p = lane % ANCH_SELF_ROW;
    for (int b0 = blockIdx.x * 4; b0 < a.B; b0 += gridDim.x * 4) {
      const int b = b0 + g;
      double v = __builtin_huge_val();
      if (b < a.B && p < a.n_pair) v = anch_self_value(a, a.Y_full + (size_t)b * a.full_N * 3, p);
      const bool nan = v != v;
      double m = fmin(__builtin_huge_val(), v);
      for (int off = ANCH_SELF_ROW / 2; off > 0; off >>= 1) m = fmin(m, __shfl_xor(m, off, ANCH_SELF_ROW));
      // the NaN flag of this goal's row alone: a NaN goal must not poison its three neighbours
      if ((__ballot(nan) >> (g * ANCH_SELF_ROW)) & 0xffffull) m = __builtin_nan("");
      if (p == 0 && b < a.B) anch_self_store(a, b, m);
    }
    return;
  }
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const double *Y = a.Y_full + (size_t)b * a.full_N * 3;
    const double m = wave_pair_min(lane, a.n_pair, [&](int p) { return anch_self_value(a, Y, p); });
    if (lane == 0) anch_self_store(a, b, m);
  }
}
#endif

__global__ void __launch_bounds__(WAVE) anch_half_clearance_kernel(AnchHalfArgs a)
#ifndef GIK_DEFINE_ANCH_SEED_KERNELS
    ;
#else
{
  const int ends = a.row_b ? 2 : 1;
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const double *Y = a.Y_full + (size_t)b * a.full_N * 3;
    double m = wave_pair_min(threadIdx.x, a.n_item * ends * a.n_half, [&](int p) {
      const int h = p % a.n_half, ie = p / a.n_half, i = ie / ends;
      const double *y = Y + ((ie - i * ends) ? a.row_b[i] : a.row_a[i]) * 3, *n = a.half + h * 4;
      // (the rounding intrinsics: no product is contracted into a sum, the numpy mirror has the same bits)
      const double s = __dsub_rn(__dadd_rn(__dadd_rn(__dmul_rn(n[0], y[0]), __dmul_rn(n[1], y[1])), __dmul_rn(n[2], y[2])), n[3]);
      return __dsub_rn(s, a.margin[i]);
    });
    if (threadIdx.x == 0) {
      if (a.merge) {
        const double old = a.clearance[b];
        m = (old != old || m != m) ? __builtin_nan("") : (old < m ? old : m);
      }
      a.clearance[b] = m;
    }
  }
}
#endif

// ---- per-goal obstacle scenes (gik_scene_set) ----
// The two clearance kernels above with the obstacle rows looked up per goal (anch_scene_rows): the same pairs through the
// same per-goal body.
__global__ void __launch_bounds__(WAVE) anch_clearance_scene_kernel(AnchClearArgs a, SceneArgs sc)
#ifndef GIK_DEFINE_ANCH_SEED_KERNELS
    ;
#else
{
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    int n_obs;
    const double *obs = anch_scene_rows(sc, a.obs, b, n_obs);
    const double m = anch_node_min(a, b, obs, n_obs);
    if (threadIdx.x == 0) a.clearance[b] = m;
  }
}
#endif

__global__ void __launch_bounds__(WAVE) anch_link_clearance_scene_kernel(AnchLinkArgs a, SceneArgs sc)
#ifndef GIK_DEFINE_ANCH_SEED_KERNELS
    ;
#else
{
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    int n_obs;
    const double *obs = anch_scene_rows(sc, a.obs, b, n_obs);
    const double m = anch_link_min(a, b, obs, n_obs);
    if (threadIdx.x == 0) a.clearance[b] = m;
  }
}
#endif

// the scene ids of a restart's compact batch: out[r] = scene_id[idx[r]], one thread per slot
__global__ void __launch_bounds__(ANCH_SCATTER_NT) scene_gather_kernel(const int *scene_id, const int *idx, int count, int *out)
#ifndef GIK_DEFINE_ANCH_SEED_KERNELS
    ;
#else
{
  const int r = blockIdx.x * ANCH_SCATTER_NT + threadIdx.x;
  if (r < count) out[r] = scene_id[idx[r]];
}
#endif

__global__ void __launch_bounds__(ANCH_SCATTER_NT) anch_sweep_interp_kernel(AnchSweepInterpArgs a)
#ifndef GIK_DEFINE_ANCH_SEED_KERNELS
    ;
#else
{
  const size_t row = (size_t)a.B * a.n, nQ = (size_t)(a.S + 1) * row, nT = (size_t)(a.S + 1) * a.B * a.pose_w;
  const size_t t = (size_t)blockIdx.x * ANCH_SCATTER_NT + threadIdx.x;
  if (t < nQ) {
    const int s = (int)(t / row);
    const size_t e = t - (size_t)s * row;
    a.q_s[t] = anch_sweep_interp(a.q_a[e], a.q_b[e], s, a.S);
  } else if (t - nQ < nT) {
    const int e = (int)((t - nQ) % (size_t)(a.D * a.D));
    a.T_id[t - nQ] = (e / a.D == e % a.D) ? 1.0 : 0.0;
  }
}
#endif

__global__ void __launch_bounds__(ANCH_SCATTER_NT) anch_sweep_min_kernel(AnchSweepMinArgs a)
#ifndef GIK_DEFINE_ANCH_SEED_KERNELS
    ;
#else
{
  const size_t b = (size_t)blockIdx.x * ANCH_SCATTER_NT + threadIdx.x;
  if (b < (size_t)a.B) a.clearance[b] = anch_sweep_min(a.cl + b, a.S + 1, (size_t)a.B);
}
#endif

}  // namespace gik
