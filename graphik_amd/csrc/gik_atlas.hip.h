// graphik_amd/csrc/gik_atlas.hip.h -- goal-aware seeds from a configuration atlas, the device side: a table of M joint
// configurations that are clear of the room, each with its KEY -- the positions its end effector's goal nodes take --, and
// per goal the K rows whose key lies nearest to the goal's own.
//
//   atlas_nearest_kernel   : one wavefront per ATLAS_GOALS compact slots: the K rows with the smallest (d, m) of every
//                            slot's goal, ascending.  64 rows per trip, one per lane, off the component-major table; the
//                            goals' keys are wave-uniform.  Per goal the 64 best so far sit sorted one per lane; a row
//                            enters only where d < tau, the K-th best so far (a ballot; rarely any lane once the list has
//                            settled), by one compare and one whole-wave shift.  Ballot lanes are served in ascending
//                            order under strict <, so the lower row wins a tie; a NaN or infinite d never enters.
//                            Mirrored, index and distance bits, by riemannian_solver.atlas_nearest_host.
//   atlas_candidate_kernel : retry_candidate_kernel's second source: candidate c of slot r (goal g) is atlas row
//                            nbr[g][first + c], written candidate-major into the arrays the screened step realizes and
//                            measures; a row of -1 (or outside the table) is a NaN row, which is measured as NaN.
//   atlas_note_kernel      : one thread per slot, behind retry_pick_kernel: the atlas row of the slot's pick, by goal.
//   atlas_kept_kernel      : one thread per goal: the noted row of the attempt the goal's kept answer came from.
// The key and the distance are written so that every product, sum and difference is rounded on its own.
// Plain kernels, defined where GIK_DEFINE_ATLAS_KERNELS is set (gik_k_atlas.hip); gik_host_anch.hip, which launches them, sees prototypes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gik_args.h"

namespace gik {

constexpr int ATLAS_WAVE = 64;
constexpr int ATLAS_MAX_K = GIK_ATLAS_MAX_NEIGHBOURS;      // a wavefront's lanes hold one list entry each
constexpr int ATLAS_GOALS = 4;                             // slots per wavefront: they share every trip's table reads
constexpr int ATLAS_NOTE_NT = 256;
static_assert(ATLAS_MAX_K == ATLAS_WAVE, "one list entry per lane");

struct AtlasNearestArgs {
  const double *keys;       // [W][M] component-major
  const double *T_goal;     // [B][pose_w]: one 4 x 4 pose per goal
  const int *idx;           // [count] goal of each slot, or null: the slot itself
  int *nbr;                 // [count][K]
  double *dist;             // [count][K], or null
  double axis_len;          // |p_e q_e|
  int M, count, K, pose_w;
  int W;                    // 6: p_e and q_e; 3: p_e alone (a position goal)
};

struct AtlasCandidateArgs {
  const double *T_goal;     // [B][pose_w]
  const int *idx;           // [count], or null: slot r is goal r
  const double *atlas_q;    // [M][n]
  const int *nbr;           // [B][nbr_stride], indexed by GOAL
  const int *scene_id;      // [B] scene of each goal, or null
  double *T_out;            // [count][pose_w]
  double *T_c;              // [C][count][pose_w]
  double *q_c;              // [C][count][n]
  int *ids_c;               // [C][count]; written only where scene_id is given
  int count, pose_w, n, candidates, first, nbr_stride, M;
};

struct AtlasNoteArgs {
  const int *idx;           // [count], or null
  const int *nbr;           // [B][nbr_stride]
  const int *pick;          // [count]: retry_pick_kernel's c per slot
  int *row;                 // [B]: out, by goal
  int count, first, nbr_stride;
};

struct AtlasKeptArgs {
  const int *attempt;       // [B]
  const int *rows;          // [attempts][B]
  int *out;                 // [B]
  int B, attempts;
};

// the key of a goal pose T (row-major 4 x 4): p_e, then q_e = p_e + len z_e with one rounded product and one rounded sum
// per component -- the bits of numpy's p + z * len (BatchProblem.goal_positions)
template <int W>
__device__ inline void atlas_goal_key(const double *T, double len, double (&g)[W]) {
#pragma clang fp contract(off)
  for (int c = 0; c < 3; ++c) {
    const double p = T[c * 4 + 3];
    g[c] = p;
    if (W == 6) {
      const double step = T[c * 4 + 2] * len;
      g[3 + c] = p + step;
    }
  }
}

// (...((t0 t0 + t1 t1) + t2 t2) ... + t_{W-1} t_{W-1}),  t_c = g[c] - k[c]
template <int W>
__device__ inline double atlas_dist(const double (&g)[W], const double (&k)[W]) {
#pragma clang fp contract(off)
  const double t0 = g[0] - k[0];
  double d = t0 * t0;
  for (int c = 1; c < W; ++c) {
    const double t = g[c] - k[c];
    const double s = t * t;
    d = d + s;
  }
  return d;
}

// lane `src` (wave-uniform) of v
__device__ inline double atlas_lane_f64(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

// (d, m) into the ascending list that lane j holds entry j of: behind every entry <= d (they are earlier rows), the rest
// one lane up, the last one off the end
__device__ inline void atlas_insert(double &bd, int &bi, double d, int m, int lane) {
  const double up_d = __shfl_up(bd, 1);
  const int up_i = __shfl_up(bi, 1);
  if (bd > d) {
    const bool here = lane == 0 || !(up_d > d);
    bd = here ? d : up_d;
    bi = here ? m : up_i;
  }
}

template <int W>
__device__ inline void atlas_nearest_group(const AtlasNearestArgs &a, int grp, int lane) {
  constexpr int G = ATLAS_GOALS;
  const double inf = __builtin_huge_val();
  double g[G][W], bd[G], tau[G];
  int bi[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {
    const int r = min(grp * G + q, a.count - 1);      // (a slot past the end repeats the last one and is not written)
    const int goal = a.idx ? a.idx[r] : r;
    atlas_goal_key<W>(a.T_goal + (size_t)goal * a.pose_w, a.axis_len, g[q]);
    bd[q] = tau[q] = inf;
    bi[q] = -1;
  }
  for (int m0 = 0; m0 < a.M; m0 += ATLAS_WAVE) {
    const int m = m0 + lane;
    double k[W];
#pragma unroll
    for (int c = 0; c < W; ++c) k[c] = m < a.M ? a.keys[(size_t)c * a.M + m] : __builtin_nan("");
#pragma unroll
    for (int q = 0; q < G; ++q) {
      const double d = atlas_dist<W>(g[q], k);
      unsigned long long mask = __ballot(d < tau[q]);
      while (mask) {      // (wave-uniform)
        const int src = __ffsll((unsigned long long)mask) - 1;
        mask &= mask - 1;
        const double ds = atlas_lane_f64(d, src);
        if (ds < tau[q]) {      // (tau may have come down since the ballot)
          atlas_insert(bd[q], bi[q], ds, m0 + src, lane);
          tau[q] = atlas_lane_f64(bd[q], a.K - 1);
        }
      }
    }
  }
#pragma unroll
  for (int q = 0; q < G; ++q) {
    const int r = grp * G + q;
    if (r < a.count && lane < a.K) {
      a.nbr[(size_t)r * a.K + lane] = bi[q];
      if (a.dist) a.dist[(size_t)r * a.K + lane] = bd[q];
    }
  }
}

__global__ void __launch_bounds__(ATLAS_WAVE) atlas_nearest_kernel(AtlasNearestArgs a)
#ifndef GIK_DEFINE_ATLAS_KERNELS
    ;      // (defined in gik_k_atlas.hip)
#else
{
  const int lane = threadIdx.x;
  const int groups = (a.count + ATLAS_GOALS - 1) / ATLAS_GOALS;
  for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {
    if (a.W == 6)
      atlas_nearest_group<6>(a, grp, lane);
    else
      atlas_nearest_group<3>(a, grp, lane);
  }
}
#endif

__global__ void __launch_bounds__(ATLAS_WAVE) atlas_candidate_kernel(AtlasCandidateArgs a)
#ifndef GIK_DEFINE_ATLAS_KERNELS
    ;
#else
{
  const int lane = threadIdx.x;
  for (int r = blockIdx.x; r < a.count; r += gridDim.x) {
    const int g = a.idx ? a.idx[r] : r;
    const double *src = a.T_goal + (size_t)g * a.pose_w;
    double *dst = a.T_out + (size_t)r * a.pose_w;
    for (int e = lane; e < a.pose_w; e += ATLAS_WAVE) dst[e] = src[e];
    for (int c = 0; c < a.candidates; ++c) {
      const size_t m = (size_t)c * a.count + r;
      const int row = a.nbr[(size_t)g * a.nbr_stride + a.first + c];
      const bool have = row >= 0 && row < a.M;
      for (int e = lane; e < a.pose_w; e += ATLAS_WAVE) a.T_c[m * a.pose_w + e] = src[e];
      for (int j = lane; j < a.n; j += ATLAS_WAVE)
        a.q_c[m * a.n + j] = have ? a.atlas_q[(size_t)row * a.n + j] : __builtin_nan("");
      if (a.scene_id && lane == 0) a.ids_c[m] = a.scene_id[g];
    }
  }
}
#endif

__global__ void __launch_bounds__(ATLAS_NOTE_NT) atlas_note_kernel(AtlasNoteArgs a)
#ifndef GIK_DEFINE_ATLAS_KERNELS
    ;
#else
{
  const int r = blockIdx.x * ATLAS_NOTE_NT + threadIdx.x;
  if (r >= a.count) return;
  const int g = a.idx ? a.idx[r] : r;
  a.row[g] = a.nbr[(size_t)g * a.nbr_stride + a.first + a.pick[r]];
}
#endif

__global__ void __launch_bounds__(ATLAS_NOTE_NT) atlas_kept_kernel(AtlasKeptArgs a)
#ifndef GIK_DEFINE_ATLAS_KERNELS
    ;
#else
{
  const int b = blockIdx.x * ATLAS_NOTE_NT + threadIdx.x;
  if (b >= a.B) return;
  const int at = a.attempt[b];
  a.out[b] = at >= 0 && at < a.attempts ? a.rows[(size_t)at * a.B + b] : -1;
}
#endif

}  // namespace gik
