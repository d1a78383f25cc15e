// graphik_amd/csrc/gik_retry.hip.h -- restarts from random joint configurations, the device side: the plain solve and
// the fixed-anchor (obstacle) solve share one rule, one seed formula and one set of kernels.
//
//   retry_select_kernel : one thread per goal: failed goals -> a compact index list (wave ballot, one atomic
//                         per wavefront; the order of the list is whatever the atomics make it).
//   retry_seed_kernel   : one wavefront per compact slot: the goal's pose rows and n joint angles drawn by a
//                         counter-based generator -- a function of (seed, goal, attempt, joint) only.  spread == 0:
//                         uniformly inside the joint limits.  spread > 0: q = clamp(c + spread (2u - 1), lo, hi) around
//                         the centre row of the GOAL (not of the slot), same u.  Mirrored bit for bit by
//                         graphik_amd.solvers.riemannian_solver.retry_seeds_host.
//   retry_merge_kernel  : one wavefront per compact slot: the retry's answer -- point row, stats, q, both errors and,
//                         where there is one, the clearance -- replaces the goal's incumbent if and only if it is
//                         better; rows that are not replaced are not written.
//   retry_candidate_kernel : retry_seed_kernel's loop over C candidates per slot (opt-in screening of the anchored
//                         restarts): candidate c of (seed, goal, attempt) is the seed formula under
//                         retry_candidate_seed(seed, c), so candidate 0 is retry_seed_kernel's row, bit for bit.  The
//                         candidates are laid out candidate-major, [C][count], with a pose row each for the robot
//                         graph's seed kernel and, with scenes, the goal's scene id.
//   retry_pick_kernel   : one wavefront per compact slot: retry_pick over the slot's C clearances, the chosen angles
//                         into the compact seed array.
// The anchored solve adds the answer's clearance to the rule (an answer that sits on its goal with a joint point -- or,
// where the caller hands in the link clearance, any part of a link -- inside a sphere has failed).  The plain solve has
// no clearance: its kernels get null clearance pointers, which read as +inf, and +inf drops out of the rule.
// The rule and the seed formula are __host__ __device__ functions, so that a host program can walk them.
// Plain kernels, defined where GIK_DEFINE_RETRY_KERNELS is set (gik_k_retry.hip); gik_host_anch.hip, which launches them, sees prototypes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "graphik_amd.h"

namespace gik {

constexpr int RETRY_WAVE = 64;

struct RetryTol {
  double pos_tol, rot_tol, clear_tol;
};

// failed: the solver did not stop on its gradient bar, an end-effector error is not within its tolerance, or the answer is
// deeper than clear_tol inside a sphere (a masked node, or a link: whichever clearance the array holds)
// (written so that a NaN error or clearance counts as failed; +inf -- no obstacle, no masked node, no clearance at all --
// never fails a goal)
__host__ __device__ inline bool retry_failed(int stop, double pos_err, double rot_err, double clearance, RetryTol t) {
  return stop != 0 || !(pos_err <= t.pos_tol) || !(rot_err <= t.rot_tol) || !(clearance >= -t.clear_tol);
}

// what the merge orders answers of one success class by: the larger of the pose errors in units of their tolerances and
// the penetration depth in units of clear_tol; a NaN scores +inf, so it never wins.  clearance = +inf: the depth is 0 and
// the score is max(pos_err / pos_tol, rot_err / rot_tol), for every pair of errors that is non-negative, +inf or NaN --
// they are norms written by recover_kernel, so nothing else occurs.
__host__ __device__ inline double retry_score(double pos_err, double rot_err, double clearance, RetryTol t) {
  if (clearance != clearance) return __builtin_huge_val();
  const double a = pos_err / t.pos_tol, b = rot_err / t.rot_tol;
  const double s = a != a || b != b ? __builtin_huge_val() : a > b ? a : b;
  const double depth = (clearance < 0.0 ? -clearance : 0.0) / t.clear_tol;
  return s > depth ? s : depth;
}

// does the restart's answer (_r) replace the incumbent (_i)?  A success beats a failure; within one class the smaller
// score wins and a tie keeps the incumbent.
__host__ __device__ inline bool retry_better(int stop_r, double pos_r, double rot_r, double clear_r, int stop_i, double pos_i,
                                             double rot_i, double clear_i, RetryTol t) {
  const bool ok_r = !retry_failed(stop_r, pos_r, rot_r, clear_r, t);
  const bool ok_i = !retry_failed(stop_i, pos_i, rot_i, clear_i, t);
  return (ok_r && !ok_i) || (ok_r == ok_i && retry_score(pos_r, rot_r, clear_r, t) < retry_score(pos_i, rot_i, clear_i, t));
}

// ---- candidate screening: C seeds per failed goal, the restart starts from the first clear one ----
constexpr int RETRY_MAX_CANDIDATES = GIK_RETRY_MAX_CANDIDATES;

// the generator seed of candidate c: candidate 0 is the call's own seed (mod 2^64, as the unsigned product wraps)
__host__ __device__ inline uint64_t retry_candidate_seed(uint64_t seed, int c) {
  return seed + (uint64_t)c * 0xD1342543DE82EF95ull;
}

// Which of C candidates a restart starts from; cl[c * stride] is the clearance of candidate c's realization.  The first
// in candidate order with clearance >= -clear_tol -- what retry_failed passes; +inf qualifies, so a problem with nothing
// to measure picks candidate 0.  None: the largest clearance, the lowest c on a tie; a NaN never wins.  All NaN: 0.
__host__ __device__ inline int retry_pick(const double *cl, int C, size_t stride, double clear_tol) {
  int best = 0;
  bool none = true;
  double best_v = 0.0;
  for (int c = 0; c < C; ++c) {
    const double v = cl[(size_t)c * stride];
    if (v >= -clear_tol) return c;
    if (v == v && (none || v > best_v)) best = c, best_v = v, none = false;
  }
  return best;
}

// one seed angle.  u = retry_uniform(seed, goal, attempt, joint).  spread == 0: lo + u (hi - lo), one rounded product and
// one rounded sum, as numpy forms it.  spread > 0: t = 2u - 1 is exact (u is a 53-bit fraction), then one rounded product
// and one rounded sum, clamped to the limits; a NaN centre passes both comparisons and comes out as NaN.
__host__ __device__ inline double retry_seed_value(double u, double lo, double hi, double center, double spread) {
#pragma clang fp contract(off)
  if (!(spread > 0.0)) {
    const double span = hi - lo;
    const double step = u * span;
    return lo + step;
  }
  const double t = 2.0 * u - 1.0;
  const double step = spread * t;
  double q = center + step;
  q = q < lo ? lo : q;
  q = q > hi ? hi : q;
  return q;
}

struct RetrySelectArgs {
  const gik_stats *stats;   // [B]
  const double *pos_err;    // [B]
  const double *rot_err;    // [B]
  const double *clearance;  // [B], or null: +inf
  RetryTol tol;
  int *idx;                 // [B] out: the failed goals, compact
  int *count;               // [1] in: 0, out: how many
  int B;
};

struct RetrySeedArgs {
  const double *T_goal;     // [B][pose_w]  pose_w = n_ee (K+1)^2
  const int *idx;           // [count]
  const double *q_lo, *q_hi;   // [n]
  const double *q_center;   // [B][n], indexed by goal; read only if spread > 0
  double *T_out;            // [count][pose_w]
  double *q_out;            // [count][n]
  double spread;
  uint64_t seed;
  int count, pose_w, n, attempt;
};

struct RetryMergeArgs {
  const int *idx;           // [count] distinct goals
  // the retry's answers, compact
  const double *Y_r;        // [count][row]  row = N K (anchored: full_N 3)
  const gik_stats *stats_r; // [count]
  const double *q_r;        // [count][n]
  const double *pos_r, *rot_r;   // [count]
  const double *clear_r;    // [count], or null: +inf
  // the incumbents
  double *Y;                // [B][row]
  gik_stats *stats;         // [B]
  double *q;                // [B][n]
  double *pos_err, *rot_err;     // [B]
  double *clearance;        // [B], or null: +inf, and never stored
  int *attempt;             // [B]
  RetryTol tol;
  int count, row, n, attempt_no;
};

struct RetryCandidateArgs {
  const double *T_goal;     // [B][pose_w]
  const int *idx;           // [count]
  const double *q_lo, *q_hi;   // [n]
  const double *q_center;   // [B][n], indexed by goal; read only if spread > 0
  const int *scene_id;      // [B] scene of each goal, or null
  double *T_out;            // [count][pose_w]: the compact pose rows, as retry_seed_kernel writes them
  double *T_c;              // [C][count][pose_w]: the same row per candidate, the seed kernel's goal argument
  double *q_c;              // [C][count][n]
  int *ids_c;               // [C][count]: scene_id[goal] per candidate; written only where scene_id is given
  double spread;
  uint64_t seed;
  int count, pose_w, n, attempt, candidates;
};

struct RetryPickArgs {
  const double *cl;         // [C][count] clearance of every candidate
  const double *q_c;        // [C][count][n]
  double *q_out;            // [count][n]: the picked candidate's angles
  int *pick;                // [count], or null
  double *pick_clearance;   // [count], or null
  double clear_tol;
  int count, n, candidates;
};

// splitmix64 finaliser over the counter of (goal, attempt, joint): 53 uniform bits in [0, 1)
__host__ __device__ inline double retry_uniform(uint64_t seed, uint64_t goal, int attempt, int joint) {
  const uint64_t c = (goal * 64u + (uint64_t)attempt) * 128u + (uint64_t)joint + 1u;
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * c;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return (double)(z >> 11) * 0x1p-53;
}

__global__ void __launch_bounds__(RETRY_WAVE) retry_select_kernel(RetrySelectArgs a)
#ifndef GIK_DEFINE_RETRY_KERNELS
    ;      // (defined in gik_k_retry.hip)
#else
{
  const int b = blockIdx.x * RETRY_WAVE + threadIdx.x, lane = threadIdx.x;
  bool failed = false;
  if (b < a.B)
    failed = retry_failed(a.stats[b].stop, a.pos_err[b], a.rot_err[b], a.clearance ? a.clearance[b] : __builtin_huge_val(), a.tol);
  const unsigned long long mask = __ballot(failed);
  if (mask == 0) return;
  int base = 0;
  if (lane == 0) base = atomicAdd(a.count, __popcll(mask));
  base = __shfl(base, 0);
  if (failed) a.idx[base + __popcll(mask & ((1ull << lane) - 1ull))] = b;
}
#endif

__global__ void __launch_bounds__(RETRY_WAVE) retry_seed_kernel(RetrySeedArgs a)
#ifndef GIK_DEFINE_RETRY_KERNELS
    ;
#else
{
  const int lane = threadIdx.x;
  const bool local = a.spread > 0.0;
  for (int r = blockIdx.x; r < a.count; r += gridDim.x) {
    const int g = a.idx[r];
    const double *src = a.T_goal + (size_t)g * a.pose_w;
    double *dst = a.T_out + (size_t)r * a.pose_w;
    for (int e = lane; e < a.pose_w; e += RETRY_WAVE) dst[e] = src[e];
    for (int j = lane; j < a.n; j += RETRY_WAVE) {
      const double u = retry_uniform(a.seed, (uint64_t)g, a.attempt, j);
      const double c = local ? a.q_center[(size_t)g * a.n + j] : 0.0;
      a.q_out[(size_t)r * a.n + j] = retry_seed_value(u, a.q_lo[j], a.q_hi[j], c, a.spread);
    }
  }
}
#endif

__global__ void __launch_bounds__(RETRY_WAVE) retry_candidate_kernel(RetryCandidateArgs a)
#ifndef GIK_DEFINE_RETRY_KERNELS
    ;
#else
{
  const int lane = threadIdx.x;
  const bool local = a.spread > 0.0;
  for (int r = blockIdx.x; r < a.count; r += gridDim.x) {
    const int g = a.idx[r];
    const double *src = a.T_goal + (size_t)g * a.pose_w;
    double *dst = a.T_out + (size_t)r * a.pose_w;
    for (int e = lane; e < a.pose_w; e += RETRY_WAVE) dst[e] = src[e];
    for (int c = 0; c < a.candidates; ++c) {
      const size_t m = (size_t)c * a.count + r;
      const uint64_t seed_c = retry_candidate_seed(a.seed, c);
      for (int e = lane; e < a.pose_w; e += RETRY_WAVE) a.T_c[m * a.pose_w + e] = src[e];
      for (int j = lane; j < a.n; j += RETRY_WAVE) {
        const double u = retry_uniform(seed_c, (uint64_t)g, a.attempt, j);
        const double ctr = local ? a.q_center[(size_t)g * a.n + j] : 0.0;
        a.q_c[m * a.n + j] = retry_seed_value(u, a.q_lo[j], a.q_hi[j], ctr, a.spread);
      }
      if (a.scene_id && lane == 0) a.ids_c[m] = a.scene_id[g];
    }
  }
}
#endif

__global__ void __launch_bounds__(RETRY_WAVE) retry_pick_kernel(RetryPickArgs a)
#ifndef GIK_DEFINE_RETRY_KERNELS
    ;
#else
{
  const int lane = threadIdx.x;
  for (int r = blockIdx.x; r < a.count; r += gridDim.x) {
    // every lane takes the same pick from the same loads
    const int c = retry_pick(a.cl + r, a.candidates, (size_t)a.count, a.clear_tol);
    const size_t m = (size_t)c * a.count + r;
    for (int j = lane; j < a.n; j += RETRY_WAVE) a.q_out[(size_t)r * a.n + j] = a.q_c[m * a.n + j];
    if (lane == 0) {
      if (a.pick) a.pick[r] = c;
      if (a.pick_clearance) a.pick_clearance[r] = a.cl[m];
    }
  }
}
#endif

__global__ void __launch_bounds__(RETRY_WAVE) retry_merge_kernel(RetryMergeArgs a)
#ifndef GIK_DEFINE_RETRY_KERNELS
    ;
#else
{
  const int lane = threadIdx.x;
  for (int r = blockIdx.x; r < a.count; r += gridDim.x) {
    const int g = a.idx[r];
    // every lane takes the same decision from the same loads
    const double pn = a.pos_r[r], rn = a.rot_r[r], cn = a.clear_r ? a.clear_r[r] : __builtin_huge_val();
    const bool better = retry_better(a.stats_r[r].stop, pn, rn, cn, a.stats[g].stop, a.pos_err[g], a.rot_err[g],
                                     a.clearance ? a.clearance[g] : __builtin_huge_val(), a.tol);
    __syncthreads();      // (the incumbent is read by all lanes before any lane overwrites it)
    if (!better) continue;
    const double *Ys = a.Y_r + (size_t)r * a.row;
    double *Yd = a.Y + (size_t)g * a.row;
    for (int e = lane; e < a.row; e += RETRY_WAVE) Yd[e] = Ys[e];
    for (int j = lane; j < a.n; j += RETRY_WAVE) a.q[(size_t)g * a.n + j] = a.q_r[(size_t)r * a.n + j];
    constexpr int SW = sizeof(gik_stats) / sizeof(double);      // the 48-byte record as six 8-byte words
    static_assert(sizeof(gik_stats) == 48 && alignof(gik_stats) == 8, "gik_stats layout");
    const double *ss = reinterpret_cast<const double *>(a.stats_r + r);
    double *sd = reinterpret_cast<double *>(a.stats + g);
    if (lane < SW) sd[lane] = ss[lane];
    if (lane == 0) {
      a.pos_err[g] = pn;
      a.rot_err[g] = rn;
      if (a.clearance) a.clearance[g] = cn;
      a.attempt[g] = a.attempt_no;
    }
  }
}
#endif

}  // namespace gik
