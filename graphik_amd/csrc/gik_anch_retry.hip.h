// graphik_amd/csrc/gik_anch_retry.hip.h -- restarts in the fixed-anchor (obstacle) solve, the device side.
//
// The restart kernels of gik_retry.hip.h with two additions: the failure rule reads the answer's clearance (an
// answer that sits on its goal with a joint point -- or, where the caller hands in the link clearance, any part of a
// link -- inside a sphere has failed), and the seeds can be drawn around a centre
// configuration instead of uniformly inside the joint limits.
//
//   anch_retry_select_kernel : one thread per goal: failed goals -> a compact index list (wave ballot, one atomic
//                              per wavefront; the order of the list is whatever the atomics make it).
//   anch_retry_seed_kernel   : one wavefront per compact slot: the goal's pose rows and n joint angles.  spread == 0:
//                              the bits of retry_seed_kernel.  spread > 0: q = clamp(c + spread (2u - 1), lo, hi) around
//                              the centre row of the GOAL (not of the slot), same u.  Mirrored bit for bit by
//                              graphik_amd.solvers.riemannian_solver.retry_seeds_host.
//   anch_retry_merge_kernel  : one wavefront per compact slot: the restart's answer -- full point row, stats, q, both
//                              errors and the clearance -- replaces the goal's incumbent if and only if it is better.
// The rule and the seed formula are __host__ __device__ functions, so that a host program can walk them.
// Plain kernels, defined where GIK_DEFINE_ANCH_RETRY_KERNELS is set (gik_k_anch_retry.hip); gik_host.hip sees prototypes.
#pragma once

#include "gik_retry.hip.h"

namespace gik {

// failed: by the rule of the plain restarts, or deeper than clear_tol inside a sphere (a masked node, or a link: whichever
// clearance the array holds)
// (written so that a NaN clearance counts as failed; +inf -- no obstacle, no masked node -- never fails a goal)
__host__ __device__ inline bool anch_retry_failed(int stop, double pos_err, double rot_err, double clearance, double pos_tol,
                                                  double rot_tol, double clear_tol) {
  return retry_failed(stop, pos_err, rot_err, pos_tol, rot_tol) || !(clearance >= -clear_tol);
}

// the larger of the pose score and the penetration depth in units of clear_tol; a NaN scores +inf, so it never wins
__host__ __device__ inline double anch_retry_score(double pos_err, double rot_err, double clearance, double pos_tol,
                                                   double rot_tol, double clear_tol) {
  if (clearance != clearance) return __builtin_huge_val();
  const double s = retry_score(pos_err, rot_err, pos_tol, rot_tol);
  const double depth = (clearance < 0.0 ? -clearance : 0.0) / clear_tol;
  return s > depth ? s : depth;
}

struct AnchRetryTol {
  double pos_tol, rot_tol, clear_tol;
};

// does the restart's answer (_r) replace the incumbent (_i)?  A tie keeps the incumbent.
__host__ __device__ inline bool anch_retry_better(int stop_r, double pos_r, double rot_r, double clear_r, int stop_i,
                                                  double pos_i, double rot_i, double clear_i, AnchRetryTol t) {
  const bool ok_r = !anch_retry_failed(stop_r, pos_r, rot_r, clear_r, t.pos_tol, t.rot_tol, t.clear_tol);
  const bool ok_i = !anch_retry_failed(stop_i, pos_i, rot_i, clear_i, t.pos_tol, t.rot_tol, t.clear_tol);
  return (ok_r && !ok_i) || (ok_r == ok_i && anch_retry_score(pos_r, rot_r, clear_r, t.pos_tol, t.rot_tol, t.clear_tol) <
                                                 anch_retry_score(pos_i, rot_i, clear_i, t.pos_tol, t.rot_tol, t.clear_tol));
}

// one seed angle.  u = retry_uniform(seed, goal, attempt, joint).  spread == 0: lo + u (hi - lo), the bits of
// retry_seed_kernel.  spread > 0: t = 2u - 1 is exact (u is a 53-bit fraction), then one rounded product and one
// rounded sum, clamped to the limits; a NaN centre passes both comparisons and comes out as NaN.
__host__ __device__ inline double anch_retry_seed_value(double u, double lo, double hi, double center, double spread) {
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

struct AnchRetrySelectArgs {
  const gik_stats *stats;   // [B]
  const double *pos_err;    // [B]
  const double *rot_err;    // [B]
  const double *clearance;  // [B]
  AnchRetryTol tol;
  int *idx;                 // [B] out: the failed goals, compact
  int *count;               // [1] in: 0, out: how many
  int B;
};

struct AnchRetrySeedArgs {
  const double *T_goal;     // [B][pose_w]
  const int *idx;           // [count]
  const double *q_lo, *q_hi;   // [n]
  const double *q_center;   // [B][n], indexed by goal; read only if spread > 0
  double *T_out;            // [count][pose_w]
  double *q_out;            // [count][n]
  double spread;
  uint64_t seed;
  int count, pose_w, n, attempt;
};

struct AnchRetryMergeArgs {
  const int *idx;           // [count] distinct goals
  // the restart's answers, compact
  const double *Y_r;        // [count][row]  row = full_N 3
  const gik_stats *stats_r; // [count]
  const double *q_r;        // [count][n]
  const double *pos_r, *rot_r, *clear_r;   // [count]
  // the incumbents
  double *Y;                // [B][row]
  gik_stats *stats;         // [B]
  double *q;                // [B][n]
  double *pos_err, *rot_err, *clearance;   // [B]
  int *attempt;             // [B]
  AnchRetryTol tol;
  int count, row, n, attempt_no;
};

__global__ void __launch_bounds__(RETRY_WAVE) anch_retry_select_kernel(AnchRetrySelectArgs a)
#ifndef GIK_DEFINE_ANCH_RETRY_KERNELS
    ;      // (defined in gik_k_anch_retry.hip)
#else
{
  const int b = blockIdx.x * RETRY_WAVE + threadIdx.x, lane = threadIdx.x;
  bool failed = false;
  if (b < a.B)
    failed = anch_retry_failed(a.stats[b].stop, a.pos_err[b], a.rot_err[b], a.clearance[b], a.tol.pos_tol, a.tol.rot_tol,
                               a.tol.clear_tol);
  const unsigned long long mask = __ballot(failed);
  if (mask == 0) return;
  int base = 0;
  if (lane == 0) base = atomicAdd(a.count, __popcll(mask));
  base = __shfl(base, 0);
  if (failed) a.idx[base + __popcll(mask & ((1ull << lane) - 1ull))] = b;
}
#endif

__global__ void __launch_bounds__(RETRY_WAVE) anch_retry_seed_kernel(AnchRetrySeedArgs a)
#ifndef GIK_DEFINE_ANCH_RETRY_KERNELS
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
      a.q_out[(size_t)r * a.n + j] = anch_retry_seed_value(u, a.q_lo[j], a.q_hi[j], c, a.spread);
    }
  }
}
#endif

__global__ void __launch_bounds__(RETRY_WAVE) anch_retry_merge_kernel(AnchRetryMergeArgs a)
#ifndef GIK_DEFINE_ANCH_RETRY_KERNELS
    ;
#else
{
  const int lane = threadIdx.x;
  for (int r = blockIdx.x; r < a.count; r += gridDim.x) {
    const int g = a.idx[r];
    // every lane takes the same decision from the same loads
    const double pn = a.pos_r[r], rn = a.rot_r[r], cn = a.clear_r[r];
    const bool better = anch_retry_better(a.stats_r[r].stop, pn, rn, cn, a.stats[g].stop, a.pos_err[g], a.rot_err[g],
                                          a.clearance[g], a.tol);
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
      a.clearance[g] = cn;
      a.attempt[g] = a.attempt_no;
    }
  }
}
#endif

}  // namespace gik
