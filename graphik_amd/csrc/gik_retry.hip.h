// graphik_amd/csrc/gik_retry.hip.h -- restarts from random joint configurations, the device side.
//
//   retry_select_kernel : one thread per goal: failed goals -> a compact index list (wave ballot, one atomic
//                         per wavefront; the order of the list is whatever the atomics make it).
//   retry_seed_kernel   : one wavefront per compact slot: the goal's pose rows and n joint angles drawn
//                         uniformly inside the joint limits by a counter-based generator -- a function of
//                         (seed, goal, attempt, joint) only, mirrored bit for bit by
//                         graphik_amd.solvers.riemannian_solver.retry_seeds_host.
//   retry_merge_kernel  : one wavefront per compact slot: the retry's answer replaces the goal's incumbent
//                         if and only if it is better; rows that are not replaced are not written.
// Plain kernels, defined where GIK_DEFINE_RETRY_KERNELS is set (gik_k_retry.hip); gik_host.hip sees prototypes.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "graphik_amd.h"

namespace gik {

constexpr int RETRY_WAVE = 64;

// failed: the solver did not stop on its gradient bar, or an end-effector error is not within its tolerance
// (written so that a NaN error counts as failed)
__host__ __device__ inline bool retry_failed(int stop, double pos_err, double rot_err, double pos_tol, double rot_tol) {
  return stop != 0 || !(pos_err <= pos_tol) || !(rot_err <= rot_tol);
}

// what the merge orders answers of one success class by; a NaN error scores +inf, so it never wins
__host__ __device__ inline double retry_score(double pos_err, double rot_err, double pos_tol, double rot_tol) {
  const double a = pos_err / pos_tol, b = rot_err / rot_tol;
  if (a != a || b != b) return __builtin_huge_val();
  return a > b ? a : b;
}

struct RetrySelectArgs {
  const gik_stats *stats;   // [B]
  const double *pos_err;    // [B]
  const double *rot_err;    // [B]
  double pos_tol, rot_tol;
  int *idx;                 // [B] out: the failed goals, compact
  int *count;               // [1] in: 0, out: how many
  int B;
};

struct RetrySeedArgs {
  const double *T_goal;     // [B][pose_w]  pose_w = n_ee (K+1)^2
  const int *idx;           // [count]
  const double *q_lo, *q_hi;   // [n]
  double *T_out;            // [count][pose_w]
  double *q_out;            // [count][n]
  uint64_t seed;
  int count, pose_w, n, attempt;
};

struct RetryMergeArgs {
  const int *idx;           // [count] distinct goals
  // the retry's answers, compact
  const double *Y_r;        // [count][row]  row = N K
  const gik_stats *stats_r; // [count]
  const double *q_r;        // [count][n]
  const double *pos_r, *rot_r;   // [count]
  // the incumbents
  double *Y;                // [B][row]
  gik_stats *stats;         // [B]
  double *q;                // [B][n]
  double *pos_err, *rot_err;     // [B]
  int *attempt;             // [B]
  double pos_tol, rot_tol;
  int count, row, n, attempt_no;
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
  if (b < a.B) failed = retry_failed(a.stats[b].stop, a.pos_err[b], a.rot_err[b], a.pos_tol, a.rot_tol);
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
#pragma clang fp contract(off)      // q = lo + u (hi - lo): one rounded product, one rounded sum, as numpy forms it
  const int lane = threadIdx.x;
  for (int r = blockIdx.x; r < a.count; r += gridDim.x) {
    const int g = a.idx[r];
    const double *src = a.T_goal + (size_t)g * a.pose_w;
    double *dst = a.T_out + (size_t)r * a.pose_w;
    for (int e = lane; e < a.pose_w; e += RETRY_WAVE) dst[e] = src[e];
    for (int j = lane; j < a.n; j += RETRY_WAVE) {
      const double u = retry_uniform(a.seed, (uint64_t)g, a.attempt, j);
      const double lo = a.q_lo[j], span = a.q_hi[j] - lo;
      const double step = u * span;
      a.q_out[(size_t)r * a.n + j] = lo + step;
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
    const double pn = a.pos_r[r], rn = a.rot_r[r], po = a.pos_err[g], ro = a.rot_err[g];
    const bool ok_new = !retry_failed(a.stats_r[r].stop, pn, rn, a.pos_tol, a.rot_tol);
    const bool ok_old = !retry_failed(a.stats[g].stop, po, ro, a.pos_tol, a.rot_tol);
    const bool better = (ok_new && !ok_old) ||
                        (ok_new == ok_old && retry_score(pn, rn, a.pos_tol, a.rot_tol) < retry_score(po, ro, a.pos_tol, a.rot_tol));
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
      a.attempt[g] = a.attempt_no;
    }
  }
}
#endif

}  // namespace gik
