// graphik_amd/csrc/gik_npt_kernels.hip.h -- the kernels of the node-per-lane family (NptCtx, gik_npt.hip.h), as templates:
// rtr_npt_kernel, kat_npt_kernel.  Instantiated in gik_k_npt.hip and gik_k_npt4.hip (gik_instances.h).
#pragma once

#include <hip/hip_runtime.h>

#include "gik_args.h"
#include "gik_npt.hip.h"
#include "gik_rtrv.hip.h"
#include "gik_sched.hip.h"

namespace gik {

// node-per-lane variants (graphs with N*k > 64, k = 3): a lane owns whole graph nodes with all their
// components (gik_npt.hip.h), driver over a small vector per thread (gik_rtrv.hip.h).  <TL, 1, 2>: one
// node per lane, two wavefronts (128 threads) per problem; <TL, 2, 1>: two nodes per lane, one
// wavefront per problem.  Persistent; problems are claimed from the same ticket counter / re-queue
// ring as the workgroup kernel's (FIFO time slicing: the long problems, unknown in advance, must
// not be the last to START).  LDS-bound at three problems per CU on the table scene.
template <int TL, int NS, int NW, bool CTG = false>
__global__ void __launch_bounds__(WAVE * NW, 1) rtr_npt_kernel(SolveArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int sh_claim[2];
  using Ctx = NptCtx<TL, NS, NW, CTG>;
  const int tid = threadIdx.x;
  const int NK = a.N * 3;
  Ctx cx;
  cx.init(a.nt, smem, CTG ? a.npt_ctg_ws + (size_t)blockIdx.x * Ctx::ctg_doubles(a.nt.n_pairs) : nullptr);
  int pass = 0;
  for (;;) {
    int b = 0, resumed = 0;
    if (a.dbg & 1) {      // static block -> problem map (keeps the claim below a scalar-branch loop, see rcg_wave_kernel)
      b = (int)blockIdx.x + pass * (int)gridDim.x;
      ++pass;
      if (b >= a.B) b = -1;
    } else if constexpr (NW == 1) {
      if (tid == 0) b = claim_work(a.work_counter, a.q_seq, a.q_ids, a.q_done, a.B, a.slice_its > 0, resumed);
      b = __builtin_amdgcn_readlane(b, 0);
      resumed = __builtin_amdgcn_readlane(resumed, 0);
    } else {
      if (tid == 0) {
        int res = 0;
        sh_claim[0] = claim_work(a.work_counter, a.q_seq, a.q_ids, a.q_done, a.B, a.slice_its > 0, res);
        sh_claim[1] = res;
      }
      __syncthreads();
      b = __builtin_amdgcn_readfirstlane(sh_claim[0]);
      resumed = __builtin_amdgcn_readfirstlane(sh_claim[1]);
      __syncthreads();
    }
    if (UNI(b < 0)) break;
    cx.load_problem(a.targets + (size_t)b * a.T, a.nt);
    // (unconditional load of the resume state from a zeroed array: a conditional one makes the solver's
    // counters divergent -- NOTEBOOK 8.3)
    RtrResume rs = {0.0, 0, 0, 0, 0, 0, 0};
    if (a.slice_its > 0) {
      rs = load_slice_state(&a.q_state[b]);
      rs.resumed = resumed;
    }
    const double *src = resumed ? a.Y_out : a.Y_init;
    double x[Ctx::NE];
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int q = 0; q < 3; ++q)
        x[3 * s + q] = cx.live[s] ? __builtin_nontemporal_load(&src[(size_t)b * NK + cx.gnode[s] * 3 + q]) : 0.0;
    RtrOut ro;
    rtr_solve_vec<true, true>(cx, a.p, a.trace, a.has_trace, a.dbg, a.dbg_buf, b, x, ro, rs, a.slice_its);
#pragma unroll
    for (int s = 0; s < NS; ++s)
      if (cx.live[s]) {
#pragma unroll
        for (int q = 0; q < 3; ++q) a.Y_out[(size_t)b * NK + cx.gnode[s] * 3 + q] = x[3 * s + q];
      }
    if (UNI(ro.paused)) {
      if (tid == 0) {
        a.q_state[b] = slice_state_of(ro, rs.resumes + 1);
      }
      __threadfence();
      Ctx::block_sync();
      if (tid == 0) requeue_work(a.q_tail, a.q_ids, a.q_seq, a.B, b);
      continue;
    }
    if (tid == 0) {
      a.stats[b] = stats_of(ro, cx.lowrank ? 1 : 0);
      if (a.slice_its > 0) __hip_atomic_fetch_add(a.q_done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <int TL, int NS, int NW, bool CTG = false>
__global__ void __launch_bounds__(WAVE * NW, 1) kat_npt_kernel(KatArgs a) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  using Ctx = NptCtx<TL, NS, NW, CTG>;
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int NK = a.N * 3;
  Ctx cx;
  cx.init(a.nt, smem, CTG ? a.npt_ctg_ws + (size_t)blockIdx.x * Ctx::ctg_doubles(a.nt.n_pairs) : nullptr);
  cx.load_problem(a.targets ? a.targets + (size_t)b * a.T : nullptr, a.nt);
  double y[Ctx::NE], w[Ctx::NE], res[Ctx::NE];
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const size_t at = (size_t)b * NK + (cx.live[s] ? cx.gnode[s] : 0) * 3 + q;
      y[3 * s + q] = cx.live[s] ? a.Y[at] : 0.0;
      w[3 * s + q] = (a.W && cx.live[s]) ? a.W[at] : 0.0;
      res[3 * s + q] = 0.0;
    }
  const double f = cx.cost(y);
  if (a.mode == 0) {
    if (tid == 0) a.out[b] = f;
    return;
  }
  if (a.mode == 4 && tid == 0) a.out_f[b] = f;
  cx.commit(y, res);
  if (a.mode == 2) {
    cx.ehess(w, res);
  } else if (a.mode == 3) {     // PSDFixedRank.proj: Z - Q Q^T Z
    cx.proj_setup(y);
    double v[3], u[3];
    cx.vert_dots(w, v[0], v[1], v[2]);
    cx.template sum_n<3>(v);
    cx.vert_coords(v, u);
    cx.vert_apply(u, w, res);
  }
#pragma unroll
  for (int s = 0; s < NS; ++s)
    if (cx.live[s]) {
#pragma unroll
      for (int q = 0; q < 3; ++q) a.out[(size_t)b * NK + cx.gnode[s] * 3 + q] = res[3 * s + q];
    }
}

}  // namespace gik
