// graphik_amd/csrc/gik_block_kernels.hip.h -- the kernels of the workgroup-per-problem family (BlockCtx, gik_block.hip.h),
// as templates: rtr_block_kernel, rcg_block_kernel, kat_block_kernel.  Instantiated in gik_k_block.hip (gik_instances.h).
#pragma once

#include <hip/hip_runtime.h>

#include "gik_args.h"
#include "gik_block.hip.h"
#include "gik_rcg.hip.h"
#include "gik_rtr.hip.h"
#include "gik_sched.hip.h"

namespace gik {

// workgroup-per-problem variants (graphs with N*k > 64)
template <int K>
__device__ inline uint32_t *block_stage(BlockCtx<K> &cx, double *smem, const uint32_t *g_slots, int N,
                                        const BlockTabs &bt, int SL) {
  const int tid = threadIdx.x;
  const int T = bt.Tc;
  for (int t = tid; t < 3 * BLOCK_MAXN * BlockCtx<K>::RS; t += BLOCK_NT) smem[t] = 0.0;
  double *tg = smem + 3 * BLOCK_MAXN * BlockCtx<K>::RS;
  uint32_t *slots =
      reinterpret_cast<uint32_t *>(tg + ((T + 1) & ~1) + 2 * 8 * BLOCK_WAVES + CLQ_NMOM * BLOCK_WAVES + CLQ_NCQ +
                                   32 * BLOCK_WAVES);
  for (int s = 0; s < SL; ++s) slots[s * BLOCK_NT + tid] = g_slots[s * BLOCK_NT + tid];
  cx.init(N, SL, bt, smem, slots, T);
  if constexpr (K == 3) {   // pair ids of every thread's clique partners (launch invariant)
    unsigned short *pid = const_cast<unsigned short *>(cx.sh_pid);
    for (int m = 0; m < cx.M_clq; ++m) pid[m * BLOCK_NT + tid] = bt.clq_pid_t[m * BLOCK_NT + tid];
  }
  __syncthreads();
  return slots;
}

template <int K>
__global__ void __launch_bounds__(BLOCK_NT) rtr_block_kernel(SolveArgs a, int SL) {
  // 16-byte alignment matters: the static `sh_b` below would otherwise push the dynamic segment
  // to offset 8, and every ds_read_b128 of a point row would be misaligned (measured 5x slower)
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int sh_b, sh_resumed;
  const int tid = threadIdx.x;
  const int NK = a.N * K;
  BlockCtx<K> cx;
  block_stage<K>(cx, smem, a.slot_meta, a.N, a.bt, SL);
  double *sh_tgt = smem + 3 * BLOCK_MAXN * BlockCtx<K>::RS;
  for (;;) {
    if (tid == 0) {
      int res = 0;
      sh_b = claim_work(a.work_counter, a.q_seq, a.q_ids, a.q_done, a.B, a.slice_its > 0, res);
      sh_resumed = res;
    }
    __syncthreads();
    const int b = sh_b, resumed = sh_resumed;
    __syncthreads();
    if (UNI(b < 0)) break;
    cx.load_problem(a.targets + (size_t)b * a.T, a.bt, sh_tgt);
    RtrResume rs = {0.0, 0, 0, 0, 0, 0, 0};
    double x = 0.0;
    if (resumed) {
      rs = load_slice_state(&a.q_state[b]);
      if (cx.active) x = __builtin_nontemporal_load(&a.Y_out[(size_t)b * NK + cx.gnode * K + cx.part]);
    } else if (cx.active) {
      x = a.Y_init[(size_t)b * NK + cx.gnode * K + cx.part];
    }
    RtrOut ro;
#ifdef GIK_BLK_PROF
    cx.prof = ((a.dbg & 8) && b == 0) ? a.dbg_buf : nullptr;
#endif
    rtr_solve_one<K, false, true>(cx, a.p, a.trace, a.has_trace, a.dbg, a.dbg_buf, b, x, ro, rs, a.slice_its);
    if (cx.active) a.Y_out[(size_t)b * NK + cx.gnode * K + cx.part] = x;
    if (UNI(ro.paused)) {
      if (tid == 0) {
        a.q_state[b] = slice_state_of(ro, rs.resumes + 1);
      }
      __threadfence();
      __syncthreads();
      if (tid == 0) requeue_work(a.q_tail, a.q_ids, a.q_seq, a.B, b);
      continue;
    }
    if (tid == 0) {
      a.stats[b] = stats_of(ro, cx.lowrank ? 1 : 0);
      if (a.slice_its > 0) __hip_atomic_fetch_add(a.q_done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

template <int K>
__global__ void __launch_bounds__(BLOCK_NT) rcg_block_kernel(SolveArgs a, int SL) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  __shared__ int sh_b;
  const int tid = threadIdx.x;
  const int NK = a.N * K;
  BlockCtx<K> cx;
  block_stage<K>(cx, smem, a.slot_meta, a.N, a.bt, SL);
  double *sh_tgt = smem + 3 * BLOCK_MAXN * BlockCtx<K>::RS;
  for (;;) {
    if (tid == 0) sh_b = (int)atomicAdd(a.work_counter, 1u);
    __syncthreads();
    const int b = sh_b;
    __syncthreads();
    if (UNI(b >= a.B)) break;
    cx.load_problem(a.targets + (size_t)b * a.T, a.bt, sh_tgt);
    double x = cx.active ? a.Y_init[(size_t)b * NK + cx.gnode * K + cx.part] : 0.0;
    RtrOut ro;
    rcg_solve_one<K>(cx, a.cg, a.trace, a.has_trace, b, x, ro);
    if (cx.active) a.Y_out[(size_t)b * NK + cx.gnode * K + cx.part] = x;
    if (tid == 0) {
      a.stats[b] = stats_of(ro, cx.lowrank ? 1 : 0);
    }
  }
}

template <int K>
__global__ void __launch_bounds__(BLOCK_NT) kat_block_kernel(KatArgs a, int SL) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int NK = a.N * K;
  BlockCtx<K> cx;
  block_stage<K>(cx, smem, a.slot_meta, a.N, a.bt, SL);
  double *sh_tgt = smem + 3 * BLOCK_MAXN * BlockCtx<K>::RS;
  cx.load_problem(a.targets ? a.targets + (size_t)b * a.T : nullptr, a.bt, sh_tgt);
  const size_t at = (size_t)b * NK + cx.gnode * K + cx.part;
  const double y = cx.active ? a.Y[at] : 0.0;
  const double w = (a.W && cx.active) ? a.W[at] : 0.0;
  const double f = cx.cost(y);
  if (a.mode == 0) {
    if (tid == 0) a.out[b] = f;
    return;
  }
  if (a.mode == 4 && tid == 0) a.out_f[b] = f;
  double res = cx.commit();
  if (a.mode == 2) {
    res = cx.ehess(w);
  } else if (a.mode == 3) {
    cx.proj_setup(a.planar_proj_exact);
    res = cx.proj(w);
  }
  if (cx.active) a.out[at] = res;
}

}  // namespace gik
