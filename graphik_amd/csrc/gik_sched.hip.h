// graphik_amd/csrc/gik_sched.hip.h -- how the persistent solve kernels get their work: the ticket counter and the re-queue
// ring of the time slicing (claim_work, requeue_work, the paused state of SliceState), the helper side of the tail
// spreading (mig_wait; MigCtl is gik_rtr.hip.h's) and, in the developer build, the event log of the scheduling probes.
// Device functions only; the queues themselves are fields of SolveArgs (gik_args.h).
#pragma once

#include <hip/hip_runtime.h>

#include "gik_args.h"
#include "gik_rtr.hip.h"

namespace gik {

// Claim the next piece of work for this wave / workgroup (called by one thread).  Returns the
// problem index, or -1 when every problem of the launch has finished.
__device__ inline int claim_work(unsigned int *ticket_counter, const unsigned int *q_seq, const int *q_ids,
                                 const unsigned int *q_done, int B, int slicing, int &resumed) {
  const unsigned int ticket = atomicAdd(ticket_counter, 1u);
  resumed = 0;
  if (ticket < (unsigned)B) return (int)ticket;
  if (!slicing) return -1;
  const unsigned int t = ticket - (unsigned)B;
  for (;;) {
    if (__hip_atomic_load(&q_seq[t], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == ticket) break;
    if (__hip_atomic_load(q_done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= (unsigned)B) return -1;
    __builtin_amdgcn_s_sleep(32);
  }
  resumed = 1;
  return __hip_atomic_load(&q_ids[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (cache-bypassing loads: the state was written by another CU; the acquire in claim_work was one
// thread's)
// The values are the same in every lane; readfirstlane moves them to scalar registers, where the
// solver's counters live (as vector loads they would occupy VGPRs for the whole solve -- enough
// to push the 9-slot kernel over 256 registers and into scratch).
__device__ inline int uniform_i32(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ inline double uniform_f64(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)),
                          __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
__device__ inline RtrResume load_slice_state(const SliceState *st) {
  RtrResume rs;
  rs.Delta = uniform_f64(__builtin_nontemporal_load(&st->Delta));
  rs.kiter = uniform_i32(__builtin_nontemporal_load(&st->kiter));
  rs.inner_total = uniform_i32(__builtin_nontemporal_load(&st->inner_total));
  rs.inner_exec = uniform_i32(__builtin_nontemporal_load(&st->inner_exec));
  rs.n_accept = uniform_i32(__builtin_nontemporal_load(&st->n_accept));
  rs.resumes = uniform_i32(__builtin_nontemporal_load(&st->resumes));
  rs.resumed = 1;
  return rs;
}
// ... what a paused problem leaves there (resumes: counting this pause), and what a finished one reports
__device__ __forceinline__ SliceState slice_state_of(const RtrOut &ro, int resumes) {
  SliceState st;
  st.Delta = ro.Delta;
  st.kiter = ro.iterations;
  st.inner_total = ro.inner_total;
  st.inner_exec = ro.inner_executed;
  st.n_accept = ro.n_accept;
  st.resumes = resumes;
  st.pad = 0;
  return st;
}
__device__ __forceinline__ gik_stats stats_of(const RtrOut &ro, int flags) {
  gik_stats s;
  s.f = ro.f;
  s.gradnorm = ro.gradnorm;
  s.iterations = ro.iterations;
  s.inner_total = ro.inner_total;
  s.stop = ro.stop;
  s.n_accept = ro.n_accept;
  s.inner_executed = ro.inner_executed;
  s.flags = flags;
  s.stepsize = ro.Delta;
  return s;
}

// publish a paused problem (one thread; the state stores of all threads must be complete and
// fenced before the call)
__device__ inline void requeue_work(unsigned int *q_tail, int *q_ids, unsigned int *q_seq, int B, int b) {
  const unsigned int t = atomicAdd(q_tail, 1u);
  __hip_atomic_store(&q_ids[t], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&q_seq[t], (unsigned)B + t, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// This wave's physical SIMD: XCC_ID[3:0] and the SIMD / CU / SH / SE fields of HW_ID (bits 4-5 and
// 8-15; the wave slot, pipe and queue fields in between and above say nothing about the place).
__device__ inline int hw_simd_id() {
  const unsigned hw = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (15 << 11));    // HW_REG_HW_ID[15:0]
  const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));   // HW_REG_XCC_ID[3:0]
  return (int)(((hw >> 4) & 3u) | (((hw >> 8) & 0xffu) << 2) | (xcc << 10));
}

// Helper side of the tail spreading (MigCtl, gik_rtr.hip.h), one thread: wait until every problem is
// done (-> -1) or a paused problem is handed to this wave (-> its index).  The wave first has to
// find its SIMD empty and reserve it; while the SIMD is busy with the partner wave's problem it
// polls slowly.
// (-2: the yield queue of the round-robin slicing has an entry again -- the caller goes back to it; a
// helper only commits to a hand-over ticket while that queue is empty.)
__device__ inline int mig_wait(const MigCtl &m, unsigned int *q_head, const unsigned int *q_seq, const int *q_ids,
                               const unsigned int *q_done, int B) {
  for (;;) {
    if (__hip_atomic_load(q_done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= (unsigned)B) return -1;
    if (__hip_atomic_load(m.y_avail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0) return -2;
    int expect = 0;
    // (commit to a hand-over only in the tail: while there are more unfinished problems than waves the
    // yield queue refills at once)
    if ((unsigned)B <= __hip_atomic_load(q_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + (unsigned)m.waves &&
        __hip_atomic_load(&m.simd_run[m.sid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 &&
        __hip_atomic_compare_exchange_strong(&m.simd_run[m.sid], &expect, 1, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT)) {
      const unsigned int t = __hip_atomic_fetch_add(q_head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_add(m.credits, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      for (;;) {
        if (__hip_atomic_load(&q_seq[t], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)B + t)
          return __hip_atomic_load(&q_ids[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (__hip_atomic_load(q_done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) >= (unsigned)B) return -1;
        __builtin_amdgcn_s_sleep(64);
      }
    }
    for (int i = 0; i < 2; ++i) __builtin_amdgcn_s_sleep(127);   // ~7 us
  }
}

#ifdef GIK_DEV
// event log of the scheduling probes: dbg_buf[8] = entries, entry e at 16 + 4 e = {time in 10 ns, wave, type, problem}
__device__ inline void dev_log(double *buf, int type, int b) {
  const int e = (int)atomicAdd(&buf[8], 1.0);
  if (e >= 250000) return;
  double *p = buf + 16 + 4 * (size_t)e;
  p[0] = (double)__builtin_amdgcn_s_memrealtime();
  p[1] = (double)blockIdx.x;
  p[2] = (double)type;
  p[3] = (double)b;
}
#endif

}  // namespace gik
