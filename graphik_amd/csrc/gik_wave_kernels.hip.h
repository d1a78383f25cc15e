// graphik_amd/csrc/gik_wave_kernels.hip.h -- the kernels of the one-wavefront-per-problem family (gfx950), as templates.
// Instantiated in gik_k_wave3.hip, gik_k_wave3_strict.hip, gik_k_wave2.hip, gik_k_anch.hip, gik_k_anch_link.hip,
// gik_k_anch_scene.hip, gik_k_anch_self.hip and gik_k_anch_half.hip (gik_instances.h).
//
//   rtr_wave_kernel : whole Riemannian trust-region solve (TrustRegions.solve +
//                     _truncated_conjugate_gradient, graphik/solvers/trust_region.py:112-599)
//                     of one IK problem per wavefront, one launch per batch.
//   rcg_wave_kernel : the same persistent scheme around Riemannian conjugate gradients.
//   kat_wave_kernel : the same device functions exposed one call at a time, batched
//                     (costgrd twins + PSDFixedRank.proj) for known-answer parity tests.
//   parts_kernel    : developer build only, per-component cycle cost of one wavefront.
#pragma once

#include <hip/hip_runtime.h>

#include "gik_args.h"
#include "gik_rcg.hip.h"
#include "gik_rtr.hip.h"
#include "gik_sched.hip.h"
#include "gik_wave.hip.h"
#ifdef GIK_STRICT_HEADER      // developer experiments (tools/exp/strict_bisect.sh): another rendering of WaveCtxStrict
#include GIK_STRICT_HEADER
#else
#include "gik_wave_strict.hip.h"
#endif

namespace gik {

// Stage the launch-invariant slot table into LDS and zero the gather tiles (idle lanes and
// padding slots read the never-written dump row, which must hold finite zeros).
template <typename Ctx>
__device__ inline void stage_lds(double *tiles, uint32_t *meta, const uint32_t *g_meta, int lane,
                                 int maxdeg, int N) {
  for (int t = lane; t < Ctx::NTILE * Ctx::TILE; t += WAVE) tiles[t] = 0.0;
  if constexpr (Ctx::SLIM_LAYOUT) {
    // slim layout (per-edge context): table row k of a lane is node slot comp + 3 k, the slots the lane OWNS; beyond the
    // compiled slot count: the padding word of the host's table (own row -- idle lanes: the dump row --, kind none)
    const bool active = lane < N * 3;
    const int comp = active ? lane % 3 : 0;
    const uint32_t pad = meta_pack(active ? lane / 3 : TILE_ROWS - 1, 0, 0, 0);
    for (int k = 0; k < Ctx::NSL; ++k) {
      const int s = comp + 3 * k;
      meta[k * WAVE + lane] = s < maxdeg ? g_meta[s * WAVE + lane] : pad;
    }
  } else {
    for (int s = 0; s < maxdeg; ++s) meta[s * WAVE + lane] = g_meta[s * WAVE + lane];
  }
  __builtin_amdgcn_wave_barrier();
}

// Persistent kernel: grid = (resident waves), each wavefront claims IK problems from a global
// counter until the batch is exhausted.  Iteration counts differ by >50x between goals and the
// hardware hands workgroups to XCDs round-robin, so a static block->problem map leaves whole
// XCDs idle behind a few stragglers; the queue keeps every SIMD busy until the end.
// (the fixed-anchor variant holds 34 KB of LDS per wave: four waves per CU, one per SIMD, so it may
// as well have that SIMD's whole register file -- at two waves per SIMD it spilled into the hot loop)
// A build is named by one flag word (rtr_wave_kernel<K, SLOTS, BUILD>, kat_wave_kernel<K, SLOTS, BUILD>):
enum WaveBuild : unsigned {
  W_THETA1 = 1,    // theta == 1, the reference default (without it: any theta)
  W_ANCH = 2,      // the fixed-anchor formulation, k = 3
  W_SPREAD = 4,    // tail spreading (MigCtl): two waves per SIMD, i.e. not the anchored builds
  // the Hessian product term by term as costs.py:186-203 forms it (gik_wave_strict.hip.h;
  // gik_template_desc.hessian_form = GIK_HESS_PER_EDGE), k = 3 free-free graphs
  W_PER_EDGE = 8,
  W_LINKS = 16,    // link hinges in the fixed-anchor solve (WaveCtx<.., LINKS>, gik_anchored_attach_links with hinges = 1)
  W_SELF = 32,     // self hinges in the fixed-anchor solve (WaveCtx<.., SELF>, gik_anchored_attach_self_hinges)
  W_HALF = 64,     // half-space obstacles in the fixed-anchor solve (WaveCtx<.., HALF>, gik_anchored_attach_halfspaces)
};
// the context a build runs on
template <int K, int MAXDEG, unsigned BUILD>
using WaveBuildCtx = std::conditional_t<(BUILD & W_PER_EDGE) != 0, WaveCtxStrict<MAXDEG>,
                                        WaveCtx<K, MAXDEG, (BUILD & W_ANCH) != 0, false, (BUILD & W_LINKS) != 0, (BUILD & W_SELF) != 0,
                                                (BUILD & W_HALF) != 0>>;
// SCENES is not a bit but an entry point, rtr_wave_scene_kernel: per-goal obstacle scenes in the fixed-anchor solve
// (gik_solve_batch_scenes).  The scene set is a second kernel
// argument (SceneArgs, gik_scenes.h; SolveArgs and with it every other kernel stay as they are): a.an.obs is then the
// caller's [n_scene][stride][4] array and a.an.n_obs is not read; problem b walks the first n_obs[s] rows of scene
// s = scene_id[b] (null: scene 0), and the obstacle table in LDS is restaged whenever a claimed problem's scene differs
// from the staged one.  The anchored builds are not
// time-sliced and reset their near lists per problem anyway, and the near lists are exact, so a problem's bits are those
// of a template created with its scene's spheres, whatever the wave staged before.
// The kernel's text is this function; rtr_wave_kernel and rtr_wave_scene_kernel below are its entry points.
template <int K, int MAXDEG, unsigned BUILD, bool SCENES = false>
__device__ __forceinline__ void rtr_wave_run(const SolveArgs &a, const SceneArgs &sc = SceneArgs()) {
  constexpr bool THETA_ONE = BUILD & W_THETA1, ANCH = BUILD & W_ANCH, MIG = BUILD & W_SPREAD, STRICT = BUILD & W_PER_EDGE,
                 LINKS = BUILD & W_LINKS, SELF = BUILD & W_SELF, HALF = BUILD & W_HALF;
  static_assert(!SCENES || ANCH, "scenes: the fixed-anchor kernels");
  static_assert(!HALF || (ANCH && MAXDEG == 9 && !SELF), "half-spaces: the 9-slot fixed-anchor kernel, without self hinges");
  static_assert(!SELF || (ANCH && MAXDEG == 9), "self hinges: the 9-slot fixed-anchor kernel");
  static_assert(!LINKS || (ANCH && MAXDEG == 9), "link hinges: the 9-slot fixed-anchor kernel");
  static_assert(!ANCH || K == 3, "the fixed-anchor formulation is 3-D");
  static_assert(!MIG || !ANCH, "tail spreading: two waves per SIMD, i.e. not the anchored variant");
  static_assert(!STRICT || (K == 3 && !ANCH), "the per-edge product form: 3-D free-free graphs");
  using Ctx = WaveBuildCtx<K, MAXDEG, BUILD>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x;
  const int NK = a.N * K;
  double *sh_tiles = smem;
  double *sh_tgt = smem + Ctx::NTILE * Ctx::TILE;
  uint32_t *sh_meta = reinterpret_cast<uint32_t *>(sh_tgt + ((a.T + 1) & ~1));
  stage_lds<Ctx>(sh_tiles, sh_meta, a.slot_meta, lane, MAXDEG, a.N);

  Ctx cx;
  cx.init(lane, a.N, sh_tiles, sh_tgt, sh_meta);
  if constexpr (ANCH) {
    // every target is a template constant here: records, pinned records and the constant rows of
    // the anchor table are staged once per wave; only the goal anchors change per problem
    // (a scene build starts with no obstacle staged: the first claimed problem brings its scene)
    cx.init_anchored(a.an.obs_mask, a.an.obs, SCENES ? 0 : a.an.n_obs, !(a.dbg & 128));
    if constexpr (LINKS) cx.init_links(a.an.link_rec);
    if constexpr (SELF) cx.init_self(a.an.self_desc);
    if constexpr (HALF) cx.init_half(a.half, a.n_half, a.half_mu, a.N);
    for (int t = lane; t < a.T; t += WAVE) sh_tgt[t] = a.targets[t];
    for (int t = lane; t < 4 * ANCH_MAXA; t += WAVE) cx.sh_anch[t] = a.an.anch_const[t];
    __builtin_amdgcn_wave_barrier();
    cx.load_slot_records();
    cx.load_pinned_records(a.an.pin_meta, a.an.pin_tgt);
  }
  const Params &p = a.p;
  int pass = 0;
  MigCtl mig = {a.mig_credits, a.mig_simd_run, 0, a.work_counter, a.y_avail, a.y_tail, a.B, a.y_cap, a.q_done,
                (int)gridDim.x, a.slice_cycles};
  bool tail = false;
  bool owns_entry = false;    // (lane 0) this wave has just pushed a yielded problem
  int staged_scene = -1;      // (SCENES) the scene whose rows sh_obs holds
  if constexpr (MIG) mig.sid = hw_simd_id();
#ifdef GIK_DEV
  long long dev_t_start = (long long)__builtin_readcyclecounter(), dev_t_solve = 0, dev_t_claim = 0;
  int dev_n_claim = 0;
#endif
  for (;;) {
    int b = 0, resumed = 0;
#ifdef GIK_DEV
    const long long dev_tc = (long long)__builtin_readcyclecounter();
#endif
    if constexpr (MIG) {
      // (the static block -> problem alternative is never selected together with MIG on the host; it
      // is what keeps the compiler's divergence analysis from treating this loop's exit as divergent
      // and wrapping the solver loops in exec masks -- see the note at rcg_wave_kernel)
      if (a.dbg & 1) {
        b = (int)blockIdx.x + pass * (int)gridDim.x;
        ++pass;
        if (b >= a.B) b = -1;
      } else {
        if (lane == 0) {
          b = -1;
          if (!tail) {
            const unsigned int t = atomicAdd(a.work_counter, 1u);
            if (t < (unsigned)a.B) {
              b = (int)t;
              __hip_atomic_fetch_add(&mig.simd_run[mig.sid], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
          }
          if (b >= 0 && owns_entry)      // this wave's yield stays in the queue: somebody else's to take
            __hip_atomic_fetch_add(a.y_avail, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
          if (b < 0) {      // no fresh problem left: the oldest yielder, if any, else a hand-over
            resumed = 1;
            bool pop = owns_entry;
            while (!pop) {
              if (__hip_atomic_load(a.y_avail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 0) {
                if (__hip_atomic_fetch_add(a.y_avail, -1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) > 0) {
                  pop = true;
                  break;
                }
                __hip_atomic_fetch_add(a.y_avail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              }
              b = mig_wait(mig, a.q_head, a.q_seq, a.q_ids, a.q_done, a.B);
              if (b != -2) break;       // a handed-over problem, or -1: everything is done
            }
            if (pop) {
              const unsigned int h = __hip_atomic_fetch_add(a.y_head, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              while (__hip_atomic_load(&a.y_seq[h], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != h + 1u)
                __builtin_amdgcn_s_sleep(2);      // (its publisher is between the tail increment and this store)
              b = __hip_atomic_load(&a.y_ids[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              __hip_atomic_fetch_add(&mig.simd_run[mig.sid], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
          }
          owns_entry = false;
        }
        b = __builtin_amdgcn_readlane(b, 0);  // lane 0 explicitly, independent of exec
        resumed = __builtin_amdgcn_readlane(resumed, 0);
      }
      // a fresh claim's b is its ticket: with a claim order (a permutation of 0 .. B-1) ticket t stands for problem
      // claim_order[t].  Looked up here, on the broadcast value: inside the lane-0 block above the load made the
      // compiler wrap the solver's loops in exec masks (188 -> 207 instructions per tCG step of this build)
      if (a.claim_order && !resumed && b >= 0) b = a.claim_order[b];
      tail = tail || resumed;
#ifdef GIK_DEV
      dev_t_claim += (long long)__builtin_readcyclecounter() - dev_tc;
      ++dev_n_claim;
      if ((a.dbg & 4096) && a.dbg_buf && lane == 0) dev_log(a.dbg_buf, resumed ? 1 : 0, b);
#endif
      if (UNI(b < 0)) break;
    } else {
      // b is the ticket; with a claim order (a permutation of 0 .. B-1) ticket t stands for problem claim_order[t],
      // tickets from B on stay as they are and end the loop.  (Here lane 0 looks it up before the broadcast: a lookup
      // behind the exit test, as in the MIG branch, cost this build 0.7 % of a 4096-goal LWA4D batch in index order.)
      if (a.dbg & 1) {
        b = (int)blockIdx.x + pass * (int)gridDim.x;
        ++pass;
        if (a.claim_order && b < a.B) b = a.claim_order[b];
      } else {
        if (lane == 0) {
          b = (int)atomicAdd(a.work_counter, 1u);
          if (a.claim_order && b < a.B) b = a.claim_order[b];
        }
        b = __builtin_amdgcn_readlane(b, 0);  // lane 0 explicitly, independent of exec
      }
      if (UNI(b >= a.B)) break;
    }

    if constexpr (ANCH) {
      if (lane < 3 * a.an.n_goal)
        cx.sh_anch[(a.an.goal_row0 + lane / 3) * 4 + lane % 3] =
            a.an.anchor_goal[(size_t)b * 3 * a.an.n_goal + lane];
      if constexpr (SCENES) {
        // b is wave-uniform (readlane), so id and count are scalar loads and stay in scalar registers.  Both are clamped:
        // a bad id or count in the caller's arrays reads a wrong scene, never memory outside the scene set or the table.
        const int s = uniform_i32(scene_clamp_id(sc.scene_id ? sc.scene_id[b] : 0, sc.n_scene));
        if (UNI(s != staged_scene)) {
          const int n = uniform_i32(scene_clamp_count(sc.n_obs[s], sc.stride));
          cx.stage_scene(a.an.obs + (size_t)s * (size_t)sc.stride * 4, n);
          staged_scene = s;
        }
      }
      cx.obs_reset();
      if constexpr (LINKS) cx.links_reset();
    } else {
      for (int t = lane; t < a.T; t += WAVE) sh_tgt[t] = a.targets[(size_t)b * a.T + t];
      __builtin_amdgcn_wave_barrier();
      cx.load_slot_records();
    }
    RtrOut ro;
    double x;
    int rs_resumes = 0;
    if constexpr (MIG) {
      // Branch-free on purpose: q_state is zeroed at launch, so a fresh problem reads zeros (a
      // conditional load here made the compiler treat the solver's counters as divergent and wrap
      // its loops in exec masks).  (State and point of a resumed problem were written by a wave on
      // another CU: cache-bypassing loads.)
      RtrResume rs = load_slice_state(&a.q_state[b]);
      rs.resumed = resumed;
      rs_resumes = rs.resumes;
      const double *src = resumed ? a.Y_out : a.Y_init;
      x = cx.active ? __builtin_nontemporal_load(&src[(size_t)b * NK + lane]) : 0.0;
#ifdef GIK_DEV
      const long long dev_ts = (long long)__builtin_readcyclecounter();
#endif
      rtr_solve_one<K, THETA_ONE, true, Ctx, true>(cx, p, a.trace, a.has_trace, a.dbg, a.dbg_buf, b, x, ro, rs,
                                                   a.slice_its, &mig);
#ifdef GIK_DEV
      dev_t_solve += (long long)__builtin_readcyclecounter() - dev_ts;
#endif
      if (cx.active) a.Y_out[(size_t)b * NK + lane] = x;
      if (UNI(ro.paused)) {
        if (lane == 0) {
          a.q_state[b] = slice_state_of(ro, rs.resumes + 1);
        }
        __threadfence();
#ifdef GIK_DEV
        if ((a.dbg & 4096) && a.dbg_buf && lane == 0) dev_log(a.dbg_buf, ro.paused == PAUSE_DONATE ? 3 : 2, b);
#endif
        if (lane == 0) {
          if (ro.paused == PAUSE_DONATE) {
            requeue_work(a.q_tail, a.q_ids, a.q_seq, a.B, b);      // a helper holds the ticket for it
          } else {                                                   // yield: behind everything that waits
            const unsigned int k = atomicAdd(a.y_tail, 1u);
            __hip_atomic_store(&a.y_ids[k], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&a.y_seq[k], k + 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            owns_entry = true;
          }
          __hip_atomic_fetch_add(&mig.simd_run[mig.sid], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (ro.paused == PAUSE_DONATE) tail = true;
        continue;
      }
    } else {
      x = cx.active ? a.Y_init[(size_t)b * NK + lane] : 0.0;
      const RtrResume rs = {0.0, 0, 0, 0, 0, 0, 0};
      rtr_solve_one<K, THETA_ONE, false>(cx, p, a.trace, a.has_trace, a.dbg, a.dbg_buf, b, x, ro, rs, 0);
      if (cx.active) a.Y_out[(size_t)b * NK + lane] = x;
    }
    if (lane == 0) {
      a.stats[b] = stats_of(ro, (MIG && resumed) ? (2 | (rs_resumes << 8)) : 0);
#ifdef GIK_DEV
      if (MIG && (a.dbg & 4096) && a.dbg_buf) dev_log(a.dbg_buf, 4, b);
#endif
      if constexpr (MIG) {
        __hip_atomic_fetch_add(&mig.simd_run[mig.sid], -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(a.q_done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }
#ifdef GIK_DEV
  if (MIG && (a.dbg & 4096) && a.dbg_buf && lane == 0) {
    atomicAdd(&a.dbg_buf[4], (double)dev_t_solve);
    atomicAdd(&a.dbg_buf[5], (double)dev_t_claim);
    atomicAdd(&a.dbg_buf[6], (double)((long long)__builtin_readcyclecounter() - dev_t_start));
    atomicAdd(&a.dbg_buf[7], (double)dev_n_claim);
  }
#endif
}
template <int K, int MAXDEG, unsigned BUILD>
__global__ void __launch_bounds__(WAVE, (BUILD & W_ANCH) ? 1 : 2) rtr_wave_kernel(SolveArgs a) {
  rtr_wave_run<K, MAXDEG, BUILD>(a);
}
// the scene builds of the three fixed-anchor solve kernels (9 slots, 20 slots, 9 slots with link hinges)
template <int K, int MAXDEG, unsigned BUILD>
__global__ void __launch_bounds__(WAVE, 1) rtr_wave_scene_kernel(SolveArgs a, SceneArgs sc) {
  rtr_wave_run<K, MAXDEG, BUILD, true>(a, sc);
}

// Riemannian conjugate gradients (the reference's alternative solver), same persistent scheme
template <int K, int MAXDEG>
__global__ void __launch_bounds__(WAVE, 2) rcg_wave_kernel(SolveArgs a) {
  using Ctx = WaveCtx<K, MAXDEG>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x;
  const int NK = a.N * K;
  double *sh_tiles = smem;
  double *sh_tgt = smem + Ctx::NTILE * Ctx::TILE;
  uint32_t *sh_meta = reinterpret_cast<uint32_t *>(sh_tgt + ((a.T + 1) & ~1));
  stage_lds<Ctx>(sh_tiles, sh_meta, a.slot_meta, lane, MAXDEG, a.N);
  Ctx cx;
  cx.init(lane, a.N, sh_tiles, sh_tgt, sh_meta);
  int pass = 0;
  for (;;) {
    // Same claim as rtr_wave_kernel, INCLUDING the static block -> problem alternative (dbg & 1).
    // With only the atomic claim in the loop the compiler treats the loop exit as divergent and
    // wraps this loop and the solver loop inside it in exec masks, under which the wave-wide
    // reductions dead-lock (measured: a hang at maxiter = 3; an "+s" asm pin on b does not help).
    // Checked in the ISA: no s_andn2_b64 exec besides the two strided copy loops.
    int b = 0;
    if (a.dbg & 1) {
      b = (int)blockIdx.x + pass * (int)gridDim.x;
      ++pass;
    } else {
      if (lane == 0) b = (int)atomicAdd(a.work_counter, 1u);
      b = __builtin_amdgcn_readlane(b, 0);  // lane 0 explicitly, independent of exec
    }
    if (UNI(b >= a.B)) break;
    for (int t = lane; t < a.T; t += WAVE) sh_tgt[t] = a.targets[(size_t)b * a.T + t];
    __builtin_amdgcn_wave_barrier();
    cx.load_slot_records();
    double x = cx.active ? a.Y_init[(size_t)b * NK + lane] : 0.0;
    RtrOut ro;
    rcg_solve_one<K>(cx, a.cg, a.trace, a.has_trace, b, x, ro);
    if (cx.active) a.Y_out[(size_t)b * NK + lane] = x;
    if (lane == 0) {
      a.stats[b] = stats_of(ro, 0);
    }
  }
}

template <int K, int MAXDEG, unsigned BUILD = 0>
__global__ void __launch_bounds__(WAVE) kat_wave_kernel(KatArgs a) {
  static_assert(!(BUILD & ~(W_ANCH | W_PER_EDGE | W_LINKS | W_SELF | W_HALF)),
                "known answers: the anchored, per-edge, link, self and half-space builds");
  constexpr bool ANCH = BUILD & W_ANCH, LINKS = BUILD & W_LINKS, SELF = BUILD & W_SELF, HALF = BUILD & W_HALF;
  using Ctx = WaveBuildCtx<K, MAXDEG, BUILD>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  const int NK = a.N * K;
  double *sh_tiles = smem;
  double *sh_tgt = smem + Ctx::NTILE * Ctx::TILE;
  uint32_t *sh_meta = reinterpret_cast<uint32_t *>(sh_tgt + ((a.T + 1) & ~1));
  stage_lds<Ctx>(sh_tiles, sh_meta, a.slot_meta, lane, MAXDEG, a.N);
  for (int t = lane; t < a.T; t += WAVE)
    sh_tgt[t] = a.targets ? a.targets[ANCH ? (size_t)t : (size_t)b * a.T + t] : 0.0;
  __builtin_amdgcn_wave_barrier();
  Ctx cx;
  cx.init(lane, a.N, sh_tiles, sh_tgt, sh_meta);
  if constexpr (ANCH) {
    cx.init_anchored(a.an.obs_mask, a.an.obs, a.an.n_obs, true);
    if constexpr (LINKS) cx.init_links(a.an.link_rec);
    if constexpr (SELF) cx.init_self(a.an.self_desc);
    if constexpr (HALF) cx.init_half(a.half, a.n_half, a.half_mu, a.N);
    for (int t = lane; t < 4 * ANCH_MAXA; t += WAVE) cx.sh_anch[t] = a.an.anch_const[t];
    __builtin_amdgcn_wave_barrier();
    if (lane < 3 * a.an.n_goal)
      cx.sh_anch[(a.an.goal_row0 + lane / 3) * 4 + lane % 3] =
          a.an.anchor_goal[(size_t)b * 3 * a.an.n_goal + lane];
    __builtin_amdgcn_wave_barrier();
    cx.load_pinned_records(a.an.pin_meta, a.an.pin_tgt);
  }
  cx.load_slot_records();
  const double y = cx.active ? a.Y[(size_t)b * NK + lane] : 0.0;
  const double w = (a.W && cx.active) ? a.W[(size_t)b * NK + lane] : 0.0;
  if (a.mode == 0) {
    const double f = cx.cost(y);
    if (lane == 0) a.out[b] = f;
    return;
  }
  double res = 0.0;
  if (a.mode == 1) {
    cx.put(y);
    res = cx.commit();
  } else if (a.mode == 4) {
    const double f = cx.cost(y);   // leaves the rows of y in the tiles for commit()
    res = cx.commit();
    if (lane == 0) a.out_f[b] = f;
  } else if (a.mode == 2) {
    cx.put(y);
    (void)cx.commit();
    res = cx.ehess(w);
  } else {
    cx.put(y);
    cx.proj_setup(a.planar_proj_exact);
    res = cx.proj(w);
  }
  if (cx.active) a.out[(size_t)b * NK + lane] = res;
}

// ------------------------------------------------------------------------------------------
// developer micro-benchmark: per-component cycle cost of one wavefront.  Only in the -DGIK_DEV
// build (graphik_amd/build.py --dev -> lib/exp/libgraphik_amd_dev.so); the shipped library has
// neither this kernel nor the gik_debug_* hooks.
#ifdef GIK_DEV
template <int K, int MAXDEG>
__global__ void __launch_bounds__(WAVE) parts_kernel(const uint32_t *slot_meta, int N, int T, int mode,
                                                     int iters, double *out) {
  using Ctx = WaveCtx<K, MAXDEG>;
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int lane = threadIdx.x;
  double *sh_tiles = smem;
  double *sh_tgt = smem + Ctx::NTILE * Ctx::TILE;
  uint32_t *sh_meta = reinterpret_cast<uint32_t *>(sh_tgt + ((T + 1) & ~1));
  stage_lds<Ctx>(sh_tiles, sh_meta, slot_meta, lane, MAXDEG, N);
  for (int t = lane; t < T; t += WAVE) sh_tgt[t] = 1.0 + 0.01 * t;
  Ctx cx;
  cx.init(lane, N, sh_tiles, sh_tgt, sh_meta);
  cx.load_slot_records();
  double x = cx.active ? 0.37 * lane - 0.01 * lane * lane : 0.0;
  (void)cx.cost(x);
  double g = cx.commit();
  cx.proj_setup(0);
  double acc = g, sc = 1.0;
  const long long t0 = __builtin_readcyclecounter();
  if (mode == 0) {
    for (int it = 0; it < iters; ++it) {            // ehess only
      acc = cx.ehess(acc) * 1e-3 + g;
    }
  }
  else if (mode == 1) {
    for (int it = 0; it < iters; ++it) {     // 3-value reduction
      double v[3] = {acc, acc * 0.5, acc * 0.25};
      wave_sum_n<3>(v);
      acc = g + 1e-3 * (v[0] + v[1] + v[2]);
    }
  }
  else if (mode == 2) {
    for (int it = 0; it < iters; ++it) {     // 1-value reduction
      acc = g + 1e-3 * wave_sum(acc);
    }
  }
  else if (mode == 3) {
    for (int it = 0; it < iters; ++it) {     // fp64 division chain
      sc = 1.0 / (sc + 1.5);
      acc = acc + sc;
    }
  }
  else if (mode == 4) {
    for (int it = 0; it < iters; ++it) {     // proj(ehess)
      acc = cx.proj(cx.ehess(acc)) * 1e-3 + g;
    }
  }
  else if (mode == 5) {
    for (int it = 0; it < iters; ++it) {     // dependent fma chain (8 per iteration)
      for (int q = 0; q < 8; ++q) acc = fma(acc, 0.999, g);
    }
  }
  else if (mode == 6) {
    for (int it = 0; it < iters; ++it) {     // sqrt chain
      sc = sqrt(sc + 1.5);
      acc = acc + sc;
    }
  }
  else if (mode == 7) {
    for (int it = 0; it < iters; ++it) {     // 8 independent fma chains x 8 (64 fma / iteration)
      double c0 = acc, c1 = acc + 1, c2 = acc + 2, c3 = acc + 3, c4 = acc + 4, c5 = acc + 5,
             c6 = acc + 6, c7 = acc + 7;
      for (int q = 0; q < 8; ++q) {
        c0 = fma(c0, 0.999, g); c1 = fma(c1, 0.999, g); c2 = fma(c2, 0.999, g);
        c3 = fma(c3, 0.999, g); c4 = fma(c4, 0.999, g); c5 = fma(c5, 0.999, g);
        c6 = fma(c6, 0.999, g); c7 = fma(c7, 0.999, g);
      }
      acc = ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7));
    }
  }
  else if (mode == 8) {
    for (int it = 0; it < iters; ++it) {     // LDS write + dependent read round trip
      cx.put(acc);
      acc = cx.read_row(cx.own_off).v[1] + g;
    }
  }
  else if (mode == 9) {
    for (int it = 0; it < iters; ++it) {     // one DPP move + add (dependent)
      acc = acc + dpp_f64<0xB1>(acc) * 1e-3;
    }
  }
  else if (mode == 10) {
    for (int it = 0; it < iters; ++it) {    // readlane + add (dependent)
      acc = g + readlane_f64(acc, 17) * 1e-3;
    }
  }
  else if (mode == 11) {
    for (int it = 0; it < iters; ++it) {    // 8 dependent f32 fma
      float fa = (float)acc;
      for (int q = 0; q < 8; ++q) fa = fmaf(fa, 0.999f, 0.5f);
      acc = fa;
    }
  }
  else if (mode == 12 || mode == 13 || mode == 14) {
    for (int it = 0; it < iters; ++it) {  // 64 independent add / mul / fma(vvv)
      double c0 = acc, c1 = acc + 1, c2 = acc + 2, c3 = acc + 3, c4 = acc + 4, c5 = acc + 5,
             c6 = acc + 6, c7 = acc + 7;
      const double h = g * 0.5 + 1.0;
#define OP8(EXPR)                                                                    \
  for (int q = 0; q < 8; ++q) {                                                      \
    { double &c = c0; c = EXPR; } { double &c = c1; c = EXPR; } { double &c = c2; c = EXPR; } \
    { double &c = c3; c = EXPR; } { double &c = c4; c = EXPR; } { double &c = c5; c = EXPR; } \
    { double &c = c6; c = EXPR; } { double &c = c7; c = EXPR; }                        \
  }
      if (mode == 12) { OP8(c + g) } else if (mode == 13) { OP8(c * h) } else { OP8(fma(c, h, g)) }
      acc = ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7));
    }
  }
  else if (mode == 15) {
    for (int it = 0; it < iters; ++it) {    // 64 independent 32-bit ops (v_add_u32 / xor mix)
      int c[8];
      for (int q = 0; q < 8; ++q) c[q] = __double2loint(acc) + q;
      for (int q = 0; q < 8; ++q)
        for (int w = 0; w < 8; ++w) c[w] = (c[w] ^ (c[w] >> 3)) + lane;   // 3 ops each
      int z = 0;
      for (int q = 0; q < 8; ++q) z ^= c[q];
      acc = g + 1e-9 * z;
    }
  }
  else if (mode == 16) {
    for (int it = 0; it < iters; ++it) {    // 32 independent DPP f64 moves (64 v_mov_dpp) + adds
      double c[8];
      for (int q = 0; q < 8; ++q) c[q] = acc + q;
      for (int q = 0; q < 4; ++q)
        for (int w = 0; w < 8; ++w) c[w] = dpp_f64<0xB1>(c[w]);
      acc = ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7]));
    }
  }
  else if (mode == 17) {
    for (int it = 0; it < iters; ++it) {    // 32 selects on f64 (64 v_cndmask)
      double c[8];
      for (int q = 0; q < 8; ++q) c[q] = acc + q;
      for (int q = 0; q < 4; ++q)
        for (int w = 0; w < 8; ++w) c[w] = ((lane >> q) & 1) ? c[w] : c[(w + 1) & 7];
      acc = ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7]));
    }
  }
  else if (mode == 18) {
    for (int it = 0; it < iters; ++it) {    // 11 x (ds_read_b128 + ds_read_b64) of the gather, no math
      cx.put(acc);
      double z = 0.0;
      for (int s2 = 0; s2 < MAXDEG; ++s2) {
        const Row<K> r = cx.read_row(cx.rowoff(s2));
        z += r.v[0];
      }
      acc = g + z * 1e-3;
    }
  }
  else if (mode == 23) {
    for (int it = 0; it < iters; ++it) {     // 1-value reduction, pure DPP butterfly
      double t = acc;
      t += dpp_f64<0xB1>(t);
      t += dpp_f64<0x4E>(t);
      t += dpp_f64<0x141>(t);
      t += dpp_f64<0x140>(t);
      const double r0 = readlane_f64(t, 0), r1 = readlane_f64(t, 16), r2 = readlane_f64(t, 32), r3 = readlane_f64(t, 48);
      acc = g + 1e-3 * ((r0 + r1) + (r2 + r3));
    }
  }
  else if (mode == 19) {
    for (int it = 0; it < iters; ++it) acc = acc * 1e-9 + cx.cost(x + acc * 1e-12);
  } else if (mode == 20) {
    for (int it = 0; it < iters; ++it) acc = acc * 1e-9 + cx.commit();
  } else if (mode == 21) {
    for (int it = 0; it < iters; ++it) {
      cx.proj_setup(0);
      acc = acc * 1e-9 + cx.Q[0];
    }
  } else if (mode == 22) {
    for (int it = 0; it < iters; ++it) acc = acc * 1e-9 + sqrt(cx.sum1(acc * acc + g));
  }
  const long long t1 = __builtin_readcyclecounter();
  if (lane == 0) {
    out[0] = (double)(t1 - t0) / iters;
    out[1] = acc + sc;
  }
}
#endif  // GIK_DEV

}  // namespace gik
