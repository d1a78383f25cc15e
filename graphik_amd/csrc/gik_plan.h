// graphik_amd/csrc/gik_plan.h -- the scheduling decisions of one batch call (gik_solve_batch): which kernel runs,
// its grid, the time slice, whether the tail is spread, the queue capacities and the layout of the pooled workspace.
// Below it the same for the device prepare (gik_pipeline_attach: which of the six prepare kernels, its LDS bytes, waves per
// CU, slab and grids) and the layouts of the caller-owned workspaces: the anchored calls' scratch, the two restart loops'
// and the sweep's.
// Integer arithmetic over facts that are fixed at template creation or at attach, plus the batch size: plain C++17, no
// HIP, so that tests/host/solve_plan_table.cpp, prep_plan_table.cpp and ws_layout_table.cpp can tabulate it without a device.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/graphik_amd.h"      // (gik_stats, 48 bytes, in the restart workspaces; after <cstddef>: it uses size_t)
#include "gik_args.h"      // what the plan knows of the kernels' data: their constants and sizeof(SliceState)

namespace gik {

constexpr int PLAN_CLAIM_KEY_MAX_TERMS = CLAIM_KEY_MAX_TERMS;      // (the name tests/host/claim_order_plan.cpp checks)
// Largest batch whose claims are ordered.  The rank kernel compares every pair of keys: ~10 us at 4096 problems and
// about 0.3 ms here, against a solve of several hundred ms; beyond it a batch is hundreds of problems deep per wave and
// its time is throughput, not the start of one problem, so the plan keeps index order rather than pay B^2.
constexpr int PLAN_CLAIM_ORDER_MAX_BATCH = 65536;

// a claim key as gik_template_set_claim_key accepts it: at most PLAN_CLAIM_KEY_MAX_TERMS terms, each an index into the
// template's T terms (n == 0: index order, always accepted)
inline bool claim_key_ok(int n, const int *terms, int T) {
  if (n < 0 || n > PLAN_CLAIM_KEY_MAX_TERMS || (n > 0 && !terms)) return false;
  for (int i = 0; i < n; ++i)
    if (terms[i] < 0 || terms[i] >= T) return false;
  return true;
}

// What plan_solve reads from a handle: filled during template creation, constant afterwards.
struct SolveFacts {
  int K = 0;
  bool is_block = false;  // workgroup-per-problem path
  bool is_npt = false;    // node-per-lane path (rtr_npt_kernel)
  bool cg = false;        // solver == GIK_SOLVER_CONJUGATE_GRADIENT
  int n_cu = 0;
  int waves_per_cu = 0;   // resident solve wavefronts per CU (from the occupancy query)
  int npt_waves_per_cu = 1;
  int wpc_override = 0;   // persistent waves per CU, 0 = automatic
  // scheduling knobs, fixed at creation (descriptor fields, overridden once by the environment)
  int slice_its = 0;         // time slice of the block kernel in outer iterations, 0 = off
  int npt_slice_its = 192;   // ... of the node-per-lane kernel
  int maxiter = 0;           // Params::maxiter
  int dbg = 0;               // SolveArgs::dbg
  bool has_spread = false;   // kernels.solve_spread is set
  int wave_slice_its = 0;    // round-robin slice of the wavefront kernel (large batches), 0 = off
  bool wave_slice_auto = true;       // ... scaled with the queue depth (plan_solve)
  int wave_slice_cycles = 2000000;   // ... and its shortest duration (GIK_SLICE_CYCLES)
  bool has_quad = false;       // quad_solve is set
  int quad_min_batch = -1;     // smallest batch that runs it (GIK_QUAD_MIN_BATCH; else 12 problems per CU, set with quad_solve)
  int quad_waves_per_cu = 8;
  size_t ctg_doubles = 0;      // node-per-lane path: npt_variant->ctg(nt.n_pairs), else 0
  int claim_terms = 0;         // terms of the claim key (gik_template_set_claim_key), 0 = index order
};

enum class Launch { QUAD, NPT, BLOCK, WAVE, WAVE_SPREAD };

struct SolvePlan {
  Launch launch;
  int grid;          // resident waves / workgroups: what the queues and the workspace are sized for ...
  int launch_grid;   // ... and the grid of the launch (the quad kernel's differs)
  int wpc;
  int slice_its, slice_cycles;   // SolveArgs::slice_its / slice_cycles
  bool mig;                      // the tail is spread
  size_t cap, ycap;              // entries of the re-queue ring and of the yield queue
  bool order;                    // claims in ascending key order: key and rank kernels in front of the solve
  bool needs_ws;                 // everything below: only then
  size_t off_simd, off_seq, off_ids, off_state, off_yseq, off_yids, off_ctg, bytes;
  size_t ctg_bytes;              // of the clique-target region at off_ctg (0: none, SolveArgs::npt_ctg_ws stays null)
  // memsets: [0, zero_head) = 0; q_seq: seq_fill bytes of 0xFF; q_state: state_zero bytes of 0; y_seq: yseq_zero of 0
  size_t zero_head, seq_fill, state_zero, yseq_zero;
  size_t off_key, off_order;     // order: [B] float keys, [B] int ticket -> problem
};

inline SolvePlan plan_solve(const SolveFacts &t, int B) {
  SolvePlan p = {};
  // Persistent waves per CU: as many as fit (two per SIMD at 249 VGPRs).  Two waves share a SIMD's
  // fp64 pipe and each runs 20-50 % slower than alone, which used to cost small batches -- whose
  // time is that of their slowest problem -- more than the extra throughput returned; with the age
  // priority of rtr_solve_one the old problems keep a lone wave's speed next to a young neighbour
  // (kernel ms at 1 / 2 waves per SIMD without, and 2 per SIMD with priorities -- LWA4D B=4096:
  // 116.9 / 132.4 / 116.3, B=16384: 190.6 / 196.7 / 187.7; KUKA B=8192: 182.8 / 156.4 / 155.4,
  // B=65536: 755.7 / 545.5 / 544.2).
  // Small batches still get one wave per SIMD: their time is the run time of the few problems that
  // go to maxiter, and two of THOSE on one SIMD (equal priority) slow each other down -- at 4096
  // LWA4D goals a third of the launches drew such a pair (128 instead of 116 ms).
  int wpc = t.is_npt ? t.npt_waves_per_cu : t.waves_per_cu;
  if (!t.is_block && t.K == 3 && wpc > 4 && (long long)B <= 6LL * 4 * t.n_cu) wpc = 4;
  // THREE waves per SIMD (the per-edge form: 153 VGPRs, 8.3 KB of LDS) only for queues of 128 problems per CU and more:
  // measured round 6 on KUKA, 65536 goals 130.5 k -> 134.2 k solves/s (+2.9 %), but 8192 goals 55.4 k -> 51.5 k (-7 %) --
  // a mid-size batch is its stragglers, and a straggler with two co-resident waves runs slower than with one
  if (!t.is_block && t.K == 3 && wpc > 8 && (long long)B < 128LL * t.n_cu) wpc = 8;
  if (t.wpc_override > 0) wpc = t.wpc_override;
  const int grid = std::min(B, t.n_cu * wpc);
  // Time slicing (workgroup-per-problem kernel): only when there are more problems than resident
  // workgroups (otherwise everything starts at once anyway).  Slice length: the handle's
  // slice_outer_its, 0 disables.  Measured on UR10 + table, 4096 goals: 8.9 -> 7.7 s.
  int slice = t.is_npt ? t.npt_slice_its : t.slice_its;
  if (!t.is_block || t.cg || B <= grid || (t.dbg & 1) || slice <= 0 || t.maxiter <= slice) slice = 0;
  // Tail spreading (wavefront kernel): only where two waves share a SIMD and the batch outlasts
  // the queue -- more problems than resident waves -- and only on the tuned default variant
  // (trust-region solver, theta = 1, not anchored).  debug_flags 512 turns it off (tests compare).
  // (At one wave per SIMD -- batches up to 6 problems per SIMD -- round-robin slicing LOSES 5-8 %: a
  // straggler that happens to start at t = 0 is better off keeping its slot than sharing it for the
  // first ~20 ms; measured on 4096 LWA4D / KUKA / UR10 goals, four seeds each, tools/attic/dev_rr_midbatch.py.)
  // (kernels.solve_spread is the build of the form that runs: <3, 10> has a per-edge one but no column-form one)
  const bool mig = t.has_spread && wpc > 4 && B > grid && !(t.dbg & (1 | 512));
  // graphs beyond 128 nodes (node-per-lane kernel on four wavefronts): the clique's target triangle of every resident
  // workgroup lives in global memory -- a region of the same pooled workspace
  const size_t ctg_bytes = t.is_npt ? t.ctg_doubles * sizeof(double) * (size_t)grid : 0;
  p.wpc = wpc;
  p.grid = p.launch_grid = grid;
  p.slice_its = slice;
  p.mig = mig;
  // Claim order (NOTEBOOK 21): the 3-D trust-region wavefront kernels only, where the template has a key, and only
  // where a problem can wait for a wave at all -- with a wave per problem every claim happens at once.
  p.order = t.claim_terms > 0 && !t.is_block && !t.is_npt && t.K == 3 && !t.cg && B > grid && B <= PLAN_CLAIM_ORDER_MAX_BATCH;
  const bool queues = slice > 0 || mig || ctg_bytes;
  p.needs_ws = queues || p.order;
  if (p.needs_ws) {
    const size_t cap = mig ? (size_t)B + (size_t)grid + 64 : (slice > 0 ? (size_t)B * (size_t)(t.maxiter / slice + 1) : 0);
    // wavefront kernel: round-robin slicing (slice length: the handle's wave_slice_its)
    // Slice length grows with the queue: 256 iterations up to 8 problems per wave, 4 x that from 32 per wave on.
    // A hand-over moves ~4.5 KB through HBM (point, state, the targets re-read; PMC, round 3: 624 MB per 65536-goal
    // KUKA launch = 6.3 x the algorithmic bytes at 118 k hand-overs); measured round 4 (tools/slice_scan.py), KUKA
    // 65536: slice 256 / 512 / 1024 / 2048 -> 501.5 / 500.9 / 510.6 / 514.0 ms and 118 k / 51 k / 19 k / 7.5 k
    // hand-overs; KUKA 8192: 145.5 / 147.7 / 161.6 ms -- short queues want the short slice.
    int wslice = (mig && !(t.dbg & 1024)) ? t.wave_slice_its : 0;
    // (PMC, round 4, 65536 KUKA goals, tools/attic/c4_slice_traffic.sh: no slicing 202 MB per launch = 2.0 x the
    // algorithmic bytes -- the floor of this kernel's 432 / 600-byte rows -- at 555 ms; slice 1024: 287 MB, 519 ms;
    // 1536: 526 ms; 2048: 239 MB = 2.4 x, 537 ms.  Throughput decides: 1024.)
    if (wslice > 0 && t.wave_slice_auto && (long long)B > 8LL * grid)
      wslice = (int)std::min<long long>(4LL * wslice, (long long)wslice * B / (8LL * grid));
    // yield queue: a problem yields at most maxiter / slice + 1 times; the margin covers the waves that may be
    // between the capacity test and their push (mig_anyone_waiting)
    const size_t ycap = wslice > 0 ? std::min((size_t)B * (size_t)(t.maxiter / wslice + 2), (size_t)16 * B + 8192) +
                                         2 * (size_t)grid + 256
                                   : 0;      // (very short slices: the queue fills and the problems stop yielding)
    const size_t off_simd = 32, off_seq = off_simd + (mig ? sizeof(int) * MIG_SIMDS : 0), off_ids = off_seq + cap * 4,
                 off_state = (off_ids + cap * 4 + 15) & ~(size_t)15,
                 off_yseq = off_state + (((size_t)B * sizeof(SliceState) + 15) & ~(size_t)15), off_yids = off_yseq + ycap * 4;
    const size_t off_ctg = (off_yids + ycap * 4 + 63) & ~(size_t)63;
    // (the order's buffers come last: a plan without them is laid out as it always was)
    const size_t off_key = (off_ctg + ctg_bytes + 63) & ~(size_t)63, off_order = off_key + (p.order ? 4 * (size_t)B : 0);
    const size_t bytes = p.order ? off_order + 4 * (size_t)B : off_ctg + ctg_bytes;
    if (mig) { p.slice_its = wslice; p.slice_cycles = t.wave_slice_cycles; }
    p.cap = cap;
    p.ycap = ycap;
    p.off_simd = off_simd;
    p.off_seq = off_seq;
    p.off_ids = off_ids;
    p.off_state = off_state;
    p.off_yseq = off_yseq;
    p.off_yids = off_yids;
    p.off_ctg = off_ctg;
    p.ctg_bytes = ctg_bytes;
    p.bytes = bytes;
    p.off_key = off_key;
    p.off_order = off_order;
    p.zero_head = queues ? off_seq : 0;      // (no queue: nothing reads the head)
    p.seq_fill = cap * 4;
    p.state_zero = (mig || t.is_npt) ? (size_t)B * sizeof(SliceState) : 0;
    p.yseq_zero = ycap * 4;
  }
  // four planar problems per wavefront: from 12 problems per CU on (measured, planar-10, events around the call:
  // 4..64 problems 158 against 95 us, 1024: 206 / 150, 4096: 259 / 282 -- below that every problem has a wavefront
  // of its own anyway and the lone problem is faster there); debug_flags 16384: at any batch size
  const bool quad = t.has_quad && !(t.dbg & (1 | 8192)) && ((t.dbg & 16384) || B >= t.quad_min_batch);
  if (quad) {
    // a wavefront holds four problems: a quarter of the waves (at least one slot each), no slicing
    int qw = t.quad_waves_per_cu;
    if (t.wpc_override > 0) qw = t.wpc_override;
    p.launch_grid = std::max(1, std::min((B + QUAD_SLOTS - 1) / QUAD_SLOTS, t.n_cu * qw));
    p.launch = Launch::QUAD;
  } else if (t.is_npt) {
    p.launch = Launch::NPT;
  } else if (t.is_block) {
    p.launch = Launch::BLOCK;
  } else {
    p.launch = mig ? Launch::WAVE_SPREAD : Launch::WAVE;
  }
  return p;
}

// ---- the device prepare (gik_pipeline_attach, gik_prepare_batch): which of the six prepare kernels a template runs, its
// dynamic LDS bytes, resident waves per CU, slab and grids.  Decided once, at attach.

// prep_quad_lds_bytes of gik_prep_quad.hip.h (tests/golden/prep_plan.json pins the two equal)
constexpr size_t plan_prep_quad_lds_bytes(int N, int n_gd) {
  const int NS = N * (N | 1), stride = NS + ((16 - NS % 32) + 32) % 32;
  return sizeof(double) * ((size_t)12 * stride + 4 * (size_t)((n_gd + 1) & ~1) + 4 * PREPQ_VEC_STRIDE);
}

// What plan_prepare reads: the graph and the pipeline descriptor, and the developer switches of the environment, which
// gik_pipeline_attach reads once.
struct PrepFacts {
  int N = 0, K = 0;      // (no rule reads K: the 2-D and the 3-D pipeline plan alike)
  int n_anchor = 0, n_ee = 1, n_gg = 0;
  bool inert_goal_slot = false;       // a goal slot of -1 (every prepare kernel skips it)
  bool position_goals = false;        // ... and every one of them is the odd slot of a position end effector
                                      // (position_goal_mask).  A planar tree's parent slot that an earlier pose pins keeps
                                      // prep_wave_kernel, as it always has: the recorded plans (tests/golden/prep_plan.json)
  bool force_block_prepare = false;   // gik_pipeline_desc::force_block_prepare
  bool env_force_block = false;       // GIK_PREP_FORCE_BLOCK
  bool env_no_compress = false;       // GIK_PREP_NO_COMPRESS
  bool env_a_global = false;          // GIK_PREP_A_GLOBAL
  bool env_no_quad = false;           // GIK_NO_PREP_QUAD
  bool env_waves_set = false;         // GIK_PREP_WAVES_PER_CU ...
  int env_waves = 0;                  // ... and its atoi
  int n_cu = 0;
};

// QUAD13 / QUAD: prep_quad_kernel<13> / <0>; WAVE: prep_wave_kernel; BLOCK_LDS / BLOCK / BLOCK_BIG: prep_block_kernel<true> /
// <false> / <false, PREP_BIGN>
enum class Prep { QUAD13, QUAD, WAVE, BLOCK_LDS, BLOCK, BLOCK_BIG };

struct PrepPlan {
  Prep variant = Prep::WAVE;
  size_t lds = 0;       // dynamic LDS bytes of its launch
  int wpc = 8;          // resident prepare waves (workgroups on the block variants) per CU
  // prep_wave_kernel: a quad template runs the diagnostics of gik_prepare_batch_debug on it (WAVE: lds and wpc again)
  size_t wave_lds = 0;
  int wave_wpc = 8;
  bool no_compress = false;   // block variants: full N x N Jacobi even where the Gram matrix is rank deficient
  size_t slab_bytes = 0;      // block variants: [n_cu * wpc][5 (BLOCK_BIG: 6)][N * N] doubles of global workspace
  int n_cu = 0;
  bool block() const { return variant >= Prep::BLOCK_LDS; }
  bool quad() const { return variant <= Prep::QUAD; }
  int threads() const { return block() ? PREP_NT : WAVE; }
  int launch_grid(int B) const {
    return std::min(quad() ? (B + QUAD_SLOTS - 1) / QUAD_SLOTS : B, n_cu * wpc);
  }
  // the plan of a launch with diagnostics (gik_prepare_batch_debug): the quad kernel has none, prep_wave_kernel runs instead
  PrepPlan diagnostics() const {
    PrepPlan p = *this;
    if (quad()) {
      p.variant = Prep::WAVE;
      p.lds = wave_lds;
      p.wpc = wave_wpc;
    }
    return p;
  }
};

// occupancy(variant, threads, lds): resident workgroups of that kernel per CU, below 0 where the query failed.  For
// BLOCK_LDS it raises the kernel's LDS allowance first, and a refusal there is a failed query too.
template <typename Occupancy>
inline PrepPlan plan_prepare(const PrepFacts &f, Occupancy occupancy) {
  PrepPlan p;
  const size_t NN = (size_t)f.N * f.N;
  const int N = f.N, n_gd = 2 * f.n_ee * f.n_anchor + f.n_gg;
  p.n_cu = f.n_cu;
  p.no_compress = f.env_no_compress;
  p.wave_lds = sizeof(double) * ((size_t)5 * N * N + n_gd + 96) +
               sizeof(int) * (48 + (size_t)((N + 1) / 2) * ((N | 1) + (N + 1) / 2 + 1));   // (+ jacobi_lds's pair tables)
  // graphs beyond one wavefront's LDS: workgroup-per-goal kernel with its matrices in a global slab
  if (N > 32 || f.n_anchor > 32 || f.force_block_prepare || f.env_force_block) {
    int occ = 0;
    if (N > PREP_MAXN) {      // graphs of 129 .. 255 nodes: six matrices per slab
      p.variant = Prep::BLOCK_BIG;
      if ((occ = occupancy(p.variant, PREP_NT, p.lds)) < 0) occ = 1;
    } else {
      // work matrix in LDS when it fits next to the kernel's static arrays (N <= 123), one workgroup per CU
      p.variant = Prep::BLOCK_LDS;
      p.lds = sizeof(double) * NN;
      if (f.env_a_global || (occ = occupancy(p.variant, PREP_NT, p.lds)) < 1) {
        p.variant = Prep::BLOCK;
        p.lds = 0;
        if ((occ = occupancy(p.variant, PREP_NT, p.lds)) < 0) occ = 1;
      }
    }
    occ = std::max(1, std::min(occ, 2));   // 5 N^2 doubles per workgroup: keep the slabs cache-resident
    if (f.env_waves_set) occ = std::max(1, f.env_waves);
    p.wpc = occ;
    p.slab_bytes = sizeof(double) * (p.variant == Prep::BLOCK_BIG ? 6 : 5) * NN * (size_t)f.n_cu * occ;
    return p;
  }
  // the prepare kernel is latency-bound (dependent Jacobi chains, LDS round trips): run as many
  // resident waves per CU as its registers and LDS allow (a fixed 8 per CU left half of them
  // unused: planar-10 prepare 2.3 -> see NOTEBOOK 4.2)
  int occ = occupancy(Prep::WAVE, WAVE, p.wave_lds);
  if (occ < 0) occ = 8;
  if (f.env_waves_set) occ = f.env_waves;   // developer override
  p.lds = p.wave_lds;
  p.wpc = p.wave_wpc = std::max(1, std::min(occ, 32));
  if (N <= PREPQ_MAXN && (!f.inert_goal_slot || f.position_goals) && !f.env_no_quad) {
    const Prep quad = N == 13 ? Prep::QUAD13 : Prep::QUAD;
    const size_t quad_lds = plan_prep_quad_lds_bytes(N, n_gd);
    int qocc = 0;
    if (quad_lds <= 40 * 1024 && (qocc = occupancy(quad, WAVE, quad_lds)) >= 1) {
      if (f.env_waves_set) qocc = f.env_waves;
      p.variant = quad;
      p.lds = quad_lds;
      p.wpc = std::max(1, std::min(qocc, 32));
    }
  }
  return p;
}

// ---- caller-owned workspaces
// Carves a caller-owned workspace into arrays, each padded to 8 bytes.  A null base only adds up the size.
struct WsCarve {
  uintptr_t base;
  size_t off;
  template <typename T>
  T *take(size_t n) {
    T *at = reinterpret_cast<T *>(base + off);
    off += (n * sizeof(T) + 7) / 8 * 8;
    return at;
  }
};

// The scratch of one anchored call (gik_anchored_ws_doubles), B goals: what the robot graph's prepare or seed kernel
// writes, then the start point and the goal anchors of the fixed-anchor solve
//   targets [B][T_base] | Y_full0 [B][N_base * 3] | Y_free [B][N_free * 3] | goal [B][n_goal * 3]
struct AnchWs {
  double *targets, *Y_full0, *Y_free, *goal;
  size_t doubles;
};
inline AnchWs anch_ws(int base_T, int base_N, int free_N, int n_goal, int B, double *ws) {
  const size_t b = (size_t)B;
  WsCarve c = {reinterpret_cast<uintptr_t>(ws), 0};
  AnchWs w;
  w.targets = c.take<double>(b * (size_t)base_T);
  w.Y_full0 = c.take<double>(b * (size_t)base_N * 3);
  w.Y_free = c.take<double>(b * (size_t)free_N * 3);
  w.goal = c.take<double>(b * (size_t)n_goal * 3);
  w.doubles = c.off / sizeof(double);
  return w;
}

// The workspace of gik_ik_batch_retry (gik_retry_ws_bytes), every array sized for B failed goals; n joints, pose_w doubles
// per goal pose, the template's T terms and N nodes in K dimensions:
//   count (8 bytes) | idx [B] int32, padded to 8 bytes | poses | seed angles | targets | Y | stats | q | pos_err | rot_err
struct RetryWs {
  int32_t *count, *idx;
  double *T, *q_seed, *targets, *Y, *q, *pos_err, *rot_err;
  gik_stats *stats;
  size_t bytes;
};
inline RetryWs retry_ws(int n_joints, int pose_w, int T, int N, int K, int B, void *base) {
  const size_t b = (size_t)B, n = (size_t)n_joints;
  WsCarve c = {reinterpret_cast<uintptr_t>(base), 0};
  RetryWs w;
  w.count = c.take<int32_t>(2);
  w.idx = c.take<int32_t>(b);
  w.T = c.take<double>(b * (size_t)pose_w);
  w.q_seed = c.take<double>(b * n);
  w.targets = c.take<double>(b * (size_t)T);
  w.Y = c.take<double>(b * (size_t)N * (size_t)K);
  w.stats = c.take<gik_stats>(b);
  w.q = c.take<double>(b * n);
  w.pos_err = c.take<double>(b);
  w.rot_err = c.take<double>(b);
  w.bytes = c.off;
  return w;
}

// The workspace of gik_anchored_sweep_clearance (gik_anchored_sweep_ws_bytes), M = B (S + 1) configurations, all doubles:
//   q_s [M][n] | identity poses [M][pose_w] | seed_kernel's targets [M][T_base] (not read) | Y [M][full_N*3] | clearance [M]
struct AnchSweepWs {
  double *q, *T, *targets, *Y, *cl;
  size_t doubles;
};
inline AnchSweepWs anch_sweep_ws(int n_joints, int pose_w, int base_T, int full_N, int B, int S, double *ws) {
  const size_t M = (size_t)B * ((size_t)S + 1);
  WsCarve c = {reinterpret_cast<uintptr_t>(ws), 0};
  AnchSweepWs w;
  w.q = c.take<double>(M * (size_t)n_joints);
  w.T = c.take<double>(M * (size_t)pose_w);
  w.targets = c.take<double>(M * (size_t)base_T);
  w.Y = c.take<double>(M * (size_t)full_N * 3);
  w.cl = c.take<double>(M);
  w.doubles = c.off / sizeof(double);
  return w;
}

// The workspace of gik_anchored_ik_batch_retry (gik_anchored_retry_ws_bytes = bytes), every array sized for B failed goals:
//   the scratch of one anchored call (AnchWs; attempt 0 and every restart use it in turn) |
//   count (8 bytes) | idx [B] int32, padded to 8 bytes | poses | seed angles | centre angles | Y_full | stats | q |
//   pos_err | rot_err | clearance
// and behind those bytes, for gik_anchored_ik_batch_retry_scenes alone, whose workspace is that much longer:
//   ids [B] int32, the scene ids of a compact batch
struct AnchRetryWs {
  double *scratch;
  int32_t *count, *idx;
  double *T, *q_seed, *q_center, *Y, *q, *pos_err, *rot_err, *clearance;
  gik_stats *stats;
  size_t bytes;
  int32_t *ids;
};
inline AnchRetryWs anch_retry_ws(int n_joints, int pose_w, int base_T, int base_N, int free_N, int n_goal, int full_N, int B,
                                 void *ws) {
  const size_t b = (size_t)B, n = (size_t)n_joints;
  WsCarve c = {reinterpret_cast<uintptr_t>(ws), 0};
  AnchRetryWs w;
  w.scratch = c.take<double>(anch_ws(base_T, base_N, free_N, n_goal, B, nullptr).doubles);
  w.count = c.take<int32_t>(2);
  w.idx = c.take<int32_t>(b);
  w.T = c.take<double>(b * (size_t)pose_w);
  w.q_seed = c.take<double>(b * n);
  w.q_center = c.take<double>(b * n);
  w.Y = c.take<double>(b * (size_t)full_N * 3);
  w.stats = c.take<gik_stats>(b);
  w.q = c.take<double>(b * n);
  w.pos_err = c.take<double>(b);
  w.rot_err = c.take<double>(b);
  w.clearance = c.take<double>(b);
  w.bytes = c.off;
  w.ids = c.take<int32_t>(b);
  return w;
}

// The workspace of the screened restart seeds (gik_anchored_retry_seeds_screened: gik_anchored_retry_seeds_screened_ws_bytes = bytes),
// every array sized for M = B C candidates, candidate-major [C][B]:
//   candidate angles [M][n] | poses for the seed kernel [M][pose_w] | its targets [M][T_base] (not read) |
//   point matrices [M][full_N*3] | clearances [M] | tiled scene ids [M] int32 | picks [B] int32
// In gik_anchored_ik_batch_retry_screened it lies behind the anchored restart workspace and its ids, at `head` bytes:
// head = 0 for the stand-alone step; anch_screen_head(...) for the loop, so that the arrays in front keep their places.
struct AnchScreenWs {
  double *q, *T, *targets, *Y, *cl;
  int32_t *ids, *pick;
  size_t bytes;      // head included
};
inline AnchScreenWs anch_screen_ws(int n_joints, int pose_w, int base_T, int full_N, int B, int C, size_t head, void *ws) {
  const size_t M = (size_t)B * (size_t)C;
  WsCarve c = {reinterpret_cast<uintptr_t>(ws), head};
  AnchScreenWs w;
  w.q = c.take<double>(M * (size_t)n_joints);
  w.T = c.take<double>(M * (size_t)pose_w);
  w.targets = c.take<double>(M * (size_t)base_T);
  w.Y = c.take<double>(M * (size_t)full_N * 3);
  w.cl = c.take<double>(M);
  w.ids = c.take<int32_t>(M);
  w.pick = c.take<int32_t>((size_t)B);
  w.bytes = c.off;
  return w;
}
// where the screen arrays begin in the workspace of gik_anchored_ik_batch_retry_screened: behind AnchRetryWs and its ids
inline size_t anch_screen_head(int n_joints, int pose_w, int base_T, int base_N, int free_N, int n_goal, int full_N, int B) {
  const AnchRetryWs w = anch_retry_ws(n_joints, pose_w, base_T, base_N, free_N, n_goal, full_N, B, nullptr);
  return reinterpret_cast<uintptr_t>(w.ids) + ((size_t)B * sizeof(int32_t) + 7) / 8 * 8;
}

// The workspace of gik_anchored_ik_batch_atlas (gik_anchored_ik_batch_atlas_ws_bytes = bytes): behind the anchored restart
// workspace and its ids (`head` = anch_screen_head(...), so that every array in front keeps its place), with
// K = (retries + 1) C neighbours per goal:
//   neighbour table [B][K] int32 | attempt-0 seed angles [B][n] | noted atlas rows [retries + 1][B] int32 |
//   the screened step's arrays for B C candidates (AnchScreenWs at screen_head)
struct AnchAtlasWs {
  int32_t *nbr, *rows;
  double *q0;
  size_t screen_head;      // where the AnchScreenWs begins
  size_t bytes;            // head and the screen arrays included
};
inline AnchAtlasWs anch_atlas_ws(int n_joints, int pose_w, int base_T, int full_N, int B, int C, int retries, size_t head, void *ws) {
  const size_t b = (size_t)B, K = ((size_t)retries + 1) * (size_t)C;
  WsCarve c = {reinterpret_cast<uintptr_t>(ws), head};
  AnchAtlasWs w;
  w.nbr = c.take<int32_t>(b * K);
  w.q0 = c.take<double>(b * (size_t)n_joints);
  w.rows = c.take<int32_t>(b * ((size_t)retries + 1));
  w.screen_head = c.off;
  w.bytes = anch_screen_ws(n_joints, pose_w, base_T, full_N, B, C, w.screen_head, nullptr).bytes;
  return w;
}

}  // namespace gik
