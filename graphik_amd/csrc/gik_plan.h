// graphik_amd/csrc/gik_plan.h -- the scheduling decisions of one batch call (gik_solve_batch): which kernel runs,
// its grid, the time slice, whether the tail is spread, the queue capacities and the layout of the pooled workspace.
// Integer arithmetic over facts that are fixed at template creation, plus the batch size: plain C++17, no HIP, so
// that tests/host/solve_plan_table.cpp can tabulate it without a device.
#pragma once

#include <algorithm>
#include <cstddef>

namespace gik {

// what the plan knows of the kernels' data (gik_host.hip static_asserts them against the kernel headers)
constexpr int PLAN_MIG_SIMDS = 1 << 14;          // SIMD slots of the spread table (MIG_SIMDS)
constexpr size_t PLAN_SLICE_STATE_BYTES = 32;    // sizeof(SliceState)
constexpr int PLAN_QUAD_SLOTS = 4;               // problems per quad wavefront (QUAD_SLOTS)
constexpr int PLAN_CLAIM_KEY_MAX_TERMS = 8;      // terms of a template's claim key (CLAIM_KEY_MAX_TERMS)
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
    const size_t off_simd = 32, off_seq = off_simd + (mig ? sizeof(int) * PLAN_MIG_SIMDS : 0), off_ids = off_seq + cap * 4,
                 off_state = (off_ids + cap * 4 + 15) & ~(size_t)15,
                 off_yseq = off_state + (((size_t)B * PLAN_SLICE_STATE_BYTES + 15) & ~(size_t)15), off_yids = off_yseq + ycap * 4;
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
    p.state_zero = (mig || t.is_npt) ? (size_t)B * PLAN_SLICE_STATE_BYTES : 0;
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
    p.launch_grid = std::max(1, std::min((B + PLAN_QUAD_SLOTS - 1) / PLAN_QUAD_SLOTS, t.n_cu * qw));
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

}  // namespace gik
