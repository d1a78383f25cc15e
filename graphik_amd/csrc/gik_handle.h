// graphik_amd/csrc/gik_handle.h -- the handle behind include/graphik_amd.h and the few helpers that both host units call:
// gik_host.hip, which defines them, and its client gik_host_anch.hip.  Nothing that only creation or the solve path uses
// belongs here.
#pragma once

#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "gik_args.h"
#include "gik_order.hip.h"
#include "gik_plan.h"
#define GIK_INTERNAL __attribute__((visibility("hidden")))      // shared between the two units, not an export

namespace gik {
struct NptVariant;      // a row of gik_host.hip's table of node-per-lane builds
GIK_INTERNAL int fail(const std::string &m);      // sets the text of gik_last_error, returns -1
}  // namespace gik
#define HIP_OK(expr)                                                                      \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return fail(std::string(#expr) + ": " + hipGetErrorString(e_));                     \
  } while (0)

struct gik_template {
  int N, T, maxdeg;
  gik::SolveFacts f;   // what the launch plan of a batch call reads (gik_plan.h); complete at the end of creation
  // fixed-anchor formulation (gik_template_create_anchored)
  bool anchored = false;
  hipEvent_t ev_solve0 = nullptr, ev_solve1 = nullptr;   // around the solve kernel of the last gik_anchored_ik_batch
  gik::AnchArgs an = {};            // device pointers + counts (anchor_goal filled per call)
  double *d_targets_const = nullptr;   // [T] template-constant targets of the free-free terms
  int full_N = 0, n_anchor = 0;
  int *d_free_full = nullptr, *d_anchor_full = nullptr;   // node index in the full robot graph
  int *d_clear_full = nullptr;      // [n_clear] ... of the free nodes that carry the obstacle hinges (anch_clearance_kernel)
  int n_clear = 0;
  // the link set of gik_anchored_attach_links (anch_link_clearance_kernel); n_link < 0: none attached
  int *d_link_a = nullptr, *d_link_b = nullptr;   // [n_link] rows of the full point matrix
  double *d_link_rho = nullptr;                   // [n_link]
  int n_link = -1;
  bool link_hinges = false;                       // ... attached with hinges = 1: the solve kernels are the LINKS builds
  // the link pairs of gik_anchored_attach_self_pairs (anch_self_clearance_kernel); n_self < 0: none attached
  int *d_self_l = nullptr, *d_self_m = nullptr;   // [n_self] indices into the link arrays
  int n_self = -1;
  bool self_hinges = false;                       // gik_anchored_attach_self_hinges: the solve kernels are the SELF builds
  // the half-spaces of gik_anchored_attach_halfspaces (n_half == 0: none attached): the solve kernels are the HALF builds
  double *d_half = nullptr;                       // [n_half][4] nx, ny, nz, d0
  double *d_half_mu = nullptr;                    // [N] margin per free node (0 where the node carries no hinges)
  double *d_half_mu_clear = nullptr;              // [n_clear] ... of the masked nodes, in d_clear_full's order (anch_half_clearance_kernel)
  int n_half = 0;
  std::vector<int> h_link_a, h_link_b, h_self_l, h_self_m;   // host copies of the link set and the pairs, and the radii:
  std::vector<double> h_link_rho;                 // what gik_anchored_attach_self_hinges builds its descriptors from
  std::vector<int> h_free_full, h_anchor_full;    // host copies of d_free_full / d_anchor_full and of the slot table:
  std::vector<uint32_t> h_slot_meta;              // what the attach call builds the per-node link records from
  double axis_length = 1.0;
  int solver;
  gik::CgParams cg;
  gik::Params p;
  // the kernels of this template, resolved once at creation (resolve_kernels)
  struct Kernels {
    void (*solve)(gik::SolveArgs) = nullptr;          // wavefront path: the solve kernel ...
    void (*solve_spread)(gik::SolveArgs) = nullptr;   // ... its tail-spreading build, or null: none compiled for this solver / theta / form
    void (*solve_scene)(gik::SolveArgs, gik::SceneArgs) = nullptr;   // ... its scene build (anchored templates), same LDS bytes
    void (*kat)(gik::KatArgs) = nullptr;              // ... and the known-answer kernel
    void (*block_solve)(gik::SolveArgs, int) = nullptr;   // workgroup path
    void (*block_kat)(gik::KatArgs, int) = nullptr;
    const void *occupancy = nullptr;                  // the kernel waves_per_cu was queried on
  } kernels;
  uint32_t *d_slot_meta = nullptr;
  gik::ClaimKey claim_key;      // gik_template_set_claim_key (f.claim_terms = claim_key.n); n == 0: index order
  // Ring of work-queue heads, one per in-flight solve call.  A slot is handed out again only
  // behind the event recorded after the launch that used it last (the new call's stream waits for
  // it), so a wrap of the ring can never reset the counter of a kernel that is still running --
  // whatever the number of calls in flight.
  unsigned int *d_counters = nullptr;
  struct CounterSlot {
    hipEvent_t done = nullptr;
    bool pending = false;
    bool in_use = false;     // handed to a call that has not recorded `done` yet
  };
  std::vector<CounterSlot> counter_slot;   // [kCounterRing]
  unsigned next_counter = 0;
  int counter_ring = 256;   // slots in use (GIK_COUNTER_RING at creation: tests shrink it to force wraps)
  std::mutex call_mutex;    // counter ring + time-slicing pool: held for the slot hand-out and the hand-back only
                            // (a slot marked in_use belongs to its call: blocking work happens outside the lock)
  std::mutex ev_mutex;      // ev_solve0 / ev_solve1 (anchored templates)
  int clique_mode = 0;      // gik_template_desc::clique_closed_form as resolved at creation
  bool hess_per_edge = false;   // the wavefront kernel (k = 3) runs the per-edge product form (gik_template_desc::hessian_form)
  // time-slicing workspaces (re-queue ring + paused state), a small pool handed out round-robin;
  // a launch that gets a slot still in use by an earlier launch waits for it on its stream
  struct SliceWs {
    void *base = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
    bool pending = false;
    bool in_use = false;     // handed to a call that has not recorded `done` yet (only its owner touches the slot)
  };
  static constexpr int kSlicePool = 32;
  SliceWs slice_ws[kSlicePool];
  unsigned next_slice = 0;
  int slice_pool = kSlicePool;   // slots in use (GIK_SLICE_POOL at creation: tests shrink it to force reuse)
  int device;
  size_t smem_bytes;
  int SL;         // slots per thread on the block path
  gik::BlockTabs bt = {nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, 0};
  // node-per-lane path (rtr_npt_kernel): trust-region solves and the known-answer entry points of
  // 3-D graphs beyond one wavefront's 64 unknowns; the workgroup tables above stay (ConjugateGradient)
  gik::NptTabs nt = {};
  const gik::NptVariant *npt_variant = nullptr;
  size_t npt_smem = 0;
  // four-problems-per-wavefront path (rtr_quad_kernel): trust-region solves of planar graphs with at most
  // 16 nodes and 6 terms per node; everything else of such a template stays on the wavefront kernels
  void (*quad_solve)(gik::SolveArgs) = nullptr;
  size_t quad_smem = 0;
  bool no_npt = false, no_quad = false;   // GIK_NO_NPT / GIK_NO_QUAD: creation leaves these kernels out
  // device pre/post-processing (gik_pipeline_attach)
  bool has_pipe = false;
  gik::PipeConst pc = {};
  std::vector<void *> pipe_allocs;
  // the prepare kernel of this template, resolved once at attach (plan_prepare, gik_plan.h), and what a block variant needs
  struct Prepare {
    gik::PrepPlan plan;
    int sweeps = 10;
    double *ws = nullptr;        // the slab, plan.slab_bytes
    hipEvent_t done = nullptr;   // launches share the slab, so each one waits for the
    std::mutex mutex;            // previous one (whatever stream it ran on)
    bool pending = false;
  } prep;
  // joint-configuration seeds (gik_seed_batch): FK tables built at attach; seed_ok is false (and seed_why says why)
  // for a graph with a node that neither a frame nor an anchor places
  gik::SeedConst sc = {};
  size_t seed_smem = 0;
  bool seed_ok = false;
  std::string seed_why;
};

GIK_INTERNAL int refuse_capture(const char *entry, void *stream);      // a capturing stream, refused under the entry's name
// what is wrong with the scene set of a scene call on t, refused under the entry's name, or 0; the set as kernel arguments
GIK_INTERNAL int scene_refusal(const char *entry, const gik_template *t, const gik_scene_set *sc);
GIK_INTERNAL gik::SceneArgs scene_args(const gik_scene_set *sc);
