// graphik_amd/csrc/gik_host.hip -- host side of the library: template creation (the path, the kernels, the uploads; the
// tables themselves are built by gik_tables.hip.h; gik_anchored_attach_links, which re-resolves them), pipeline attach,
// prepare / recover / seed, the known-answer entries, the solve with the scheduling slots of a batch call, the claim order
// and the info call: the core of the C ABI of include/graphik_amd.h.  The restarts and the fixed-anchor entries are a
// client of these exports in a unit of their own, gik_host_anch.hip; the handle and the helpers both units call are
// gik_handle.h's, defined here.  No device code is compiled here: the kernels live in gik_k_*.hip (gik_instances.h).

#include "gik_handle.h"
#include "gik_kernels.hip.h"
#include "gik_instances.h"
#include "gik_anch_seed.hip.h"
#include "gik_slots.h"
#include "gik_tables.hip.h"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>

namespace gik {
GIK_ALL_KERNELS(GIK_EXTERN_TEMPLATE)      // (every group of gik_instances.h: the one expansion on the host side)

// the compiled node-per-lane variants
struct NptVariant {
  int TL, NW;
  void (*solve)(SolveArgs);
  void (*kat)(KatArgs);
  size_t (*lds)(int, int, int, int);
  size_t (*ctg)(int);      // doubles of global clique-target workspace per workgroup (0: the triangle sits in LDS)
};
#define GIK_NPT_VARIANT(TL, NS, NW, CTG) \
  {TL, NW, rtr_npt_kernel<TL, NS, NW, CTG>, kat_npt_kernel<TL, NS, NW, CTG>, NptCtx<TL, NS, NW, CTG>::lds_bytes, NptCtx<TL, NS, NW, CTG>::ctg_doubles}
// (four wavefronts per problem: graphs of 129 .. 255 nodes, clique targets in global memory)
static const NptVariant kNptVariants[] = {GIK_NPT_VARIANT(1, 1, 2, false), GIK_NPT_VARIANT(4, 1, 2, false),
                                          GIK_NPT_VARIANT(1, 2, 1, false), GIK_NPT_VARIANT(4, 2, 1, false),
                                          GIK_NPT_VARIANT(1, 1, 4, true),  GIK_NPT_VARIANT(4, 1, 4, true)};

// ------------------------------------------------------------------------------------------
thread_local std::string g_err;
#ifdef GIK_DEV
static double *g_dbg_buf = nullptr;
#endif
int fail(const std::string &m) {
  g_err = m;
  return -1;
}

typedef void (*solve_fn)(SolveArgs);
typedef void (*scene_fn)(SolveArgs, SceneArgs);
typedef void (*kat_fn)(KatArgs);
typedef size_t (*lds_fn)(int);

// The compiled one-unknown-per-lane builds: one row per (K, slots, build word), exactly what gik_instances.h instantiates.
// A row is named by the WaveBuild bits its kernels share: the word without W_THETA1 and W_SPREAD, which name kernels
// within a row.  A kernel a row does not have stays null.  (PER_EDGE: hessian_form = GIK_HESS_PER_EDGE, k = 3, TrustRegions;
// W_ANCH: the fixed-anchor formulation, k = 3, theta == 1.  Creation asks for COLUMN or W_ANCH only: the rows with
// W_LINKS, W_SELF, W_HALF are what the attach entries re-resolve a 9-slot fixed-anchor template to, reresolve_anchored)
constexpr unsigned COLUMN = 0u, PER_EDGE = W_PER_EDGE;
struct WaveRow {
  int K, slots;
  unsigned build;
  solve_fn solve = nullptr;         // theta == 1 (reference default)
  solve_fn solve_theta = nullptr;   // any theta
  solve_fn solve_cg = nullptr;      // ConjugateGradient
  solve_fn solve_spread = nullptr;  // theta == 1 with tail spreading (MigCtl)
  scene_fn solve_scene = nullptr;   // anchored forms: the scene build of `solve` (gik_solve_batch_scenes)
  kat_fn kat = nullptr;
  lds_fn lds = nullptr;
};
// Every kernel of a row, named by the row's word B.  The free-free rows compile an any-theta build, the column row
// ConjugateGradient, the anchored rows a scene entry; MORE: W_SPREAD where the row has a tail-spreading build -- the
// per-edge rows always, the column row at <3, 9> only.
template <int K, int D, unsigned B, unsigned MORE = (B == PER_EDGE ? W_SPREAD : 0u)>
static WaveRow wave_row() {
  WaveRow r{K, D, B};
  r.solve = rtr_wave_kernel<K, D, B | W_THETA1>;
  if constexpr ((B & W_ANCH) == 0) r.solve_theta = rtr_wave_kernel<K, D, B>;
  if constexpr (B == COLUMN) r.solve_cg = rcg_wave_kernel<K, D>;
  if constexpr ((MORE & W_SPREAD) != 0) r.solve_spread = rtr_wave_kernel<K, D, B | W_THETA1 | W_SPREAD>;
  if constexpr ((B & W_ANCH) != 0) r.solve_scene = rtr_wave_scene_kernel<K, D, B | W_THETA1>;
  r.kat = kat_wave_kernel<K, D, B>;
  r.lds = WaveBuildCtx<K, D, B>::lds_bytes;
  return r;
}
// <3, 20> is compiled for anchored templates only: the free-free formulation with more than 10 terms at a node runs
// on the workgroup kernels (the 20-slot wavefront variant needed 796 B of scratch per lane: measured on the
// two-end-effector tree of tests/golden/tree5.npz, 13 terms, 144 k against 382 k solves/s;
// tools/gpu_variants.py.  <3,10> 48 B: -1.3 % against <3,9>; <2,16> 168 B: 5x faster than the
// workgroup kernels on the planar trees -- both stay)
static const WaveRow kWaveRows[] = {
    wave_row<3, 9, COLUMN, W_SPREAD>(), wave_row<3, 9, PER_EDGE>(), wave_row<3, 9, W_ANCH>(), wave_row<3, 9, W_ANCH | W_LINKS>(),
    wave_row<3, 9, W_ANCH | W_SELF>(), wave_row<3, 9, W_ANCH | W_LINKS | W_SELF>(),
    wave_row<3, 9, W_ANCH | W_HALF>(), wave_row<3, 9, W_ANCH | W_LINKS | W_HALF>(),
    wave_row<3, 10, COLUMN>(), wave_row<3, 10, PER_EDGE>(),
    wave_row<3, 20, W_ANCH>(),
    wave_row<2, 6, COLUMN>(), wave_row<2, 16, COLUMN>(), wave_row<2, 31, COLUMN>()};

// the row of (K, build) with the fewest slots that hold `slots` terms per node, or null
static const WaveRow *find_row(int K, unsigned build, int slots) {
  const WaveRow *best = nullptr;
  for (const WaveRow &r : kWaveRows)
    if (r.K == K && r.build == build && r.slots >= slots && (!best || r.slots < best->slots)) best = &r;
  return best;
}
// the row word of a fixed-anchor template's state: what its kernels are the builds of (gik_template_get_info reports it)
static unsigned anchored_build(const gik_template *t) {
  return W_ANCH | (t->link_hinges ? W_LINKS : 0u) | (t->self_hinges ? W_SELF : 0u) | (t->n_half > 0 ? W_HALF : 0u);
}

}  // namespace gik

static constexpr int kCounterRing = 256;

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of the kernel, not of a launch: several
// templates share a kernel, so the allowance is only ever raised (a later, smaller template must
// not take it away from an earlier one).
static hipError_t raise_dynamic_lds(const void *fn, size_t bytes) {
  struct Grant { const void *fn; int device; size_t bytes; };
  static std::mutex mu;
  static std::vector<Grant> granted;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return hipErrorInvalidDevice;
  std::lock_guard<std::mutex> lock(mu);
  for (Grant &g : granted)
    if (g.fn == fn && g.device == dev) {
      if (g.bytes >= bytes) return hipSuccess;
      const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
      if (e == hipSuccess) g.bytes = bytes;
      return e;
    }
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) granted.push_back({fn, dev, bytes});
  return e;
}

static bool capturing_stream(void *stream) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (!stream) return false;      // (the null stream cannot capture)
  if (hipStreamIsCapturing((hipStream_t)stream, &st) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return st != hipStreamCaptureStatusNone;
}
// the refusal of an entry point whose bookkeeping (events, workspaces, counters) cannot happen under capture
int refuse_capture(const char *entry, void *stream) {
  if (!capturing_stream(stream)) return 0;
  return gik::fail(std::string(entry) + ": the stream is capturing (hipStreamBeginCapture); batch calls cannot be captured into a graph");
}

// What is wrong with the scene set of a scene call on `t`, as a refusal with the entry's name, or 0 (gik_scenes.h holds
// the host-checkable part; the contents of d_n_obs and d_scene_id are the caller's precondition)
int scene_refusal(const char *entry, const gik_template *t, const gik_scene_set *sc) {
  using gik::fail;
  const std::string e(entry);
  if (!t->anchored || !t->kernels.solve_scene)
    return fail(e + ": the handle must be a fixed-anchor template (gik_template_create_anchored): scenes replace its obstacles");
  if (!sc) return fail(e + ": null scene set");
  if (const char *why = gik::scene_set_fault(sc->n_scene, sc->stride, sc->d_obs, sc->d_n_obs, sc->d_scene_id))
    return fail(e + ": " + why);
  return 0;
}
gik::SceneArgs scene_args(const gik_scene_set *sc) {
  gik::SceneArgs a;
  a.scene_id = sc->d_scene_id;
  a.n_obs = sc->d_n_obs;
  a.n_scene = sc->n_scene;
  a.stride = sc->stride;
  return a;
}

template <typename T>
static const T *upload(gik_template *t, const T *host, size_t count, bool &ok) {
  if (count == 0 || !host) return nullptr;
  void *d = nullptr;
  if (hipMalloc(&d, count * sizeof(T)) != hipSuccess ||
      hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
    ok = false;
    return nullptr;
  }
  t->pipe_allocs.push_back(d);
  return static_cast<const T *>(d);
}

namespace gik {      // ---- template creation, step by step (create_impl below) ----

// everything that needs no table; the order of the checks is the order in which two faults are reported
static int validate_desc(const gik_template_desc *d, const gik_anchored_desc *ad) {
  if (ad) {
    if (d->k != 3 || d->solver != GIK_SOLVER_TRUST_REGIONS || d->theta != 1.0 || d->force_block_path)
      return fail("anchored templates: k = 3, TrustRegions, theta = 1, wavefront path");
    if (ad->n_anchor < 1 || ad->n_anchor > ANCH_MAXA || ad->n_goal_anchor < 0 || ad->n_goal_anchor > ad->n_anchor)
      return fail("anchored templates: 1 <= n_anchor <= 16, goal anchors are the last rows");
    if (ad->n_obs > ANCH_MAXOBS) return fail("anchored templates: at most 128 obstacles");
    if (ad->n_obs < 0 || ad->n_pin < 0 || d->N > 63 || !ad->term_target || !ad->free_full_index ||
        !ad->anchor_full_index || !ad->anchor_pos)
      return fail("anchored templates: bad descriptor");
  }
  if (d->abi_version != GIK_ABI_VERSION) return fail("ABI version mismatch");
  if (d->k != 2 && d->k != 3) return fail("k must be 2 or 3");
  if (d->solver != GIK_SOLVER_TRUST_REGIONS && d->solver != GIK_SOLVER_CONJUGATE_GRADIENT)
    return fail("solver must be GIK_SOLVER_TRUST_REGIONS or GIK_SOLVER_CONJUGATE_GRADIENT");
  if (d->cg_beta_type < 0 || d->cg_beta_type > 3) return fail("cg_beta_type must be 0..3");
  if (d->clique_closed_form < GIK_CLIQUE_AUTO || d->clique_closed_form > GIK_CLIQUE_DENSE)
    return fail("clique_closed_form must be GIK_CLIQUE_AUTO, _OFF or _DENSE");
  if (d->hessian_form != GIK_HESS_COLUMN && d->hessian_form != GIK_HESS_PER_EDGE && d->hessian_form != GIK_HESS_AUTO)
    return fail("hessian_form must be GIK_HESS_AUTO, GIK_HESS_COLUMN or GIK_HESS_PER_EDGE");
  // 255 = what the node-per-lane kernel's 8-bit row fields take (four wavefronts per problem beyond 128 nodes);
  // every other kernel stops at 128 (checked in create_impl, where the kernel is chosen)
  if (d->N < 2 || d->N > 255) return fail("N must be in [2, 255]");
  if (d->N > BLOCK_MAXN &&
      (ad || d->k != 3 || d->solver != GIK_SOLVER_TRUST_REGIONS || d->theta != 1.0 || d->force_block_path == 1))
    return fail("graphs of more than 128 nodes run on the node-per-lane kernel only: k = 3, TrustRegions, theta = 1, "
                "not anchored, force_block_path != 1");
  if (d->n_terms < 1 || d->n_terms > 65535) return fail("n_terms out of range");
  return 0;
}

// solver parameters and scheduling knobs: the descriptor's, then the developer overrides of the environment -- read
// once, here, never inside a batch call
static void read_params(gik_template *t, const gik_template_desc *d) {
  t->N = d->N;
  t->f.K = d->k;
  t->T = d->n_terms;
  t->p.mingradnorm = d->mingradnorm;
  t->p.theta = d->theta;
  t->p.kappa = d->kappa;
  t->p.rho_prime = d->rho_prime;
  t->p.rho_regularization = d->rho_regularization;
  t->p.maxiter = d->maxiter;
  t->p.maxinner = d->maxinner;
  t->p.mininner = d->mininner;
  t->p.planar_proj_exact = d->planar_proj_exact;
  t->solver = d->solver;
  t->cg.mingradnorm = d->mingradnorm;
  t->cg.minstepsize = d->cg_minstepsize;
  t->cg.orth_value = d->cg_orth_value;
  t->cg.maxiter = d->maxiter;
  t->cg.beta_type = d->cg_beta_type;
  t->cg.planar_proj_exact = d->planar_proj_exact;
  t->f.dbg = d->debug_flags;
  if (const char *e = getenv("GIK_DBG")) t->f.dbg = atoi(e);
  t->f.wpc_override = std::max(0, d->waves_per_cu);
  if (const char *e = getenv("GIK_WAVES_PER_CU")) t->f.wpc_override = std::max(1, atoi(e));
  // workgroup kernel, table scene, 4096 goals (round 3): slice 96 / 160 / 256 -> 1430 / 1430 / 1409 solves/s and
  // 755 / 586 / 368 MB of HBM traffic per launch (every resumed slice re-reads the problem's 45 KB of
  // targets; 207 MB are the algorithmic bytes).  Without slicing: ~15 % slower (round 2: 795 vs 929).
  t->f.slice_its = d->slice_outer_its < 0 ? 256 : d->slice_outer_its;
  // node-per-lane kernel, table scene, 4096 goals (round 4): slice 0 / 48 / 96 / 256 / 600 -> 1689 / 1896 / 1894 / 1861 /
  // 1774 solves/s (two problems per CU: 512 slots, a third of the requeues of the workgroup kernel)
  // HBM traffic per launch (PMC): 603 MB at 128 = 2.9 x the algorithmic 207 MB (every resume re-reads the problem's 45 KB of
  // clique targets); 192 is the compromise
  t->f.npt_slice_its = d->slice_outer_its < 0 ? 192 : d->slice_outer_its;
  // wavefront kernel: 256 ... 32 iterations per slice give the same time (NOTEBOOK 8.3); the longest of
  // them moves the fewest problems through HBM (KUKA 65536: 118 k hand-overs of ~1.5 KB instead of 562 k at 64)
  t->f.wave_slice_its = d->slice_outer_its < 0 ? 256 : d->slice_outer_its;
  t->f.wave_slice_auto = d->slice_outer_its < 0 && !getenv("GIK_SLICE");   // (an explicit length is taken literally)
  if (const char *e = getenv("GIK_SLICE")) t->f.slice_its = t->f.npt_slice_its = t->f.wave_slice_its = std::max(0, atoi(e));
  if (const char *e = getenv("GIK_SLICE_CYCLES")) t->f.wave_slice_cycles = std::max(0, atoi(e));
  t->counter_slot.resize(kCounterRing);
  if (const char *e = getenv("GIK_COUNTER_RING")) t->counter_ring = std::min(kCounterRing, std::max(1, atoi(e)));
  if (const char *e = getenv("GIK_SLICE_POOL")) t->slice_pool = std::min(gik_template::kSlicePool, std::max(1, atoi(e)));
  t->no_npt = getenv("GIK_NO_NPT") != nullptr;      // (developer A/B switches)
  t->no_quad = getenv("GIK_NO_QUAD") != nullptr;
  if (const char *e = getenv("GIK_QUAD_MIN_BATCH")) t->f.quad_min_batch = std::max(0, atoi(e));
}

// A row's kernels on a template, by its solver and theta, with the LDS bytes of a launch.
// occupancy: of the build large batches run -- the small-batch build trades registers for latency, gik_rtr.hip.h SPLIT.  (Per-edge
// form: the tail-spreading build where there is one; every other form: always the theta == 1 build.  The grids were tuned on these.)
static void install_row(gik_template *t, const WaveRow *r) {
  const bool cg = t->solver == GIK_SOLVER_CONJUGATE_GRADIENT, theta1 = t->p.theta == 1.0;
  gik_template::Kernels &kn = t->kernels;
  kn.solve = cg ? r->solve_cg : (theta1 ? r->solve : r->solve_theta);
  kn.solve_spread = (cg || !theta1) ? nullptr : r->solve_spread;
  kn.solve_scene = r->solve_scene;
  kn.kat = r->kat;
  kn.occupancy = (const void *)(r->build == PER_EDGE ? (kn.solve_spread ? kn.solve_spread : kn.solve) : (cg ? r->solve_cg : r->solve));
  t->smem_bytes = r->lds(t->T);
}
// A 9-slot fixed-anchor template's kernels resolved again, to the row of `build` (an attach entry's: anchored_build with
// its family's bit), with their LDS bytes and occupancy.  Nothing of the template changes unless the device answers.
static int reresolve_anchored(gik_template *anch, unsigned build, const std::string &entry) {
  const WaveRow *row = find_row(3, build, 9);
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void *)row->solve, WAVE, row->lds(anch->T)) != hipSuccess)
    return fail(entry + ": device upload failed");
  install_row(anch, row);
  anch->f.waves_per_cu = std::max(1, std::min(occ, 32));
  return 0;
}

// The kernels this template launches, chosen once from path, solver, theta, anchored and Hessian form; with them
// hess_per_edge and the LDS bytes of a launch.  `row`: the wavefront path's table row (column form or anchored).
static int resolve_kernels(gik_template *t, const gik_template_desc *d, const WaveRow *row, size_t block_lds) {
  const bool cg = d->solver == GIK_SOLVER_CONJUGATE_GRADIENT, k3 = d->k == 3;
  gik_template::Kernels &kn = t->kernels;
  if (t->f.is_block) {
    kn.block_solve = cg ? (k3 ? rcg_block_kernel<3> : rcg_block_kernel<2>) : (k3 ? rtr_block_kernel<3> : rtr_block_kernel<2>);
    kn.block_kat = k3 ? kat_block_kernel<3> : kat_block_kernel<2>;
    kn.occupancy = (const void *)kn.block_solve;
    t->smem_bytes = block_lds;
    return block_lds > 160 * 1024 ? fail("graph too large for the LDS-resident block path") : 0;
  }
  // The product form concerns the one-unknown-per-lane kernel only (every other kernel forms s = y . w per edge
  // anyway).  There the per-edge form exists for k = 3, TrustRegions, free-free graphs and is what GIK_HESS_AUTO
  // selects; an explicit GIK_HESS_PER_EDGE without such a kernel is refused.
  const WaveRow *pe = find_row(d->k, PER_EDGE, row->slots);
  if (k3 && d->hessian_form != GIK_HESS_COLUMN) {
    const bool have = row->build == COLUMN && !cg && pe && pe->slots == row->slots && pe->solve && pe->solve_theta;
    if (!have && d->hessian_form == GIK_HESS_PER_EDGE)
      return fail("hessian_form = GIK_HESS_PER_EDGE: wavefront kernel of 3-D free-free graphs, TrustRegions only");
    t->hess_per_edge = have;
  }
  install_row(t, t->hess_per_edge ? pe : row);
  return 0;
}

// device, slot table, work-queue heads, occupancy; `occ`: the unclamped answer of the occupancy query
static int device_setup(gik_template *t, const gik_template_desc *d, const std::vector<uint32_t> &meta, int &occ) {
  if (t->f.is_block && t->smem_bytes > 48 * 1024) {
    // more than the default dynamic-LDS allowance: opt in for exactly what this template needs
    for (const void *fn : {t->kernels.occupancy, (const void *)t->kernels.block_kat})
      if (raise_dynamic_lds(fn, t->smem_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail("cannot reserve " + std::to_string(t->smem_bytes) + " bytes of LDS per workgroup");
      }
  }
  hipDeviceProp_t prop;
  if (hipGetDevice(&t->device) != hipSuccess ||
      hipGetDeviceProperties(&prop, t->device) != hipSuccess ||
      hipMalloc((void **)&t->d_slot_meta, meta.size() * sizeof(uint32_t)) != hipSuccess ||
      hipMalloc((void **)&t->d_counters, kCounterRing * sizeof(unsigned int)) != hipSuccess ||
      hipMemcpy(t->d_slot_meta, meta.data(), meta.size() * sizeof(uint32_t),
                hipMemcpyHostToDevice) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, t->kernels.occupancy, t->f.is_block ? BLOCK_NT : WAVE,
                                                   t->smem_bytes) != hipSuccess)
    return fail("HIP device setup failed (no GPU?)");
  t->f.n_cu = prop.multiProcessorCount;
  t->f.waves_per_cu = std::max(1, std::min(occ, 32));
  if (!t->f.is_block && !t->anchored && t->solver == GIK_SOLVER_TRUST_REGIONS && t->f.K == 2 && t->N <= QUAD_NODES &&
      t->maxdeg == 6 && d->theta == 1.0 && !(d->debug_flags & 8192) && !t->no_quad) {
    t->quad_solve = rtr_quad_kernel<6>;
    t->quad_smem = QuadCtx<6>::lds_bytes();
    int qocc = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&qocc, (const void *)t->quad_solve, WAVE, t->quad_smem) == hipSuccess)
      t->f.quad_waves_per_cu = std::max(1, std::min(qocc, 32));
    if (t->f.quad_min_batch < 0) t->f.quad_min_batch = 12 * t->f.n_cu;
  }
  return 0;
}

// ---- fixed-anchor data ----
static int upload_anchored(gik_template *t, const gik_anchored_desc *ad) {
  const int N = t->N;
  bool ok = true;
  std::vector<double> tab(4 * ANCH_MAXA, 0.0);
  for (int r = 0; r < ad->n_anchor; ++r)
    for (int c = 0; c < 3; ++c) tab[r * 4 + c] = ad->anchor_pos[r * 3 + c];
  std::vector<uint32_t> pm((size_t)ANCH_PMAX * WAVE, 0u);
  std::vector<double> pt((size_t)ANCH_PMAX * WAVE, 0.0);
  std::vector<int> cnt(N, 0);
  for (int q = 0; q < ad->n_pin; ++q) {
    const int i = ad->pin_node[q], r = ad->pin_anchor[q], kind = ad->pin_kind[q];
    if (i < 0 || i >= N || r < 0 || r >= ad->n_anchor || kind < GIK_TERM_EQ || kind > GIK_TERM_UPPER || cnt[i] >= ANCH_PMAX) {
      ok = false;
      break;
    }
    for (int c = 0; c < 3; ++c) {      // every lane of the node walks all of the node's pinned terms
      pm[(size_t)cnt[i] * WAVE + i * 3 + c] = (uint32_t)r | ((uint32_t)kind << 8);
      pt[(size_t)cnt[i] * WAVE + i * 3 + c] = ad->pin_target[q];
    }
    ++cnt[i];
  }
  unsigned long long mask = 0;
  std::vector<int> clear_full;
  for (int i = 0; i < N && ad->obs_node_mask; ++i)
    if (ad->obs_node_mask[i]) {
      mask |= 1ull << i;
      clear_full.push_back(ad->free_full_index[i]);
    }
  // rows of the full point matrix that the glue kernels read and write
  for (int i = 0; i < N; ++i)
    if (ad->free_full_index[i] < 0 || ad->free_full_index[i] >= ad->full_N) return fail("anchored templates: free_full_index out of range");
  for (int r = 0; r < ad->n_anchor; ++r)
    if (ad->anchor_full_index[r] < 0 || ad->anchor_full_index[r] >= ad->full_N) return fail("anchored templates: anchor_full_index out of range");
  AnchArgs &an = t->an;
  an.anch_const = ok ? upload(t, tab.data(), tab.size(), ok) : nullptr;
  an.pin_meta = upload(t, pm.data(), pm.size(), ok);
  an.pin_tgt = upload(t, pt.data(), pt.size(), ok);
  an.obs = ad->n_obs ? upload(t, ad->obs, (size_t)ad->n_obs * 4, ok) : nullptr;
  an.obs_mask = mask;
  an.n_obs = ad->n_obs;
  an.n_goal = ad->n_goal_anchor;
  an.goal_row0 = ad->n_anchor - ad->n_goal_anchor;
  t->d_targets_const = const_cast<double *>(upload(t, ad->term_target, (size_t)t->T, ok));
  t->d_free_full = const_cast<int *>(upload(t, ad->free_full_index, (size_t)N, ok));
  t->d_anchor_full = const_cast<int *>(upload(t, ad->anchor_full_index, (size_t)ad->n_anchor, ok));
  t->d_clear_full = const_cast<int *>(upload(t, clear_full.data(), clear_full.size(), ok));
  t->n_clear = (int)clear_full.size();
  t->h_free_full.assign(ad->free_full_index, ad->free_full_index + N);
  t->h_anchor_full.assign(ad->anchor_full_index, ad->anchor_full_index + ad->n_anchor);
  t->full_N = ad->full_N;
  t->n_anchor = ad->n_anchor;
  t->axis_length = ad->axis_length;
  if (hipEventCreate(&t->ev_solve0) != hipSuccess || hipEventCreate(&t->ev_solve1) != hipSuccess) ok = false;
  return ok ? 0 : fail("anchored templates: bad pinned term (node / anchor / kind out of range, or more than 8 per node) "
                       "or device upload failed");
}

// upload of the node-per-lane tables and the kernel's LDS / occupancy; a template that did not ask for this kernel
// (force_block_path != 2) stays on the workgroup kernels when the device refuses
static int setup_npt(gik_template *t, const gik_template_desc *d, const NptHost &h, int NW) {
  bool ok = true;
  t->nt = h.n;
  t->nt.node_of_row = upload(t, h.node_of_row.data(), h.node_of_row.size(), ok);
  t->nt.clq_pair_term = upload(t, h.clq_pair_term.data(), h.clq_pair_term.size(), ok);
  t->nt.term_rec = upload(t, h.term_rec.data(), h.term_rec.size(), ok);
  t->nt.term_tgt = upload(t, h.term_tgt.data(), h.term_tgt.size(), ok);
  t->nt.gather = upload(t, h.gather.data(), h.gather.size(), ok);
  t->nt.wslot_of_row = upload(t, h.wslot_of_row.data(), h.wslot_of_row.size(), ok);
  t->nt.prow_of_slot = upload(t, h.prow_of_slot.data(), h.prow_of_slot.size(), ok);
  t->nt.clq_euclid = t->bt.clq_euclid;
  for (const NptVariant &v : kNptVariants)
    if (v.TL == h.n.TL && v.NW == NW) t->npt_variant = &v;
  t->npt_smem = t->npt_variant->lds(h.n.n_pairs, h.n.n_wrows, h.n.n_rows, h.n.n_terms);
  const void *fns[2] = {(const void *)t->npt_variant->solve, (const void *)t->npt_variant->kat};
  int occ_npt = 0;
  ok = ok && t->npt_smem <= 160 * 1024;
  if (ok && t->npt_smem > 48 * 1024)
    for (const void *fn : fns) ok = ok && raise_dynamic_lds(fn, t->npt_smem) == hipSuccess;
  ok = ok && hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ_npt, fns[0], WAVE * NW, t->npt_smem) == hipSuccess;
  if (!ok) {
    (void)hipGetLastError();
    return d->force_block_path == 2 ? fail("node-per-lane kernel: device setup failed (LDS)") : 0;
  }
  t->f.is_npt = true;
  t->f.npt_waves_per_cu = std::max(1, std::min(occ_npt, 4));   // problems (workgroups) per CU
  return 0;
}

}  // namespace gik

static int create_impl(const gik_template_desc *d, const gik_anchored_desc *ad, gik_template **out) {
  using namespace gik;
  if (!d || !out) return fail("null argument");
  if (validate_desc(d, ad)) return -1;
  std::unique_ptr<gik_template, void (*)(gik_template *)> t(new gik_template(), gik_template_destroy);   // (every error return releases it)
  read_params(t.get(), d);
  t->anchored = ad != nullptr;
  SlotLists ents;
  int maxdeg = 0;
  const std::string bad_terms = slot_lists(d, ents, maxdeg);
  if (!bad_terms.empty()) return fail(bad_terms);
  // the path: one unknown per lane with the smallest compiled slot count that holds the busiest node, else a workgroup per problem; there
  // the node-per-lane kernel for 3-D graphs beyond one wavefront, trust-region solver, theta = 1 (force_block_path: 1 = never, 2 = always)
  const bool big = d->N > BLOCK_MAXN;
  const WaveRow *row = nullptr;
  if (d->N * d->k <= WAVE && d->N <= 32 && !d->force_block_path) row = find_row(d->k, ad ? W_ANCH : COLUMN, maxdeg);
  t->f.is_block = !row;      // (also: a node busier than any wave variant)
  if (t->f.is_block && ad) return fail("anchored templates need N * k <= 64 free unknowns and at most 20 terms per node");
  const bool npt_wanted = t->f.is_block && d->k == 3 && d->solver == GIK_SOLVER_TRUST_REGIONS && d->theta == 1.0 && !ad &&
                          (d->force_block_path == 2 || (d->force_block_path == 0 && d->N * d->k > WAVE && !t->no_npt));
  const bool npt_two_waves = big || !(t->f.dbg & 2048);      // 2048: one wavefront per problem, two nodes per lane
  const int npt_NW = big ? 4 : (npt_two_waves ? 2 : 1);    // wavefronts per problem ("two_waves": one node per lane)
  CliqueRows clq;
  BlockHost bh;      // (the workgroup tables stay next to the node-per-lane ones: ConjugateGradient, known answers)
  NptHost npt;
  if (t->f.is_block) {
    clq = clique_rows(d, t->f.dbg, big ? 256 : BLOCK_MAXN);      // rows of the host-side tables (the workgroup kernels' are 128)
    if (!big) bh = block_tables(d->N, d->n_terms, clq);
    if (npt_wanted) npt = npt_tables(d, clq, npt_two_waves, npt_NW, big ? 4 * WAVE : NPT_MAXN);
  } else {
    bh.meta = wave_slot_table(d, ents, row->slots);
  }
  t->SL = bh.SL;
  t->maxdeg = t->f.is_block ? bh.SL : row->slots;
  const int Tc = (int)clq.nc_term.size(), n_pairs = (int)bh.clq_pair_term.size();
  const size_t block_lds = !t->f.is_block ? 0 : d->k == 3 ? BlockCtx<3>::lds_bytes(Tc, bh.SL, n_pairs, clq.n_clq) : BlockCtx<2>::lds_bytes(Tc, bh.SL);
  int occ = 0;
  if (resolve_kernels(t.get(), d, row, block_lds) || device_setup(t.get(), d, bh.meta, occ)) return -1;
  if (ad && upload_anchored(t.get(), ad)) return -1;
  if (ad) t->h_slot_meta = bh.meta;
  if (t->f.is_block) {
    bool ok = true;
    t->bt.nc_term = upload(t.get(), clq.nc_term.data(), clq.nc_term.size(), ok);
    t->bt.clq_term = upload(t.get(), bh.clq_term.data(), bh.clq_term.size(), ok);
    t->bt.clq_pair_term = upload(t.get(), bh.clq_pair_term.data(), bh.clq_pair_term.size(), ok);
    t->bt.clq_pid_t = upload(t.get(), bh.clq_pid.data(), bh.clq_pid.size(), ok);
    t->bt.n_pairs = n_pairs;
    t->bt.node_of_row = upload(t.get(), clq.node_of_row.data(), clq.node_of_row.size(), ok);
    t->bt.wave_sl = upload(t.get(), bh.wave_sl.data(), bh.wave_sl.size(), ok);
    t->bt.Tc = Tc;
    t->bt.n_clq = clq.n_clq;
    t->bt.clq_euclid = (clq.n_clq && !(t->f.dbg & 256) && d->clique_closed_form != GIK_CLIQUE_DENSE) ? 1 : 0;   // 256: always the dense D w product
    t->clique_mode = !clq.n_clq ? GIK_CLIQUE_OFF : (t->bt.clq_euclid ? GIK_CLIQUE_AUTO : GIK_CLIQUE_DENSE);
    if (!ok) return fail("device upload of the workgroup-path tables failed");
  }
  if (d->force_block_path == 2 && !npt.ok)
    return fail("node-per-lane kernel: k = 3, TrustRegions, theta = 1, at most 256 terms outside the rigid clique, at most 16 per lane");
  if (npt.ok && setup_npt(t.get(), d, npt, npt_NW)) return -1;
  if (big && !t->f.is_npt)
    return fail("graphs of more than 128 nodes need the node-per-lane kernel: at most 256 terms outside the rigid clique "
                "(16 per node), at most 127 nodes that carry such terms");
  if ((t->f.dbg & 32) && t->f.is_npt)
    fprintf(stderr, "  node-per-lane kernel: %d wavefront(s) per problem, TL=%d, %d slot terms (sync %d), %d direction rows, gather lists %d + %d, "
            "clique rows from %d, lds=%zu B, %d problems per CU\n",
            t->npt_variant->NW, t->nt.TL, t->nt.n_terms, t->nt.term_sync, t->nt.n_wrows, t->nt.DEG0, t->nt.DEG1, t->nt.cbase,
            t->npt_smem, t->f.npt_waves_per_cu);
  if (t->f.dbg & 32)
      fprintf(stderr, "gik_template_create: N=%d k=%d T=%d %s maxdeg=%d lds=%zu B occupancy=%d per CU, %d CUs; "
              "clique %d, slot terms %d, slots %d\n",
              t->N, t->f.K, t->T, t->f.is_block ? "block" : "wave", t->f.is_block ? 0 : t->maxdeg,
              t->smem_bytes, occ, t->f.n_cu, clq.n_clq, t->f.is_block ? Tc : t->T, t->SL);
  if ((t->f.dbg & 32) && t->f.is_block) {
    fprintf(stderr, "  slot loop bounds per wavefront {equalities, all}:");
    for (int w = 0; w < BLOCK_WAVES; ++w) fprintf(stderr, " {%d, %d}", bh.wave_sl[2 * w], bh.wave_sl[2 * w + 1]);
    fprintf(stderr, "\n");
  }
  // the rest of what a batch call's plan reads, now that kernels, parameters and tables are settled
  t->f.cg = t->solver == GIK_SOLVER_CONJUGATE_GRADIENT;
  t->f.maxiter = t->p.maxiter;
  t->f.has_spread = t->kernels.solve_spread != nullptr;
  t->f.has_quad = t->quad_solve != nullptr;
  t->f.ctg_doubles = t->f.is_npt ? t->npt_variant->ctg(t->nt.n_pairs) : 0;
  *out = t.release();
  return 0;
}

extern "C" {

const char *gik_last_error(void) { return gik::g_err.c_str(); }
int gik_abi_version(void) { return GIK_ABI_VERSION; }

int gik_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void gik_default_params(gik_template_desc *d) {
  d->abi_version = GIK_ABI_VERSION;
  d->mingradnorm = 0.5 * 1e-9;  // riemannian_solver.py:45
  d->maxiter = 3000;            // :47
  d->maxinner = 10000;          // trust_region.py:118
  d->mininner = 1;              // trust_region.py:116
  d->theta = 1.0;               // riemannian_solver.py:48
  d->kappa = 0.1;               // :49
  d->rho_prime = 0.1;           // trust_region.py:90
  d->rho_regularization = 1e3;  // trust_region.py:92
  d->planar_proj_exact = 0;
  d->force_block_path = 0;
  d->waves_per_cu = 0;
  d->slice_outer_its = -1;
  d->debug_flags = 0;
  d->solver = GIK_SOLVER_TRUST_REGIONS;
  d->cg_minstepsize = 1e-10;    // riemannian_solver.py:56
  d->cg_orth_value = 10e10;     // :57
  d->cg_beta_type = 3;          // :58  BetaTypes[3] = HagerZhang
  d->clique_closed_form = GIK_CLIQUE_AUTO;
  d->hessian_form = GIK_HESS_AUTO;
}

void gik_default_cg_params(gik_template_desc *d) {
  gik_default_params(d);
  d->solver = GIK_SOLVER_CONJUGATE_GRADIENT;
  d->mingradnorm = 1e-9;        // riemannian_solver.py:53
  d->maxiter = 100000;          // :55  (10e4)
}

int gik_template_create(const gik_template_desc *d, gik_template **out) {
  return create_impl(d, nullptr, out);
}

int gik_template_create_anchored(const gik_template_desc *d, const gik_anchored_desc *ad, gik_template **out) {
  if (!ad) return gik::fail("null argument");
  return create_impl(d, ad, out);
}

// the links of the link clearance; with hinges = 1 the template's kernels are resolved again (the W_LINKS row)
int gik_anchored_attach_links(gik_template *anch, const gik_link_desc *d) {
  using namespace gik;
  const std::string e("gik_anchored_attach_links");
  if (!anch || !d) return fail(e + ": null argument");
  if (!anch->anchored) return fail(e + ": the handle must be a fixed-anchor template (gik_template_create_anchored)");
  if (anch->n_link >= 0) return fail(e + ": links already attached");
  if (d->hinges != 0 && d->hinges != 1) return fail(e + ": hinges must be 0 (measure only) or 1 (the solve carries link hinges)");
  if (d->hinges && anch->n_half > 0)
    return fail(e + ": half-spaces are attached; link hinges come before gik_anchored_attach_halfspaces, which is called last");
  if (d->n_link < 0 || d->n_link > ANCH_MAXLINK) return fail(e + ": n_link must be within 0 .. 64");
  if (d->n_link > 0 && (!d->link_a || !d->link_b || !d->link_radius)) return fail(e + ": null link array");
  for (int l = 0; l < d->n_link; ++l) {
    if (d->link_a[l] < 0 || d->link_a[l] >= anch->full_N || d->link_b[l] < 0 || d->link_b[l] >= anch->full_N)
      return fail(e + ": link " + std::to_string(l) + " names a row outside [0, full_N)");
    if (!(d->link_radius[l] >= 0.0) || d->link_radius[l] == __builtin_huge_val())
      return fail(e + ": link_radius[" + std::to_string(l) + "] must be finite and at least 0");
  }
  std::vector<AnchLinkRec> recs;
  if (d->hinges) {
    const std::string why = link_hinge_records(anch->N, anch->maxdeg, anch->h_slot_meta, anch->h_free_full, anch->h_anchor_full, d, recs);
    if (!why.empty()) return fail(e + ": " + why);
  }
  bool ok = true;
  int *la = const_cast<int *>(upload(anch, d->link_a, (size_t)d->n_link, ok));
  int *lb = const_cast<int *>(upload(anch, d->link_b, (size_t)d->n_link, ok));
  double *lr = const_cast<double *>(upload(anch, d->link_radius, (size_t)d->n_link, ok));
  if (!ok) return fail(e + ": device upload failed");
  anch->d_link_a = la;
  anch->d_link_b = lb;
  anch->d_link_rho = lr;
  anch->h_link_a.assign(d->link_a, d->link_a + d->n_link);
  anch->h_link_b.assign(d->link_b, d->link_b + d->n_link);
  anch->h_link_rho.assign(d->link_radius, d->link_radius + d->n_link);
  if (d->hinges) {
    // the template's solve and known-answer kernels become the link row's, with their LDS bytes and occupancy
    const AnchLinkRec *dr = upload(anch, recs.data(), recs.size(), ok);
    if (!ok) return fail(e + ": device upload failed");
    if (reresolve_anchored(anch, anchored_build(anch) | W_LINKS, e)) return -1;
    anch->an.link_rec = dr;
    anch->link_hinges = true;
  }
  anch->n_link = d->n_link;
  return 0;
}

// the link pairs of the self clearance: indices into the attached link set, once, after the links
int gik_anchored_attach_self_pairs(gik_template *anch, int n_pair, const int32_t *pair_l, const int32_t *pair_m) {
  using namespace gik;
  const std::string e("gik_anchored_attach_self_pairs");
  if (!anch) return fail(e + ": null argument");
  if (!anch->anchored) return fail(e + ": the handle must be a fixed-anchor template (gik_template_create_anchored)");
  if (anch->n_link < 0) return fail(e + ": no links attached (gik_anchored_attach_links comes first)");
  if (anch->n_self >= 0) return fail(e + ": self pairs already attached");
  if (n_pair < 0 || n_pair > ANCH_MAXSELF) return fail(e + ": n_pair must be within 0 .. 2016");
  if (n_pair > 0 && (!pair_l || !pair_m)) return fail(e + ": null pair array");
  for (int p = 0; p < n_pair; ++p) {
    if (pair_l[p] < 0 || pair_l[p] >= anch->n_link || pair_m[p] < 0 || pair_m[p] >= anch->n_link)
      return fail(e + ": pair " + std::to_string(p) + " names a link outside [0, n_link)");
    if (pair_l[p] == pair_m[p]) return fail(e + ": pair " + std::to_string(p) + " names one link twice");
  }
  bool ok = true;
  int *pl = const_cast<int *>(upload(anch, pair_l, (size_t)n_pair, ok));
  int *pm = const_cast<int *>(upload(anch, pair_m, (size_t)n_pair, ok));
  if (!ok) return fail(e + ": device upload failed");
  anch->d_self_l = pl;
  anch->d_self_m = pm;
  anch->h_self_l.assign(pair_l, pair_l + n_pair);
  anch->h_self_m.assign(pair_m, pair_m + n_pair);
  anch->n_self = n_pair;
  return 0;
}

// self hinges: the attached pairs become terms of the solve.  The template's solve, known-answer and scene kernels are
// resolved again, to the SELF row of its current form (with or without link hinges), with their LDS bytes and occupancy.
int gik_anchored_attach_self_hinges(gik_template *anch) {
  using namespace gik;
  const std::string e("gik_anchored_attach_self_hinges");
  if (!anch) return fail(e + ": null argument");
  if (!anch->anchored) return fail(e + ": the handle must be a fixed-anchor template (gik_template_create_anchored)");
  if (anch->self_hinges) return fail(e + ": self hinges already attached");
  if (anch->n_half > 0) return fail(e + ": half-spaces are attached; the solve has no build with self hinges and half-spaces");
  if (anch->n_link < 0) return fail(e + ": no links attached (gik_anchored_attach_links comes first)");
  if (anch->n_self < 0) return fail(e + ": no self pairs attached (gik_anchored_attach_self_pairs comes first)");
  if (anch->n_self > ANCH_SELF_HMAX)
    return fail(e + ": " + std::to_string(anch->n_self) + " self pairs attached; the solve carries hinges for at most 16");
  if (anch->maxdeg != 9)
    return fail(e + ": self hinges need the 9-slot fixed-anchor kernel; this template runs the " + std::to_string(anch->maxdeg) +
                "-slot variant, which has none");
  std::vector<AnchSelfDesc> descs;
  const std::string why = self_hinge_descs(anch->h_free_full, anch->h_anchor_full, anch->h_link_a, anch->h_link_b, anch->h_link_rho,
                                           anch->h_self_l, anch->h_self_m, descs);
  if (!why.empty()) return fail(e + ": " + why);
  bool ok = true;
  const AnchSelfDesc *dd = upload(anch, descs.data(), descs.size(), ok);
  if (!ok) return fail(e + ": device upload failed");
  if (reresolve_anchored(anch, anchored_build(anch) | W_SELF, e)) return -1;
  anch->an.self_desc = dd;
  anch->self_hinges = true;
  return 0;
}

// half-space obstacles: floors and walls as terms of the solve and of every clearance the library reports.  Called last.  The
// template's solve, known-answer and scene kernels are resolved again, to the HALF row of its current form.
int gik_anchored_attach_halfspaces(gik_template *anch, int n_half, const double *halfspaces, const double *node_margin) {
  using namespace gik;
  const std::string e("gik_anchored_attach_halfspaces");
  if (!anch) return fail(e + ": null argument");
  if (!anch->anchored) return fail(e + ": the handle must be a fixed-anchor template (gik_template_create_anchored)");
  if (anch->n_half > 0) return fail(e + ": half-spaces already attached");
  if (n_half < 1 || n_half > ANCH_HALF_MAX) return fail(e + ": n_half must be within 1 .. 8");
  if (!halfspaces || !node_margin) return fail(e + ": null array");
  for (int h = 0; h < n_half; ++h) {
    const double *p = halfspaces + 4 * h;
    for (int q = 0; q < 4; ++q)
      if (!(p[q] - p[q] == 0.0)) return fail(e + ": half-space " + std::to_string(h) + " has an entry that is not finite");
    const double n2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
    if (!(n2 - 1.0 <= 1e-12 && 1.0 - n2 <= 1e-12))
      return fail(e + ": half-space " + std::to_string(h) + ": the normal must have unit length (| |n|^2 - 1 | <= 1e-12)");
  }
  std::vector<double> mu((size_t)anch->N, 0.0), mu_clear;
  for (int i = 0; i < anch->N; ++i) {
    if (!((anch->an.obs_mask >> i) & 1ull)) continue;      // (read where obs_node_mask is 1)
    if (!(node_margin[i] >= 0.0) || node_margin[i] == __builtin_huge_val())
      return fail(e + ": node_margin[" + std::to_string(i) + "] must be finite and at least 0");
    mu[(size_t)i] = node_margin[i];
    mu_clear.push_back(node_margin[i]);      // (d_clear_full lists the masked nodes in this order)
  }
  if ((int)mu_clear.size() != anch->n_clear) return fail(e + ": the handle's masked nodes and its clearance rows disagree");
  if (anch->maxdeg != 9)
    return fail(e + ": half-spaces need the 9-slot fixed-anchor kernel; this template runs the " + std::to_string(anch->maxdeg) +
                "-slot variant, which has none");
  if (anch->self_hinges) return fail(e + ": self hinges are attached; the solve has no build with self hinges and half-spaces");
  bool ok = true;
  double *dh = const_cast<double *>(upload(anch, halfspaces, (size_t)n_half * 4, ok));
  double *dm = const_cast<double *>(upload(anch, mu.data(), mu.size(), ok));
  double *dc = const_cast<double *>(upload(anch, mu_clear.data(), mu_clear.size(), ok));
  if (!ok) return fail(e + ": device upload failed");
  if (reresolve_anchored(anch, anchored_build(anch) | W_HALF, e)) return -1;
  anch->d_half = dh;
  anch->d_half_mu = dm;
  anch->d_half_mu_clear = dc;
  anch->n_half = n_half;
  return 0;
}

void gik_template_destroy(gik_template *t) {
  if (!t) return;
  if (t->d_slot_meta) (void)hipFree(t->d_slot_meta);
  if (t->d_counters) (void)hipFree(t->d_counters);
  for (void *p : t->pipe_allocs) (void)hipFree(p);
  if (t->ev_solve0) (void)hipEventDestroy(t->ev_solve0);
  if (t->ev_solve1) (void)hipEventDestroy(t->ev_solve1);
  if (t->prep.done) (void)hipEventDestroy(t->prep.done);
  for (auto &c : t->counter_slot)
    if (c.done) (void)hipEventDestroy(c.done);
  for (auto &w : t->slice_ws) {
    if (w.base) (void)hipFree(w.base);
    if (w.done) (void)hipEventDestroy(w.done);
  }
  delete t;
}

// The tables of seed_kernel (seed_recipe, gik_tables.hip.h) on the device.  Returns false only when an upload fails; a
// graph the recipe does not cover leaves seed_ok false.
static bool seed_tables(gik_template *t, const gik_pipeline_desc *d, const std::vector<int> &path, int n_ee) {
  const int D = t->f.K + 1;
  const gik::SeedRecipe r = gik::seed_recipe(t->N, t->f.K, d, path, n_ee);
  if (!r.ok) {
    t->seed_why = r.why;
    return true;
  }
  bool ok = true;
  gik::SeedConst sc;
  sc.Trel = upload(t, r.Trel.data(), r.Trel.size(), ok);
  sc.fk_parent = upload(t, r.parent.data(), r.parent.size(), ok);
  sc.fk_order = upload(t, r.order.data(), r.order.size(), ok);
  sc.node_frame = upload(t, r.frame.data(), r.frame.size(), ok);
  sc.node_coef = upload(t, r.coef.data(), r.coef.size(), ok);
  sc.node_anchor = upload(t, r.anchor.data(), r.anchor.size(), ok);
  sc.n_fk = (int)r.order.size();
  if (!ok) return false;
  t->sc = sc;
  t->seed_smem = sizeof(double) * (size_t)(d->n_joints + 1) * D * D;
  t->seed_ok = true;
  return true;
}

namespace gik {      // ---- gik_pipeline_attach, step by step ----

static int validate_pipeline(const gik_template *t, const gik_pipeline_desc *d) {
  if (!t || !d) return fail("null argument");
  if (t->has_pipe) return fail("pipeline already attached");
  const int N = t->N, K = t->f.K, n = d->n_joints;
  if (n < 1 || n > 125) return fail("n_joints out of range (1 .. 125)");
  if (d->n_anchor < 1 || d->n_anchor > PREP_MAXA) return fail("n_anchor must be in [1, 256]");
  if (N > PREP_BIGN - 1 || (N > PREP_MAXN && K != 3))
    return fail("the device pipeline handles graphs of up to 128 nodes (3-D: 255)");
  if (!d->T0 || !d->p_index || !d->base_lower || !d->base_upper || !d->anchor_index ||
      !d->anchor_pos || !d->pair_i || !d->pair_j || !d->term_src || !d->term_static)
    return fail("null pipeline array");
  if (K == 3 && !d->q_index) return fail("q_index required for k=3");
  return 0;
}

// the descriptor's arrays on the device and its scalars (uploads stay in pipe_allocs for gik_template_destroy)
static int upload_pipe_const(gik_template *t, const gik_pipeline_desc *d, PipeConst &pc) {
  const int N = t->N, K = t->f.K, n = d->n_joints, DD = (K + 1) * (K + 1);
  bool ok = true;
  pc.T0 = upload(t, d->T0, (size_t)(n + 1) * DD, ok);
  pc.p_idx = upload(t, d->p_index, n + 1, ok);
  pc.q_idx = (K == 3) ? upload(t, d->q_index, n + 1, ok) : pc.p_idx;
  pc.base_lower = upload(t, d->base_lower, (size_t)N * N, ok);
  pc.base_upper = upload(t, d->base_upper, (size_t)N * N, ok);
  pc.anchor_idx = upload(t, d->anchor_index, d->n_anchor, ok);
  pc.anchor_pos = upload(t, d->anchor_pos, (size_t)d->n_anchor * K, ok);
  pc.pair_i = upload(t, d->pair_i, d->n_pairs, ok);
  pc.pair_j = upload(t, d->pair_j, d->n_pairs, ok);
  pc.term_src = upload(t, d->term_src, t->T, ok);
  pc.term_static = upload(t, d->term_static, t->T, ok);
  if (!ok) return fail("device upload failed");
  pc.N = N;
  pc.K = K;
  pc.T = t->T;
  pc.n_anchor = d->n_anchor;
  pc.n_pairs = d->n_pairs;
  pc.n_joints = n;
  pc.goal0 = d->goal_node0;
  pc.goal1 = d->goal_node1;
  pc.x_idx = d->x_index;
  pc.y_idx = d->y_index;
  pc.goal_len = d->goal_len;
  pc.axis_length = d->axis_length;
  pc.last_along_z = d->last_link_along_z;
  return 0;
}

// end effectors: a chain is one path 0..n with goal nodes (goal_node0, goal_node1).  path: [n_ee][n + 1], -1 past an end
// inert_goal_slot: a goal slot of -1; position_goals: every such slot is the odd slot of a position end effector
static int end_effector_paths(gik_template *t, const gik_pipeline_desc *d, PipeConst &pc, std::vector<int> &path,
                              bool &inert_goal_slot, bool &position_goals) {
  const int N = t->N, K = t->f.K, n = d->n_joints;
  bool ok = true;
  const int n_ee = d->n_ee > 1 ? d->n_ee : 1;
  if (n_ee > PREP_MAX_EE) return fail("at most 8 end effectors");
  if (n_ee > 1 && (!d->ee_goal_nodes || !d->ee_path || d->n_goal_pairs < 0 || (K == 2 && !d->ee_goal_len) ||
                   (d->n_goal_pairs > 0 && (!d->goal_pair_a || !d->goal_pair_b))))
    return fail("several end effectors: ee_goal_nodes / ee_path / goal pairs (k = 2: ee_goal_len) required");
  // position goals: one bit per end effector, its odd slot inert, no T_final correction
  const uint32_t mask = (uint32_t)d->position_goal_mask;
  if (mask >> n_ee) return fail("position_goal_mask: a bit at or beyond n_ee");
  if (mask & (uint32_t)d->last_link_along_z)
    return fail("position_goal_mask: a position goal takes no T_final correction; clear its bit of last_link_along_z");
  const char *odd_slot = "position_goal_mask: the odd goal slot of a position goal (goal_node1, ee_goal_nodes[2 e + 1]) must be -1";
  pc.pos_goal_mask = (int)mask;
  pc.pos_qs0_mask = 0;
  for (auto &xy : pc.pos_qs0) xy[0] = xy[1] = 0.0;
  bool inert_other = false;
  pc.n_ee = n_ee;
  pc.n_gg = n_ee > 1 ? d->n_goal_pairs : 0;
  path.assign((size_t)n_ee * (n + 1), -1);
  for (int e = 0; e < PREP_MAX_EE; ++e) pc.ee_len[e] = (n_ee > 1 && K == 2 && e < n_ee) ? d->ee_goal_len[e] : d->goal_len;
  if (n_ee > 1) {
    for (int g = 0; g < 2 * n_ee; ++g) {
      pc.goal_node[g] = d->ee_goal_nodes[g];
      const bool pos_odd = (g & 1) && ((mask >> (g >> 1)) & 1);      // the odd slot of a position goal
      // -1: a planar tree's parent node that an earlier end effector's pose pins already, or a position goal (odd slots only)
      if (pc.goal_node[g] < 0 && !((K == 2 && (g & 1)) || pos_odd)) return fail("bad ee_goal_nodes");
      if (pc.goal_node[g] >= N) return fail("bad ee_goal_nodes");
      if (pos_odd && pc.goal_node[g] >= 0) return fail(odd_slot);
      inert_goal_slot = inert_goal_slot || pc.goal_node[g] < 0;
      inert_other = inert_other || (pc.goal_node[g] < 0 && !pos_odd);
    }
    for (size_t t = 0; t < path.size(); ++t) path[t] = d->ee_path[t];
    for (int e = 0; e < n_ee; ++e)
      for (int k = 0; k <= n; ++k) {
        const int j = path[(size_t)e * (n + 1) + k];
        if (j < -1 || j > n || (k == 0 && j != 0)) return fail("bad ee_path");
      }
  } else {
    pc.goal_node[0] = d->goal_node0;
    pc.goal_node[1] = d->goal_node1;
    if (mask & 1) {
      if (d->goal_node1 >= 0) return fail(odd_slot);
      inert_goal_slot = true;
    }
    for (int k = 0; k <= n; ++k) path[k] = k;
  }
  position_goals = inert_goal_slot && !inert_other;
  pc.ee_path = upload(t, path.data(), path.size(), ok);

  pc.gg_a = pc.n_gg ? upload(t, d->goal_pair_a, pc.n_gg, ok) : nullptr;
  pc.gg_b = pc.n_gg ? upload(t, d->goal_pair_b, pc.n_gg, ok) : nullptr;
  if (2 * n_ee * d->n_anchor + pc.n_gg > 2 * PREP_MAXA + 16) return fail("too many anchor-goal pairs");
  if (!ok) return fail("device upload failed");
  return 0;
}

// the kernel of a prepare variant: the one place that names the six
static const void *prep_kernel(Prep v) {
  switch (v) {
    case Prep::QUAD13: return (const void *)prep_quad_kernel<13>;
    case Prep::QUAD: return (const void *)prep_quad_kernel<0>;
    case Prep::WAVE: return (const void *)prep_wave_kernel;
    case Prep::BLOCK_LDS: return (const void *)prep_block_kernel<true>;
    case Prep::BLOCK: return (const void *)prep_block_kernel<false>;
    case Prep::BLOCK_BIG: return (const void *)prep_block_kernel<false, PREP_BIGN>;
  }
  return nullptr;
}

// plan_prepare's occupancy answer: resident workgroups per CU, -1 where the query -- for the LDS variant, raising the
// kernel's allowance first -- failed
static int prep_occupancy(Prep v, int threads, size_t lds) {
  int occ = 0;
  if ((v != Prep::BLOCK_LDS || raise_dynamic_lds(prep_kernel(v), lds) == hipSuccess) &&
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, prep_kernel(v), threads, lds) == hipSuccess)
    return occ;
  (void)hipGetLastError();
  return -1;
}

// the prepare kernel of this template (plan_prepare), and the slab and the event of a block variant.  The developer
// switches of the environment are read once, here.
static int plan_and_acquire_prepare(gik_template *t, const gik_pipeline_desc *d, bool inert_goal_slot, bool position_goals) {
  PrepFacts f;
  f.N = t->N;
  f.K = t->f.K;
  f.n_anchor = d->n_anchor;
  f.n_ee = t->pc.n_ee;
  f.n_gg = t->pc.n_gg;
  f.inert_goal_slot = inert_goal_slot;
  f.position_goals = position_goals;
  f.force_block_prepare = d->force_block_prepare != 0;
  f.env_force_block = getenv("GIK_PREP_FORCE_BLOCK") != nullptr;
  f.env_no_compress = getenv("GIK_PREP_NO_COMPRESS") != nullptr;
  f.env_a_global = getenv("GIK_PREP_A_GLOBAL") != nullptr;
  f.env_no_quad = getenv("GIK_NO_PREP_QUAD") != nullptr;
  if (const char *e = getenv("GIK_PREP_WAVES_PER_CU")) {
    f.env_waves_set = true;
    f.env_waves = atoi(e);
  }
  f.n_cu = t->f.n_cu;
  // The Jacobi loops stop by themselves, after the first sweep without a rotation; this is the bound behind that rule.
  // A bound of 10 was the reason to stop on full-rank Gram matrices from about 50 rows on (planar chains: 11 sweeps at
  // N = 47, up to 13 at N = 66 and 15 at N = 123 .. 128, where the spectrum was left at 2e-9 instead of 1e-14 and
  // Gram(Y_init) at 3e-6; NOTEBOOK 36).  Graphs of one wavefront keep 10, and with it every bit of their results.
  t->prep.sweeps = d->jacobi_sweeps > 0 ? d->jacobi_sweeps : (t->N <= 32 ? 10 : 30);
  t->prep.plan = plan_prepare(f, prep_occupancy);
  if (!t->prep.plan.block()) return 0;
  void *ws = nullptr;
  if (hipMalloc(&ws, t->prep.plan.slab_bytes) != hipSuccess) return fail("cannot allocate the prepare workspace");
  t->pipe_allocs.push_back(ws);
  t->prep.ws = static_cast<double *>(ws);
  if (hipEventCreateWithFlags(&t->prep.done, hipEventDisableTiming) != hipSuccess) return fail("hipEventCreate failed");
  return 0;
}

}  // namespace gik

int gik_pipeline_attach(gik_template *t, const gik_pipeline_desc *d) {
  using namespace gik;
  if (validate_pipeline(t, d)) return -1;
  PipeConst pc;
  std::vector<int> path;
  bool inert_goal_slot = false, position_goals = false;
  if (upload_pipe_const(t, d, pc) || end_effector_paths(t, d, pc, path, inert_goal_slot, position_goals)) return -1;
  t->pc = pc;
  if (plan_and_acquire_prepare(t, d, inert_goal_slot, position_goals)) return -1;
  if (!seed_tables(t, d, path, pc.n_ee)) return fail("device upload failed");
  t->has_pipe = true;
  return 0;
}

int gik_pipeline_set_point_axis(gik_template *t, int ee, double x, double y) {
  using namespace gik;
  if (!t) return fail("gik_pipeline_set_point_axis: bad argument");
  if (!t->has_pipe) return fail("gik_pipeline_set_point_axis: no pipeline attached (gik_pipeline_attach)");
  if (t->f.K != 3) return fail("gik_pipeline_set_point_axis: k = 3 only");
  if (ee < 0 || ee >= t->pc.n_ee || !((t->pc.pos_goal_mask >> ee) & 1))
    return fail("gik_pipeline_set_point_axis: ee must be an end effector with a position goal (position_goal_mask)");
  if (!std::isfinite(x) || !std::isfinite(y)) return fail("gik_pipeline_set_point_axis: x and y must be finite");
  t->pc.pos_qs0[ee][0] = x;
  t->pc.pos_qs0[ee][1] = y;
  t->pc.pos_qs0_mask |= 1 << ee;
  return 0;
}

int gik_prepare_batch(const gik_template *t, const double *d_T_goal, int B, double *d_targets,
                      double *d_Y_init, int32_t *d_K_out, void *stream) {
  return gik_prepare_batch_debug(t, d_T_goal, B, d_targets, d_Y_init, d_K_out, nullptr, stream);
}

// One prepare launch.  The block variants share the slab: each launch waits for the one before it, whatever stream that ran on.
static int launch_prepare(const gik_template *t, const gik::PrepPlan &p, gik::PrepArgs a, hipStream_t s) {
  using namespace gik;
  gik_template::Prepare &m = const_cast<gik_template *>(t)->prep;   // the workspace hand-over is the mutable part
  std::unique_lock<std::mutex> lock(m.mutex, std::defer_lock);
  if (p.block()) {
    lock.lock();
    if (m.pending) HIP_OK(hipStreamWaitEvent(s, m.done, 0));
  }
  void *args[] = {&a, &m.ws};      // (the wavefront kernels take the first only)
  (void)hipLaunchKernel(prep_kernel(p.variant), dim3(p.launch_grid(a.B)), dim3(p.threads()), args, p.lds, s);
  if (p.block()) {
    HIP_OK(hipEventRecord(m.done, s));
    m.pending = true;
  }
  HIP_OK(hipGetLastError());
  return 0;
}

int gik_prepare_batch_debug(const gik_template *t, const double *d_T_goal, int B, double *d_targets,
                            double *d_Y_init, int32_t *d_K_out, const gik_prepare_diag *diag,
                            void *stream) {
  using namespace gik;
  if (!t || B < 0) return fail("bad argument");
  if (!t->has_pipe) return fail("no pipeline attached (gik_pipeline_attach)");
  if (B == 0) return 0;
  if (!d_T_goal || !d_targets || !d_Y_init) return fail("null buffer");
  if (t->prep.plan.block() && refuse_capture("gik_prepare_batch", stream)) return -1;      // (the block variants chain their launches by an event)
  PrepArgs a;
  a.pc = t->pc;
  a.T_goal = d_T_goal;
  a.targets = d_targets;
  a.Y_init = d_Y_init;
  a.K_out = d_K_out;
  a.dbg_lb = diag ? diag->d_lb : nullptr;
  a.dbg_ub = diag ? diag->d_ub : nullptr;
  a.dbg_eig = diag ? diag->d_eig : nullptr;
  if ((a.dbg_lb == nullptr) != (a.dbg_ub == nullptr)) return fail("d_lb and d_ub go together");
  a.B = B;
  a.sweeps = t->prep.sweeps;
  a.stop_phase = 0;
  a.no_compress = t->prep.plan.no_compress ? 1 : 0;
#ifdef GIK_DEV
  if (const char *e = getenv("GIK_PREP_STOP")) a.stop_phase = atoi(e);   // developer build: timing of the phases
#endif
  // (the diagnostics -- bounds and spectra -- come from the one-goal-per-wavefront kernel)
  return launch_prepare(t, (a.dbg_lb || a.dbg_eig) ? t->prep.plan.diagnostics() : t->prep.plan, a, (hipStream_t)stream);
}

int gik_recover_batch(const gik_template *t, const double *d_Y, const double *d_T_goal, int B,
                      double *d_q, double *d_pos_err, double *d_rot_err, void *stream) {
  using namespace gik;
  if (!t || B < 0) return fail("bad argument");
  if (!t->has_pipe) return fail("no pipeline attached (gik_pipeline_attach)");
  if (B == 0) return 0;
  if (!d_Y || !d_T_goal || !d_q || !d_pos_err || !d_rot_err) return fail("null buffer");
  RecoverArgs a;
  a.pc = t->pc;
  a.Y = d_Y;
  a.T_goal = d_T_goal;
  a.q = d_q;
  a.pos_err = d_pos_err;
  a.rot_err = d_rot_err;
  a.B = B;
  hipLaunchKernelGGL(recover_kernel, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream, a);
  HIP_OK(hipGetLastError());
  return 0;
}

int gik_ik_batch(const gik_template *t, const double *d_T_goal, int B, double *d_targets,
                 double *d_Y, gik_stats *d_stats, double *d_q, double *d_pos_err,
                 double *d_rot_err, void *stream) {
  int rc = gik_prepare_batch(t, d_T_goal, B, d_targets, d_Y, nullptr, stream);
  if (rc) return rc;
  rc = gik_solve_batch(t, d_Y, d_targets, B, d_Y, d_stats, nullptr, stream);
  if (rc) return rc;
  return gik_recover_batch(t, d_Y, d_T_goal, B, d_q, d_pos_err, d_rot_err, stream);
}

int gik_seed_batch(const gik_template *t, const double *d_T_goal, const double *d_q_init, int B, double *d_targets,
                   double *d_Y_init, void *stream) {
  using namespace gik;
  if (!t || B < 0) return fail("bad argument");
  if (!t->has_pipe) return fail("no pipeline attached (gik_pipeline_attach)");
  if (!t->seed_ok) return fail("gik_seed_batch: this graph cannot be seeded on the device: " + t->seed_why);
  if (B == 0) return 0;
  if (!d_q_init) return fail("gik_seed_batch: null d_q_init (seed joint angles [B][n] are required)");
  if (!d_T_goal || !d_targets || !d_Y_init) return fail("null buffer");
  SeedArgs a;
  a.pc = t->pc;
  a.sc = t->sc;
  a.T_goal = d_T_goal;
  a.q_init = d_q_init;
  a.targets = d_targets;
  a.Y_init = d_Y_init;
  a.B = B;
  const int grid = std::min(B, t->f.n_cu * 8);
  hipLaunchKernelGGL(seed_kernel, dim3(grid), dim3(WAVE), t->seed_smem, (hipStream_t)stream, a);
  HIP_OK(hipGetLastError());
  return 0;
}

int gik_ik_batch_seeded(const gik_template *t, const double *d_T_goal, const double *d_q_init, int B,
                        double *d_targets, double *d_Y, gik_stats *d_stats, double *d_q, double *d_pos_err,
                        double *d_rot_err, void *stream) {
  using namespace gik;
  if (!t || B < 0) return fail("bad argument");
  if (!t->has_pipe) return fail("no pipeline attached (gik_pipeline_attach)");
  if (B == 0) return 0;
  if (!d_q_init) return fail("gik_ik_batch_seeded: null d_q_init (seed joint angles [B][n] are required)");
  if (!d_T_goal || !d_targets || !d_Y || !d_stats || !d_q || !d_pos_err || !d_rot_err) return fail("null buffer");
  // refused before the seed kernel is queued, so that a capture is left without half a call in it
  if (refuse_capture("gik_ik_batch_seeded", stream)) return -1;
  int rc = gik_seed_batch(t, d_T_goal, d_q_init, B, d_targets, d_Y, stream);
  if (rc) return rc;
  rc = gik_solve_batch(t, d_Y, d_targets, B, d_Y, d_stats, nullptr, stream);
  if (rc) return rc;
  return gik_recover_batch(t, d_Y, d_T_goal, B, d_q, d_pos_err, d_rot_err, stream);
}

static int launch_kat(const gik_template *t, int mode, const double *d_Y, const double *d_W,
                      const double *d_targets, int B, double *d_out, void *stream,
                      double *d_out_f = nullptr) {
  using namespace gik;
  if (!t || B < 0) return fail("bad argument");
  if (B == 0) return 0;
  if (!d_Y || !d_out) return fail("null buffer");
  KatArgs a;
  a.out_f = d_out_f;
  a.slot_meta = t->d_slot_meta;
  a.bt = t->bt;
  a.targets = d_targets;
  a.Y = d_Y;
  a.W = d_W;
  a.out = d_out;
  a.N = t->N;
  a.T = t->T;
  a.B = B;
  a.mode = mode;
  a.planar_proj_exact = t->p.planar_proj_exact;
  if (t->anchored && mode == 3) {          // the anchors fix the gauge: proj is the identity
    HIP_OK(hipMemcpyAsync(d_out, d_W, sizeof(double) * (size_t)B * t->N * t->f.K, hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
    return 0;
  }
  if (t->anchored) {
    a.an = t->an;
    a.an.anchor_goal = d_targets;          // (anchored templates: the per-problem input is the goal anchors)
    a.targets = t->d_targets_const;
    a.half = t->d_half;
    a.half_mu = t->d_half_mu;
    a.n_half = t->n_half;
  }
  if (t->quad_solve && (t->f.dbg & 16384) && !(t->f.dbg & (1 | 8192))) {
    hipLaunchKernelGGL(kat_quad_kernel<6>, dim3((B + QUAD_SLOTS - 1) / QUAD_SLOTS), dim3(WAVE), t->quad_smem,
                       (hipStream_t)stream, a);
  } else if (t->f.is_npt) {
    a.nt = t->nt;
    // (graphs beyond 128 nodes: a stream-ordered scratch for the clique target triangles of this call's workgroups;
    //  these one-call-at-a-time entry points are the known-answer interface, not the batch path)
    const size_t ctg = t->f.ctg_doubles * sizeof(double) * (size_t)B;
    void *ws = nullptr;
    if (ctg) HIP_OK(hipMallocAsync(&ws, ctg, (hipStream_t)stream));
    a.npt_ctg_ws = static_cast<double *>(ws);
    hipLaunchKernelGGL(t->npt_variant->kat, dim3(B), dim3(WAVE * t->npt_variant->NW), t->npt_smem, (hipStream_t)stream, a);
    if (ws) HIP_OK(hipFreeAsync(ws, (hipStream_t)stream));
  } else if (t->f.is_block) {
    hipLaunchKernelGGL(t->kernels.block_kat, dim3(B), dim3(BLOCK_NT), t->smem_bytes, (hipStream_t)stream, a, t->SL);
  } else {
    hipLaunchKernelGGL(t->kernels.kat, dim3(B), dim3(WAVE), t->smem_bytes, (hipStream_t)stream, a);
  }
  HIP_OK(hipGetLastError());
  return 0;
}

int gik_cost(const gik_template *t, const double *d_Y, const double *d_targets, int B,
             double *d_f, void *stream) {
  if (!d_targets) return gik::fail("targets required");
  return launch_kat(t, 0, d_Y, nullptr, d_targets, B, d_f, stream);
}
int gik_grad(const gik_template *t, const double *d_Y, const double *d_targets, int B,
             double *d_out, void *stream) {
  if (!d_targets) return gik::fail("targets required");
  return launch_kat(t, 1, d_Y, nullptr, d_targets, B, d_out, stream);
}
int gik_cost_and_grad(const gik_template *t, const double *d_Y, const double *d_targets, int B,
                      double *d_f, double *d_grad, void *stream) {
  if (!d_targets) return gik::fail("targets required");
  if (B > 0 && !d_f) return gik::fail("null buffer");
  return launch_kat(t, 4, d_Y, nullptr, d_targets, B, d_grad, stream, d_f);
}
int gik_hess(const gik_template *t, const double *d_Y, const double *d_W,
             const double *d_targets, int B, double *d_out, void *stream) {
  if (!d_targets || !d_W) return gik::fail("targets and W required");
  return launch_kat(t, 2, d_Y, d_W, d_targets, B, d_out, stream);
}
int gik_proj(const gik_template *t, const double *d_Y, const double *d_Z, int B, double *d_out,
             void *stream) {
  if (!d_Z) return gik::fail("Z required");
  return launch_kat(t, 3, d_Y, d_Z, nullptr, B, d_out, stream);
}

// ---- one batch call, step by step (gik_solve_batch below) ----

#ifdef GIK_DEV
// the dump buffer of debug_flags 4 / 8 / 4096, zeroed for this call (gik_debug_fetch copies it to the host)
static double *dev_debug_buffer() {
  static double *buf = nullptr;
  if (!buf) (void)hipMalloc((void **)&buf, (1 << 20) * sizeof(double));
  (void)hipMemset(buf, 0, (1 << 20) * sizeof(double));
  gik::g_dbg_buf = buf;
  return buf;
}
#endif

// everything of SolveArgs that does not depend on the plan; the queues start out absent
static void fill_args(const gik_template *t, gik::SolveArgs &a, const double *d_Y_init, const double *d_targets, int B,
                      double *d_Y_out, gik_stats *d_stats, const gik_trace *trace) {
  a.slot_meta = t->d_slot_meta;
  a.bt = t->bt;
  a.targets = d_targets;
  a.Y_init = d_Y_init;
  a.Y_out = d_Y_out;
  a.stats = d_stats;
  a.has_trace = (trace && trace->cap > 0) ? 1 : 0;
  if (a.has_trace)
    a.trace = *trace;
  else
    std::memset(&a.trace, 0, sizeof(a.trace));
  a.N = t->N;
  a.T = t->T;
  a.B = B;
  a.p = t->p;
  a.cg = t->cg;
  if (t->anchored) {
    a.an = t->an;
    a.an.anchor_goal = d_targets;          // anchored templates: per-problem goal anchors [B][n_goal*3]
    a.targets = t->d_targets_const;
    a.half = t->d_half;
    a.half_mu = t->d_half_mu;
    a.n_half = t->n_half;
  }
  a.dbg = t->f.dbg;
  a.dbg_buf = nullptr;
  a.claim_order = nullptr;
#ifdef GIK_DEV
  if (a.dbg & (4 | 8 | 4096)) a.dbg_buf = dev_debug_buffer();
#endif
  a.y_head = a.y_tail = a.y_seq = nullptr;
  a.y_ids = a.y_avail = nullptr;
  a.y_cap = 0;
  a.q_tail = a.q_done = a.q_head = nullptr;
  a.mig_credits = a.mig_simd_run = nullptr;
  a.q_ids = nullptr;
  a.q_seq = nullptr;
  a.q_state = nullptr;
}

// "the launch that used this slot last has completed" (gik_slots.h asks it under call_mutex)
static bool event_done(hipEvent_t e) {
  if (hipEventQuery(e) == hipSuccess) return true;
  (void)hipGetLastError();      // (hipErrorNotReady of the query)
  return false;
}

typedef gik::SlotLease<gik_template::CounterSlot> CounterLease;
typedef gik::SlotLease<gik_template::SliceWs> WorkspaceLease;

// a work-queue head of this call's own, zeroed on the stream behind the launch that used it last
static int lease_counter(gik_template *mt, CounterLease &lease, gik::SolveArgs &a, hipStream_t stream) {
  using namespace gik;
  gik_template::CounterSlot &cs = lease.take(mt->counter_slot, mt->next_counter, (unsigned)mt->counter_ring, event_done);
  a.work_counter = mt->d_counters + (&cs - mt->counter_slot.data());
  if (!cs.done && hipEventCreateWithFlags(&cs.done, hipEventDisableTiming) != hipSuccess)
    return fail("hipEventCreate failed");
  if (cs.pending) HIP_OK(hipStreamWaitEvent(stream, cs.done, 0));   // ring wrapped: previous user first
  HIP_OK(hipMemsetAsync(a.work_counter, 0, sizeof(unsigned int), stream));
  return 0;
}

// key and rank kernels (gik_order.hip.h) on the stream: order[0 .. B) = the problems in ascending key order
static void launch_claim_order(const gik::ClaimKey &k, const double *d_targets, int T, int B, float *d_key, int *d_order,
                               hipStream_t stream) {
  using namespace gik;
  if (d_targets) hipLaunchKernelGGL(claim_key_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, d_targets, T, B, k, d_key);
  hipLaunchKernelGGL(claim_rank_kernel, dim3((B + ORDER_ROWS - 1) / ORDER_ROWS), dim3(ORDER_NT), 0, stream, d_key, B, d_order);
}

// a pooled workspace of at least the plan's size (grown outside the lock, behind its previous user), the queue
// pointers of SolveArgs into it, and its memsets on the stream
static int bind_workspace(gik_template *mt, WorkspaceLease &lease, const gik::SolvePlan &p, gik::SolveArgs &a,
                          hipStream_t stream) {
  using namespace gik;
  gik_template::SliceWs *sw = &lease.take(mt->slice_ws, mt->next_slice, (unsigned)mt->slice_pool, event_done);
  if (!sw->done && hipEventCreateWithFlags(&sw->done, hipEventDisableTiming) != hipSuccess)
    return fail("hipEventCreate failed");
  if (sw->bytes < p.bytes) {
    if (sw->pending) (void)hipEventSynchronize(sw->done);
    if (sw->base) (void)hipFree(sw->base);
    sw->base = nullptr;
    sw->bytes = 0;
    if (hipMalloc(&sw->base, p.bytes) != hipSuccess) return fail("cannot allocate the time-slicing workspace");
    sw->bytes = p.bytes;
    sw->pending = false;
  }
  if (sw->pending) HIP_OK(hipStreamWaitEvent(stream, sw->done, 0));
  char *base = static_cast<char *>(sw->base);
  a.q_tail = reinterpret_cast<unsigned int *>(base);
  a.q_done = a.q_tail + 1;
  a.q_head = a.q_tail + 2;
  a.mig_credits = reinterpret_cast<int *>(a.q_tail + 3);
  a.mig_simd_run = reinterpret_cast<int *>(base + p.off_simd);
  a.q_seq = reinterpret_cast<unsigned int *>(base + p.off_seq);
  a.q_ids = reinterpret_cast<int *>(base + p.off_ids);
  a.q_state = reinterpret_cast<SliceState *>(base + p.off_state);
  a.y_head = a.q_tail + 4;
  a.y_tail = a.q_tail + 5;
  a.y_avail = reinterpret_cast<int *>(a.q_tail + 6);
  a.y_seq = reinterpret_cast<unsigned int *>(base + p.off_yseq);
  a.y_ids = reinterpret_cast<int *>(base + p.off_yids);
  a.y_cap = (unsigned int)p.ycap;
  a.npt_ctg_ws = p.ctg_bytes ? reinterpret_cast<double *>(base + p.off_ctg) : nullptr;
  if (p.zero_head) HIP_OK(hipMemsetAsync(base, 0, p.zero_head, stream));
  if (p.seq_fill) HIP_OK(hipMemsetAsync(a.q_seq, 0xFF, p.seq_fill, stream));
  if (p.state_zero) HIP_OK(hipMemsetAsync(a.q_state, 0, p.state_zero, stream));
  if (p.yseq_zero) HIP_OK(hipMemsetAsync(a.y_seq, 0, p.yseq_zero, stream));
  if (p.order) {
    // ticket -> problem, ascending in the template's key of THIS call's targets: two small launches in front of the solve
    float *key = reinterpret_cast<float *>(base + p.off_key);
    int *order = reinterpret_cast<int *>(base + p.off_order);
    launch_claim_order(mt->claim_key, a.targets, a.T, a.B, key, order, stream);
    HIP_OK(hipGetLastError());
    a.claim_order = order;
  }
  return 0;
}

// `scenes`: the scene build of the wavefront kernel instead (anchored templates, whose plan is always Launch::WAVE)
static void launch(const gik_template *t, const gik::SolvePlan &p, gik::SolveArgs &a, const gik::SceneArgs *scenes,
                   hipStream_t stream) {
  using namespace gik;
  const dim3 grid(p.launch_grid);
  if (scenes) {
    hipLaunchKernelGGL(t->kernels.solve_scene, grid, dim3(WAVE), t->smem_bytes, stream, a, *scenes);
    return;
  }
  switch (p.launch) {
    case Launch::QUAD:
      hipLaunchKernelGGL(t->quad_solve, grid, dim3(WAVE), t->quad_smem, stream, a);
      break;
    case Launch::NPT:
      a.nt = t->nt;
      hipLaunchKernelGGL(t->npt_variant->solve, grid, dim3(WAVE * t->npt_variant->NW), t->npt_smem, stream, a);
      break;
    case Launch::BLOCK:
      hipLaunchKernelGGL(t->kernels.block_solve, grid, dim3(BLOCK_NT), t->smem_bytes, stream, a, t->SL);
      break;
    case Launch::WAVE:
      hipLaunchKernelGGL(t->kernels.solve, grid, dim3(WAVE), t->smem_bytes, stream, a);
      break;
    case Launch::WAVE_SPREAD:
      hipLaunchKernelGGL(t->kernels.solve_spread, grid, dim3(WAVE), t->smem_bytes, stream, a);
      break;
  }
}

// gik_solve_batch, and with a (checked) scene set gik_solve_batch_scenes
static int solve_batch_impl(const char *entry, const gik_template *t, const double *d_Y_init, const double *d_targets,
                            int B, double *d_Y_out, gik_stats *d_stats, const gik_trace *trace, const gik_scene_set *scenes,
                            void *stream_) {
  using namespace gik;
  if (B == 0) return 0;
  if (!d_Y_init || !d_targets || !d_Y_out || !d_stats) return fail("null buffer");
  hipStream_t stream = (hipStream_t)stream_;
  SolveArgs a;
  fill_args(t, a, d_Y_init, d_targets, B, d_Y_out, d_stats, trace);
  SceneArgs sa;
  if (scenes) {      // the template's own spheres play no part: the kernel walks the rows of each problem's scene
    sa = scene_args(scenes);
    a.an.obs = scenes->d_obs;
    a.an.n_obs = 0;
  }
  // Stream capture is refused: the slot protocol below queries, waits for and records events, grows workspaces
  // (hipMalloc / hipFree) and resets a counter the kernel consumes -- none of which may happen under capture, and a
  // replayed graph would reuse this call's counter slot and workspace behind the library's back.  A batch is ONE
  // persistent launch; there is no launch overhead for a graph to remove.
  if (refuse_capture(entry, stream_)) return -1;
  const SolvePlan plan = plan_solve(t->f, B);
  if (scenes && plan.launch != Launch::WAVE) return fail(std::string(entry) + ": the template's plan is not the wavefront kernel");
  a.slice_its = plan.slice_its;
  a.slice_cycles = plan.slice_cycles;
  // The handle's mutable parts: the ring of work-queue heads and the time-slicing workspaces.  Each is leased
  // under call_mutex (gik_slots.h) and held until the event that guards its reuse is recorded, so concurrent calls
  // on one handle (any number of host threads and streams) are safe; every return hands the leases back.
  gik_template *mt = const_cast<gik_template *>(t);
  CounterLease counter(mt->call_mutex);
  WorkspaceLease workspace(mt->call_mutex);
  if (lease_counter(mt, counter, a, stream)) return -1;
  if (plan.needs_ws && bind_workspace(mt, workspace, plan, a, stream)) return -1;
  launch(t, plan, a, scenes ? &sa : nullptr, stream);
  HIP_OK(hipGetLastError());
  // The slots go back "pending" only behind an event that really covers this launch.  If a record fails,
  // nothing guards the counter / workspace against the next caller: wait for the kernel here and hand the
  // slots back idle instead.
  const hipError_t e_cs = hipEventRecord(counter.get()->done, stream);
  const hipError_t e_sw = workspace.get() ? hipEventRecord(workspace.get()->done, stream) : hipSuccess;
  if (e_cs != hipSuccess || e_sw != hipSuccess) {
    (void)hipStreamSynchronize(stream);
    return fail(std::string("hipEventRecord failed after the launch: ") + hipGetErrorString(e_cs != hipSuccess ? e_cs : e_sw));
  }
  counter.covered_by_event();
  workspace.covered_by_event();
  return 0;
}

int gik_solve_batch(const gik_template *t, const double *d_Y_init, const double *d_targets,
                    int B, double *d_Y_out, gik_stats *d_stats, const gik_trace *trace,
                    void *stream_) {
  if (!t || B < 0) return gik::fail("bad argument");
  return solve_batch_impl("gik_solve_batch", t, d_Y_init, d_targets, B, d_Y_out, d_stats, trace, nullptr, stream_);
}

int gik_solve_batch_scenes(const gik_template *t, const double *d_Y_init, const double *d_targets, int B, double *d_Y_out,
                           gik_stats *d_stats, const gik_trace *trace, const gik_scene_set *scenes, void *stream_) {
  if (!t || B < 0) return gik::fail("gik_solve_batch_scenes: bad argument");
  if (scene_refusal("gik_solve_batch_scenes", t, scenes) || refuse_capture("gik_solve_batch_scenes", stream_)) return -1;
  return solve_batch_impl("gik_solve_batch_scenes", t, d_Y_init, d_targets, B, d_Y_out, d_stats, trace, scenes, stream_);
}

int gik_template_set_claim_key(gik_template *t, int n, const int32_t *terms, const double *weights) {
  using namespace gik;
  if (!t) return fail("null argument");
  if (n > 0 && !weights) return fail("claim key: weights required");
  if (!claim_key_ok(n, terms, t->T))
    return fail("claim key: at most " + std::to_string(PLAN_CLAIM_KEY_MAX_TERMS) + " terms, each an index into the template's " +
                std::to_string(t->T) + " terms");
  // only the 3-D trust-region wavefront kernels order their claims: any other template takes the call and stays on
  // index order (the caller need not know which kernels a graph got; gik_template_get_info says what is in effect)
  if (t->anchored || t->f.is_block || t->f.K != 3 || t->f.cg) n = 0;
  // GIK_CLAIM_ORDER=off (developer override, like GIK_DBG): every template stays on index order
  if (const char *e = getenv("GIK_CLAIM_ORDER"))
    if (!std::strcmp(e, "off") || !std::strcmp(e, "0")) n = 0;
  ClaimKey k;
  k.n = n;
  for (int i = 0; i < n; ++i) {
    k.term[i] = terms[i];
    k.w[i] = weights[i];
  }
  std::lock_guard<std::mutex> lock(t->call_mutex);      // (calls in flight keep the plan they made)
  t->claim_key = k;
  t->f.claim_terms = n;
  return 0;
}

int gik_claim_order_max_batch(void) { return gik::PLAN_CLAIM_ORDER_MAX_BATCH; }

int gik_claim_order_keys(const gik_template *t, const double *d_targets, int B, float *d_keys, void *stream) {
  using namespace gik;
  if (!t || B < 0) return fail("bad argument");
  if (t->claim_key.n == 0) return fail("the template has no claim key");
  if (B == 0) return 0;
  if (!d_targets || !d_keys) return fail("null buffer");
  hipLaunchKernelGGL(claim_key_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, d_targets, t->T, B,
                     t->claim_key, d_keys);
  HIP_OK(hipGetLastError());
  return 0;
}

int gik_claim_order_sort(const float *d_keys, int B, int32_t *d_order, void *stream) {
  using namespace gik;
  if (B < 0 || B > PLAN_CLAIM_ORDER_MAX_BATCH) return fail("claim order: 0 .. " + std::to_string(PLAN_CLAIM_ORDER_MAX_BATCH) + " keys");
  if (B == 0) return 0;
  if (!d_keys || !d_order) return fail("null buffer");
  launch_claim_order(ClaimKey(), nullptr, 0, B, const_cast<float *>(d_keys), d_order, (hipStream_t)stream);
  HIP_OK(hipGetLastError());
  return 0;
}

int gik_template_get_info(const gik_template *t, gik_template_info *info) {
  if (!t || !info) return gik::fail("null argument");
  std::memset(info, 0, sizeof(*info));
  info->is_block = t->f.is_block ? 1 : 0;
  info->max_terms_per_node = t->f.is_block ? 0 : t->maxdeg;
  info->n_clique = t->bt.n_clq;
  info->n_slot_terms = t->f.is_block ? t->bt.Tc : t->T;
  info->slots_per_thread = t->SL;
  info->waves_per_cu = t->f.waves_per_cu;
  info->n_cu = t->f.n_cu;
  info->lds_bytes = (int32_t)t->smem_bytes;
  info->clique_closed_form = t->clique_mode;
  info->hessian_form = (t->hess_per_edge || t->f.is_block) ? GIK_HESS_PER_EDGE : GIK_HESS_COLUMN;
  const unsigned build = t->anchored ? gik::anchored_build(t) : 0u;      // (the ABI's bits are not the W_* bits: mapped one by one)
  info->anchored = (build & gik::W_ANCH ? 1 : 0) | (build & gik::W_LINKS ? 2 : 0) | (build & gik::W_SELF ? 4 : 0) | (build & gik::W_HALF ? 8 : 0);
  info->has_pipeline = t->has_pipe ? 1 : 0;
  info->prepare_is_block = t->prep.plan.block() ? 1 : 0;
  info->node_per_lane = t->f.is_npt ? t->npt_variant->NW : 0;
  info->goals_per_wave = !t->has_pipe || t->prep.plan.block() ? 0 : (t->prep.plan.quad() ? gik::QUAD_SLOTS : 1);
  info->claim_key_terms = t->f.claim_terms;
  info->problems_per_wave = t->f.is_block ? 0 : ((t->quad_solve && !(t->f.dbg & (1 | 8192))) ? gik::QUAD_SLOTS : 1);
  if (t->f.is_npt) {
    info->waves_per_cu = t->f.npt_waves_per_cu;
    info->lds_bytes = (int32_t)t->npt_smem;
  }
  return 0;
}

#ifdef GIK_DEV
// developer hook (not part of the ABI header): cycles per iteration of one kernel component
double gik_debug_parts(const gik_template *t, int mode, int iters) {
  using namespace gik;
  double *d = nullptr, h[2] = {0, 0};
  if (hipMalloc((void **)&d, 2 * sizeof(double)) != hipSuccess) return -1;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  (void)hipEventRecord(e0, 0);
  if (t->f.K == 3 && t->maxdeg == 9)
    hipLaunchKernelGGL((parts_kernel<3, 9>), dim3(1), dim3(WAVE), t->smem_bytes, 0, t->d_slot_meta,
                       t->N, t->T, mode % 100, iters, d);
  else if (t->f.K == 3 && t->maxdeg == 10)
    hipLaunchKernelGGL((parts_kernel<3, 10>), dim3(1), dim3(WAVE), t->smem_bytes, 0, t->d_slot_meta,
                       t->N, t->T, mode % 100, iters, d);
  else if (t->f.K == 3)
    return -1;
  else
    hipLaunchKernelGGL((parts_kernel<2, 6>), dim3(1), dim3(WAVE), t->smem_bytes, 0, t->d_slot_meta,
                       t->N, t->T, mode % 100, iters, d);
  (void)hipEventRecord(e1, 0);
  (void)hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipFree(d);
  if (mode >= 100) return ms * 1e6 / iters;  // ns per iteration (wall)
  return h[0];
}

// developer hook (not part of the ABI header): copy the GIK_DBG=4 dump to the host
int gik_debug_fetch(double *host, int n) {
  if (!gik::g_dbg_buf) return -1;
  return hipMemcpy(host, gik::g_dbg_buf, sizeof(double) * n, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif  // GIK_DEV

}  // extern "C"
