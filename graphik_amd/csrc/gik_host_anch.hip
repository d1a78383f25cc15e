// graphik_amd/csrc/gik_host_anch.hip -- the second host unit: the restarts and the fixed-anchor (obstacle) solve, with
// their part of the C ABI of include/graphik_amd.h.  A client of gik_host.hip: it reaches templates and the prepare / seed /
// solve / recover path only through the library's exports and the helpers of gik_handle.h (gik_anchored_attach_links is
// creation and lives there).  It launches the plain kernels of gik_retry.hip.h, gik_atlas.hip.h, gik_anch_seed.hip.h and
// gik_anch_glue.hip.h by their prototypes: no device code is compiled here, and no solve kernel's header is seen.
// Written once: a kernel launch (launch), the refusal pair of a workspace (workspace_refusal), one anchored solve
// (anchored_attempt), the screened seed step behind its two exports (screened_step_entry) and the restart driver behind the
// four restart entries (anchored_restarts), which takes where the seeds come from as a value (SeedSource).

#include "gik_handle.h"
#include "gik_retry.hip.h"
#include "gik_atlas.hip.h"
#include "gik_anch_glue.hip.h"
#include "gik_anch_seed.hip.h"
#include "gik_plan.h"
#include "gik_scenes.h"
#include <algorithm>
#include <climits>

// doubles of one goal: a (K+1) x (K+1) pose per end effector
static int pose_width(const gik_template *t) { return t->pc.n_ee * (t->f.K + 1) * (t->f.K + 1); }

// one kernel launch of this unit: no dynamic LDS; 0, or -1 with the launch error as the message
template <typename... Params, typename... Args>
static int launch(void (*kernel)(Params...), dim3 grid, dim3 block, void *stream, const Args &...args) {
  using gik::fail;
  hipLaunchKernelGGL(kernel, grid, block, 0, (hipStream_t)stream, args...);
  HIP_OK(hipGetLastError());
  return 0;
}

// the refusal pair of a caller-owned workspace, under the entry's name e; size_query: the export that says how large it is
static int workspace_refusal(const std::string &e, const void *d_ws, const char *size_query) {
  if (!d_ws) return gik::fail(e + ": null workspace (" + size_query + ")");
  if ((uintptr_t)d_ws % 8) return gik::fail(e + ": the workspace must be 8-byte aligned");
  return 0;
}

// ---- restarts from random joint configurations (gik_retry.hip.h) --------------------------------------
// The three launches behind gik_retry_* and gik_anchored_retry_*.  Those exports make their refusals and fill the arguments,
// in the order of the structs; the plain ones have no clearance (null pointers: +inf, and any positive clear_tol), no centre
// and spread 0.  t gives the grid (the anchored calls: the base template).
static int retry_select_launch(const gik::RetrySelectArgs &a, void *stream) {
  using namespace gik;
  return launch(retry_select_kernel, dim3((a.B + RETRY_WAVE - 1) / RETRY_WAVE), dim3(RETRY_WAVE), stream, a);
}

static int retry_grid(const gik_template *t, int count) { return std::min(count, t->f.n_cu * 8); }

static int retry_seed_launch(const gik_template *t, const gik::RetrySeedArgs &a, void *stream) {
  return launch(gik::retry_seed_kernel, dim3(retry_grid(t, a.count)), dim3(gik::RETRY_WAVE), stream, a);
}

static int retry_merge_launch(const gik_template *t, const gik::RetryMergeArgs &a, void *stream) {
  return launch(gik::retry_merge_kernel, dim3(retry_grid(t, a.count)), dim3(gik::RETRY_WAVE), stream, a);
}

// gik_retry_select and, with a clearance in the rule, gik_anchored_retry_select, which says its name (e) in every message.
// (The seeds and the merge exports stay pairs: they word their pipeline refusals differently and test different handles.)
static int retry_select_entry(const std::string &e, bool with_clearance, const gik::RetrySelectArgs &a, void *stream) {
  using gik::fail;
  if (a.B < 0) return fail(e + "bad argument");
  if (!a.idx || !a.count) return fail(e + "null buffer");
  HIP_OK(hipMemsetAsync(a.count, 0, sizeof(int32_t), (hipStream_t)stream));
  if (a.B == 0) return 0;
  if (!a.stats || !a.pos_err || !a.rot_err || (with_clearance && !a.clearance)) return fail(e + "null buffer");
  return retry_select_launch(a, stream);
}
int gik_retry_select(const gik_stats *d_stats, const double *d_pos_err, const double *d_rot_err, int B, double pos_tol,
                     double rot_tol, int32_t *d_idx, int32_t *d_count, void *stream) {
  return retry_select_entry("", false, {d_stats, d_pos_err, d_rot_err, nullptr, {pos_tol, rot_tol, 1.0}, d_idx, d_count, B}, stream);
}

int gik_retry_seeds(const gik_template *t, const double *d_T_goal, const int32_t *d_idx, int count, uint64_t seed,
                    int attempt, const double *d_q_lo, const double *d_q_hi, double *d_T_out, double *d_q_out,
                    void *stream) {
  using namespace gik;
  if (!t || count < 0) return fail("bad argument");
  if (!t->has_pipe) return fail("no pipeline attached (gik_pipeline_attach)");
  if (attempt < 0 || attempt > 63) return fail("gik_retry_seeds: attempt must be within 0 .. 63");
  if (!d_q_lo || !d_q_hi) return fail("gik_retry_seeds: null joint limits (d_q_lo / d_q_hi, [n] each, are required)");
  if (count == 0) return 0;
  if (!d_T_goal || !d_idx || !d_T_out || !d_q_out) return fail("null buffer");
  const RetrySeedArgs a = {d_T_goal, d_idx, d_q_lo, d_q_hi, nullptr, d_T_out, d_q_out, 0.0, seed,
                           count, pose_width(t), t->pc.n_joints, attempt};
  return retry_seed_launch(t, a, stream);
}

int gik_retry_merge(const gik_template *t, const int32_t *d_idx, int count, int attempt, double pos_tol, double rot_tol,
                    const double *d_Y_r, const gik_stats *d_stats_r, const double *d_q_r, const double *d_pos_err_r,
                    const double *d_rot_err_r, double *d_Y, gik_stats *d_stats, double *d_q, double *d_pos_err,
                    double *d_rot_err, int32_t *d_attempt, void *stream) {
  using namespace gik;
  if (!t || count < 0) return fail("bad argument");
  if (!t->has_pipe) return fail("no pipeline attached (gik_pipeline_attach)");
  if (count == 0) return 0;
  if (!d_idx || !d_Y_r || !d_stats_r || !d_q_r || !d_pos_err_r || !d_rot_err_r || !d_Y || !d_stats || !d_q ||
      !d_pos_err || !d_rot_err || !d_attempt)
    return fail("null buffer");
  const RetryMergeArgs a = {d_idx,
                            d_Y_r, d_stats_r, d_q_r, d_pos_err_r, d_rot_err_r, nullptr,
                            d_Y, d_stats, d_q, d_pos_err, d_rot_err, nullptr, d_attempt,
                            {pos_tol, rot_tol, 1.0}, count, t->N * t->f.K, t->pc.n_joints, attempt};
  return retry_merge_launch(t, a, stream);
}

// the caller-owned workspace of gik_ik_batch_retry over d_ws (gik_plan.h), or with a null d_ws its size
static gik::RetryWs retry_ws(const gik_template *t, int B, void *d_ws) {
  return gik::retry_ws(t->pc.n_joints, pose_width(t), t->T, t->N, t->f.K, B, d_ws);
}

size_t gik_retry_ws_bytes(const gik_template *t, int B) {
  if (!t || !t->has_pipe || B < 0) return 0;
  return retry_ws(t, B, nullptr).bytes;
}

// The restart loop of gik_ik_batch_retry and the anchored restart entries, after their attempt 0.  The caller fills the three
// argument structs as the step exports fill them, but for count and attempt number, and its own refusals have ruled out
// what those exports refuse (NOTEBOOK 31); seed_step(seeds) queues the seeds of the compact slots (retry_seed_launch, or
// the screened step); attempt(count) queues one solve of the compact arrays.  t gives the grid.
template <typename SeedStep, typename Attempt>
static int retry_loop(const char *entry, const gik_template *t, int retries, const gik::RetrySelectArgs &select,
                      gik::RetrySeedArgs seeds, gik::RetryMergeArgs merge, void *stream, SeedStep seed_step, Attempt attempt) {
  using gik::fail;
  hipStream_t s = (hipStream_t)stream;
  for (int a = 1, rc = 0; a <= retries; ++a) {
    HIP_OK(hipMemsetAsync(select.count, 0, sizeof(int32_t), s));
    if ((rc = retry_select_launch(select, stream))) return rc;
    // the solve kernels take their batch size from the host: the failed-goal count comes back, the stream drains
    int32_t count = 0;
    HIP_OK(hipMemcpyAsync(&count, select.count, sizeof(count), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (count < 0 || count > select.B) return fail(std::string(entry) + ": the failed-goal count came back out of range");
    if (count == 0) break;
    seeds.count = merge.count = count;
    seeds.attempt = merge.attempt_no = a;
    if ((rc = seed_step(seeds)) || (rc = attempt(count)) || (rc = retry_merge_launch(t, merge, stream))) return rc;
  }
  return 0;
}

int gik_ik_batch_retry(const gik_template *t, const double *d_T_goal, const double *d_q_init, int B,
                       const gik_retry_opts *opts, void *d_ws, double *d_targets, double *d_Y, gik_stats *d_stats,
                       double *d_q, double *d_pos_err, double *d_rot_err, int32_t *d_attempt, void *stream) {
  using namespace gik;
  // every refusal comes before anything is queued
  if (!t || B < 0 || !opts) return fail("bad argument");
  if (!t->has_pipe) return fail("gik_ik_batch_retry: no pipeline attached (gik_pipeline_attach)");
  if (opts->retries < 0 || opts->retries > 63) return fail("gik_ik_batch_retry: retries must be within 0 .. 63");
  if (opts->retries > 0) {
    if (!t->seed_ok) return fail("gik_ik_batch_retry: this graph cannot be seeded on the device: " + t->seed_why);
    if (!opts->d_q_lo || !opts->d_q_hi)
      return fail("gik_ik_batch_retry: null joint limits (opts->d_q_lo / d_q_hi, [n] each, are what the seeds are drawn from)");
    if (!(opts->pos_tol > 0.0) || !(opts->rot_tol > 0.0)) return fail("gik_ik_batch_retry: pos_tol and rot_tol must be positive");
    if ((d_ws || B > 0) && workspace_refusal("gik_ik_batch_retry", d_ws, "gik_retry_ws_bytes")) return -1;      // (B == 0: may be null)
  }
  if (refuse_capture("gik_ik_batch_retry", stream)) return -1;
  if (B == 0) return 0;
  if (!d_T_goal || !d_targets || !d_Y || !d_stats || !d_q || !d_pos_err || !d_rot_err || !d_attempt) return fail("null buffer");
  HIP_OK(hipMemsetAsync(d_attempt, 0, (size_t)B * sizeof(int32_t), (hipStream_t)stream));
  const int rc = d_q_init ? gik_ik_batch_seeded(t, d_T_goal, d_q_init, B, d_targets, d_Y, d_stats, d_q, d_pos_err, d_rot_err, stream)
                          : gik_ik_batch(t, d_T_goal, B, d_targets, d_Y, d_stats, d_q, d_pos_err, d_rot_err, stream);
  if (rc) return rc;
  const RetryWs w = retry_ws(t, B, d_ws);
  const RetryTol tol = {opts->pos_tol, opts->rot_tol, 1.0};
  const RetrySelectArgs select = {d_stats, d_pos_err, d_rot_err, nullptr, tol, w.idx, w.count, B};
  const RetrySeedArgs seeds = {d_T_goal, w.idx, opts->d_q_lo, opts->d_q_hi, nullptr, w.T, w.q_seed, 0.0, opts->seed,
                               0, pose_width(t), t->pc.n_joints, 0};
  const RetryMergeArgs merge = {w.idx, w.Y, w.stats, w.q, w.pos_err, w.rot_err, nullptr,
                                d_Y, d_stats, d_q, d_pos_err, d_rot_err, nullptr, d_attempt, tol, 0, t->N * t->f.K, t->pc.n_joints, 0};
  const auto seed_step = [&](const RetrySeedArgs &a) { return retry_seed_launch(t, a, stream); };
  return retry_loop("gik_ik_batch_retry", t, opts->retries, select, seeds, merge, stream, seed_step, [&](int count) {
    int rc = gik_seed_batch(t, w.T, w.q_seed, count, w.targets, w.Y, stream);
    if (!rc) rc = gik_solve_batch(t, w.Y, w.targets, count, w.Y, w.stats, nullptr, stream);
    return rc ? rc : gik_recover_batch(t, w.Y, w.T, count, w.q, w.pos_err, w.rot_err, stream);
  });
}

// ---- the fixed-anchor (obstacle) solve on the robot graph's pipeline -------------------------------------------------
// Every solve entry -- cold, seeded, with scenes, and each attempt of the restart loop -- refuses what it has always
// refused, under its own name, and then queues its work through anchored_attempt, the one place that writes the launch
// sequence.  The four obstacle clearance exports are anchored_clearance_entry with two booleans; clearance_mode_refusal is the mode
// check of the scene entry and the restart entries.  The helpers stand in order of use.  The layouts of the caller-owned
// workspaces are gik_plan.h's; the wrappers here read their integers off the handles.

// the scratch of one anchored call over d_ws (gik_plan.h), or with a null d_ws its size
static gik::AnchWs anch_ws(const gik_template *anch, const gik_template *base, int B, double *d_ws) {
  return gik::anch_ws(base->T, base->N, anch->N, anch->an.n_goal, B, d_ws);
}

size_t gik_anchored_ws_doubles(const gik_template *anch, const gik_template *base, int B) {
  if (!anch || !base || !anch->anchored || B < 0) return 0;
  return anch_ws(anch, base, B, nullptr).doubles;
}

// the arguments of the glue kernels between the robot-graph pipeline and the anchored solve
static gik::AnchGlueArgs anch_glue_args(const gik_template *anch, const double *d_T_goal, int B, const double *Y_full_in,
                                        double *Y_free, double *goal, double *Y_full_out) {
  gik::AnchGlueArgs g;
  g.T_goal = d_T_goal;
  g.Y_full_in = Y_full_in;
  g.Y_free = Y_free;
  g.anchor_goal = goal;
  g.Y_full_out = Y_full_out;
  g.anch_const = anch->an.anch_const;
  g.free_full = anch->d_free_full;
  g.anchor_full = anch->d_anchor_full;
  g.B = B;
  g.Nf = anch->N;
  g.full_N = anch->full_N;
  g.n_anchor = anch->n_anchor;
  g.n_goal = anch->an.n_goal;
  g.goal_row0 = anch->an.goal_row0;
  g.axis_length = anch->axis_length;
  return g;
}

// What is wrong with the handle pair of an anchored call, or nothing: anch is a fixed-anchor template and base the robot
// graph it was cut from, full_N nodes with its pipeline attached.  PAIR_3D: base is also 3-D; PAIR_SEEDABLE: and can be seeded
// on the device.  Each entry names the terms it has always tested.  (Non-null handles.)
enum { PAIR_3D = 1, PAIR_SEEDABLE = 2 };
static std::string anchored_pair_fault(const gik_template *anch, const gik_template *base, int terms) {
  if (!anch->anchored) return "the first handle must be a fixed-anchor template (gik_template_create_anchored)";
  if (!base->has_pipe || ((terms & PAIR_3D) && base->f.K != 3) || base->N != anch->full_N)
    return "the base template must be the robot graph (full_N nodes) with its pipeline attached";
  if (base->pc.pos_goal_mask)
    return "the base template has position goals (position_goal_mask); the fixed-anchor formulation takes pose goals";
  if ((terms & PAIR_SEEDABLE) && !base->seed_ok) return "the base graph cannot be seeded on the device: " + base->seed_why;
  return std::string();
}

// (scenes: a checked scene set, or null: the template's own obstacles)
static int anchored_clearance_launch(const gik_template *anch, const double *d_Y_full, int B, double *d_clearance,
                                     void *stream, const gik_scene_set *scenes = nullptr) {
  using namespace gik;
  AnchClearArgs c;
  c.Y_full = d_Y_full;
  c.obs = scenes ? scenes->d_obs : anch->an.obs;
  c.node_full = anch->d_clear_full;
  c.clearance = d_clearance;
  c.B = B;
  c.full_N = anch->full_N;
  c.n_node = anch->n_clear;
  c.n_obs = scenes ? 0 : anch->an.n_obs;
  const dim3 grid(std::min(B, anch->f.n_cu * 32));
  return scenes ? launch(anch_clearance_scene_kernel, grid, dim3(WAVE), stream, c, scene_args(scenes))
                : launch(anch_clearance_kernel, grid, dim3(WAVE), stream, c);
}

// the same of whole links (gik_anchored_attach_links; gik_anch_seed.hip.h)
static int anchored_link_clearance_launch(const gik_template *anch, const double *d_Y_full, int B, double *d_clearance,
                                          void *stream, const gik_scene_set *scenes = nullptr) {
  using namespace gik;
  AnchLinkArgs c;
  c.Y_full = d_Y_full;
  c.obs = scenes ? scenes->d_obs : anch->an.obs;
  c.link_a = anch->d_link_a;
  c.link_b = anch->d_link_b;
  c.link_rho = anch->d_link_rho;
  c.clearance = d_clearance;
  c.B = B;
  c.full_N = anch->full_N;
  c.n_link = anch->n_link;
  c.n_obs = scenes ? 0 : anch->an.n_obs;
  const dim3 grid(std::min(B, anch->f.n_cu * 32));
  return scenes ? launch(anch_link_clearance_scene_kernel, grid, dim3(WAVE), stream, c, scene_args(scenes))
                : launch(anch_link_clearance_kernel, grid, dim3(WAVE), stream, c);
}

// link against link (gik_anchored_attach_self_pairs; gik_anch_seed.hip.h): up to 16 pairs four goals share a wavefront.
// merge: the minimum with what d_clearance holds, the link clearance of the same points queued before it on the stream.
static int anchored_self_clearance_launch(const gik_template *anch, const double *d_Y_full, int B, double *d_clearance,
                                          bool merge, void *stream) {
  using namespace gik;
  AnchSelfArgs c;
  c.Y_full = d_Y_full;
  c.link_a = anch->d_link_a;
  c.link_b = anch->d_link_b;
  c.link_rho = anch->d_link_rho;
  c.pair_l = anch->d_self_l;
  c.pair_m = anch->d_self_m;
  c.clearance = d_clearance;
  c.B = B;
  c.full_N = anch->full_N;
  c.n_pair = anch->n_self;
  c.merge = merge ? 1 : 0;
  const int waves = c.n_pair <= ANCH_SELF_ROW ? (B + 3) / 4 : B;
  return launch(anch_self_clearance_kernel, dim3(std::min(waves, anch->f.n_cu * 32)), dim3(WAVE), stream, c);
}

// against the half-spaces of gik_anchored_attach_halfspaces (the handle has some): the masked nodes with their margins, or
// with links the attached links with their radii.  merge: the minimum with what d_clearance holds.
static int anchored_half_clearance_launch(const gik_template *anch, const double *d_Y_full, int B, double *d_clearance, bool links,
                                          bool merge, void *stream) {
  using namespace gik;
  AnchHalfArgs c;
  c.Y_full = d_Y_full;
  c.half = anch->d_half;
  c.row_a = links ? anch->d_link_a : anch->d_clear_full;
  c.row_b = links ? anch->d_link_b : nullptr;
  c.margin = links ? anch->d_link_rho : anch->d_half_mu_clear;
  c.clearance = d_clearance;
  c.B = B;
  c.full_N = anch->full_N;
  c.n_item = links ? anch->n_link : anch->n_clear;
  c.n_half = anch->n_half;
  c.merge = merge ? 1 : 0;
  return launch(anch_half_clearance_kernel, dim3(std::min(B, anch->f.n_cu * 32)), dim3(WAVE), stream, c);
}

// on a handle with half-spaces every clearance the library reports is the minimum of the spheres' and theirs: the merge
// launch behind the sphere launch, on the same stream
static int fold_halfspaces(const gik_template *anch, const double *d_Y_full, int B, double *d_clearance, bool links, void *stream) {
  return anch->n_half > 0 ? anchored_half_clearance_launch(anch, d_Y_full, B, d_clearance, links, true, stream) : 0;
}

// the clearance of one clearance_mode (checked: clearance_mode_refusal) of B point matrices.  GIK_CLEARANCE_LINKS_SELF:
// the link launch, then the self kernel merging into its output -- the self clearance does not depend on the scene.
static int anchored_mode_clearance_launch(const gik_template *anch, const double *d_Y_full, int B, double *d_clearance, int mode,
                                          void *stream, const gik_scene_set *scenes) {
  if (mode == GIK_CLEARANCE_NODES) {
    const int rc = anchored_clearance_launch(anch, d_Y_full, B, d_clearance, stream, scenes);
    return rc ? rc : fold_halfspaces(anch, d_Y_full, B, d_clearance, false, stream);
  }
  int rc = anchored_link_clearance_launch(anch, d_Y_full, B, d_clearance, stream, scenes);
  if (!rc && mode != GIK_CLEARANCE_LINKS) rc = anchored_self_clearance_launch(anch, d_Y_full, B, d_clearance, true, stream);
  return rc ? rc : fold_halfspaces(anch, d_Y_full, B, d_clearance, true, stream);      // (the room is the same in every scene)
}

// the start point from joint-configuration seeds (gik_anch_seed.hip.h): seed_kernel on the robot graph into the workspace,
// then the row gather + goal anchors
static int anchored_seed_launch(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                                const double *d_q_init, int B, double *d_ws, double *Y_free, double *goal, void *stream) {
  using namespace gik;
  const AnchWs w = anch_ws(anch, base, B, d_ws);      // (its head: Y_free and goal may be the caller's own arrays)
  const int rc = gik_seed_batch(base, d_T_goal, d_q_init, B, w.targets, w.Y_full0, stream);
  if (rc) return rc;
  const AnchGlueArgs g = anch_glue_args(anch, d_T_goal, B, w.Y_full0, Y_free, goal, nullptr);
  const size_t n = (size_t)B * ((size_t)g.Nf + (size_t)g.n_goal) * 3;
  return launch(anch_scatter_kernel, dim3((unsigned)((n + ANCH_SCATTER_NT - 1) / ANCH_SCATTER_NT)), dim3(ANCH_SCATTER_NT), stream, g);
}

// One anchored solve on checked arguments, B > 0: what every solve entry and every restart queues.  The start point, cold
// (d_q_init null: the robot graph's prepare, fitted to the anchors) or seeded; the solve between the event pair of
// gik_anchored_last_solve_ms; the gather into d_Y_full; the recovery; and, where d_clearance is given, the clearance of the
// answer in the call's clearance_mode (`mode`: nodes, whole links, or links and self pairs).  scenes: a checked scene set for the solve and the
// clearance, or null: the template's own obstacles.
static int anchored_attempt(const gik_template *anch, const gik_template *base, const double *d_T_goal, const double *d_q_init,
                            int B, const gik_scene_set *scenes, double *d_ws, double *d_Y_full, gik_stats *d_stats, double *d_q,
                            double *d_pos_err, double *d_rot_err, double *d_clearance, int mode, void *stream) {
  using namespace gik;
  const AnchWs w = anch_ws(anch, base, B, d_ws);
  AnchGlueArgs g;
  if (d_q_init) {      // (read here and nowhere later: d_q_init may be d_q)
    const int rc = anchored_seed_launch(anch, base, d_T_goal, d_q_init, B, d_ws, w.Y_free, w.goal, stream);
    if (rc) return rc;
    g = anch_glue_args(anch, d_T_goal, B, nullptr, w.Y_free, w.goal, d_Y_full);
  } else {
    // initial point of the robot graph (bound smoothing + MDS, obstacles play no part in it) ...
    const int rc = gik_prepare_batch(base, d_T_goal, B, w.targets, w.Y_full0, nullptr, stream);
    if (rc) return rc;
    g = anch_glue_args(anch, d_T_goal, B, w.Y_full0, w.Y_free, w.goal, d_Y_full);
    // ... mapped onto the world frame by its anchors; free rows = anchored start point
    if (launch(anch_init_kernel, dim3((B + 63) / 64), dim3(64), stream, g)) return -1;
  }
  // timing events around the solve (diagnostics only; created with the handle).  The pair is
  // recorded under a lock so that gik_anchored_last_solve_ms never reads a half-recorded pair;
  // with concurrent callers it reports whichever call recorded last.
  gik_template *ma = const_cast<gik_template *>(anch);
  {
    std::lock_guard<std::mutex> lock(ma->ev_mutex);
    (void)hipEventRecord(ma->ev_solve0, (hipStream_t)stream);
  }
  int rc = scenes ? gik_solve_batch_scenes(anch, g.Y_free, g.anchor_goal, g.B, g.Y_free, d_stats, nullptr, scenes, stream)
                  : gik_solve_batch(anch, g.Y_free, g.anchor_goal, g.B, g.Y_free, d_stats, nullptr, stream);     // (not under ev_mutex:
  if (rc) return rc;                                                                                   // other threads launch meanwhile)
  {
    std::lock_guard<std::mutex> lock(ma->ev_mutex);
    (void)hipEventRecord(ma->ev_solve1, (hipStream_t)stream);
  }
  if (launch(anch_gather_kernel, dim3((g.B + 63) / 64), dim3(64), stream, g)) return -1;
  rc = gik_recover_batch(base, g.Y_full_out, g.T_goal, g.B, d_q, d_pos_err, d_rot_err, stream);
  if (rc || !d_clearance) return rc;
  return anchored_mode_clearance_launch(anch, g.Y_full_out, g.B, d_clearance, mode, stream, scenes);
}

int gik_anchored_ik_batch(const gik_template *anch, const gik_template *base, const double *d_T_goal, int B,
                          double *d_ws, double *d_Y_full, gik_stats *d_stats, double *d_q,
                          double *d_pos_err, double *d_rot_err, void *stream) {
  using namespace gik;
  if (!anch || !base || !anch->anchored || B < 0) return fail("bad argument");
  if (const std::string why = anchored_pair_fault(anch, base, PAIR_3D); !why.empty()) return fail("gik_anchored_ik_batch: " + why);
  if (B == 0) return 0;
  if (!d_T_goal || !d_ws || !d_Y_full || !d_stats || !d_q || !d_pos_err || !d_rot_err) return fail("null buffer");
  return anchored_attempt(anch, base, d_T_goal, nullptr, B, nullptr, d_ws, d_Y_full, d_stats, d_q, d_pos_err, d_rot_err, nullptr,
                          GIK_CLEARANCE_NODES, stream);
}

// what the seeded anchored calls refuse, before anything is queued
static int anchored_seed_refusal(const char *entry, const gik_template *anch, const gik_template *base, const double *d_q_init,
                                 int B, void *stream) {
  using gik::fail;
  const std::string e(entry);
  if (!anch || !base || B < 0) return fail(e + ": bad argument");
  if (const std::string why = anchored_pair_fault(anch, base, PAIR_3D | PAIR_SEEDABLE); !why.empty()) return fail(e + ": " + why);
  if (refuse_capture(entry, stream)) return -1;
  if (B > 0 && !d_q_init) return fail(e + ": null d_q_init (seed joint angles [B][n] are required)");
  return 0;
}

int gik_anchored_seed_batch(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                            const double *d_q_init, int B, double *d_ws, double *d_Y_free, double *d_goal, void *stream) {
  if (anchored_seed_refusal("gik_anchored_seed_batch", anch, base, d_q_init, B, stream)) return -1;
  if (B == 0) return 0;
  if (!d_T_goal || !d_ws || !d_Y_free || !d_goal) return gik::fail("gik_anchored_seed_batch: null buffer");
  return anchored_seed_launch(anch, base, d_T_goal, d_q_init, B, d_ws, d_Y_free, d_goal, stream);
}

int gik_anchored_ik_batch_seeded(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                                 const double *d_q_init, int B, double *d_ws, double *d_Y_full, gik_stats *d_stats,
                                 double *d_q, double *d_pos_err, double *d_rot_err, double *d_clearance, void *stream) {
  if (anchored_seed_refusal("gik_anchored_ik_batch_seeded", anch, base, d_q_init, B, stream)) return -1;
  if (B == 0) return 0;
  if (!d_T_goal || !d_ws || !d_Y_full || !d_stats || !d_q || !d_pos_err || !d_rot_err)
    return gik::fail("gik_anchored_ik_batch_seeded: null buffer");
  return anchored_attempt(anch, base, d_T_goal, d_q_init, B, nullptr, d_ws, d_Y_full, d_stats, d_q, d_pos_err, d_rot_err,
                          d_clearance, GIK_CLEARANCE_NODES, stream);
}

// what a call that takes a clearance_mode refuses about it, under the entry's name e
static int clearance_mode_refusal(const std::string &e, const gik_template *anch, int clearance_mode) {
  using gik::fail;
  // (GIK_CLEARANCE_LINKS_SELF is a value only where self pairs are attached: on every other template the call is
  // refused in the words it has always been refused in)
  const bool has_self = anch->n_self >= 0;
  if (clearance_mode != GIK_CLEARANCE_NODES && clearance_mode != GIK_CLEARANCE_LINKS &&
      !(has_self && clearance_mode == GIK_CLEARANCE_LINKS_SELF))
    return fail(e + ": clearance_mode must be GIK_CLEARANCE_NODES (0) or GIK_CLEARANCE_LINKS (1)" +
                (has_self ? " or GIK_CLEARANCE_LINKS_SELF (2)" : ""));
  if (clearance_mode == GIK_CLEARANCE_LINKS && anch->n_link < 0)
    return fail(e + ": clearance_mode = links, but no links attached (gik_anchored_attach_links)");
  return 0;
}

// ---- per-goal obstacle scenes: the solve entry (the solve kernel's: gik_solve_batch_scenes) ----
int gik_anchored_ik_batch_scenes(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                                 const double *d_q_init, int B, const gik_scene_set *scenes, double *d_ws, double *d_Y_full,
                                 gik_stats *d_stats, double *d_q, double *d_pos_err, double *d_rot_err, double *d_clearance,
                                 int clearance_mode, void *stream) {
  using namespace gik;
  const std::string e("gik_anchored_ik_batch_scenes");
  if (!anch || !base || B < 0) return fail(e + ": bad argument");
  if (const std::string why = anchored_pair_fault(anch, base, PAIR_3D | (d_q_init ? PAIR_SEEDABLE : 0)); !why.empty())
    return fail(e + ": " + why);
  if (scene_refusal("gik_anchored_ik_batch_scenes", anch, scenes)) return -1;
  if (clearance_mode_refusal(e, anch, clearance_mode)) return -1;
  if (refuse_capture("gik_anchored_ik_batch_scenes", stream)) return -1;
  if (B == 0) return 0;
  if (!d_T_goal || !d_ws || !d_Y_full || !d_stats || !d_q || !d_pos_err || !d_rot_err) return fail(e + ": null buffer");
  return anchored_attempt(anch, base, d_T_goal, d_q_init, B, scenes, d_ws, d_Y_full, d_stats, d_q, d_pos_err, d_rot_err,
                          d_clearance, clearance_mode, stream);
}

// ---- the clearance of an answer: of the masked nodes or of whole links, against the template's obstacles or per-goal scenes ----
static int anchored_clearance_entry(const char *entry, const gik_template *anch, bool links, bool with_scenes,
                                    const gik_scene_set *scenes, const double *d_Y_full, int B, double *d_clearance, void *stream) {
  using gik::fail;
  const std::string e(entry);
  if (!anch || B < 0) return fail(e + ": bad argument");
  if (with_scenes) {
    if (scene_refusal(entry, anch, scenes)) return -1;
  } else if (!anch->anchored) {
    return fail(e + ": the handle must be a fixed-anchor template (gik_template_create_anchored)");
  }
  if (links && anch->n_link < 0) return fail(e + ": no links attached (gik_anchored_attach_links)");
  if (refuse_capture(entry, stream)) return -1;
  if (B == 0) return 0;
  if (!d_Y_full || !d_clearance) return fail(e + ": null buffer");
  const int rc = links ? anchored_link_clearance_launch(anch, d_Y_full, B, d_clearance, stream, scenes)      // (scenes: null without)
                       : anchored_clearance_launch(anch, d_Y_full, B, d_clearance, stream, scenes);
  return rc ? rc : fold_halfspaces(anch, d_Y_full, B, d_clearance, links, stream);
}

int gik_anchored_clearance(const gik_template *anch, const double *d_Y_full, int B, double *d_clearance, void *stream) {
  return anchored_clearance_entry("gik_anchored_clearance", anch, false, false, nullptr, d_Y_full, B, d_clearance, stream);
}
int gik_anchored_link_clearance(const gik_template *anch, const double *d_Y_full, int B, double *d_clearance, void *stream) {
  return anchored_clearance_entry("gik_anchored_link_clearance", anch, true, false, nullptr, d_Y_full, B, d_clearance, stream);
}
int gik_anchored_clearance_scenes(const gik_template *anch, const double *d_Y_full, int B, const gik_scene_set *scenes,
                                  double *d_clearance, void *stream) {
  return anchored_clearance_entry("gik_anchored_clearance_scenes", anch, false, true, scenes, d_Y_full, B, d_clearance, stream);
}
int gik_anchored_link_clearance_scenes(const gik_template *anch, const double *d_Y_full, int B, const gik_scene_set *scenes,
                                       double *d_clearance, void *stream) {
  return anchored_clearance_entry("gik_anchored_link_clearance_scenes", anch, true, true, scenes, d_Y_full, B, d_clearance, stream);
}

// against the half-spaces alone (gik_anchored_attach_halfspaces): what the entries above fold into theirs
int gik_anchored_halfspace_clearance(const gik_template *anch, const double *d_Y_full, int B, int links, double *d_clearance,
                                     void *stream) {
  using gik::fail;
  const std::string e("gik_anchored_halfspace_clearance");
  if (!anch || B < 0) return fail(e + ": bad argument");
  if (!anch->anchored) return fail(e + ": the handle must be a fixed-anchor template (gik_template_create_anchored)");
  if (anch->n_half <= 0) return fail(e + ": no half-spaces attached (gik_anchored_attach_halfspaces)");
  if (links != 0 && links != 1) return fail(e + ": links must be 0 (the masked nodes) or 1 (the attached links)");
  if (links && anch->n_link < 0) return fail(e + ": no links attached (gik_anchored_attach_links)");
  if (refuse_capture("gik_anchored_halfspace_clearance", stream)) return -1;
  if (B == 0) return 0;
  if (!d_Y_full || !d_clearance) return fail(e + ": null buffer");
  return anchored_half_clearance_launch(anch, d_Y_full, B, d_clearance, links != 0, false, stream);
}

// link against link: the pairs of gik_anchored_attach_self_pairs (none: +infinity, as the kernel leaves it)
int gik_anchored_self_clearance(const gik_template *anch, const double *d_Y_full, int B, double *d_clearance, void *stream) {
  using gik::fail;
  const std::string e("gik_anchored_self_clearance");
  if (!anch || B < 0) return fail(e + ": bad argument");
  if (!anch->anchored) return fail(e + ": the handle must be a fixed-anchor template (gik_template_create_anchored)");
  if (anch->n_link < 0) return fail(e + ": no links attached (gik_anchored_attach_links)");
  if (anch->n_self < 0) return fail(e + ": no self pairs attached (gik_anchored_attach_self_pairs)");
  if (refuse_capture("gik_anchored_self_clearance", stream)) return -1;
  if (B == 0) return 0;
  if (!d_Y_full || !d_clearance) return fail(e + ": null buffer");
  return anchored_self_clearance_launch(anch, d_Y_full, B, d_clearance, false, stream);
}

// ---- the sweep of the link clearance between two configurations (gik_anch_seed.hip.h) -----------
// the caller-owned workspace of gik_anchored_sweep_clearance over d_ws (gik_plan.h), or with a null d_ws its size
static gik::AnchSweepWs anch_sweep_ws(const gik_template *anch, const gik_template *base, int B, int S, double *d_ws) {
  return gik::anch_sweep_ws(base->pc.n_joints, pose_width(base), base->T, anch->full_N, B, S, d_ws);
}

size_t gik_anchored_sweep_ws_bytes(const gik_template *anch, const gik_template *base, int B, int samples) {
  if (!anch || !base || !anchored_pair_fault(anch, base, 0).empty() || B < 0 || samples < 1 ||
      (size_t)B * ((size_t)samples + 1) > (size_t)INT_MAX)
    return 0;
  return anch_sweep_ws(anch, base, B, samples, nullptr).doubles * sizeof(double);
}

// gik_anchored_sweep_clearance (d_link_out is its d_clearance) and gik_anchored_sweep_clearances (two_outputs: either may
// be null): one interpolate launch, one realization, then per output the clearance of all M configurations into the one
// [S+1][B] array and its minimum over the samples.
static int anchored_sweep_impl(const char *entry, bool two_outputs, const gik_template *anch, const gik_template *base,
                               const double *d_q_a, const double *d_q_b, int B, int samples, double *d_ws, double *d_link_out,
                               double *d_self_out, void *stream) {
  using namespace gik;
  const std::string e(entry);
  if (!anch || !base || B < 0) return fail(e + ": bad argument");
  if (const std::string why = anchored_pair_fault(anch, base, PAIR_3D | PAIR_SEEDABLE); !why.empty()) return fail(e + ": " + why);
  if (anch->n_link < 0) return fail(e + ": no links attached (gik_anchored_attach_links)");
  if (samples < 1) return fail(e + ": samples must be at least 1");
  if ((size_t)B * ((size_t)samples + 1) > (size_t)INT_MAX) return fail(e + ": B (samples + 1) must fit an int");
  if (two_outputs && !d_link_out && !d_self_out) return fail(e + ": both outputs are null (d_link_out, d_self_out: one at least)");
  if (d_self_out && anch->n_self < 0) return fail(e + ": d_self_out given, but no self pairs attached (gik_anchored_attach_self_pairs)");
  if (refuse_capture(entry, stream)) return -1;
  if (B == 0) return 0;
  if (!d_q_a || !d_q_b || !d_ws || (!two_outputs && !d_link_out)) return fail(e + ": null buffer");
  const AnchSweepWs w = anch_sweep_ws(anch, base, B, samples, d_ws);
  const int M = B * (samples + 1);
  AnchSweepInterpArgs ia;
  ia.q_a = d_q_a;
  ia.q_b = d_q_b;
  ia.q_s = w.q;
  ia.T_id = w.T;
  ia.B = B;
  ia.n = base->pc.n_joints;
  ia.S = samples;
  ia.D = base->f.K + 1;
  ia.pose_w = pose_width(base);
  const size_t nt = (size_t)M * ((size_t)ia.n + (size_t)ia.pose_w);
  if ((nt + ANCH_SCATTER_NT - 1) / ANCH_SCATTER_NT > (size_t)INT_MAX) return fail(e + ": the batch is too large");
  const dim3 interp_grid((unsigned)((nt + ANCH_SCATTER_NT - 1) / ANCH_SCATTER_NT));
  int rc = launch(anch_sweep_interp_kernel, interp_grid, dim3(ANCH_SCATTER_NT), stream, ia);
  // the realization of every sample: seed_kernel's joint-frame walk on the robot graph (its targets go unread)
  if (!rc) rc = gik_seed_batch(base, w.T, w.q, M, w.targets, w.Y, stream);
  if (rc) return rc;
  for (int k = 0; k < 2; ++k) {      // (one stream: the second clearance overwrites w.cl behind the first minimum)
    double *out = k == 0 ? d_link_out : d_self_out;
    if (!out) continue;
    rc = k == 0 ? anchored_link_clearance_launch(anch, w.Y, M, w.cl, stream)
                : anchored_self_clearance_launch(anch, w.Y, M, w.cl, false, stream);
    if (!rc && k == 0) rc = fold_halfspaces(anch, w.Y, M, w.cl, true, stream);      // (per sample, before the minimum)
    if (rc) return rc;
    AnchSweepMinArgs ma;
    ma.cl = w.cl;
    ma.clearance = out;
    ma.B = B;
    ma.S = samples;
    if (launch(anch_sweep_min_kernel, dim3((B + ANCH_SCATTER_NT - 1) / ANCH_SCATTER_NT), dim3(ANCH_SCATTER_NT), stream, ma)) return -1;
  }
  return 0;
}

int gik_anchored_sweep_clearance(const gik_template *anch, const gik_template *base, const double *d_q_a,
                                 const double *d_q_b, int B, int samples, double *d_ws, double *d_clearance, void *stream) {
  return anchored_sweep_impl("gik_anchored_sweep_clearance", false, anch, base, d_q_a, d_q_b, B, samples, d_ws, d_clearance, nullptr,
                             stream);
}

int gik_anchored_sweep_clearances(const gik_template *anch, const gik_template *base, const double *d_q_a,
                                  const double *d_q_b, int B, int samples, double *d_ws, double *d_link_out,
                                  double *d_self_out, void *stream) {
  return anchored_sweep_impl("gik_anchored_sweep_clearances", true, anch, base, d_q_a, d_q_b, B, samples, d_ws, d_link_out, d_self_out,
                             stream);
}

// ---- restarts in the anchored solve: the kernels of gik_retry.hip.h with a clearance in the rule -------------
int gik_anchored_retry_select(const gik_stats *d_stats, const double *d_pos_err, const double *d_rot_err,
                              const double *d_clearance, int B, double pos_tol, double rot_tol, double clear_tol,
                              int32_t *d_idx, int32_t *d_count, void *stream) {
  return retry_select_entry("gik_anchored_retry_select: ", true,
                            {d_stats, d_pos_err, d_rot_err, d_clearance, {pos_tol, rot_tol, clear_tol}, d_idx, d_count, B}, stream);
}

int gik_anchored_retry_seeds(const gik_template *base, const double *d_T_goal, const int32_t *d_idx, int count,
                             uint64_t seed, int attempt, const double *d_q_lo, const double *d_q_hi,
                             const double *d_q_center, double spread, double *d_T_out, double *d_q_out, void *stream) {
  using namespace gik;
  if (!base || count < 0) return fail("gik_anchored_retry_seeds: bad argument");
  if (!base->has_pipe) return fail("gik_anchored_retry_seeds: no pipeline attached to the base template (gik_pipeline_attach)");
  if (base->pc.pos_goal_mask)
    return fail("gik_anchored_retry_seeds: the base template has position goals (position_goal_mask); the fixed-anchor "
                "formulation takes pose goals");
  if (attempt < 0 || attempt > 63) return fail("gik_anchored_retry_seeds: attempt must be within 0 .. 63");
  if (!d_q_lo || !d_q_hi) return fail("gik_anchored_retry_seeds: null joint limits (d_q_lo / d_q_hi, [n] each, are required)");
  if (!(spread >= 0.0)) return fail("gik_anchored_retry_seeds: spread must be at least 0");
  if (spread > 0.0 && !d_q_center) return fail("gik_anchored_retry_seeds: spread > 0 needs the centre rows d_q_center [B][n]");
  if (count == 0) return 0;
  if (!d_T_goal || !d_idx || !d_T_out || !d_q_out) return fail("gik_anchored_retry_seeds: null buffer");
  const RetrySeedArgs a = {d_T_goal, d_idx, d_q_lo, d_q_hi, d_q_center, d_T_out, d_q_out, spread, seed,
                           count, pose_width(base), base->pc.n_joints, attempt};
  return retry_seed_launch(base, a, stream);
}

int gik_anchored_retry_merge(const gik_template *anch, const gik_template *base, const int32_t *d_idx, int count,
                             int attempt, double pos_tol, double rot_tol, double clear_tol, const double *d_Y_r,
                             const gik_stats *d_stats_r, const double *d_q_r, const double *d_pos_err_r,
                             const double *d_rot_err_r, const double *d_clearance_r, double *d_Y_full, gik_stats *d_stats,
                             double *d_q, double *d_pos_err, double *d_rot_err, double *d_clearance, int32_t *d_attempt,
                             void *stream) {
  using namespace gik;
  if (!anch || !base || count < 0) return fail("gik_anchored_retry_merge: bad argument");
  if (const std::string why = anchored_pair_fault(anch, base, 0); !why.empty()) return fail("gik_anchored_retry_merge: " + why);
  if (count == 0) return 0;
  if (!d_idx || !d_Y_r || !d_stats_r || !d_q_r || !d_pos_err_r || !d_rot_err_r || !d_clearance_r || !d_Y_full || !d_stats ||
      !d_q || !d_pos_err || !d_rot_err || !d_clearance || !d_attempt)
    return fail("gik_anchored_retry_merge: null buffer");
  const RetryMergeArgs a = {d_idx,
                            d_Y_r, d_stats_r, d_q_r, d_pos_err_r, d_rot_err_r, d_clearance_r,
                            d_Y_full, d_stats, d_q, d_pos_err, d_rot_err, d_clearance, d_attempt,
                            {pos_tol, rot_tol, clear_tol}, count, anch->full_N * 3, base->pc.n_joints, attempt};
  return retry_merge_launch(base, a, stream);
}

// the caller-owned workspace of the anchored restart entries over d_ws (gik_plan.h), or with a null d_ws its size
static gik::AnchRetryWs anch_retry_ws(const gik_template *anch, const gik_template *base, int B, void *d_ws) {
  return gik::anch_retry_ws(base->pc.n_joints, pose_width(base), base->T, base->N, anch->N, anch->an.n_goal, anch->full_N, B, d_ws);
}

size_t gik_anchored_retry_ws_bytes(const gik_template *anch, const gik_template *base, int B) {
  if (!anch || !base || !anchored_pair_fault(anch, base, 0).empty() || B < 0) return 0;
  return anch_retry_ws(anch, base, B, nullptr).bytes;      // (without the scene entry's ids)
}

// ---- screened restart seeds: C candidates per failed goal, the first clear one starts the restart ----
// the workspace of the screened step over d_ws behind `head` bytes (gik_plan.h), or with a null d_ws its size
static gik::AnchScreenWs anch_screen_ws(const gik_template *anch, const gik_template *base, int B, int C, size_t head, void *d_ws) {
  return gik::anch_screen_ws(base->pc.n_joints, pose_width(base), base->T, anch->full_N, B, C, head, d_ws);
}
static size_t anch_screen_head(const gik_template *anch, const gik_template *base, int B) {
  return gik::anch_screen_head(base->pc.n_joints, pose_width(base), base->T, base->N, anch->N, anch->an.n_goal, anch->full_N, B);
}

// what is wrong with a candidate count or a batch of that many candidates, or nothing
static std::string candidates_fault(int candidates, int B) {
  if (candidates < 1 || candidates > gik::RETRY_MAX_CANDIDATES) return "candidates must be within 1 .. 16";
  if ((size_t)B * (size_t)candidates > (size_t)INT_MAX) return "B * candidates must fit an int";
  return std::string();
}

// The screened seed step on checked arguments, a.count > 0: the candidates of every slot, candidate-major; their
// realization by the robot graph's seed kernel (its targets go unread), as the sweep realizes its samples; their
// clearance in the call's mode, against the goal's scene where there are scenes (the ids tiled to the candidates);
// the pick, whose angles go where retry_seed_kernel would have written its one row.  atlas: null -- the candidates are
// drawn (retry_candidate_kernel) --, or the second candidate source: neighbour ranks [first, first + candidates) of every
// slot's goal (atlas_candidate_kernel; a.idx may then be null: slot r is goal r), and with `note` the picked row by goal.
struct AtlasSource {
  const double *q;        // [M][n]
  const int32_t *nbr;     // [B][stride], by goal
  int M, stride, first;
  int32_t *note;          // [B], or null
};
static int screened_seed_launch(const gik_template *anch, const gik_template *base, const gik::RetrySeedArgs &a, int candidates,
                                int mode, double clear_tol, const gik_scene_set *scenes, const gik::AnchScreenWs &w,
                                int32_t *d_pick, double *d_pick_clearance, void *stream, const AtlasSource *atlas = nullptr) {
  using namespace gik;
  const int M = a.count * candidates;
  const int32_t *goal_ids = scenes ? scenes->d_scene_id : nullptr;
  int rc = 0;
  if (atlas) {
    const AtlasCandidateArgs ca = {a.T_goal, a.idx, atlas->q, atlas->nbr, goal_ids, a.T_out, w.T, w.q, w.ids,
                                   a.count, a.pose_w, a.n, candidates, atlas->first, atlas->stride, atlas->M};
    rc = launch(atlas_candidate_kernel, dim3(retry_grid(base, a.count)), dim3(ATLAS_WAVE), stream, ca);
  } else {
    const RetryCandidateArgs ca = {a.T_goal, a.idx, a.q_lo, a.q_hi, a.q_center, goal_ids, a.T_out, w.T, w.q, w.ids,
                                   a.spread, a.seed, a.count, a.pose_w, a.n, a.attempt, candidates};
    rc = launch(retry_candidate_kernel, dim3(retry_grid(base, a.count)), dim3(RETRY_WAVE), stream, ca);
  }
  if (!rc) rc = gik_seed_batch(base, w.T, w.q, M, w.targets, w.Y, stream);
  if (rc) return rc;
  gik_scene_set tiled;
  if (scenes) {
    tiled = *scenes;
    if (goal_ids) tiled.d_scene_id = w.ids;
  }
  if ((rc = anchored_mode_clearance_launch(anch, w.Y, M, w.cl, mode, stream, scenes ? &tiled : nullptr))) return rc;
  const RetryPickArgs pa = {w.cl, w.q, a.q_out, d_pick ? d_pick : w.pick, d_pick_clearance, clear_tol, a.count, a.n, candidates};
  rc = launch(retry_pick_kernel, dim3(retry_grid(base, a.count)), dim3(RETRY_WAVE), stream, pa);
  if (rc || !atlas || !atlas->note) return rc;
  // the atlas row each slot's pick names, by goal
  const AtlasNoteArgs na = {a.idx, atlas->nbr, pa.pick, atlas->note, a.count, atlas->first, atlas->stride};
  return launch(atlas_note_kernel, dim3((a.count + ATLAS_NOTE_NT - 1) / ATLAS_NOTE_NT), dim3(ATLAS_NOTE_NT), stream, na);
}

// The two exports of that step, gik_anchored_retry_seeds_screened and gik_anchored_atlas_seeds: the refusals they share --
// the pair, the scene set, the mode; behind own_fault(), the entry's own in its order (what is wrong, or nothing), the
// capture, the workspace and the buffers -- and the launch.  a: the step's arguments but for pose_w and n, filled here.
template <typename OwnFault>
static int screened_step_entry(const char *entry, const char *size_query, const gik_template *anch, const gik_template *base,
                               gik::RetrySeedArgs a, int candidates, int mode, double clear_tol, const gik_scene_set *scenes,
                               void *d_ws, int32_t *d_pick, double *d_pick_clearance, void *stream, const AtlasSource *atlas,
                               OwnFault own_fault) {
  using namespace gik;
  const std::string e(entry);
  if (!anch || !base || a.count < 0) return fail(e + ": bad argument");
  if (const std::string why = anchored_pair_fault(anch, base, PAIR_3D | PAIR_SEEDABLE); !why.empty()) return fail(e + ": " + why);
  if (scenes && scene_refusal(entry, anch, scenes)) return -1;
  if (clearance_mode_refusal(e, anch, mode)) return -1;
  if (const std::string why = own_fault(); !why.empty()) return fail(e + ": " + why);
  if (refuse_capture(entry, stream)) return -1;
  if (a.count == 0) return 0;
  if (workspace_refusal(e, d_ws, size_query)) return -1;
  const int32_t *rows_of = atlas ? atlas->nbr : a.idx;      // (an atlas call may have no idx: slot r is goal r)
  if (!a.T_goal || !rows_of || !a.T_out || !a.q_out) return fail(e + ": null buffer");
  a.pose_w = pose_width(base);
  a.n = base->pc.n_joints;
  return screened_seed_launch(anch, base, a, candidates, mode, clear_tol, scenes, anch_screen_ws(anch, base, a.count, candidates, 0, d_ws),
                              d_pick, d_pick_clearance, stream, atlas);
}

size_t gik_anchored_retry_seeds_screened_ws_bytes(const gik_template *anch, const gik_template *base, int count, int candidates) {
  if (!anch || !base || !anchored_pair_fault(anch, base, 0).empty() || count < 0 || !candidates_fault(candidates, count).empty())
    return 0;
  return anch_screen_ws(anch, base, count, candidates, 0, nullptr).bytes;
}

int gik_anchored_retry_seeds_screened(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                                      const int32_t *d_idx, int count, uint64_t seed, int attempt, const double *d_q_lo,
                                      const double *d_q_hi, const double *d_q_center, double spread, int candidates,
                                      int clearance_mode, double clear_tol, const gik_scene_set *scenes, void *d_ws,
                                      double *d_T_out, double *d_q_out, int32_t *d_pick, double *d_pick_clearance, void *stream) {
  const gik::RetrySeedArgs a = {d_T_goal, d_idx, d_q_lo, d_q_hi, d_q_center, d_T_out, d_q_out, spread, seed, count, 0, 0, attempt};
  const auto own_fault = [&]() -> std::string {      // what this entry alone refuses, in its order
    if (attempt < 0 || attempt > 63) return "attempt must be within 0 .. 63";
    if (!d_q_lo || !d_q_hi) return "null joint limits (d_q_lo / d_q_hi, [n] each, are required)";
    if (!(spread >= 0.0)) return "spread must be at least 0";
    if (spread > 0.0 && !d_q_center) return "spread > 0 needs the centre rows d_q_center [B][n]";
    if (const std::string why = candidates_fault(candidates, count); !why.empty()) return why;
    if (!(clear_tol > 0.0)) return "clear_tol must be positive";
    return std::string();
  };
  return screened_step_entry("gik_anchored_retry_seeds_screened", "gik_anchored_retry_seeds_screened_ws_bytes", anch, base, a,
                             candidates, clearance_mode, clear_tol, scenes, d_ws, d_pick, d_pick_clearance, stream, nullptr,
                             own_fault);
}

// ---- the restart entries: each makes its own refusals, under its own name, and hands over to anchored_restarts ----
// Where the restart seeds come from.  candidates 0: one blind draw per failed goal (retry_seed_kernel).  C > 0: the screened
// step picks among C draws per failed goal or, with the tables of an atlas, among the C neighbour ranks [a C, (a + 1) C) of
// restart a -- and a cold attempt 0 then starts from the pick among ranks [0, C).
struct SeedSource {
  int candidates;
  const double *atlas_keys, *atlas_q;      // [W][M] and [M][n], or null: draws
  int atlas_count, key_width;              // M, W
  const char *size_query;                  // the export that sizes the entry's workspace
};
static int anchored_restarts(const char *entry, const gik_template *anch, const gik_template *base, const double *d_T_goal,
                             const double *d_q_init, int B, const gik_anchored_retry_opts *opts, const gik_scene_set *scenes,
                             const SeedSource &src, void *d_ws, double *d_Y_full, gik_stats *d_stats, double *d_q, double *d_pos_err,
                             double *d_rot_err, double *d_clearance, int32_t *d_attempt, void *stream);

// The refusals of gik_anchored_ik_batch_retry and, with a scene set, gik_anchored_ik_batch_retry_scenes; screened:
// gik_anchored_ik_batch_retry_screened, `candidates` draws per slot (not screened: `candidates` is not read).
static int anchored_retry_impl(const char *entry, const gik_template *anch, const gik_template *base, const double *d_T_goal,
                               const double *d_q_init, int B, const gik_anchored_retry_opts *opts, const gik_scene_set *scenes,
                               bool with_scenes, void *d_ws, double *d_Y_full, gik_stats *d_stats, double *d_q, double *d_pos_err,
                               double *d_rot_err, double *d_clearance, int32_t *d_attempt, void *stream, bool screened, int candidates) {
  using namespace gik;
  const std::string e(entry);
  // every refusal comes before anything is queued
  if (!anch || !base || B < 0 || !opts) return fail(e + ": bad argument");
  if (const std::string why = anchored_pair_fault(anch, base, PAIR_3D); !why.empty()) return fail(e + ": " + why);
  if (with_scenes && scene_refusal(entry, anch, scenes)) return -1;
  if (opts->retries < 0 || opts->retries > 63) return fail(e + ": retries must be within 0 .. 63");
  if (clearance_mode_refusal(e, anch, opts->clearance_mode)) return -1;
  if ((d_q_init || opts->retries > 0) && !base->seed_ok)
    return fail(e + ": the base graph cannot be seeded on the device: " + base->seed_why);
  if (opts->retries > 0) {
    if (!opts->d_q_lo || !opts->d_q_hi)
      return fail(e + ": null joint limits (opts->d_q_lo / d_q_hi, [n] each, are what the seeds are drawn from)");
    if (!(opts->pos_tol > 0.0) || !(opts->rot_tol > 0.0)) return fail(e + ": pos_tol and rot_tol must be positive");
    if (!(opts->clear_tol > 0.0)) return fail(e + ": clear_tol must be positive");
    if (!(opts->spread >= 0.0)) return fail(e + ": spread must be at least 0 (radians; 0: uniform inside the limits)");
    if (opts->spread > 0.0 && !d_q_init)
      return fail(e + ": spread > 0 needs d_q_init, the centre the seeds are drawn around (a cold batch has none)");
  }
  if (screened) {
    if (const std::string why = candidates_fault(candidates, B); !why.empty()) return fail(e + ": " + why);
    if (!(opts->clear_tol > 0.0)) return fail(e + ": clear_tol must be positive");
  }
  const SeedSource src = {screened ? candidates : 0, nullptr, nullptr, 0, 0,
                          screened ? "gik_anchored_ik_batch_retry_screened_ws_bytes" : "gik_anchored_retry_ws_bytes"};
  return anchored_restarts(entry, anch, base, d_T_goal, d_q_init, B, opts, scenes, src, d_ws, d_Y_full, d_stats, d_q, d_pos_err, d_rot_err,
                           d_clearance, d_attempt, stream);
}

int gik_anchored_ik_batch_retry(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                                const double *d_q_init, int B, const gik_anchored_retry_opts *opts, void *d_ws,
                                double *d_Y_full, gik_stats *d_stats, double *d_q, double *d_pos_err, double *d_rot_err,
                                double *d_clearance, int32_t *d_attempt, void *stream) {
  return anchored_retry_impl("gik_anchored_ik_batch_retry", anch, base, d_T_goal, d_q_init, B, opts, nullptr, false, d_ws, d_Y_full,
                             d_stats, d_q, d_pos_err, d_rot_err, d_clearance, d_attempt, stream, false, 1);
}

int gik_anchored_ik_batch_retry_scenes(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                                       const double *d_q_init, int B, const gik_anchored_retry_opts *opts,
                                       const gik_scene_set *scenes, void *d_ws, double *d_Y_full, gik_stats *d_stats, double *d_q,
                                       double *d_pos_err, double *d_rot_err, double *d_clearance, int32_t *d_attempt, void *stream) {
  return anchored_retry_impl("gik_anchored_ik_batch_retry_scenes", anch, base, d_T_goal, d_q_init, B, opts, scenes, true, d_ws,
                             d_Y_full, d_stats, d_q, d_pos_err, d_rot_err, d_clearance, d_attempt, stream, false, 1);
}

size_t gik_anchored_ik_batch_retry_screened_ws_bytes(const gik_template *anch, const gik_template *base, int B, int candidates) {
  if (!anch || !base || !anchored_pair_fault(anch, base, 0).empty() || B < 0 || !candidates_fault(candidates, B).empty()) return 0;
  return anch_screen_ws(anch, base, B, candidates, anch_screen_head(anch, base, B), nullptr).bytes;
}

int gik_anchored_ik_batch_retry_screened(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                                         const double *d_q_init, int B, const gik_anchored_retry_opts *opts, int candidates,
                                         const gik_scene_set *scenes, void *d_ws, double *d_Y_full, gik_stats *d_stats,
                                         double *d_q, double *d_pos_err, double *d_rot_err, double *d_clearance,
                                         int32_t *d_attempt, void *stream) {
  return anchored_retry_impl("gik_anchored_ik_batch_retry_screened", anch, base, d_T_goal, d_q_init, B, opts, scenes, scenes != nullptr,
                             d_ws, d_Y_full, d_stats, d_q, d_pos_err, d_rot_err, d_clearance, d_attempt, stream, true, candidates);
}

// ---- goal-aware seeds from a configuration atlas (gik_atlas.hip.h) ----------------------------------------
// the key width of a base template -- 6: p_e and q_e, 3: the p_e of a position goal -- or 0 with the reason in *why
static int atlas_key_width(const gik_template *base, std::string *why) {
  if (!base->has_pipe) return *why = "no pipeline attached to the base template (gik_pipeline_attach)", 0;
  if (base->f.K != 3) return *why = "the base template is planar: the atlas key is that of a 3-D graph", 0;
  if (base->pc.n_ee != 1) return *why = "the base template has more than one end effector", 0;
  if (base->pc.goal_node[0] < 0) return *why = "the base template's first goal slot is inert", 0;
  if (base->pc.goal_node[1] >= 0) return 6;
  if (base->pc.pos_goal_mask & 1) return 3;
  return *why = "the base template has an inert goal slot that is not a position goal's", 0;
}

// what is wrong with a neighbour count, a table size or a batch of that many neighbours, or nothing
static std::string atlas_fault(int K, int atlas_count, int count) {
  if (K < 1 || K > gik::ATLAS_MAX_K) return "K must be within 1 .. 64";
  if (atlas_count < 1 || atlas_count > (1 << 30)) return "atlas_count must be within 1 .. 2^30";
  if ((size_t)count * (size_t)K > (size_t)INT_MAX) return "count * K must fit an int";
  return std::string();
}

// the nearest launch on checked arguments, count > 0
static int atlas_nearest_launch(const gik_template *base, int W, const double *d_keys, int M, const double *d_T_goal,
                                const int32_t *d_idx, int count, int K, int32_t *d_nbr, double *d_dist, void *stream) {
  using namespace gik;
  const AtlasNearestArgs a = {d_keys, d_T_goal, d_idx, d_nbr, d_dist, base->pc.ee_len[0], M, count, K, pose_width(base), W};
  const int groups = (count + ATLAS_GOALS - 1) / ATLAS_GOALS;
  return launch(atlas_nearest_kernel, dim3(std::min(groups, base->f.n_cu * 32)), dim3(ATLAS_WAVE), stream, a);
}

int gik_atlas_nearest(const gik_template *base, const double *d_atlas_keys, int atlas_count, const double *d_T_goal,
                      const int32_t *d_idx, int count, int K, int32_t *d_nbr, double *d_dist, void *stream) {
  using namespace gik;
  const std::string e("gik_atlas_nearest");
  if (!base || count < 0) return fail(e + ": bad argument");
  std::string why;
  const int W = atlas_key_width(base, &why);
  if (!W) return fail(e + ": " + why);
  if (why = atlas_fault(K, atlas_count, count); !why.empty()) return fail(e + ": " + why);
  if (!d_atlas_keys) return fail(e + ": null atlas (d_atlas_keys [W][atlas_count] is required)");
  if (refuse_capture("gik_atlas_nearest", stream)) return -1;
  if (count == 0) return 0;
  if (!d_T_goal || !d_nbr) return fail(e + ": null buffer");
  return atlas_nearest_launch(base, W, d_atlas_keys, atlas_count, d_T_goal, d_idx, count, K, d_nbr, d_dist, stream);
}

size_t gik_anchored_atlas_seeds_ws_bytes(const gik_template *anch, const gik_template *base, int count, int candidates) {
  return gik_anchored_retry_seeds_screened_ws_bytes(anch, base, count, candidates);      // (the screened step's arrays)
}

int gik_anchored_atlas_seeds(const gik_template *anch, const gik_template *base, const double *d_atlas_q, int atlas_count,
                             const double *d_T_goal, const int32_t *d_idx, int count, const int32_t *d_nbr, int nbr_stride,
                             int first, int candidates, int clearance_mode, double clear_tol, const gik_scene_set *scenes,
                             void *d_ws, double *d_T_out, double *d_q_out, int32_t *d_pick, double *d_pick_clearance,
                             void *stream) {
  const gik::RetrySeedArgs a = {d_T_goal, d_idx, nullptr, nullptr, nullptr, d_T_out, d_q_out, 0.0, 0, count, 0, 0, 0};
  const AtlasSource rows = {d_atlas_q, d_nbr, atlas_count, nbr_stride, first, nullptr};
  const auto own_fault = [&]() -> std::string {      // what this entry alone refuses, in its order
    if (const std::string why = candidates_fault(candidates, count); !why.empty()) return why;
    if (atlas_count < 1 || atlas_count > (1 << 30)) return "atlas_count must be within 1 .. 2^30";
    if (first < 0 || nbr_stride < 1 || first > nbr_stride - candidates)
      return "ranks first .. first + candidates - 1 must lie within 0 .. nbr_stride - 1";
    if (!(clear_tol > 0.0)) return "clear_tol must be positive";
    if (!d_atlas_q) return "null atlas (d_atlas_q [atlas_count][n] is required)";
    return std::string();
  };
  return screened_step_entry("gik_anchored_atlas_seeds", "gik_anchored_atlas_seeds_ws_bytes", anch, base, a, candidates,
                             clearance_mode, clear_tol, scenes, d_ws, d_pick, d_pick_clearance, stream, &rows, own_fault);
}

// the workspace of gik_anchored_ik_batch_atlas over d_ws (gik_plan.h), or with a null d_ws its size
static gik::AnchAtlasWs anch_atlas_ws(const gik_template *anch, const gik_template *base, int B, int C, int retries, void *d_ws) {
  return gik::anch_atlas_ws(base->pc.n_joints, pose_width(base), base->T, anch->full_N, B, C, retries,
                            anch_screen_head(anch, base, B), d_ws);
}

// what is wrong with the (candidates, retries) of an atlas batch, or nothing
static std::string atlas_batch_fault(int candidates, int retries, int B) {
  if (retries < 0 || retries > 63) return "retries must be within 0 .. 63";
  if (const std::string why = candidates_fault(candidates, B); !why.empty()) return why;
  if ((retries + 1) * candidates > gik::ATLAS_MAX_K) return "K = (retries + 1) * candidates must be within 1 .. 64";
  return std::string();
}

size_t gik_anchored_ik_batch_atlas_ws_bytes(const gik_template *anch, const gik_template *base, int B, int candidates, int retries) {
  if (!anch || !base || !anchored_pair_fault(anch, base, 0).empty() || B < 0 || !atlas_batch_fault(candidates, retries, B).empty() ||
      (size_t)B * (size_t)((retries + 1) * candidates) > (size_t)INT_MAX)
    return 0;
  return anch_atlas_ws(anch, base, B, candidates, retries, nullptr).bytes;
}

// The one restart driver, behind gik_anchored_ik_batch_retry, _retry_scenes, _retry_screened and _atlas, on arguments their
// refusals have checked.  It ends the refusal sequence they share -- the capture, the empty batch, the outputs, the workspace,
// the buffers -- and then queues, in this order: the centre copy of local mode; the memset of d_attempt; with an atlas the
// memset of the noted rows (-1: no atlas row), the nearest launch over all goals and, cold, the pick among ranks [0, C) of
// every goal (slot r is goal r); attempt 0; retry_loop.  A scene set goes through attempt 0, every compact batch (its ids
// gathered into w.ids) and every clearance.  In the link modes the rule is the same: the array it reads holds the clearance
// of whole links, or the minimum of that and the self clearance.
static int anchored_restarts(const char *entry, const gik_template *anch, const gik_template *base, const double *d_T_goal,
                             const double *d_q_init, int B, const gik_anchored_retry_opts *opts, const gik_scene_set *scenes,
                             const SeedSource &src, void *d_ws, double *d_Y_full, gik_stats *d_stats, double *d_q, double *d_pos_err,
                             double *d_rot_err, double *d_clearance, int32_t *d_attempt, void *stream) {
  using namespace gik;
  const std::string e(entry);
  if (refuse_capture(entry, stream)) return -1;
  if (B == 0) return 0;
  if (!d_clearance || !d_attempt) return fail(e + ": null d_clearance or d_attempt");
  if (workspace_refusal(e, d_ws, src.size_query)) return -1;
  if (!d_T_goal || !d_Y_full || !d_stats || !d_q || !d_pos_err || !d_rot_err) return fail(e + ": null buffer");
  hipStream_t s = (hipStream_t)stream;
  const int mode = opts->clearance_mode, retries = opts->retries, C = src.candidates, n = base->pc.n_joints;
  const bool atlas = src.atlas_q != nullptr, local = retries > 0 && opts->spread > 0.0;
  // the workspace: the restart arrays; behind them the screened step's, with an atlas the neighbour table in between
  const AnchRetryWs w = anch_retry_ws(anch, base, B, d_ws);
  const AnchAtlasWs aw = atlas ? anch_atlas_ws(anch, base, B, C, retries, d_ws) : AnchAtlasWs();
  const size_t screen_head = atlas ? aw.screen_head : anch_screen_head(anch, base, B);
  const AnchScreenWs sw = C ? anch_screen_ws(anch, base, B, C, screen_head, d_ws) : AnchScreenWs();
  gik_scene_set compact;      // the scene set of a compact batch: its ids are gathered into w.ids
  if (scenes) {
    compact = *scenes;
    if (scenes->d_scene_id) compact.d_scene_id = w.ids;
  }
  const RetryTol tol = {opts->pos_tol, opts->rot_tol, opts->clear_tol};
  const RetrySelectArgs select = {d_stats, d_pos_err, d_rot_err, d_clearance, tol, w.idx, w.count, B};
  // (an atlas step reads none of the draws' fields: the limits, the centre, the spread, the seed)
  const RetrySeedArgs seeds = {d_T_goal, w.idx, opts->d_q_lo, opts->d_q_hi, local ? w.q_center : nullptr, w.T, w.q_seed,
                               local ? opts->spread : 0.0, opts->seed, 0, pose_width(base), n, 0};
  const RetryMergeArgs merge = {w.idx, w.Y, w.stats, w.q, w.pos_err, w.rot_err, w.clearance,
                                d_Y_full, d_stats, d_q, d_pos_err, d_rot_err, d_clearance, d_attempt, tol, 0, anch->full_N * 3, n, 0};
  AtlasSource rows = {src.atlas_q, aw.nbr, src.atlas_count, (retries + 1) * C, 0, aw.rows};
  const auto seed_step = [&](const RetrySeedArgs &a) {      // the seeds of attempt a.attempt; atlas: from ranks [a C, (a + 1) C)
    if (!C) return retry_seed_launch(base, a, stream);
    if (atlas) {
      rows.first = a.attempt * C;
      rows.note = aw.rows + (size_t)a.attempt * (size_t)B;
    }
    return screened_seed_launch(anch, base, a, C, mode, opts->clear_tol, scenes, sw, nullptr, nullptr, stream, atlas ? &rows : nullptr);
  };
  // the centre of local mode is what attempt 0 started from; d_q_init may be d_q, which attempt 0 overwrites
  if (local) HIP_OK(hipMemcpyAsync(w.q_center, d_q_init, (size_t)B * (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, s));
  HIP_OK(hipMemsetAsync(d_attempt, 0, (size_t)B * sizeof(int32_t), s));
  int rc = 0;
  if (atlas) {
    HIP_OK(hipMemsetAsync(aw.rows, 0xFF, (size_t)B * (size_t)(retries + 1) * sizeof(int32_t), s));
    rc = atlas_nearest_launch(base, src.key_width, src.atlas_keys, src.atlas_count, d_T_goal, nullptr, B, rows.stride, aw.nbr, nullptr,
                              stream);
    if (!rc && !d_q_init) {
      RetrySeedArgs all = seeds;
      all.idx = nullptr;
      all.q_out = aw.q0;
      all.count = B;
      rc = seed_step(all);
      d_q_init = aw.q0;
    }
  }
  if (!rc) rc = anchored_attempt(anch, base, d_T_goal, d_q_init, B, scenes, w.scratch, d_Y_full, d_stats, d_q, d_pos_err, d_rot_err,
                                 d_clearance, mode, stream);
  if (rc) return rc;
  return retry_loop(entry, base, retries, select, seeds, merge, stream, seed_step, [&](int count) {
    if (scenes && scenes->d_scene_id) {      // the compact batch's scene ids
      const dim3 grid((count + ANCH_SCATTER_NT - 1) / ANCH_SCATTER_NT);
      if (launch(scene_gather_kernel, grid, dim3(ANCH_SCATTER_NT), stream, scenes->d_scene_id, w.idx, count, w.ids)) return -1;
    }
    return anchored_attempt(anch, base, w.T, w.q_seed, count, scenes ? &compact : nullptr, w.scratch, w.Y, w.stats, w.q, w.pos_err,
                            w.rot_err, w.clearance, mode, stream);
  });
}

int gik_anchored_ik_batch_atlas(const gik_template *anch, const gik_template *base, const double *d_T_goal, const double *d_q_init,
                                int B, const gik_anchored_retry_opts *opts, int candidates, const double *d_atlas_keys,
                                const double *d_atlas_q, int atlas_count, const gik_scene_set *scenes, void *d_ws, double *d_Y_full,
                                gik_stats *d_stats, double *d_q, double *d_pos_err, double *d_rot_err, double *d_clearance,
                                int32_t *d_attempt, void *stream) {
  using namespace gik;
  const char *entry = "gik_anchored_ik_batch_atlas";
  const std::string e(entry);
  // every refusal comes before anything is queued
  if (!anch || !base || B < 0 || !opts) return fail(e + ": bad argument");
  if (const std::string why = anchored_pair_fault(anch, base, PAIR_3D | PAIR_SEEDABLE); !why.empty()) return fail(e + ": " + why);
  if (scenes && scene_refusal(entry, anch, scenes)) return -1;
  if (clearance_mode_refusal(e, anch, opts->clearance_mode)) return -1;
  const int retries = opts->retries;
  std::string why;
  const int W = atlas_key_width(base, &why);
  if (!W) return fail(e + ": " + why);
  if (why = atlas_batch_fault(candidates, retries, B); !why.empty()) return fail(e + ": " + why);
  const int K = (retries + 1) * candidates;
  if (why = atlas_fault(K, atlas_count, B); !why.empty()) return fail(e + ": " + why);
  if (K > atlas_count) return fail(e + ": K = (retries + 1) * candidates exceeds atlas_count");
  if (!(opts->pos_tol > 0.0) || !(opts->rot_tol > 0.0)) return fail(e + ": pos_tol and rot_tol must be positive");
  if (!(opts->clear_tol > 0.0)) return fail(e + ": clear_tol must be positive");
  if (opts->spread != 0.0) return fail(e + ": spread must be 0 (the restarts start from atlas rows, not from draws around d_q_init)");
  if (!d_atlas_keys || !d_atlas_q) return fail(e + ": null atlas (d_atlas_keys [W][atlas_count] and d_atlas_q [atlas_count][n] are required)");
  const SeedSource src = {candidates, d_atlas_keys, d_atlas_q, atlas_count, W, "gik_anchored_ik_batch_atlas_ws_bytes"};
  return anchored_restarts(entry, anch, base, d_T_goal, d_q_init, B, opts, scenes, src, d_ws, d_Y_full, d_stats, d_q, d_pos_err, d_rot_err,
                           d_clearance, d_attempt, stream);
}

int gik_anchored_atlas_picks(const gik_template *anch, const gik_template *base, int B, int candidates, int retries, const void *d_ws,
                             const int32_t *d_attempt, int32_t *d_atlas_pick, void *stream) {
  using namespace gik;
  const std::string e("gik_anchored_atlas_picks");
  if (!anch || !base || B < 0) return fail(e + ": bad argument");
  if (const std::string why = anchored_pair_fault(anch, base, 0); !why.empty()) return fail(e + ": " + why);
  if (const std::string why = atlas_batch_fault(candidates, retries, B); !why.empty()) return fail(e + ": " + why);
  if (refuse_capture("gik_anchored_atlas_picks", stream)) return -1;
  if (B == 0) return 0;
  if (!d_ws || (uintptr_t)d_ws % 8) return fail(e + ": null or misaligned workspace (that of gik_anchored_ik_batch_atlas)");
  if (!d_attempt || !d_atlas_pick) return fail(e + ": null buffer");
  const AnchAtlasWs aw = anch_atlas_ws(anch, base, B, candidates, retries, const_cast<void *>(d_ws));
  const AtlasKeptArgs a = {d_attempt, aw.rows, d_atlas_pick, B, retries + 1};
  return launch(atlas_kept_kernel, dim3((B + ATLAS_NOTE_NT - 1) / ATLAS_NOTE_NT), dim3(ATLAS_NOTE_NT), stream, a);
}

double gik_anchored_last_solve_ms(const gik_template *anch) {
  if (!anch || !anch->ev_solve0) return -1.0;
  float ms = -1.0f;
  hipEvent_t e0, e1;
  {   // the handles under the lock (a record in another thread is not interleaved with this read), the wait outside it
    std::lock_guard<std::mutex> lock(const_cast<gik_template *>(anch)->ev_mutex);
    e0 = anch->ev_solve0;
    e1 = anch->ev_solve1;
  }
  if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) {
    (void)hipGetLastError();      // (a pair recorded by two different concurrent calls has no defined duration)
    return -1.0;
  }
  return (double)ms;
}
