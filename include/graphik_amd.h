/*
 * include/graphik_amd.h -- C ABI of the MI355X-native batched distance-geometric IK engine.
 *
 * This is the drop-in boundary for GraphIK's RiemannianSolver hot path.  The reference has no
 * FFI of its own (it is pure Python); the interfaces these entry points replace are
 *
 *   (1) the numba-AOT extension `graphik.solvers.costgrd`
 *       (graphik/solvers/costs.py:5-207, imported at graphik/solvers/riemannian_solver.py:18-21):
 *           jcost/jgrad/jhess, lcost/lgrad/lhess            -> gik_cost / gik_grad / gik_hess
 *           jcost_and_grad (:61-77), lcost_and_grad (:126-169)       -> gik_cost_and_grad
 *   (2) the numba-jitted manifold methods
 *       (graphik/utils/manifolds/fixed_rank_psd_sym.py:75-113): proj            -> gik_proj
 *   (3) pymanopt-style `TrustRegions.solve(problem, x)` as called from
 *       RiemannianSolver.solve (graphik/solvers/riemannian_solver.py:178-218,
 *       graphik/solvers/trust_region.py:112-599)                         -> gik_solve_batch
 *   (4) the per-goal pre/post-processing of solve_with_riemannian
 *       (riemannian_solver.py:220-234; dgp.py:42-65,150-183,192-231;
 *        graph_revolute.py:243-318, graph_planar.py:136-176)               -> gik_ik_batch
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  No torch / numpy types.
 *   - All `d_*` pointers are DEVICE pointers (HBM) owned by the caller (e.g. the data_ptr() of
 *     a PyTorch-ROCm tensor); the library never allocates inside a batch call except for the
 *     handle's own persistent workspace, which grows monotonically with the largest B seen.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are
 *     asynchronous with respect to the host; synchronise the stream before reading results.
 *   - Every function returns 0 on success, <0 on error; gik_last_error() returns a
 *     thread-local message for the last failure.
 *   - All floating point data is fp64 (IEEE double); vectors are N x k row-major like the
 *     reference's numpy arrays.
 */
#ifndef GRAPHIK_AMD_H
#define GRAPHIK_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GIK_ABI_VERSION 12

/* Residual-term kinds: one "term" per (index pair, kind) exactly as the loops of
 * costs.py:80-207 visit them: equality (omega != 0), lower hinge (psi_L != 0), upper hinge
 * (psi_U != 0).                                                                           */
enum { GIK_TERM_EQ = 1, GIK_TERM_LOWER = 2, GIK_TERM_UPPER = 3 };

/* Problem-graph template: everything that does not depend on the goal pose.  Mirrors the
 * arguments create_cost_limits() closes over (riemannian_solver.py:121-128): the index pairs
 * `inds` (row-major upper triangle), and which of omega / psi_L / psi_U is set on each.   */
typedef struct {
  int32_t abi_version;   /* GIK_ABI_VERSION                                               */
  int32_t N;             /* number of graph nodes (rows of Y): 2 .. 255; beyond 128 only k = 3, TrustRegions,
                            theta = 1 graphs with at most 256 terms outside a rigid clique (obstacle scenes)  */
  int32_t k;             /* embedding dimension: 3 (revolute) or 2 (planar)               */
  int32_t n_terms;       /* number of residual terms T                                    */
  const int32_t *term_i; /* [T] first node index  (i < j)                                 */
  const int32_t *term_j; /* [T] second node index                                         */
  const int32_t *term_kind; /* [T] GIK_TERM_*; terms sorted by (i, j, kind)               */
  /* trust-region parameters (riemannian_solver.py:44-50, trust_region.py:85-121)          */
  double mingradnorm;    /* 0.5e-9                                                        */
  int32_t maxiter;       /* 3000                                                          */
  int32_t maxinner;      /* 10000                                                         */
  int32_t mininner;      /* 1                                                             */
  double theta;          /* 1.0                                                           */
  double kappa;          /* 0.1                                                           */
  double rho_prime;      /* 0.1                                                           */
  double rho_regularization; /* 1e3                                                       */
  int32_t planar_proj_exact; /* 0: reproduce fixed_rank_psd_sym.py:107-110 literally (k=2) */
  int32_t force_block_path;  /* graphs with N*k > 64 (or a node busier than any wavefront variant) leave the
                                one-unknown-per-lane kernel; 0: automatic (k = 3, N*k > 64, TrustRegions: the
                                node-per-lane wavefront kernel, else the workgroup kernels), 1: the
                                workgroup-per-problem kernels even if N*k <= 64, 2: the node-per-lane kernel
                                (k = 3, TrustRegions, theta = 1, <= 256 terms outside a rigid clique)        */
  /* scheduling knobs, fixed for the life of the handle (results never depend on them; the
   * environment variables GIK_WAVES_PER_CU / GIK_SLICE / GIK_DBG are read ONCE, at
   * gik_template_create, as developer overrides of these fields)                             */
  int32_t waves_per_cu;      /* persistent solve waves (workgroups) per CU; 0 = automatic      */
  int32_t slice_outer_its;   /* time slice in outer iterations: a problem yields its slot to whatever
                                waits after that many; -1 = default (256; node-per-lane kernel 192; on the
                                wavefront kernel only for batches beyond the resident waves), 0 = off */
  int32_t debug_flags;       /* developer flags (gik_kernels.hip.h: SolveArgs::dbg); 16 = rerun tCG
                                after a rejected step instead of resuming from the checkpoint;
                                workgroup path: 64 = closed form for rigid cliques from 4 nodes
                                up (default: 16 nodes); 128 / 256 = older spellings of
                                clique_closed_form = GIK_CLIQUE_OFF / GIK_CLIQUE_DENSE; 2048 = node-per-lane
                                kernel with one wavefront per problem (two nodes per lane); 8192 = planar graphs: one
                                problem per wavefront instead of four, 16384 = four at any batch size (default: from
                                12 problems per CU on); 512 = neither round-robin
                                slicing nor tail spreading on the wavefront kernel, 1024 = no slicing
                                (scheduling measures of large batches, bit-neutral: tests compare) */
  /* which of the reference's two solvers gik_solve_batch runs (riemannian_solver.py:40-65):
   * GIK_SOLVER_TRUST_REGIONS (default) or GIK_SOLVER_CONJUGATE_GRADIENT = pymanopt 0.2.5
   * ConjugateGradient + LineSearchAdaptive as configured at :51-59.  The CG defaults of
   * mingradnorm / maxiter differ (1e-9 / 100000): gik_default_cg_params() sets them.           */
  int32_t solver;
  double cg_minstepsize;     /* 1e-10                                                         */
  double cg_orth_value;      /* 10e10                                                         */
  int32_t cg_beta_type;      /* 0 FletcherReeves, 1 PolakRibiere, 2 HestenesStiefel, 3 HagerZhang
                                (the reference passes BetaTypes[3])                           */
  /* Workgroup-per-problem path only (N*k > 64): a rigid clique -- >= 16 nodes every pair of which
   * is tied by an equality term, i.e. the anchors of a scene with obstacles (graph_base.py:182-199)
   * -- is taken out of the per-term loops and its share of lhess (costs.py:175-207) is evaluated
   * in closed form from 18 moments (+ 9 when the clique's targets are distances of points).  Same
   * function, different SUMMATION ORDER: Hessian products agree with the reference's edge loop to
   * round-off (<= 2e-15 relative), not bit for bit, so trust-region iteration counts near an
   * accept / reject threshold can differ from a run with GIK_CLIQUE_OFF (which sums the terms in
   * the reference's order).  gik_stats.flags bit 0 and gik_template_get_info report what ran.   */
  int32_t clique_closed_form; /* GIK_CLIQUE_AUTO (default) | GIK_CLIQUE_OFF | GIK_CLIQUE_DENSE     */
  /* One-unknown-per-lane wavefront kernel, k = 3 (graphs of N * k <= 64 unknowns: the arms): how lhess
   * (costs.py:175-207) is rendered.
   *   GIK_HESS_PER_EDGE: the reference's arithmetic -- per edge  s = y . (W_i - W_j),  t = 2 s a y + c w,  +t to one end
   *     and -t to the other (costs.py:186-203), the form every other kernel of the library uses.  The three lanes of a
   *     node split its term list, each evaluates its terms completely from whole rows and the three partial vectors are
   *     added (gik_wave_strict.hip.h).  Exists for TrustRegions (any theta), free-free (not anchored) graphs.
   *     Against the CPU oracle from the same start points (8192 random KUKA goals): Hessian products +1.7 %, share of
   *     goals at maxiter 668 / 677, p90 of the outer iterations 0.99 x; 7-DOF end configurations 2.9e-3 rad from the
   *     reference in the median (the reference's own two code paths: 3.0e-3).
   *   GIK_HESS_COLUMN: rows of the 3 x 3 blocks 2 a y y^T + c I, cached per accepted point, times the neighbour's
   *     entries.  s is never formed: the Gauss-Newton part's round-off leaves range(J^T) and truncated CG needs 5-8 %
   *     more Hessian products than the reference's arithmetic (7-DOF end configurations 8.4e-3 rad from the reference,
   *     2.8 x the reference pair's own spread).  Until round 5 the default; since round 6 NOT faster either (c2 34.5 k
   *     against 35.3 k solves/s, c4 125.6 k against 136.0 k: DESIGN.md 4.1, 6) -- kept as the form of the ConjugateGradient
   *     (which takes no Hessian products), anchored and planar wavefront kernels, and as an explicit choice for comparisons.
   *   GIK_HESS_AUTO (default): PER_EDGE where that kernel exists (3-D, TrustRegions, not anchored), else
   *     COLUMN.  An explicit GIK_HESS_PER_EDGE on a wavefront template without such a kernel is refused.
   * Graphs on the workgroup / node-per-lane kernels form s per edge whatever this field says (gik_template_info
   * reports GIK_HESS_PER_EDGE for them).                                                                          */
  int32_t hessian_form;
} gik_template_desc;
enum { GIK_HESS_COLUMN = 0, GIK_HESS_PER_EDGE = 1, GIK_HESS_AUTO = 2 };

enum { GIK_SOLVER_TRUST_REGIONS = 0, GIK_SOLVER_CONJUGATE_GRADIENT = 1 };
enum {
  GIK_CLIQUE_AUTO = 0,  /* closed form; (D w) by moments when the targets are Euclidean (checked per problem) */
  GIK_CLIQUE_OFF = 1,   /* every term in the per-term loops, the reference's summation order               */
  GIK_CLIQUE_DENSE = 2  /* closed form with the dense (D w) product always                                 */
};

/* Opaque handle.  The problem description in it is immutable after gik_template_create /
 * gik_pipeline_attach; what a batch call mutates is bookkeeping only, guarded inside the library:
 *   - a ring of work-queue counters and a pool of time-slicing workspaces, handed out per call
 *     under a mutex; a slot is reused only behind the event recorded after its previous launch, so
 *     any number of calls may be in flight on any number of streams and host threads;
 *   - the workgroup-per-goal prepare kernel's scratch slab (N > 32): launches on different streams
 *     are chained by an event (they serialise; results are unaffected);
 *   - anchored templates: the event pair read by gik_anchored_last_solve_ms (diagnostic; with
 *     concurrent callers it reports whichever call recorded last).
 * Because of that bookkeeping a batch call cannot be captured into a HIP graph: on a stream that is capturing
 * (hipStreamBeginCapture) gik_solve_batch / gik_ik_batch / gik_ik_batch_seeded / gik_anchored_ik_batch, the seeded anchored
 * calls (gik_anchored_seed_batch, gik_anchored_ik_batch_seeded, gik_anchored_clearance) -- and gik_prepare_batch where it
 * uses the workgroup kernel -- return an error before touching the stream.  (A batch is one persistent launch; there
 * is no launch overhead for a graph to remove.)
 * Results never depend on that bookkeeping, on the stream, on the number of calls in flight or on how the problems of
 * a batch are scheduled.  ONE property of a call does select arithmetic, and it is the number of goals in it: planar
 * graphs of at most 16 nodes run four problems to a wavefront (rtr_quad_kernel: the k = 2 projector by substitution,
 * inner products summed per node first) in batches of at least 12 problems per CU and one problem per wavefront below
 * that, so the same goal can come back with different last bits (x agrees to ~1e-9, iteration counts on 100 %,
 * inner_total on 99.3 % of 65536 goals) depending on how many goals share the call.  debug_flags 16384 / 8192 pin the
 * four-problem / one-problem kernel at every batch size; graphik_amd.distributed.solve_batch_sharded applies the rule
 * to the GLOBAL batch and pins the result, so what it gathers does not depend on the world size.  Destroying a handle
 * while calls on it are in flight is undefined; synchronise first.                                          */
typedef struct gik_template gik_template;

/* Per-problem solver statistics (final_values of the reference's optlog + counters). */
typedef struct {
  double f;            /* final cost  f(x)                                                */
  double gradnorm;     /* final ||grad||_F                                                */
  int32_t iterations;  /* outer (trust-region) iterations                                 */
  int32_t inner_total; /* tCG iterations as the reference counts them (sum of numit+1); a
                          "model increased" exit costs one product more than it reports  */
  int32_t stop;        /* 0: gradnorm < mingradnorm, 1: maxiter, 2: NaN encountered,
                          3: step size < cg_minstepsize (ConjugateGradient only)           */
  int32_t n_accept;    /* accepted steps                                                  */
  int32_t inner_executed; /* Hessian products actually evaluated: after a rejected step the
                          reference's next tCG solve repeats the previous one up to the smaller
                          radius, and the engine resumes from a checkpoint instead (same result,
                          bit for bit); inner_total counts what the reference would have run   */
  int32_t flags;       /* bit 0: workgroup kernels, rigid clique: the clique's target distances were
                          those of a point set in R^3 and its dense D w product was replaced by
                          moments (informational; results agree to round-off either way);
                          bit 1: wavefront kernel, large batch: the problem was paused at least once
                          (round-robin time slice, or handed to a wave on an idle SIMD in the tail)
                          and resumed by another wave (same result bit for bit); bits 8..31: how
                          often.  Bit 1, bits 8.. and inner_executed depend on timing            */
  double stepsize;     /* ConjugateGradient: step of the last line search (the `stepsize` entry of
                          pymanopt's final_values); TrustRegions: trust-region radius at return  */
} gik_stats;            /* 48 bytes                                                         */

/* Optional per-outer-iteration trace (device arrays of B x cap; pass NULL to disable). */
typedef struct {
  int32_t cap;
  double *d_Delta;
  int32_t *d_numit;
  int32_t *d_stop;
  double *d_f_before;
  double *d_gradnorm_after;
  int32_t *d_accept;
} gik_trace;

const char *gik_last_error(void);
int gik_abi_version(void);
int gik_device_count(void);

/* Set `desc->` trust-region fields to the reference defaults. */
void gik_default_params(gik_template_desc *desc);
/* ... and for params["solver"] = "ConjugateGradient" (riemannian_solver.py:51-59): solver,
 * mingradnorm 1e-9, maxiter 10e4, cg_minstepsize 1e-10, cg_orth_value 10e10, cg_beta_type 3.
 * With this solver gik_stats reports: iterations = CG iterations, inner_total = inner_executed =
 * cost evaluations of the line searches, n_accept = line searches that moved, stop = 0 gradnorm,
 * 1 maxiter, 2 NaN, 3 step size below cg_minstepsize; gik_trace columns: d_f_before / d_gradnorm_after
 * = cost / |grad| before step q, d_Delta = step size, d_numit = cost evaluations of the line
 * search, d_stop = direction reset to -grad, d_accept = the line search moved.               */
void gik_default_cg_params(gik_template_desc *desc);

int gik_template_create(const gik_template_desc *desc, gik_template **out);
void gik_template_destroy(gik_template *t);

/* What gik_template_create decided (informational; e.g. bench.py's executed-flop count).        */
typedef struct {
  int32_t is_block;            /* 1: workgroup-per-problem kernels (N*k > 64 or forced)             */
  int32_t max_terms_per_node;  /* compiled slot count of the wavefront kernel variant (0 on the block path) */
  int32_t n_clique;            /* nodes of the rigid clique handled in closed form (0 = none)       */
  int32_t n_slot_terms;        /* terms left in the per-term loops (= T without a clique)           */
  int32_t slots_per_thread;    /* block path: padded per-thread slot count                          */
  int32_t waves_per_cu;        /* resident solve wavefronts (workgroups) per CU                     */
  int32_t n_cu;
  int32_t lds_bytes;           /* dynamic LDS per wavefront / workgroup of the solve kernel         */
  int32_t clique_closed_form;  /* GIK_CLIQUE_* in effect                                            */
  int32_t anchored;            /* bit 0: fixed-anchor template; bit 1: link hinges are on (gik_anchored_attach_links
                                  with hinges = 1): 0, 1 or 3; bit 2: self hinges (5, 7); bit 3: half-space
                                  obstacles (gik_anchored_attach_halfspaces): 9, or 11 with link hinges   */
  int32_t has_pipeline;
  int32_t prepare_is_block;    /* workgroup-per-goal prepare kernel                                 */
  int32_t node_per_lane;       /* != 0: an is_block graph solved by the node-per-lane kernel instead of the
                                  512-thread workgroup kernel; the value is its wavefronts per problem (2: one
                                  node per lane, 1: two nodes per lane, 4: one node per lane, graphs of 129 .. 255
                                  nodes -- the only kernel that takes them)                               */
  int32_t problems_per_wave;   /* 4: planar graph (k = 2, <= 16 nodes, <= 6 terms per node) whose trust-region
                                  solves run four problems to a wavefront (rtr_quad_kernel) in batches of at
                                  least 12 problems per CU (smaller batches: one per wavefront, see the note on
                                  the handle above); else 1 (0: block) */
  int32_t goals_per_wave;      /* prepare kernel: 4 = graph of at most 16 nodes, four goals to a wavefront
                                  (prep_quad_kernel); 1 = one (prep_wave_kernel); 0 = workgroup per goal / no pipeline */
  int32_t hessian_form;        /* what the solve kernel of this template does: GIK_HESS_PER_EDGE or GIK_HESS_COLUMN
                                  (never _AUTO; workgroup and node-per-lane kernels: always _PER_EDGE)              */
  int32_t claim_key_terms;     /* terms of the claim key in effect (gik_template_set_claim_key); 0: index order        */
} gik_template_info;
int gik_template_get_info(const gik_template *t, gik_template_info *info);

/* Claim order of gik_solve_batch (and the calls built on it).  The persistent solve kernels hand out problems by
 * ticket, and a batch of a few problems per wave is as long as its longest problem plus the time that problem waited
 * for a wave.  A template may carry a KEY -- a short linear form of each problem's targets,
 *     key[b] = sum_i weights[i] * targets[b][terms[i]],   n <= 8 terms, each an index into the template's T terms --
 * and the call then hands the tickets out in ascending key order (ties in index order, NaN last): two small kernels in
 * front of the solve compute the keys and the permutation from THIS call's targets, in a leased workspace.  Which
 * problems are likely long is a property of the robot: graphik_amd passes the squared reach of the goal (the targets of
 * the terms between the base origin and the end effector's point) for robots whose goals close to the base are the
 * slow ones (tools/claim_order_study.py).  n = 0 (the default of every template) keeps index order.
 * Results never depend on it: problems are independent, the order only decides when each one starts.  It applies to
 * the one-unknown-per-lane trust-region kernels of 3-D graphs (a template on other kernels accepts a valid key and stays
 * on index order: gik_template_get_info().claim_key_terms reads 0), in batches of more problems than resident waves and
 * of at most gik_claim_order_max_batch() problems; any other call keeps index order.  Not to be
 * called while batch calls on the handle are being issued.  The environment variable GIK_CLAIM_ORDER=off makes this a
 * no-op (developer override).                                                                                     */
int gik_template_set_claim_key(gik_template *t, int n, const int32_t *terms, const double *weights);
int gik_claim_order_max_batch(void);
/* The two kernels on their own (tests, tools): d_keys [B] float from d_targets [B][T] by the template's key;
 * d_order [B] = the indices 0 .. B-1 in ascending key order (stable, NaN last), B <= gik_claim_order_max_batch().   */
int gik_claim_order_keys(const gik_template *t, const double *d_targets, int B, float *d_keys, void *stream);
int gik_claim_order_sort(const float *d_keys, int B, int32_t *d_order, void *stream);

/* costgrd twins, batched over B problems.  d_Y, d_W, d_out: [B][N*k]; d_targets: [B][T]
 * (squared goal distance for EQ terms, psi_L / psi_U for hinge terms); d_f: [B].          */
int gik_cost(const gik_template *t, const double *d_Y, const double *d_targets, int B,
             double *d_f, void *stream);                      /* lcost / jcost            */
int gik_grad(const gik_template *t, const double *d_Y, const double *d_targets, int B,
             double *d_out, void *stream);                    /* lgrad / jgrad            */
int gik_cost_and_grad(const gik_template *t, const double *d_Y, const double *d_targets, int B,
                      double *d_f, double *d_grad, void *stream); /* lcost_and_grad / jcost_and_grad:
                                                 one pass over the residual terms, same (f, G) */
int gik_hess(const gik_template *t, const double *d_Y, const double *d_W,
             const double *d_targets, int B, double *d_out, void *stream); /* lhess/jhess */
int gik_proj(const gik_template *t, const double *d_Y, const double *d_Z, int B,
             double *d_out, void *stream);                    /* PSDFixedRank.proj        */

/* TrustRegions.solve for B problems: d_Y_init -> d_Y_out ([B][N*k]), d_stats [B].          */
int gik_solve_batch(const gik_template *t, const double *d_Y_init, const double *d_targets,
                    int B, double *d_Y_out, gik_stats *d_stats, const gik_trace *trace,
                    void *stream);

/* ---- whole solve_with_riemannian pipeline on the device ------------------------------------
 * Goal-independent description of the per-goal pre/post-processing of
 * solve_with_riemannian (riemannian_solver.py:220-234): how a goal pose pins the goal nodes
 * (graph_revolute.py:243-249 / graph_planar.py:136-145), the LOWER/UPPER attributes bound
 * smoothing runs on (dgp.py:192-231), the omega pairs of linear_projection (dgp.py:174-183),
 * and the robot frames joint_variables needs (graph_revolute.py:251-318).                   */
typedef struct {
  int32_t n_joints;          /* n (1 .. 125)                                               */
  const double *T0;          /* [(n+1)][(k+1)*(k+1)] frames at zero configuration, row-major */
  const int32_t *p_index;    /* [n+1] node index of p_i                                    */
  const int32_t *q_index;    /* [n+1] node index of q_i (k=3; ignored for k=2)             */
  int32_t x_index, y_index;  /* base anchor nodes "x", "y"                                 */
  double axis_length;        /* graph.axis_length                                          */
  int32_t goal_node0;        /* node pinned at the goal position (p_n)                     */
  int32_t goal_node1;        /* q_n (k=3: p_n + axis_length*z) or p_{n-1} (k=2: p_n - len*x);
                                -1 for a position goal (position_goal_mask bit 0)            */
  double goal_len;           /* axis_length (k=3) / DIST(p_{n-1}, p_n) (k=2)               */
  const double *base_lower;  /* [N*N] LOWER of the goal-independent edges, NaN = no edge   */
  const double *base_upper;  /* [N*N] UPPER                                                */
  int32_t n_anchor;          /* nodes with a known position besides the goal nodes (<= 256;
                                graphs with N > 32 or more than 32 anchors, up to N = 128, are
                                prepared by a workgroup-per-goal kernel, same arithmetic)     */
  const int32_t *anchor_index; /* [n_anchor]                                               */
  const double *anchor_pos;  /* [n_anchor][k]                                              */
  int32_t n_pairs;           /* omega pairs (i<j) of the goal graph                        */
  const int32_t *pair_i, *pair_j;
  const int32_t *term_src;   /* [T] -1: term_static[t]; else anchor_slot*2 + goal_slot     */
  const double *term_static; /* [T] psi_L / psi_U / goal-independent squared distances     */
  int32_t last_link_along_z; /* the T_final correction of graph_revolute.py:314-316 applies */
  int32_t jacobi_sweeps;     /* 0 = default (10; graphs of more than 32 nodes: 30)          */
  int32_t force_block_prepare; /* 1: workgroup-per-goal prepare kernel even for small graphs
                                (tests; GIK_PREP_FORCE_BLOCK is read once, at attach)         */
  /* Robots with several end effectors (k = 3 trees, robot_base.py:29-41; round 6: planar trees,
   * graph_planar.py:50-88; at most 8): goal poses are [B][n_ee][(k+1)^2] in the order of `ee_goal_nodes`;
   * n_ee <= 1 (or 0) is the chain above and the arrays below may be NULL.  last_link_along_z then
   * holds one bit per end effector.                                                             */
  int32_t n_ee;
  const int32_t *ee_goal_nodes; /* [2 * n_ee] graph nodes pinned by goal pose e: (p_e, q_e); k = 2: (the end effector,
                                   its parent -- or -1 where an earlier end effector's pose pins that parent already:
                                   graph_planar.py:136-145 keeps the first); either k: (p_e, -1) for a position goal
                                   (position_goal_mask)                                          */
  const int32_t *ee_path;       /* [n_ee][n + 1] joint numbers from the root to end effector e
                                   (path[0] = 0), -1 padded; a parent's number precedes its
                                   children's nowhere assumed                                   */
  int32_t n_goal_pairs;         /* goal-node pairs of DIFFERENT end effectors tied by an edge   */
  int32_t position_goal_mask;   /* bit e: end effector e has a POSITION goal -- the reference's graph.from_pos({p_e: xyz})
                                   (graph_base.py:146-165): p_e alone is pinned and its orientation is free.  0: every goal
                                   is a pose, the behaviour of every earlier build (the field was reserved1, zero).
                                   Where bit e is set:
                                   - goal_node1 (a chain) or ee_goal_nodes[2 e + 1] must be -1: the odd slot is inert, no
                                     term_src may name it, and base_lower / base_upper / term_static hold what the graph
                                     holds between q_e (k = 2: the parent) and the anchors;
                                   - of pose e in d_T_goal only the translation column is read (pack a point into an
                                     identity-rotation pose);
                                   - no T_final correction applies to it (graph_revolute.py:314-316 runs only for an end
                                     effector with a T_final entry): bit e of last_link_along_z must be clear, and the last
                                     angle of such an arm is what the point formula gives, as in the reference;
                                   - gik_recover_batch's rot_err excludes it: 0.0 when every goal is a position, else the
                                     worst of the pose end effectors.  The restart rule rot_err > rot_tol then never fires.
                                   gik_pipeline_attach refuses a set bit with a non-negative odd slot, a bit at or beyond
                                   n_ee, and a bit that last_link_along_z also has.  Every gik_anchored_* entry that takes a
                                   `base` template refuses one with a non-zero mask.                              */
  const int32_t *goal_pair_a, *goal_pair_b;  /* [n_goal_pairs] slots into ee_goal_nodes; term_src
                                   of such a term = 2 n_ee n_anchor + pair; of an anchor<->goal
                                   term = anchor_slot * 2 n_ee + goal slot                     */
  const double *ee_goal_len;    /* [n_ee] k = 2 trees: length of the link parent(e) -> e (goal_len of a chain)      */
} gik_pipeline_desc;

int gik_pipeline_attach(gik_template *t, const gik_pipeline_desc *desc);

/* k = 3, after gik_pipeline_attach and before the first gik_recover_batch, optional.  End effector `ee` has a position goal
 * and its last link lies along its joint's z axis.  joint_variables' point formula (graph_revolute.py:308) takes the last
 * angle from atan2 of qs_0 = (T0[pred]^-1 T0[ee] trans_z(axis_length)).trans against the recovered point, and with no
 * T_final to correct it (:314-316) that is the answer.  For such a link the x, y of qs_0 are round-off residues of the frame
 * product: their DIRECTION alone decides the angle, and it depends on the order of the operations that formed them.  (x, y)
 * replaces what gik_recover_batch forms from T0, so that a caller who mirrors a host implementation -- the Python layer
 * passes the residues of the reference's own operations -- gets that implementation's angle.  Any angle is a solution: the
 * joint turns about an axis through the goal point.  Errors: no pipeline, k = 2, ee without a position goal, a non-finite
 * value.                                                                                                              */
int gik_pipeline_set_point_axis(gik_template *t, int ee, double x, double y);

/* goal poses [B][n_ee][(k+1)^2] (row-major homogeneous matrices) -> per-term targets [B][T] and the
 * initial point [B][N*k] (from_pose + bound_smoothing + generate_initialization).
 * d_K_out (optional, [B] int32): the MDS column count chosen per goal.                     */
int gik_prepare_batch(const gik_template *t, const double *d_T_goal, int B, double *d_targets,
                      double *d_Y_init, int32_t *d_K_out, void *stream);

/* Diagnostic twin of gik_prepare_batch: also returns what the reference computes on the way, so
 * that each stage can be checked against captured reference data on its own -- bound_smoothing's
 * output (dgp.py:192-231) and the eigenvalue spectra behind generate_initialization
 * (riemannian_solver.py:67-75; dgp.py:150-183): row 0 the Gram matrix of the interpolated bounds,
 * row 1 the matrix MDS() takes its rank from (dgp.py:166-167), row 2 the scatter matrix of
 * linear_projection (zero beyond the MDS rank); all unsorted.  Any pointer may be NULL.        */
typedef struct {
  double *d_lb, *d_ub;   /* [B][N*N]  (both or neither)                                       */
  double *d_eig;         /* [B][3][N]                                                         */
} gik_prepare_diag;
int gik_prepare_batch_debug(const gik_template *t, const double *d_T_goal, int B,
                            double *d_targets, double *d_Y_init, int32_t *d_K_out,
                            const gik_prepare_diag *diag, void *stream);

/* points [B][N*k] + goal poses -> joint angles [B][n], EE position / rotation error of
 * FK(q) against the goal [B] (joint_variables + robot.pose + the examples' error metric).  */
int gik_recover_batch(const gik_template *t, const double *d_Y, const double *d_T_goal, int B,
                      double *d_q, double *d_pos_err, double *d_rot_err, void *stream);

/* prepare + solve + recover on one stream.  d_Y [B][N*k] receives the solution points and
 * doubles as the Y_init buffer; d_targets [B][T] is caller-provided scratch.               */
int gik_ik_batch(const gik_template *t, const double *d_T_goal, int B, double *d_targets,
                 double *d_Y, gik_stats *d_stats, double *d_q, double *d_pos_err,
                 double *d_rot_err, void *stream);

/* ---- joint-configuration warm starts --------------------------------------------------------
 * The reference's warm start is RiemannianSolver.solve(D_goal, omega, Y_init=..., bounds=None)
 * (riemannian_solver.py:178-218; a `bounds` argument would discard the seed, :197-198), with the seed
 * built as its examples build it: Y_init = pos_from_graph(graph.realization(q_init))
 * (experiments/simple_ik_examples/test_chain_2d_new.py:46-59; graph_base.py:112-120).
 *
 * gik_seed_batch: goal poses [B][n_ee][(k+1)^2] + seed angles d_q_init [B][n] (joint p_i in column i-1)
 *   -> per-term targets [B][T], bit-identical to gik_prepare_batch's, and Y_init [B][N*k]: the realization of
 *   q_init in node order -- p_i = translation of frame i and (k = 3) q_i = p_i + axis_length z_i
 *   (graph_revolute.py:243-249); k = 2: graph_planar.py:136-145 (a child u pins p_u and its parent's
 *   p_u - |parent u| x_u); every other node (x, y, obstacles) at its anchor_pos.  The goal nodes take the
 *   SEED's positions, as in the reference.  Frames follow ee_path from T0 (gik_recover_batch's walk).  No
 *   bound smoothing, no MDS.  Errors: no pipeline attached, B < 0, a null buffer; a graph with a node that
 *   neither a joint frame nor an anchor places.
 * gik_ik_batch_seeded: gik_seed_batch -> gik_solve_batch -> gik_recover_batch on one stream; the buffers
 *   are gik_ik_batch's.  d_q_init MAY alias d_q (the seed is read by the first kernel, q written by the
 *   last; path tracking feeds each waypoint's answer back this way).  A capturing stream is refused before
 *   anything is queued, like gik_ik_batch.                                                      */
int gik_seed_batch(const gik_template *t, const double *d_T_goal, const double *d_q_init, int B,
                   double *d_targets, double *d_Y_init, void *stream);
int gik_ik_batch_seeded(const gik_template *t, const double *d_T_goal, const double *d_q_init, int B,
                        double *d_targets, double *d_Y, gik_stats *d_stats, double *d_q,
                        double *d_pos_err, double *d_rot_err, void *stream);

/* ---- restarts from random joint configurations (opt-in) ---------------------------------------
 * The reference has ONE start per goal (the 0.9-interpolated bounds + MDS, riemannian_solver.py:67-75), and a goal
 * that start does not solve stays unsolved.  Here a failed goal can be solved again from joint angles drawn uniformly
 * inside the joint limits (the seeded solve above), and the better of the answers is kept -- without the batch
 * leaving the device: the failed goals are compacted, seeded, solved as a batch of their own and merged back.
 *
 * failed(goal)  :=  stats.stop != 0  ||  !(pos_err <= pos_tol)  ||  !(rot_err <= rot_tol)      (NaN counts as failed)
 * score(goal)   :=  max(pos_err / pos_tol, rot_err / rot_tol);  +inf if either error is NaN
 * better(r, i)  :=  (r succeeds and i failed)  ||  (same success class  &&  score(r) < score(i))
 *                   -- a NaN never wins, a tie keeps the incumbent.
 *
 * gik_retry_select: d_idx[0 .. *d_count) = the failed goals of the batch, in NO particular order (one atomic per
 *   wavefront); *d_count is zeroed by the call.  d_idx holds B entries.
 * gik_retry_seeds: for compact slot r, goal g = d_idx[r]: d_T_out[r] = d_T_goal[g] (n_ee (k+1)^2 doubles) and
 *   d_q_out[r][j] = q_lo[j] + u (q_hi[j] - q_lo[j]) (one rounded product, one rounded sum), u in [0, 1) from a
 *   counter-based generator -- a function of (seed, g, attempt, j) alone, so a goal's seed depends neither on which
 *   other goals failed nor on its slot:
 *       c = (g * 64 + attempt) * 128 + j + 1;   z = seed + 0x9E3779B97F4A7C15 * c   (mod 2^64)
 *       z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31   (splitmix64)
 *       u = (z >> 11) * 2^-53
 *   (attempt 0 .. 63, n <= 125.)  graphik_amd.solvers.riemannian_solver.retry_seeds_host returns the same bits.
 * gik_retry_merge: for compact slot r (one wavefront each), goal g = d_idx[r] (entries distinct): if the retry's
 *   answer is better than the incumbent's, the Y row, the gik_stats record, the q row, pos_err and rot_err of goal g
 *   are replaced together and d_attempt[g] = attempt; otherwise nothing of goal g is written.
 * gik_ik_batch_retry: attempt 0 is exactly gik_ik_batch (d_q_init NULL) or gik_ik_batch_seeded on the caller's
 *   buffers, preceded by a memset of d_attempt [B] to 0; with retries = 0 the call queues exactly that and nothing
 *   else.  Then for a = 1 .. retries: select -> the 4-byte count is copied to the host -> stop if it is 0 -> seeds ->
 *   gik_seed_batch, gik_solve_batch, gik_recover_batch on the compact buffers in d_ws with B' = count -> merge.
 *   THIS CALL SYNCHRONISES ITS STREAM (hipStreamSynchronize) ONCE PER ATTEMPT after the first: the solve kernels take
 *   their batch size from the host.  The last merge is queued like every other batch call: synchronise the stream
 *   before reading the results.
 *   What comes back: d_attempt[g] = the attempt whose answer goal g holds (0: the first).  A 3-D problem's bits do not
 *   depend on the batch it is solved in (see the note on the handle), so a goal with d_attempt[g] = a > 0 holds exactly
 *   what gik_ik_batch_seeded returns for that goal alone from the seed of (seed, g, a); planar graphs' last bits may
 *   depend on the batch size, as everywhere.
 *   d_ws: caller-owned, gik_retry_ws_bytes(t, B) bytes (sized for the case that every goal fails), 8-byte aligned.
 *   Refused, with a message, before anything is queued: a capturing stream; a template without a pipeline; retries
 *   outside 0 .. 63; and with retries > 0 a graph gik_seed_batch cannot seed (its reason is passed on), null limits,
 *   a tolerance that is not positive, a null workspace.                                                       */
typedef struct {
  int32_t retries;        /* further attempts for goals that failed: 0 .. 63                              */
  int32_t clearance_mode; /* not read here (this rule has no clearance part); set 0.  Named as the field of
                           * gik_anchored_retry_opts, whose first fields are this struct's                  */
  uint64_t seed;          /* of the generator; the same seed gives the same answers                       */
  double pos_tol;         /* a goal succeeds with stop == 0, pos_err <= pos_tol and rot_err <= rot_tol    */
  double rot_tol;
  const double *d_q_lo;   /* [n] device: the seeds are drawn uniformly in [q_lo[j], q_hi[j]]              */
  const double *d_q_hi;   /* [n] device                                                                   */
} gik_retry_opts;

int gik_retry_select(const gik_stats *d_stats, const double *d_pos_err, const double *d_rot_err, int B,
                     double pos_tol, double rot_tol, int32_t *d_idx, int32_t *d_count, void *stream);
int gik_retry_seeds(const gik_template *t, const double *d_T_goal, const int32_t *d_idx, int count, uint64_t seed,
                    int attempt, const double *d_q_lo, const double *d_q_hi, double *d_T_out, double *d_q_out,
                    void *stream);
int gik_retry_merge(const gik_template *t, const int32_t *d_idx, int count, int attempt, double pos_tol,
                    double rot_tol, const double *d_Y_r, const gik_stats *d_stats_r, const double *d_q_r,
                    const double *d_pos_err_r, const double *d_rot_err_r, double *d_Y, gik_stats *d_stats,
                    double *d_q, double *d_pos_err, double *d_rot_err, int32_t *d_attempt, void *stream);
size_t gik_retry_ws_bytes(const gik_template *t, int B);
int gik_ik_batch_retry(const gik_template *t, const double *d_T_goal, const double *d_q_init /* may be NULL */,
                       int B, const gik_retry_opts *opts, void *d_ws, double *d_targets, double *d_Y,
                       gik_stats *d_stats, double *d_q, double *d_pos_err, double *d_rot_err,
                       int32_t *d_attempt, void *stream);

/* ---- fixed-anchor formulation: "intended" obstacle semantics (opt-in) -----------------------
 * graph_base.py:182-211 ties every node with a known position (base frame, goal nodes, obstacle
 * centres) to the others by equality edges and MEANS to add robot<->obstacle lower-bound hinges
 * (:205-211; the TYPE comparison at :207 never fires, so the reference creates none -- that
 * observable behaviour stays the default of this library).  Here those nodes are constants
 * instead of rows of Y, and the hinges exist: UR10 + table_environment() is a 10-node problem with
 * 100 point-to-obstacle hinges per p-node instead of N = 116 / 5612 terms.  The free nodes are the
 * template's N nodes; its terms are the free-free terms (targets are template constants:
 * `term_target`).  With an anchored template
 *   - gik_solve_batch's `d_targets` argument carries the per-problem goal anchors [B][n_goal*3],
 *     and so does the `d_targets` argument of gik_cost / gik_grad / gik_cost_and_grad / gik_hess;
 *   - gik_proj is the identity (the anchors fix the gauge; the search space is Euclidean).     */
typedef struct {
  int32_t n_anchor;              /* rows of the pinned-anchor table (<= 16): base + goal anchors */
  int32_t n_goal_anchor;         /* the LAST n_goal_anchor rows are per-problem (goal nodes)     */
  const double *anchor_pos;      /* [n_anchor][3] world positions (goal rows ignored)            */
  const double *term_target;     /* [T] squared targets of the template's (free-free) terms      */
  int32_t n_pin;                 /* point-to-anchor terms, at most 8 per free node               */
  const int32_t *pin_node;       /* [n_pin] free node                                            */
  const int32_t *pin_anchor;     /* [n_pin] anchor row                                           */
  const int32_t *pin_kind;       /* [n_pin] GIK_TERM_*                                           */
  const double *pin_target;      /* [n_pin] squared distance / psi_L / psi_U                     */
  int32_t n_obs;                 /* spherical obstacles                                          */
  int32_t reserved0;
  const double *obs;             /* [n_obs][4] centre x, y, z and SQUARED radius                 */
  const int32_t *obs_node_mask;  /* [N] 1: the free node keeps |Y_i - centre| >= radius          */
  /* mapping to the robot graph (gik_anchored_ik_batch) */
  int32_t full_N;                /* nodes of the robot graph                                     */
  int32_t reserved1;
  const int32_t *free_full_index;    /* [N]                                                      */
  const int32_t *anchor_full_index;  /* [n_anchor]; goal rows: p_n then q_n                      */
  double axis_length;
} gik_anchored_desc;

int gik_template_create_anchored(const gik_template_desc *desc, const gik_anchored_desc *adesc,
                                 gik_template **out);

/* goal poses -> joint angles through the anchored solve, one stream, no host round trip:
 * gik_prepare_batch on `base` (the robot graph WITHOUT obstacles, pipeline attached: bound
 * smoothing + MDS initial point) -> orthogonal Procrustes fit of that point's anchor rows onto the
 * world frame -> anchored trust-region solve -> full point matrix d_Y_full [B][full_N*3] ->
 * gik_recover_batch on `base`.  d_ws: scratch of gik_anchored_ws_doubles(anch, base, B) doubles. */
size_t gik_anchored_ws_doubles(const gik_template *anch, const gik_template *base, int B);
int gik_anchored_ik_batch(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                          int B, double *d_ws, double *d_Y_full, gik_stats *d_stats, double *d_q,
                          double *d_pos_err, double *d_rot_err, void *stream);

/* ---- the anchored solve from a joint-configuration seed; clearance ---------------------------
 * The seed: joint angles d_q_init [B][n] (as gik_seed_batch takes them).  gik_seed_batch on `base` writes
 * graph.realization(q_init) of the robot graph, which is already in the world frame with the base anchors
 * at their positions; the anchored start point is a row gather of it -- Y_free[f] = Y_full[free_full_index[f]],
 * copied bit for bit, no Procrustes fit.  The goal nodes do NOT come from the seed: they are constants of the
 * goal here, so their seed rows are dropped and d_goal [B][n_goal*3] is computed from the goal pose (p_n = t,
 * q_n = t + axis_length z), exactly as the cold call computes it.
 *
 * gik_anchored_seed_batch: the start point alone -- d_Y_free [B][N*3] and d_goal [B][n_goal*3], what
 *   gik_solve_batch on `anch` takes.  d_ws: gik_anchored_ws_doubles(anch, base, B) doubles.
 * gik_anchored_ik_batch_seeded: seed -> gather -> gik_solve_batch on `anch` -> full point matrix ->
 *   gik_recover_batch on `base` -> clearance if d_clearance is not NULL; one stream, no host synchronisation.
 *   The seed angles are read by the first kernel only, so d_q_init may alias d_q (path tracking: waypoint l
 *   starts from waypoint l-1's answer in place).  The outputs are those of gik_anchored_ik_batch; the event
 *   pair of gik_anchored_last_solve_ms is recorded around the solve kernel as there.
 * gik_anchored_clearance: d_clearance [B] = min over (free node i with obs_node_mask[i] == 1, obstacle o) of
 *   |Y_i - centre_o| - radius_o, read from a full point matrix d_Y_full [B][full_N*3] (radius_o is the square
 *   root of the descriptor's squared radius).  >= 0: no masked node is inside a sphere -- which says nothing of
 *   the links BETWEEN the nodes (gik_anchored_link_clearance below).  Anchors are not
 *   counted (the end effector sits where the goal puts it).  No obstacle, or no masked node: +infinity.  A NaN
 *   coordinate of a masked node: NaN for that goal alone.
 * Refused with a message before anything is queued: a capturing stream; an `anch` that is not a fixed-anchor
 * template; a `base` without pipeline, with N != full_N, or that gik_seed_batch cannot seed (its reason is
 * passed on); a null d_q_init or any other null buffer; B < 0.  B == 0 returns 0.                       */
int gik_anchored_seed_batch(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                            const double *d_q_init, int B, double *d_ws, double *d_Y_free, double *d_goal,
                            void *stream);
int gik_anchored_clearance(const gik_template *anch, const double *d_Y_full, int B, double *d_clearance,
                           void *stream);
int gik_anchored_ik_batch_seeded(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                                 const double *d_q_init, int B, double *d_ws, double *d_Y_full,
                                 gik_stats *d_stats, double *d_q, double *d_pos_err, double *d_rot_err,
                                 double *d_clearance /* may be NULL */, void *stream);

/* ---- clearance of whole links, and its sweep between two configurations -------------------------
 * gik_anchored_clearance measures the joint points.  A link is the segment between two rows of the full point matrix
 * (on a chain, consecutive p-nodes); it can pass through a sphere with both of its ends outside.
 *
 * gik_anchored_attach_links: the link set of an anchored template, attached once after creation (as
 *   gik_pipeline_attach): link l runs from row link_a[l] to row link_b[l] of the full point matrix and is a capsule of
 *   radius link_radius[l] >= 0 metres.  Any row may be named, anchors and goal rows included (the last link ends at the
 *   end effector).  Refused with a message: a handle that is not a fixed-anchor template, n_link outside 0 .. 64, a row
 *   outside [0, full_N), a radius that is negative, NaN or infinite, a second attach.
 *   hinges = 0: the links are measured only.  hinges = 1: the solve kernel also carries LINK HINGES -- per (link, sphere),
 *   with A, B the link's ends, R = radius_o + link_radius[l] and the foot parameter t below,
 *       m = (1 - t) A + t B - c_o;  d = m.m;  res = R^2 - d;  active <=> res > 0;  c = d - R^2
 *       f += res^2;   G_A += (1 - t) 2 c m;   G_B += t 2 c m          (f = sum res^2, G = 1/2 grad f)
 *       H_A += (1 - t) 2 (2 (m.w) m + c w);  H_B += t (...);   w = (1 - t) W_A + t W_B   (W of a constant end is 0)
 *   on top of the node hinges of obs_node_mask, which stay (where t clamps to a masked end of a link of radius 0 that
 *   node's residual is counted once more: the same zero set, a heavier weight).  The gradient is exact (the distance to a
 *   segment is C^1; envelope theorem).  The Hessian is the frozen-t model on purpose; the trust-region ratio is taken on
 *   the true cost, so its error costs iterations, not correctness.  The template's solve and known-answer kernels are
 *   re-resolved to their link builds, so every call on the handle -- gik_anchored_ik_batch, _seeded, _retry,
 *   gik_solve_batch, gik_cost / gik_grad / gik_cost_and_grad / gik_hess -- then runs them; gik_template_get_info reports
 *   anchored = 3.  A link with two constant ends carries no hinge (it is still measured).  Refused with hinges = 1, each
 *   with a message and before anything is uploaded: a value other than 0 or 1; a template on the 20-slot kernel variant;
 *   more than 2 hinge links at one free node; a link whose two free ends share no term; a link end that is neither a free
 *   node nor an anchor row.
 * gik_anchored_link_clearance: d_clearance [B] = min over (link l, obstacle o) of
 *       d = b - a;  L2 = d.d;  u = c_o - a;   t = L2 > 0 ? min(max((u.d) / L2, 0), 1) : 0;   v = u - t d
 *       |v| - radius_o - link_radius[l]
 *   on d_Y_full [B][full_N*3]: the distance from the sphere to the capsule (a zero-length link is its point).  With
 *   radius 0 and the chain's skeleton it is <= gik_anchored_clearance of the same points, since a segment holds its
 *   ends.  No obstacle, or no link: +infinity.  A NaN coordinate of a link end: NaN for that goal alone.  One wavefront
 *   per goal.  Refused: what gik_anchored_clearance refuses, and a template without links.  B == 0 returns 0.
 * gik_anchored_sweep_clearance: d_clearance [B] = min over s = 0 .. samples of the link clearance of the robot at
 *       q_s = (1 - w) q_a + w q_b,   w = s / samples      (two rounded products, one rounded sum; s = 0 is q_a, s = S is q_b)
 *   for d_q_a, d_q_b [B][n]: the joint-space line between two configurations, realized by gik_seed_batch's walk on
 *   `base` (every row comes from q_s, the end effector too).  A NaN at any sample gives NaN.
 *   THE SWEEP IS SAMPLED, NOT CONSERVATIVE: a link can enter and leave a sphere between two samples.  The caller picks
 *   `samples` from its joint step -- a link of length L turning by dq moves its far end by about L dq, so samples >=
 *   L max|q_b - q_a| / (the penetration that matters) bounds what is missed.
 *   One stream, four launches (interpolate, realize, link clearance of all B (samples + 1) configurations, minimum), no
 *   host synchronisation.  d_ws: gik_anchored_sweep_ws_bytes(anch, base, B, samples) bytes, 8-byte aligned (0: bad
 *   arguments).  Refused: what gik_anchored_seed_batch refuses of the handles and the stream, a template without
 *   links, samples < 1, B (samples + 1) beyond an int, a null buffer.  B == 0 returns 0.                          */
typedef struct {
  int32_t n_link;               /* 0 .. 64                                                        */
  int32_t hinges;               /* 0: measure only; 1: the solve carries link hinges (see above)  */
  const int32_t *link_a;        /* [n_link] row of the full point matrix where the link starts    */
  const int32_t *link_b;        /* [n_link] ... and where it ends                                 */
  const double *link_radius;    /* [n_link] capsule radius, metres, >= 0                          */
} gik_link_desc;

int gik_anchored_attach_links(gik_template *anch, const gik_link_desc *links);
int gik_anchored_link_clearance(const gik_template *anch, const double *d_Y_full, int B, double *d_clearance,
                                void *stream);
size_t gik_anchored_sweep_ws_bytes(const gik_template *anch, const gik_template *base, int B, int samples);
int gik_anchored_sweep_clearance(const gik_template *anch, const gik_template *base, const double *d_q_a,
                                 const double *d_q_b, int B, int samples, double *d_ws, double *d_clearance,
                                 void *stream);

/* ---- self-collision clearance: link against link (opt-in) ----------------------------------------
 * The link clearance measures the links against the world.  Against the robot itself it sees nothing: an answer whose
 * wrist passes through its own upper arm is clear of every sphere.  The self clearance is the same measure between two
 * links of the attached set.
 *
 * gik_anchored_attach_self_pairs: the link pairs that are measured, attached once, AFTER the links: pair p is links
 *   pair_l[p] and pair_m[p] of the set of gik_anchored_attach_links.  n_pair is within 0 .. 2016 (every pair of 64
 *   links).  Refused with a message: a handle that is not a fixed-anchor template, no links attached, pairs already
 *   attached, n_pair out of range, a null array with n_pair > 0, an index outside [0, n_link), l == m.  A pair of links
 *   that SHARE AN END ROW is legal here: its distance is 0 and its value -link_radius[l] - link_radius[m], whatever the
 *   configuration -- the caller leaves such pairs out (the Python layer refuses them).
 * gik_anchored_self_clearance: d_clearance [B] = min over the attached pairs (l, m) of
 *       d1 = b1 - a1, d2 = b2 - a2, r = a1 - a2      (a1 -> b1: link l; a2 -> b2: link m)
 *       a = d1.d1, e = d2.d2, f = d2.r, c = d1.r, b = d1.d2, den = a e - b b
 *       s = (a > 0 && den > 0) ? clamp((b f - c e) / den, 0, 1) : 0;      t = e > 0 ? (b s + f) / e : -1
 *       t < 0:  t = 0, s = a > 0 ? clamp(-c / a, 0, 1) : 0;      t > 1:  t = 1, s = a > 0 ? clamp((b - c) / a, 0, 1) : 0
 *       v = (a1 + s d1) - (a2 + t d2);      |v| - link_radius[l] - link_radius[m]
 *   on d_Y_full [B][full_N*3]: the distance between the two capsules (a zero-length link is its point: e == 0 takes the t < 0 branch; parallel links
 *   take s = 0 and the clamps; crossing links give -link_radius[l] - link_radius[m]).  >= 0: no two measured links
 *   overlap.  No pair attached (n_pair == 0): +infinity.  A NaN coordinate of an end of a measured link: NaN for that goal
 *   alone.  Up to 16 pairs four goals share a wavefront, beyond that a goal has its own.  Refused: what
 *   gik_anchored_link_clearance refuses, and a template without self pairs attached.  B == 0 returns 0.
 * gik_anchored_sweep_clearances: gik_anchored_sweep_clearance with two optional outputs over ONE interpolation and ONE
 *   realization of the B (samples + 1) configurations: d_link_out [B] (what gik_anchored_sweep_clearance writes, bit for
 *   bit) and d_self_out [B], the minimum over the samples of the self clearance.  LIKE IT, THE SWEEP IS SAMPLED, NOT
 *   CONSERVATIVE: two links can meet and part between two samples; pick `samples` from the joint step as there.
 *   d_ws: the same workspace, gik_anchored_sweep_ws_bytes.  Refused: what gik_anchored_sweep_clearance refuses, both
 *   outputs null, d_self_out given on a template without self pairs attached.  B == 0 returns 0.
 * clearance_mode = GIK_CLEARANCE_LINKS_SELF (below) puts min(link clearance, self clearance) behind the restart rule.
 * gik_anchored_attach_self_hinges: SELF HINGES (opt-in), once, AFTER gik_anchored_attach_self_pairs: the attached pairs
 *   become terms of the solve, so that the trust-region solve itself pushes the robot's links apart.  Per pair (l, m)
 *   with R = link_radius[l] + link_radius[m] and (s, t), v of the formulas above:
 *       d = v.v,  res = R^2 - d,  active where res > 0,  c = -res,  w = (1 - s, s, -(1 - t), -t) on the ends a1, b1, a2, b2
 *       f += res^2;   G_P += w_P 2 c v;   H_P += w_P 2 (2 v v^T + c I) (sum_Q w_Q W_Q)      (a constant end: W = 0, no G, no H)
 *   sqrt(d) - R is gik_anchored_self_clearance's value of the pair bit for bit.  The gradient is exact wherever the
 *   closest pair of points is unique; the Hessian is the model with (s, t) frozen.  A pair with R == 0 is never active.
 *   The template's solve, known-answer and scene kernels become the self builds of its current form (with or without
 *   link hinges), with their LDS bytes and occupancy (gik_template_info.anchored gains bit 4: 5, or 7 with link hinges);
 *   every later call on the template runs them.  With no pair active a solve's results are those of the build without.
 *   Refused with a message, nothing launched: a handle that is not a fixed-anchor template, a second call, no links
 *   attached, no self pairs attached, more than 16 pairs attached (the clearance keeps its 2016), a template on the
 *   20-slot kernel, a link of a pair that ends at a row which is neither a free node nor an anchor row. */
int gik_anchored_attach_self_pairs(gik_template *anch, int n_pair, const int32_t *pair_l, const int32_t *pair_m);
int gik_anchored_attach_self_hinges(gik_template *anch);
int gik_anchored_self_clearance(const gik_template *anch, const double *d_Y_full, int B, double *d_clearance,
                                void *stream);
int gik_anchored_sweep_clearances(const gik_template *anch, const gik_template *base, const double *d_q_a,
                                  const double *d_q_b, int B, int samples, double *d_ws,
                                  double *d_link_out /* may be NULL */, double *d_self_out /* may be NULL */,
                                  void *stream);

/* ---- half-space obstacles in the fixed-anchor solve: floors and walls (opt-in) ---------------------
 * A half-space h is (n_h, d_h) with |n_h| = 1; the allowed side is s_h(p) = n_h.p - d_h >= 0.  The anchors fix the world
 * frame, so s_h is a linear function of one row of the point matrix.
 * gik_anchored_attach_halfspaces: once and LAST -- after gik_anchored_attach_links and gik_anchored_attach_self_pairs where
 *   those are used.  halfspaces [n_half][4] holds (nx, ny, nz, d0) per row, n_half within 1 .. 8; node_margin [N] holds a
 *   margin mu_i >= 0 in metres per free node, read where obs_node_mask is 1.  Every masked free node i then carries, per
 *   half-space,
 *       res = mu_i - s_h(Y_i),  active where res > 0 (a node exactly on the boundary is inactive)
 *       f += res^2;   G_i += -res n_h;   H_i += (n_h . W_i) n_h      (G = 1/2 grad f, H = 1/2 Hess f [W], as everywhere)
 *   The Hessian block n n^T is exact wherever the active set does not change.  Unmasked nodes and anchors carry nothing.
 *   A linear function on a segment takes its minimum at an end: with mu_i = the radius of the capsules that end at node
 *   i, the node terms keep whole links on the allowed side, with or without link hinges.
 *   The template's solve, known-answer and scene kernels become the half-space builds of its current form (with or
 *   without link hinges), with their LDS bytes and occupancy (gik_template_info.anchored gains bit 8: 9, or 11 with link
 *   hinges); every later call on the template runs them.  With no half-space active a solve's results are those of the
 *   build without.  With scenes the half-spaces stay constants of the handle -- the room; the spheres vary per goal.
 *   Refused with a message, nothing uploaded: a handle that is not a fixed-anchor template, a second call, n_half outside
 *   1 .. 8, a null array, an entry that is not finite, | |n|^2 - 1 | > 1e-12, a margin of a masked node that is negative
 *   or not finite, a template on the 20-slot kernel, a template with self hinges attached.  On a handle with half-spaces
 *   gik_anchored_attach_self_hinges, and gik_anchored_attach_links with hinges = 1, are refused and leave it unchanged.
 * gik_anchored_halfspace_clearance: d_clearance [B] on d_Y_full [B][full_N*3] =
 *       links = 0: min over (masked free node i, h) of s_h(Y_i) - mu_i
 *       links = 1: min over (attached link l, both of its end rows P -- anchors and goal rows included --, h) of
 *                  s_h(P) - link_radius[l]
 *   with s_h = ((nx x + ny y) + nz z) - d0, every product and sum rounded on its own.  No node or no link: +infinity.  A
 *   NaN coordinate: NaN for that goal alone.  Refused: what gik_anchored_link_clearance refuses, a template without
 *   half-spaces, links outside {0, 1}, and links = 1 without links attached.  B == 0 returns 0.
 * On a handle with half-spaces EVERY clearance the library reports is the NaN-propagating minimum of the spheres' value and
 * this one (links = 0 behind the node clearance, 1 behind the link modes): gik_anchored_clearance, _link_clearance and their
 * scene variants, the clearance of every solve entry and restart in every clearance_mode, and the link output of both sweep
 * entries, per sample and before the minimum over the samples.  The restart rule therefore reads the room too.
 * gik_anchored_self_clearance stays what it is. */
int gik_anchored_attach_halfspaces(gik_template *anch, int n_half, const double *halfspaces /* [n_half][4]: nx, ny, nz, d0 */,
                                   const double *node_margin /* [N] free nodes, metres; read where obs_node_mask is 1 */);
int gik_anchored_halfspace_clearance(const gik_template *anch, const double *d_Y_full, int B, int links /* 0: nodes, 1: links */,
                                     double *d_clearance, void *stream);

/* ---- restarts in the anchored solve, with a clearance rule (opt-in) -----------------------------
 * The restarts of gik_ik_batch_retry for the fixed-anchor formulation.  The obstacle hinges are soft cost terms: an
 * answer can stop on its gradient bar with the end effector on the goal and a joint point inside a sphere, which the rule
 * of the plain restarts calls a success.  Here the rule also reads the answer's clearance: that of the masked nodes
 * (gik_anchored_clearance; clearance_mode = GIK_CLEARANCE_NODES, the default), which does not see a link that crosses a
 * sphere between two nodes outside it, or that of whole links (gik_anchored_link_clearance; GIK_CLEARANCE_LINKS, for a
 * template with links attached), or the minimum of that and the self clearance (gik_anchored_self_clearance;
 * GIK_CLEARANCE_LINKS_SELF, for a template with self pairs attached).  The rule is the same for all; only the array it
 * reads differs:
 *
 * failed(goal)  :=  stats.stop != 0  ||  !(pos_err <= pos_tol)  ||  !(rot_err <= rot_tol)  ||  !(clearance >= -clear_tol)
 *                   -- a NaN clearance counts as failed; +infinity (no obstacle, no masked node) never fails a goal.
 * score(goal)   :=  max(pos_err / pos_tol, rot_err / rot_tol, max(0, -clearance) / clear_tol);  +inf if any is NaN
 * better(r, i)  :=  (r succeeds and i failed)  ||  (same success class  &&  score(r) < score(i))
 *                   -- a NaN never wins, a tie keeps the incumbent.
 *
 * And the seeds have a second, local mode, for a goal that was itself seeded (a tracked waypoint): a seed drawn
 * uniformly inside the limits usually lands on another IK branch, a joint jump; a seed drawn around the configuration
 * the attempt started from stays near it.
 *
 * gik_anchored_retry_select: gik_retry_select with d_clearance [B] added and the rule above.
 * gik_anchored_retry_seeds: the pose rows as gik_retry_seeds copies them (`base` gives their width and n), and
 *   with spread == 0 (d_q_center is not read, may be NULL) the same angles, bit for bit:  q = lo + u (hi - lo).
 *   With spread > 0, for goal g = d_idx[r] and the centre row c = d_q_center[g] (indexed by GOAL, [B][n]):
 *       t = 2u - 1  (exact in fp64);   q = min(max(c + spread * t, lo), hi)      (one rounded product, one rounded sum)
 *   with the same u(seed, g, attempt, j) as there.  A NaN centre gives a NaN seed.
 *   graphik_amd.solvers.riemannian_solver.retry_seeds_host(..., center=, spread=) returns the same bits.
 * gik_anchored_retry_merge: for compact slot r (one wavefront each), goal g = d_idx[r] (entries distinct): if the
 *   restart's answer is better, the full point row (full_N * 3 doubles), the gik_stats record, the q row, pos_err,
 *   rot_err and clearance of goal g are replaced together and d_attempt[g] = attempt; otherwise nothing of goal g
 *   is written.
 * gik_anchored_ik_batch_retry: attempt 0 is exactly gik_anchored_ik_batch followed by gik_anchored_clearance
 *   (d_q_init NULL) or gik_anchored_ik_batch_seeded with the clearance output, on the caller's buffers, preceded by a
 *   memset of d_attempt [B] to 0; with retries = 0 the call queues exactly that and nothing else.  Then for
 *   a = 1 .. retries: select -> the 4-byte count is copied to the host -> stop if it is 0 -> seeds ->
 *   gik_anchored_ik_batch_seeded with B' = count on compact buffers in d_ws, clearance included -> merge.
 *   THIS CALL SYNCHRONISES ITS STREAM (hipStreamSynchronize) ONCE PER ATTEMPT after the first, as gik_ik_batch_retry
 *   does and for its reason.  Synchronise the stream before reading the results.
 *   Local mode (spread > 0): the centre is d_q_init.  d_q_init may alias d_q (path tracking), which attempt 0
 *   overwrites, so the B n seed angles are copied into the workspace before attempt 0 and the seeds are centred on
 *   the copy.
 *   What comes back: the outputs of gik_anchored_ik_batch_seeded plus d_attempt[g] = the attempt whose answer goal g
 *   holds.  The anchored solve runs on the wavefront kernel, whose bits do not depend on the batch, so a goal with
 *   d_attempt[g] = a > 0 holds exactly what gik_anchored_ik_batch_seeded returns for that goal alone from the seed of
 *   (seed, g, a).  With clearance_mode = GIK_CLEARANCE_LINKS every clearance of the call -- attempt 0's in d_clearance,
 *   each restart's on its compact batch, what the merge moves -- is gik_anchored_link_clearance of the same point
 *   matrices instead; select, score and merge are unchanged.  With GIK_CLEARANCE_LINKS_SELF it is the NaN-propagating
 *   minimum of that and gik_anchored_self_clearance of the same point matrices: the link launch, then the self kernel
 *   merging into its output on the same stream.  gik_anchored_last_solve_ms reports the solve kernel of the LAST attempt that ran.
 *   d_ws: caller-owned, gik_anchored_retry_ws_bytes(anch, base, B) bytes, 8-byte aligned: the scratch of one anchored
 *   call (attempt 0 and the restarts use it in turn) plus compact buffers sized for the case that every goal fails.
 *   It is needed with retries = 0 as well.
 *   Refused, with a message, before anything is queued: what gik_anchored_ik_batch_seeded refuses (an `anch` that is
 *   not a fixed-anchor template, a `base` without pipeline or with N != full_N, a capturing stream; a `base` that
 *   cannot be seeded, if d_q_init is given or retries > 0); retries outside 0 .. 63; a null d_clearance, d_attempt or
 *   workspace; and with retries > 0 null limits, a pos_tol, rot_tol or clear_tol that is not positive, a spread
 *   that is negative or NaN, spread > 0 with a null d_q_init (a cold batch has no centre); a clearance_mode that is
 *   neither 0 nor 1 (nor, on a template with self pairs attached, 2), and 1 on a template without links.
 *   B == 0 returns 0.                                                                                          */
#define GIK_CLEARANCE_NODES 0
#define GIK_CLEARANCE_LINKS 1
#define GIK_CLEARANCE_LINKS_SELF 2      /* min(link clearance, self clearance); a value only with self pairs attached */
typedef struct {
  int32_t retries;        /* further attempts for goals that failed: 0 .. 63                              */
  int32_t clearance_mode; /* GIK_CLEARANCE_NODES (0), _LINKS (1) or _LINKS_SELF (2): which clearance the rule reads */
  uint64_t seed;          /* of the generator; the same seed gives the same answers                       */
  double pos_tol;         /* a goal succeeds with stop == 0, pos_err <= pos_tol, rot_err <= rot_tol ...   */
  double rot_tol;
  const double *d_q_lo;   /* [n] device: the seeds stay inside [q_lo[j], q_hi[j]]                         */
  const double *d_q_hi;   /* [n] device                                                                   */
  double clear_tol;       /* ... and clearance >= -clear_tol (metres); must be positive                   */
  double spread;          /* >= 0, radians.  0: seeds uniform inside the limits; > 0: within spread of d_q_init */
} gik_anchored_retry_opts;

int gik_anchored_retry_select(const gik_stats *d_stats, const double *d_pos_err, const double *d_rot_err,
                              const double *d_clearance, int B, double pos_tol, double rot_tol, double clear_tol,
                              int32_t *d_idx, int32_t *d_count, void *stream);
int gik_anchored_retry_seeds(const gik_template *base, const double *d_T_goal, const int32_t *d_idx, int count,
                             uint64_t seed, int attempt, const double *d_q_lo, const double *d_q_hi,
                             const double *d_q_center /* [B][n]; may be NULL if spread == 0 */, double spread,
                             double *d_T_out, double *d_q_out, void *stream);
int gik_anchored_retry_merge(const gik_template *anch, const gik_template *base, const int32_t *d_idx, int count,
                             int attempt, double pos_tol, double rot_tol, double clear_tol, const double *d_Y_r,
                             const gik_stats *d_stats_r, const double *d_q_r, const double *d_pos_err_r,
                             const double *d_rot_err_r, const double *d_clearance_r, double *d_Y_full,
                             gik_stats *d_stats, double *d_q, double *d_pos_err, double *d_rot_err,
                             double *d_clearance, int32_t *d_attempt, void *stream);
size_t gik_anchored_retry_ws_bytes(const gik_template *anch, const gik_template *base, int B);
int gik_anchored_ik_batch_retry(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                                const double *d_q_init /* may be NULL */, int B, const gik_anchored_retry_opts *opts,
                                void *d_ws, double *d_Y_full, gik_stats *d_stats, double *d_q, double *d_pos_err,
                                double *d_rot_err, double *d_clearance, int32_t *d_attempt, void *stream);

/* ---- per-goal obstacle scenes in the fixed-anchor solve (opt-in) --------------------------------
 * An anchored template holds ONE set of spheres, the same for every goal.  A scene call takes the spheres as an ARGUMENT
 * instead, caller-owned device memory like the goals: n_scene sets of at most 128 spheres and, per goal, which set it
 * is solved in.  The handle stays immutable (any number of scene calls with any scene sets may be in flight on any
 * number of streams), and the batch stays one persistent launch however many scenes it mixes: a wave restages its
 * 4 KB obstacle table when the problem it claims names another scene than the one it holds.
 *   - The template's own spheres are ignored by a scene call.  Its obs_node_mask, its links, their radii and hinges
 *     apply to every scene.  gik_cost .. gik_hess keep the template's own spheres.
 *   - The order of the spheres in a walk is the order of the scene's rows, and rows from d_n_obs[s] up to the stride are
 *     never read.  The solve kernels' near lists are exact, so a goal solved under scene s holds, BIT FOR BIT, what the
 *     plain call returns for it on a template created with the d_n_obs[s] rows of scene s -- whatever the other goals of
 *     the batch use.
 *   - d_n_obs and d_scene_id live on the device: that their entries are within 0 .. stride and 0 .. n_scene - 1 is the
 *     CALLER'S PRECONDITION, as the distinct entries of d_idx are for a merge.  The kernels clamp what they read (an id into
 *     [0, n_scene), a count into [0, min(stride, 128)]), so a bad entry gives a wrong answer, never an access outside
 *     the set.  The arrays are read while the call's kernels run: keep them unchanged until the stream has passed them.
 *
 * gik_solve_batch_scenes: gik_solve_batch on an anchored template, with the scene builds of its solve kernel.
 * gik_anchored_ik_batch_scenes: gik_anchored_ik_batch (d_q_init NULL: the cold start) or gik_anchored_ik_batch_seeded with
 *   the scene solve and, where d_clearance is given, the scene clearance of the answer: that of the masked nodes
 *   (clearance_mode = GIK_CLEARANCE_NODES), of whole links (GIK_CLEARANCE_LINKS; links attached), or the minimum of
 *   that and the self clearance, which no scene changes (GIK_CLEARANCE_LINKS_SELF; self pairs attached).
 * gik_anchored_clearance_scenes / gik_anchored_link_clearance_scenes: the two clearances with goal b measured against
 *   scene d_scene_id[b].  A scene without spheres: +infinity.
 * gik_anchored_ik_batch_retry_scenes: gik_anchored_ik_batch_retry with the scene carried through attempt 0, every
 *   compact batch (its ids are d_scene_id[d_idx[r]], gathered into the workspace) and every clearance; the rule, the
 *   seeds and the merge are the same.  d_ws: gik_anchored_retry_ws_bytes(anch, base, B) bytes PLUS 4 B bytes (rounded
 *   up to a multiple of 8) for the gathered ids, 8-byte aligned.
 * Each refuses, with a message and before anything is queued: what its plain sibling refuses (a capturing stream
 * included), a handle that is not a fixed-anchor template, a null scene set, n_scene < 1, a stride outside 0 .. 128,
 * a null d_n_obs, a null d_obs with stride > 0, a null d_scene_id with n_scene != 1.  B == 0 returns 0.           */
typedef struct {
  int32_t n_scene;            /* >= 1 */
  int32_t stride;             /* rows per scene in d_obs, 0 .. 128 */
  const double  *d_obs;       /* [n_scene][stride][4] centre x, y, z and SQUARED radius (as gik_anchored_desc.obs) */
  const int32_t *d_n_obs;     /* [n_scene] spheres of each scene, 0 .. stride */
  const int32_t *d_scene_id;  /* [B] scene of each goal; NULL: every goal uses scene 0 (n_scene must be 1) */
} gik_scene_set;

int gik_solve_batch_scenes(const gik_template *t, const double *d_Y_init, const double *d_targets, int B,
                           double *d_Y_out, gik_stats *d_stats, const gik_trace *trace /* may be NULL */,
                           const gik_scene_set *scenes, void *stream);
int gik_anchored_ik_batch_scenes(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                                 const double *d_q_init /* may be NULL: cold */, int B, const gik_scene_set *scenes,
                                 double *d_ws, double *d_Y_full, gik_stats *d_stats, double *d_q, double *d_pos_err,
                                 double *d_rot_err, double *d_clearance /* may be NULL */, int clearance_mode,
                                 void *stream);
int gik_anchored_clearance_scenes(const gik_template *anch, const double *d_Y_full, int B,
                                  const gik_scene_set *scenes, double *d_clearance, void *stream);
int gik_anchored_link_clearance_scenes(const gik_template *anch, const double *d_Y_full, int B,
                                       const gik_scene_set *scenes, double *d_clearance, void *stream);
int gik_anchored_ik_batch_retry_scenes(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                                       const double *d_q_init /* may be NULL */, int B,
                                       const gik_anchored_retry_opts *opts, const gik_scene_set *scenes, void *d_ws,
                                       double *d_Y_full, gik_stats *d_stats, double *d_q, double *d_pos_err,
                                       double *d_rot_err, double *d_clearance, int32_t *d_attempt, void *stream);

/* ---- screened restart seeds in the fixed-anchor solve (opt-in) -----------------------------------
 * A restart's seed is drawn blind: with a floor under the robot, most uniform draws already lie below it, and the rule
 * above would call the seed itself failed.  The screened step draws `candidates` (C, 1 .. 16) seeds per failed goal,
 * realizes each on the robot graph, measures each with the clearance the call's rule reads, and starts the restart from
 * the first clear one.  All of it on the device, on the call's stream, with no host synchronisation of its own.
 *
 * candidate c of (seed, g, attempt)  :=  the seed of gik_anchored_retry_seeds under seed_c = seed + c * 0xD1342543DE82EF95
 *                                        (mod 2^64): same generator, limits, centre and spread.  Candidate 0 is that
 *                                        entry's row, bit for bit; retry_seeds_host(seed_c, ...) is the numpy mirror.
 * clearance_c  :=  the clearance, in clearance_mode, of the robot graph's realization of the candidate -- every row where
 *                  the configuration puts it, the end effector included (not where the goal puts it) --, half-spaces
 *                  folded in where the handle has them, against the GOAL's scene where a scene set is given.
 * pick         :=  the first c with clearance_c >= -clear_tol (+infinity qualifies: nothing to measure picks 0); none:
 *                  the c of the largest clearance, the lowest on a tie, a NaN never winning; all NaN: 0.
 *
 * gik_anchored_retry_seeds_screened: gik_anchored_retry_seeds with the pick's angles in d_q_out [count][n]; d_T_out as
 *   there.  scenes may be NULL (the template's own obstacles); its d_scene_id is indexed by GOAL, [B], like d_q_center.
 *   Optional outputs: d_pick [count] int32, the picked c per slot, and d_pick_clearance [count], its clearance.
 *   d_ws: gik_anchored_retry_seeds_screened_ws_bytes(anch, base, count, candidates) bytes, 8-byte aligned (0: bad arguments).
 *   With candidates = 1 it writes the bits of gik_anchored_retry_seeds.
 * gik_anchored_ik_batch_retry_screened: gik_anchored_ik_batch_retry (scenes NULL) or gik_anchored_ik_batch_retry_scenes
 *   with every restart's seed step replaced by the screened one, in opts->clearance_mode and with opts->clear_tol;
 *   attempt 0, select and merge are theirs.  A goal with d_attempt[g] = a > 0 holds what gik_anchored_ik_batch_seeded
 *   returns for it alone from the pick of (seed, g, a).  d_ws: gik_anchored_ik_batch_retry_screened_ws_bytes(anch, base, B,
 *   candidates) bytes, 8-byte aligned: the workspace of the scenes entry with the screened step's behind it.
 * Refused, with a message, before anything is queued: what the siblings refuse (gik_anchored_retry_seeds; the restart
 *   entries; a scene set as the scene calls refuse it; a clearance_mode as they refuse it; a capturing stream),
 *   candidates outside 1 .. 16, a clear_tol that is not positive, a null or misaligned workspace.  count / B == 0 returns 0. */
#define GIK_RETRY_MAX_CANDIDATES 16      /* candidates per slot of the screened entries: 1 .. 16 */
size_t gik_anchored_retry_seeds_screened_ws_bytes(const gik_template *anch, const gik_template *base, int count, int candidates);
int gik_anchored_retry_seeds_screened(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                                      const int32_t *d_idx, int count, uint64_t seed, int attempt, const double *d_q_lo,
                                      const double *d_q_hi, const double *d_q_center /* [B][n]; may be NULL if spread == 0 */,
                                      double spread, int candidates, int clearance_mode, double clear_tol,
                                      const gik_scene_set *scenes /* may be NULL */, void *d_ws, double *d_T_out,
                                      double *d_q_out, int32_t *d_pick /* may be NULL */,
                                      double *d_pick_clearance /* may be NULL */, void *stream);
size_t gik_anchored_ik_batch_retry_screened_ws_bytes(const gik_template *anch, const gik_template *base, int B, int candidates);
int gik_anchored_ik_batch_retry_screened(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                                         const double *d_q_init /* may be NULL */, int B,
                                         const gik_anchored_retry_opts *opts, int candidates,
                                         const gik_scene_set *scenes /* may be NULL */, void *d_ws, double *d_Y_full,
                                         gik_stats *d_stats, double *d_q, double *d_pos_err, double *d_rot_err,
                                         double *d_clearance, int32_t *d_attempt, void *stream);

/* ---- goal-aware seeds from a configuration atlas (opt-in) --------------------------------------------
 * Every other start point -- bound smoothing + MDS, a draw inside the limits, a draw around d_q_init -- ignores the goal.
 * An atlas is a table of M joint configurations that are clear of the room, each with its KEY: the positions its end
 * effector's goal nodes take.  A goal starts from the clear configuration whose key lies nearest to its own.
 *
 * key of a configuration q  :=  rows goal_node[g] of the robot graph's realization of q (gik_seed_batch), g over the live
 *                               goal nodes: p_e and q_e for a pose goal (W = 6), p_e alone for a position goal (W = 3).
 * key of a goal pose T      :=  the same nodes as the goal puts them: p_e = T[:3, 3], q_e = p_e + axis_length * T[:3, 2],
 *                               one rounded product and one rounded sum per component.
 * d(goal, row m)            :=  (...((t0 t0 + t1 t1) + t2 t2) ... + t_{W-1} t_{W-1}), t_c = goal key[c] - d_atlas_keys[c][m]:
 *                               every difference, product and sum rounded on its own, in this order.
 * d_atlas_keys [W][M] is component-major; d_atlas_q [M][n] holds the rows' joint angles.  The library keeps neither.
 *
 * gik_atlas_nearest: for compact slot r -- goal d_idx[r], or r where d_idx is NULL -- the K (1 .. 64) rows with the
 *   smallest (d, m) in lexicographic order, ascending, into d_nbr [count][K] int32 and, where given, their d into d_dist
 *   [count][K].  A NaN or infinite d is never listed; where fewer than K rows are listed the rest is -1 / +infinity.
 *   `base` is the robot graph's template with its pipeline attached: 3-D, one end effector, pose goals or (W = 3) a
 *   position goal.  atlas_nearest_host is the numpy mirror, equal in the index and in the bits of d.
 * gik_anchored_atlas_seeds: the screened seed step (gik_anchored_retry_seeds_screened) with the atlas as its candidate
 *   source: candidate c (0 .. candidates - 1) of slot r, goal g, is row d_nbr[g * nbr_stride + first + c] of d_atlas_q --
 *   d_nbr is indexed by GOAL, [B][nbr_stride], what gik_atlas_nearest writes with a NULL d_idx.  A row of -1 is a NaN
 *   candidate: it is measured as NaN and never picked unless every candidate is one, and then that goal alone gets NaN
 *   angles.  Realization, clearance (clearance_mode, half-spaces, the goal's scene), the pick and every output are the
 *   screened step's.  With candidates = 1 and first = 0 it writes the nearest row's angles.
 *   d_ws: gik_anchored_atlas_seeds_ws_bytes(anch, base, count, candidates) bytes, 8-byte aligned.
 * gik_anchored_ik_batch_atlas: gik_anchored_ik_batch_retry_screened with the atlas in place of the random draws.  One
 *   gik_atlas_nearest launch over all B goals with K = (opts->retries + 1) * candidates.  Attempt 0 starts from the pick
 *   among ranks [0, candidates) where d_q_init is NULL (the seeded path, with or without scenes), from d_q_init
 *   otherwise; restart a >= 1 of a failed goal starts from the pick among ranks [a * candidates, (a + 1) * candidates).
 *   Select, merge and the one count copy per attempt are the restart loop's.  A goal with d_attempt[g] = a holds what
 *   gik_anchored_ik_batch_seeded returns for it alone from that pick.  opts->seed, d_q_lo and d_q_hi are not read.
 *   d_ws: gik_anchored_ik_batch_atlas_ws_bytes(anch, base, B, candidates, opts->retries) bytes, 8-byte aligned: the
 *   workspace of the scenes entry with the neighbour table, the attempt-0 seeds, the noted rows and the screened
 *   step's arrays behind it.
 * gik_anchored_atlas_picks: after gik_anchored_ik_batch_atlas on the same stream, workspace, B, candidates and retries:
 *   d_atlas_pick [B] int32, the atlas row the answer each goal holds started from; -1 where it started from d_q_init.
 * Refused, with a message, before anything is queued: what the siblings refuse (the handle pair, a base that cannot be
 *   seeded, a scene set, a clearance_mode, tolerances that are not positive, a capturing stream); a base template that
 *   is planar, has more than one end effector or an inert goal slot other than a position goal's; K outside 1 .. 64;
 *   for gik_anchored_ik_batch_atlas K > atlas_count and opts->spread != 0; count * K beyond INT_MAX; an atlas_count
 *   below 1 or above 2^30; null atlas arrays; first < 0 or first + candidates > nbr_stride; a null or misaligned
 *   workspace.  count / B == 0 returns 0. */
#define GIK_ATLAS_MAX_NEIGHBOURS 64      /* K of gik_atlas_nearest: 1 .. 64 */
int gik_atlas_nearest(const gik_template *base, const double *d_atlas_keys, int atlas_count, const double *d_T_goal,
                      const int32_t *d_idx /* may be NULL */, int count, int K, int32_t *d_nbr,
                      double *d_dist /* may be NULL */, void *stream);
size_t gik_anchored_atlas_seeds_ws_bytes(const gik_template *anch, const gik_template *base, int count, int candidates);
int gik_anchored_atlas_seeds(const gik_template *anch, const gik_template *base, const double *d_atlas_q, int atlas_count,
                             const double *d_T_goal, const int32_t *d_idx /* may be NULL */, int count,
                             const int32_t *d_nbr, int nbr_stride, int first, int candidates, int clearance_mode,
                             double clear_tol, const gik_scene_set *scenes /* may be NULL */, void *d_ws, double *d_T_out,
                             double *d_q_out, int32_t *d_pick /* may be NULL */,
                             double *d_pick_clearance /* may be NULL */, void *stream);
size_t gik_anchored_ik_batch_atlas_ws_bytes(const gik_template *anch, const gik_template *base, int B, int candidates,
                                            int retries);
int gik_anchored_ik_batch_atlas(const gik_template *anch, const gik_template *base, const double *d_T_goal,
                                const double *d_q_init /* may be NULL */, int B, const gik_anchored_retry_opts *opts,
                                int candidates, const double *d_atlas_keys, const double *d_atlas_q, int atlas_count,
                                const gik_scene_set *scenes /* may be NULL */, void *d_ws, double *d_Y_full,
                                gik_stats *d_stats, double *d_q, double *d_pos_err, double *d_rot_err,
                                double *d_clearance, int32_t *d_attempt, void *stream);
int gik_anchored_atlas_picks(const gik_template *anch, const gik_template *base, int B, int candidates, int retries,
                             const void *d_ws, const int32_t *d_attempt, int32_t *d_atlas_pick, void *stream);

/* Duration (ms, HIP events on the call's stream) of the anchored solve kernel inside the most
 * recent gik_anchored_ik_batch / gik_anchored_ik_batch_seeded on this handle; waits for it.  < 0 if there was none. */
double gik_anchored_last_solve_ms(const gik_template *anch);

#ifdef __cplusplus
}
#endif
#endif
