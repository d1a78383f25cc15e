// graphik_amd/csrc/gik_args.h -- the boundary between host and device: the argument structs the kernels are launched
// with, the plain structs those name by value, and the constants that size them or that the launch plan (gik_plan.h)
// needs.  Each is written here once; the kernel headers, the handle and the plan use them from here.
// Plain structs and constants only: plain C++17, no HIP, so that gik_plan.h and the programs under tests/host/ that
// include it compile without a device toolchain.  Layouts, member order and default member initialisers are kernel ABI.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/graphik_amd.h"      // (gik_stats, gik_trace; after <stddef.h>: it uses size_t)
#include "gik_scenes.h"

namespace gik {

constexpr int WAVE = 64;

// fixed-anchor formulation (WaveCtx<.., ANCH>, gik_wave.hip.h)
constexpr int ANCH_PMAX = 8;      // "pinned" point-to-anchor terms per free node
constexpr int ANCH_MAXA = 16;   // rows of the pinned-anchor table
constexpr int ANCH_MAXOBS = 128; // obstacles (staged in LDS: 32 B each)
static_assert(SCENE_MAX_SPHERES == ANCH_MAXOBS, "gik_scenes.h restates this constant");
constexpr int ANCH_LMAX = 2;      // link hinges (WaveCtx<.., LINKS>): links per free node
constexpr int ANCH_LROWS = 22;  // rows of the per-node link tables: 3 N <= 64 gives 21 free nodes, + one inert row for idle lanes
constexpr int ANCH_SELF_HMAX = 16;   // self hinges (WaveCtx<.., SELF>): link pairs per template, a pair per lane of a 16-lane row
constexpr int ANCH_HALF_MAX = 8;      // half-space obstacles (WaveCtx<.., HALF>): planes per template, 32 B each in LDS
constexpr int ANCH_HALF_ROWS = 34;    // rows of the per-node margin table: the 33 tile rows (idle lanes read the dump row's), even

constexpr int MIG_SIMDS = 1 << 14;      // SIMD slots of the spread table (MigCtl::simd_run, gik_rtr.hip.h)

constexpr int QUAD_SLOTS = 4;    // problems per wavefront
constexpr int QUAD_NODES = 16;   // nodes per problem

// the workgroup-per-goal prepare kernels (prep_block_kernel, gik_prep.hip.h)
constexpr int PREP_NT = 512;      // threads of a workgroup
constexpr int PREP_MAXN = 128;    // nodes of the small LDS arrays ...
constexpr int PREP_BIGN = 256;    // ... and of the build for 129 .. 255 nodes
constexpr int PREP_MAX_EE = 8;      // (4 until round 6)

// four goals per wavefront (prep_quad_kernel, gik_prep_quad.hip.h)
constexpr int PREPQ_MAXN = QUAD_NODES;
// The small per-goal arrays -- ev, sg, hv, hw (16 doubles each), the rotations (c, s) (16 double2) and the ranks (16
// ints) -- form ONE block of 104 doubles per goal slot.  104 = 8 mod 32: what the four goals of a half-wave read at
// the same index (broadcast reads, most of the traffic to these arrays; for the rotations a ds_read_b128) falls into
// four different bank groups.  Until round 5 every array had a slot stride of 16 or 32 doubles: the four goals' (c, s)
// sat on the SAME banks (every read of a rotation 4-way conflicted), the others two by two.
constexpr int PREPQ_VEC_STRIDE = 104;

constexpr int CLAIM_KEY_MAX_TERMS = 8;      // terms of a template's claim key (ClaimKey, gik_order.hip.h)

// ---- solver parameters handed to the kernels ----------------------------------------------
struct Params {
  double mingradnorm, theta, kappa, rho_prime, rho_regularization;
  int maxiter, maxinner, mininner, planar_proj_exact;
};

struct CgParams {
  double mingradnorm, minstepsize, orth_value;
  int maxiter, beta_type, planar_proj_exact;
};

// a link hinge of a free node (WaveCtx<.., LINKS>; link_meta_pack, gik_wave.hip.h)
struct AnchLinkRec {
  double rho;      // capsule radius of the link
  uint32_t meta;   // [0] valid, [1] this node is end b, [2] the other end is a row of sh_anch (constant), [15:8] the other
                   // end's row (tile row of a free node / row of sh_anch), [23:16] the slot whose neighbour it is (0xff: none)
  uint32_t pad;
};

// a self hinge (WaveCtx<.., SELF>): the four ends a1, b1, a2, b2 of a link pair, each a free row (6 * row, tile 0) or an
// anchor row (the anchor table's offset + 4 * row) as a double offset from the tiles -- the encoding of link_other -- and
// R = rho_l + rho_m.  An unused entry is all zero: R = 0 is never active.
struct AnchSelfDesc {
  uint16_t off[4];
  double R;
};
static_assert(sizeof(AnchSelfDesc) == 16, "kernel ABI");

// launch-invariant tables of the workgroup-per-problem path (device pointers; gik_template_create)
struct BlockTabs {
  const int *nc_term;      // [Tc] index in the caller's target row of each slot-table term; null = identity
  const int *clq_term;     // [M][512] target index of clique pair (row tid >> 2, row 4m + (tid & 3)); -1 = none
  const int *clq_pair_term;        // [n_pairs] target index of clique pair p (each pair once)
  const unsigned short *clq_pid_t; // [M][512] pair id of (row tid >> 2, row 4m + (tid & 3)), like clq_term; 0xffff = none
  int n_pairs;
  const int *node_of_row;  // [128] node (the caller's numbering) of each LDS row; null = identity
  const int *wave_sl;      // [8][2] slot-loop bounds {SLE, SL} of each wavefront
  int Tc;                  // terms kept in the slot tables
  int n_clq;               // clique size (rows 0..n_clq-1), 0 = none
  int clq_euclid;          // 1: look for point coordinates behind the clique's target distances
};

// launch-invariant tables (device pointers; gik_template_create)
struct NptTabs {
  const int *node_of_row;          // [128] the caller's node held by thread slot NS * thread + s, -1 = none
  const unsigned char *prow_of_slot;   // [128] its row in the point table sh_P (clique nodes: cbase + rank)
  const int *clq_pair_term;        // [n_pairs] target index of clique pair (a < b: clique ranks), p = a n - a (a + 1) / 2 + b - a - 1
  const uint32_t *term_rec;        // [TL][64] row_i | row_j << 8 | kind << 16 | wslot_i << 18 | wslot_j << 25; kind 0 = padding
  const int *term_tgt;             // [TL][64] target index of the lane's term, -1 = padding
  const unsigned short *gather;    // [DEG0 + DEG1][threads] row of the +-t table the thread adds: 2 slot (+t) or 2 slot + 1 (-t);
                                   // padding = the zero row 2 * n_terms
  const unsigned char *wslot_of_row;   // [128] (per thread slot) row of the compact direction table that publishes the node, 255 = none
  int n_clq, n_pairs, DEG0, DEG1, n_wrows, TL;
  int clq_euclid;                  // 1: look for point coordinates behind the clique's target distances
  int cbase;                       // first row of the clique (its nodes take rows cbase .. cbase + n_clq - 1, rank = row - cbase)
  int n_rows;                      // rows in use (even)
  int n_terms;                     // slot terms (the first n_terms of the TL * 64 term slots, all evaluated by wavefront 0)
  int term_sync;                   // two waves per problem: 1 = end nodes of slot terms sit in both wavefronts
  int n_helped;                    // one node per lane: lanes 2 i (i < n_helped) hold the busiest nodes, lane 2 i + 1 gathers the
                                   // second half of lane 2 i's list (the gather is as long as the longest list of any lane)
};

// ---- solve and known-answer kernels --------------------------------------------------------
// the state of a paused problem (time slicing, tail spreading: gik_sched.hip.h)
struct SliceState {
  double Delta;
  int kiter, inner_total, inner_exec, n_accept;
  int resumes, pad;    // times the problem changed hands (reported in gik_stats.flags >> 8)
};

struct AnchArgs {
  const double *anch_const;     // [ANCH_MAXA][4] pinned anchor table (goal rows are overwritten per problem)
  const double *anchor_goal;    // [B][n_goal * 3] per-problem anchor positions
  const uint32_t *pin_meta;     // [ANCH_PMAX][64] anchor row | kind << 8
  const double *pin_tgt;        // [ANCH_PMAX][64]
  const double *obs;            // [n_obs][4] x, y, z, r^2
  unsigned long long obs_mask;  // bit i: free node i carries the obstacle hinges
  int n_obs, n_goal, goal_row0; // goal anchors occupy rows goal_row0 .. goal_row0 + n_goal - 1
  const AnchLinkRec *link_rec = nullptr;   // [ANCH_LMAX][ANCH_LROWS] link hinges per free node (LINKS kernels only)
  const AnchSelfDesc *self_desc = nullptr; // [ANCH_SELF_HMAX] self hinges (SELF kernels only)
};

struct SolveArgs {
  const uint32_t *slot_meta;  // [MAXDEG][64]
  const double *targets;      // [B][T]
  const double *Y_init;       // [B][N*K]
  double *Y_out;              // [B][N*K]
  gik_stats *stats;           // [B]
  unsigned int *work_counter; // zeroed before launch; problems are claimed with atomicAdd
  const int *claim_order = nullptr;   // [B] ticket -> problem (a permutation, gik_k_order.hip), null = index order; fresh claims of
                              // rtr_wave_kernel only: likely-long problems get the early tickets (NOTEBOOK 21)
  gik_trace trace;
  int has_trace;
  int N, T, B;
  int dbg;  // debug flags (env GIK_DBG): 1 = one block per problem, 2 = skip the TR loop,
            // 4 = dump (r_r, d_Hd, alpha, model) of every inner iteration of problem 0 to dbg_buf,
            // 8 = cycle counters of problem 0: dbg_buf = {cycles in tCG loops, tCG iterations, all cycles},
            // 16 = rerun tCG after every rejected step instead of resuming from the checkpoint;
            // at template creation: 32 = print the kernel choice, 64 / 128 = clique closed form of the
            // workgroup path from 4 nodes up / off
  double *dbg_buf;
  Params p;
  CgParams cg;   // solver == GIK_SOLVER_CONJUGATE_GRADIENT (rcg_* kernels)
  // fixed-anchor formulation (anchored templates; see WaveCtx<.., ANCH>)
  AnchArgs an;
  // Time slicing (slice_its > 0): a problem that has not met a stopping rule after slice_its outer
  // iterations is written back (x in Y_out, SliceState) and re-queued behind everything that is
  // waiting, so that all problems advance at about the same rate and the long ones -- unknown in
  // advance -- are not the last to START.  Tickets < B are the fresh problems themselves;
  // ticket B + t is the t-th re-queued problem, published in q_ids[t] / q_seq[t] (no slot is ever
  // reused: the ring has room for every possible re-queue of the launch).
  int slice_its;
  int slice_cycles;   // wavefront kernel: shortest round-robin slice (MigCtl::slice_cycles)
  // tail spreading (wavefront kernel, MIG variant): q_head = hand-over tickets taken by helpers,
  // mig_credits / mig_simd_run as in MigCtl; q_tail / q_seq / q_ids / q_state / q_done as for slicing
  unsigned int *q_head;
  int *mig_credits, *mig_simd_run;
  // round-robin slicing of the wavefront kernel: yield queue (y_seq[k] == k + 1 once entry k is published)
  // Entries are taken by fetch-add tickets on y_head, never by compare-and-swap (2048 waves that
  // retry a CAS on one word serve ~50 k claims per second -- measured, the whole batch then waits for
  // its queue).  That needs a guarantee that a ticket's entry exists: a wave that yields pushes
  // first, so it owns one entry's worth of claim (it either pops at once, or, if it got a fresh
  // problem instead, passes the claim on by y_avail += 1); a wave that comes from a finished
  // problem has to win one from y_avail (fetch-add -1, undone if it went negative).
  unsigned int *y_head, *y_tail, *y_seq;
  int *y_ids, *y_avail;
  unsigned int y_cap;
  unsigned int *q_tail, *q_done;   // next to work_counter (= the ticket counter)
  int *q_ids;                      // [cap]
  unsigned int *q_seq;             // [cap], 0xffffffff = not published
  SliceState *q_state;             // [B]
  BlockTabs bt;                    // workgroup-per-problem path
  NptTabs nt;                      // node-per-lane path (rtr_npt_kernel)
  double *npt_ctg_ws = nullptr;    // graphs beyond 128 nodes: [grid][ctg_doubles] clique target triangles (global memory)
  // half-space obstacles (HALF kernels only; gik_anchored_attach_halfspaces).  At the end: every other kernel's offsets stay
  const double *half = nullptr;    // [n_half][4] unit normal nx, ny, nz and offset d0: the allowed side is n.p - d0 >= 0
  const double *half_mu = nullptr; // [N] margin of each free node, metres (read where obs_mask has the node's bit)
  int n_half = 0;
};

struct KatArgs {
  const uint32_t *slot_meta;
  const double *targets;  // [B][T] (unused for proj)
  const double *Y;        // [B][N*K]
  const double *W;        // [B][N*K] (hess, proj)
  double *out;            // cost: [B]; others: [B][N*K]
  double *out_f;          // mode 4: cost [B] next to the gradient in `out`
  int N, T, B, mode;      // 0 cost, 1 grad, 2 hess, 3 proj, 4 cost and grad (one pass)
  int planar_proj_exact;
  AnchArgs an;
  BlockTabs bt;
  NptTabs nt;
  double *npt_ctg_ws = nullptr;   // see SolveArgs
  const double *half = nullptr;   // half-space obstacles, as in SolveArgs
  const double *half_mu = nullptr;
  int n_half = 0;
};

// ---- prepare, recover, seed, anchored glue ---------------------------------------------------
struct PipeConst {
  // graph template (device pointers)
  const double *base_lower;   // [N*N]  NaN = no edge; goal edges are added per problem
  const double *base_upper;   // [N*N]
  const int *anchor_idx;      // [A]   nodes with a fixed position (base frame, obstacles)
  const double *anchor_pos;   // [A][K]
  const int *pair_i, *pair_j; // [P]   omega pairs (i<j), goal edges included
  const int *term_src;        // [T]   -1: static target, else anchor_slot*2 + goal_slot
  const double *term_static;  // [T]
  // robot
  const double *T0;           // [n+1][(K+1)^2] frames at zero configuration (row-major)
  const int *p_idx, *q_idx;   // [n+1] node index of p_i / q_i
  int N, K, T, n_anchor, n_pairs, n_joints;
  int goal0, goal1;           // ee node, and q_n (k=3) or p_{n-1} (k=2)   (first end effector)
  int x_idx, y_idx;
  double goal_len;            // axis_length (k=3) / |p_{n-1} p_n| (k=2)
  double axis_length;
  int last_along_z;           // joint_variables: last link offset parallel to z (:314), bit e = end effector e
  // several end effectors (k = 3 trees; round 6: planar trees): goal poses are [B][n_ee][(K+1)^2]; goal node 2e / 2e+1 is
  // (p, q) of end effector e (k = 2: the end effector and its parent).  Distances: gd[ai * 2 n_ee + g] anchor ai <-> goal node g, then the
  // n_gg goal-node pairs of DIFFERENT end effectors.  A chain has n_ee = 1, n_gg = 0 (the layout
  // and arithmetic of the single-end-effector kernels, bit for bit).
  int n_ee, n_gg;
  int goal_node[2 * 8];       // graph node of goal node g; -1: inert slot (k = 2 trees: a parent that an earlier
                              // end effector's pose already pins -- graph_planar.py:136-145 through BatchProblem; the
                              // odd slot of a position goal)
  int pos_goal_mask;          // bit e: end effector e is a POSITION goal (graph.from_pos({p_e: xyz})): only p_e is pinned,
                              // no T_final correction, no rotation error.  (In the padding in front of ee_len: no other
                              // member moved when it was added.)
  double ee_len[8];           // goal_len per end effector: axis_length (k = 3), |parent(e) e| (k = 2)
  const int *gg_a, *gg_b;     // [n_gg] goal-node slots of each pair
  const int *ee_path;         // [n_ee][n+1] joints from the root to end effector e, -1 padded
  // k = 3, a position goal whose last link lies along z (gik_pipeline_set_point_axis): the x, y of qs_0 that the point
  // formula of its last joint uses instead of forming them from T0.  There they are round-off residues of the frame
  // product, and their direction alone decides the angle (graph_revolute.py:308 without the T_final correction).
  double pos_qs0[8][2];
  int pos_qs0_mask;           // bit e: pos_qs0[e] is set
};

struct PrepArgs {
  PipeConst pc;
  const double *T_goal;  // [B][(K+1)^2]
  double *targets;       // [B][T]
  double *Y_init;        // [B][N*K]
  int *K_out;            // [B] MDS column count (diagnostic), may be null
  // diagnostics (gik_prepare_batch_debug), each may be null: bound_smoothing's output and the three
  // eigenvalue spectra of generate_initialization (Gram matrix, MDS's rank matrix, scatter matrix)
  double *dbg_lb, *dbg_ub;  // [B][N*N]
  double *dbg_eig;          // [B][3][N]
  int B, sweeps;
  int stop_phase;        // developer build only (GIK_PREP_STOP): leave a goal after phase p (timing)
  int no_compress;       // workgroup kernel: 1 = full N x N Jacobi even for rank-deficient Gram matrices (tests, A/B)
};

struct RecoverArgs {
  PipeConst pc;
  const double *Y;       // [B][N*K]
  const double *T_goal;  // [B][(K+1)^2]
  double *q;             // [B][n]
  double *pos_err;       // [B]
  double *rot_err;       // [B]
  int B;
};

// tables of seed_kernel (gik_recover_seed.hip.h)
struct SeedConst {
  const double *Trel;      // [n+1][(K+1)^2]  T0[parent(j)]^-1 T0[j]  (row j = 0 unused)
  const int *fk_parent;    // [n+1]  parent joint on the ee paths (-1: root)
  const int *fk_order;     // [n_fk] joints in an order that puts every parent before its children (root first)
  const int *node_frame;   // [N]  frame a node is read from, -1: anchor_pos[node_anchor]
  const double *node_coef; // [N]  row = trans + coef * axis (axis z for K = 3, x for K = 2)
  const int *node_anchor;  // [N]  anchor slot of a node without frame
  int n_fk;
};

struct SeedArgs {
  PipeConst pc;
  SeedConst sc;
  const double *T_goal;  // [B][n_ee][(K+1)^2]
  const double *q_init;  // [B][n]
  double *targets;       // [B][T]
  double *Y_init;        // [B][N*K]
  int B;
};

// arguments of anch_init_kernel, anch_gather_kernel (gik_anch_glue.hip.h) and anch_scatter_kernel (gik_anch_seed.hip.h)
struct AnchGlueArgs {
  const double *T_goal;        // [B][16]
  const double *Y_full_in;     // [B][full_N*3]   (init: prepare output)
  double *Y_free;              // [B][Nf*3]       (init: out, gather: in)
  double *anchor_goal;         // [B][n_goal*3]   (init: out, gather: in)
  double *Y_full_out;          // [B][full_N*3]   (gather: out)
  const double *anch_const;    // [ANCH_MAXA][4]
  const int *free_full;        // [Nf]
  const int *anchor_full;      // [n_anchor]
  int B, Nf, full_N, n_anchor, n_goal, goal_row0;
  double axis_length;
};

}  // namespace gik
