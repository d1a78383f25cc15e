// graphik_amd/csrc/gik_quad.hip.h -- four planar IK problems per wavefront (gfx950 / CDNA4)
//
// A planar problem is small: at most 16 nodes with two coordinates each (the 10-link chain of
// BASELINE configs[4]: N = 13).  Run one per wavefront (gik_wave.hip.h) it leaves 38 of the 64 lanes
// idle and -- worse -- every per-problem SCALAR of the trust-region solver (alpha, beta, tau, the
// literal 4 x 4 solve of the k = 2 projector, the acceptance test ...) is one wave-wide instruction
// for one number: measured, round 4, 19 k VALU instructions per problem of which the vectors need a
// fraction.  Here a wavefront holds FOUR problems:
//
//   lane l = 16 r + 4 b + i   ->   problem slot b (0..3), node n = 4 r + i (0..15)
//
// i.e. a problem is one 4-lane block column of the wave's four rows.  That is the set of lanes
// v_mfma_f64_4x4x4 sums over (see wave_sum_n in gik_wave.hip.h): two MFMAs leave every lane with the
// total over its problem's 16 lanes, bit-identical in all of them, so
//   * a lane owns a whole NODE (both coordinates of every tangent vector in registers): the Hessian
//     product needs one 16-byte row gather per neighbour and no exchange between lanes,
//   * every solver scalar is an ordinary per-lane value, equal in the 16 lanes of its problem: one
//     instruction stream serves four problems, and
//   * the problems need not be in step: each slot carries its own state, truncated CG runs until the
//     slowest of the four has left it, and a slot whose problem met a stopping rule claims the next
//     one from the batch queue at once (its first cost / gradient evaluation is the same code a
//     continuing problem runs for its proposal).
// Arithmetic per problem is trust_region.py's, term by term as in rtr_solve_one's k = 2 branch; the
// inner products are summed in a different order (per node first, then over the nodes).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gik_args.h"
#include "gik_rtr.hip.h"

namespace gik {

// Rows of the two 16-byte row tables (point, direction).  A ds_read_b128 is served in four groups of 16 lanes --
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 (MI355X_MICROARCH.md, LDS table) -- over 64 banks of
// 4 bytes: 16 rows fill the banks once.  With lane = 16 r + 4 b + i a group holds the rows (r0: slots 0 and 3) and
// (r1: slots 1 and 2) (the other group: r0: 1, 2; r1: 0, 3), four consecutive nodes each.  With the slots 16 rows
// apart (round 4-5) two slots of a group always met on the same banks: every gather took twice its cycles
// (SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE = 0.59, profiles/r05_c5).  With slots 2 and 3 shifted by eight rows the
// four windows of a group tile the sixteen bank quads whenever the lanes gather at a common node offset (the chain's
// interior): row of (slot b, node j) = quad_row0(b) + j.
constexpr int QUAD_ROWS = 72;
__host__ __device__ constexpr int quad_row0(int b) { return b == 0 ? 0 : (b == 1 ? 16 : (b == 2 ? 40 : 56)); }

// total over the 16 lanes of this lane's problem slot, identical in all of them
__device__ inline double quad_sum(double v) { return mfma_blocksum(v); }
__device__ inline bool quad_any(bool c) { return __builtin_amdgcn_ballot_w64(c) != 0ull; }

// The literal 4 x 4 system of the k = 2 projector (fixed_rank_psd_sym.py:107-110, rhs [0, 1, -1, 0]) by Gaussian
// elimination with partial pivoting, as WaveCtx::proj_setup does it.  Not inlined: QuadCtx::proj_setup needs it
// for a few per cent of the points only, and inlined its 20-entry tableau sets the register peak of the whole
// kernel (spills of every wavefront instead of a call's save / restore in the rare case).
// (round 5: the solution comes back by value -- four doubles in registers; by reference it was a 32-byte stack frame,
//  i.e. scratch memory for every wavefront of the kernel.)
struct Omega4 {
  double u0, u1, u2, u3;
};
__device__ __attribute__((noinline)) Omega4 planar_omega_by_elimination(double X00, double X01, double X11) {
  double A[4][5] = {{X00 + X00, X01, X01, 0.0, 0.0},
                    {X01, X01 + X00, 0.0, X01, 1.0},
                    {X01, 0.0, X00 + X11, X01, -1.0},
                    {0.0, X01, X01, X11 + X11, 0.0}};
#pragma unroll
  for (int col = 0; col < 4; ++col) {
#pragma unroll
    for (int r = col + 1; r < 4; ++r) {  // partial pivoting by compare-and-swap
      const bool sw = fabs(A[r][col]) > fabs(A[col][col]);
#pragma unroll
      for (int t = 0; t < 5; ++t) {
        const double p = A[col][t], q = A[r][t];
        A[col][t] = sw ? q : p;
        A[r][t] = sw ? p : q;
      }
    }
    const double ip = 1.0 / A[col][col];
#pragma unroll
    for (int r = col + 1; r < 4; ++r) {
      const double fct = A[r][col] * ip;
#pragma unroll
      for (int t = col; t < 5; ++t) A[r][t] = fma(-fct, A[col][t], A[r][t]);
    }
  }
  Omega4 o;
  o.u3 = A[3][4] / A[3][3];
  o.u2 = (A[2][4] - A[2][3] * o.u3) / A[2][2];
  o.u1 = (A[1][4] - A[1][2] * o.u2 - A[1][3] * o.u3) / A[1][1];
  o.u0 = (A[0][4] - A[0][1] * o.u1 - A[0][2] * o.u2 - A[0][3] * o.u3) / A[0][0];
  return o;
}

template <int DEG>
struct QuadCtx {
  int lane, slot, node;
  bool has_node;
  double2 *sh_P;     // [4][16] rows of the point last given to cost()
  double2 *sh_W;     // [4][16] rows of the direction given to ehess()
  int own;           // this lane's row
  // slot s: [10:0] byte offset of the neighbour's row (own row: padding), [11] the residual has no lower
  // clamp, [12] no upper clamp (residual = clamp(target - d, lo, hi) with lo = -inf / 0, hi = +inf / 0: EQ (-inf, +inf),
  // LOWER (0, +inf), UPPER (-inf, 0), padding (0, 0) -- see WaveCtx::SlotRec), [31:16] term index
  uint32_t sl[DEG];
  double *sh_tg;     // [DEG][64] per problem: squared target distances (LDS: only cost() and commit() read them)
  // per committed point: ys = 2 a (Y_i - Y_j) (a = 1 where the term is active, else 0), cc = 2 c
  double ys0[DEG], ys1[DEG], cc[DEG];
  double cl_[DEG];   // clamped residuals of the point last given to cost(): commit() takes them from here
  double pk[2], pk2[2], G2;   // k = 2 projector (fixed_rank_psd_sym.py:107-113; Pm = 1)

  __host__ __device__ static constexpr size_t lds_bytes() {
    return 2 * sizeof(double2) * QUAD_ROWS + sizeof(double) * DEG * WAVE + sizeof(int) * 2 * QUAD_SLOTS;
  }

  // g_meta: the wavefront kernel's slot table [DEG][64] (lane = 2 node + component)
  __device__ inline void init(int lane_, int N, double2 *P, double2 *W, double *TG, const uint32_t *g_meta) {
    lane = lane_;
    sh_tg = TG;
    slot = (lane >> 2) & 3;
    node = ((lane >> 4) << 2) | (lane & 3);
    has_node = node < N;
    sh_P = P;
    sh_W = W;
    own = quad_row0(slot) + node;
#pragma unroll
    for (int s = 0; s < DEG; ++s) {
      // (a padding slot of the table names the node itself with kind 0: residual clamp(., 0, 0) = 0)
      const uint32_t m = has_node ? g_meta[s * WAVE + 2 * node] : meta_pack(node, 0, 0, 0);
      const int kind = meta_kind(m);
      sl[s] = (uint32_t)((quad_row0(slot) + meta_j(m)) * sizeof(double2)) |
              ((kind == GIK_TERM_EQ || kind == GIK_TERM_UPPER) ? 0x800u : 0u) |
              ((kind == GIK_TERM_EQ || kind == GIK_TERM_LOWER) ? 0x1000u : 0u) | ((uint32_t)meta_term(m) << 16);
      sh_tg[s * WAVE + lane] = 0.0;
      ys0[s] = ys1[s] = cc[s] = cl_[s] = 0.0;
    }
    pk[0] = pk[1] = pk2[0] = pk2[1] = G2 = 0.0;
    for (int t = lane; t < QUAD_ROWS; t += WAVE) {
      sh_P[t] = make_double2(0.0, 0.0);
      sh_W[t] = make_double2(0.0, 0.0);
    }
    __builtin_amdgcn_wave_barrier();
  }

  // per problem (divergent: only the lanes of the slot that starts problem b)
  __device__ inline void load_targets(const double *targets_b) {
#pragma unroll
    for (int s = 0; s < DEG; ++s) sh_tg[s * WAVE + lane] = targets_b[opaque(sl[s]) >> 16];
  }
  // The slot word through an empty asm: what is derived from it at this use (the clamp bounds of residual() as
  // doubles, the 64-bit offsets of load_targets()) is then computed HERE, a few integer instructions once per outer
  // iteration, instead of being hoisted out of the kernel's loop and kept live across the tCG solve -- round 4's
  // build held 2 x DEG bounds and DEG offsets that way, most of them in scratch.
  __device__ static inline uint32_t opaque(uint32_t m) {
    asm volatile("" : "+v"(m));
    return m;
  }
  __device__ inline const double2 &row(const double2 *base, int s) const {
    return *reinterpret_cast<const double2 *>(reinterpret_cast<const char *>(base) + (sl[s] & 0x7ffu));
  }
  // clamp(u, lo, hi) of slot s (the bounds differ from 0 in their upper word only)
  __device__ inline double residual(int s, double u) const {
    const uint32_t m = opaque(sl[s]);
    const double lo = __hiloint2double((m & 0x800u) ? (int)0xfff00000 : 0, 0);
    const double hi = __hiloint2double((m & 0x1000u) ? 0x7ff00000 : 0, 0);
    return fmin(fmax(u, lo), hi);
  }

  // f(x): lcost / jcost (costs.py:80-93, 8-16); leaves the rows of x in sh_P.  Every term sits in
  // the slot lists of both of its nodes, so each is counted twice and the total is halved (exact).
  // Wave-uniform call; slots without a problem compute on whatever they hold.
  __device__ inline double cost(double x0, double x1) {
    __builtin_amdgcn_wave_barrier();
    sh_P[own] = make_double2(x0, x1);
    __builtin_amdgcn_wave_barrier();
    double f = 0.0;
#pragma unroll
    for (int s = 0; s < DEG; ++s) {
      const double2 r = row(sh_P, s);
      const double a = x0 - r.x, b = x1 - r.y;
      const double d = fma(b, b, a * a);
      const double cl = residual(s, sh_tg[s * WAVE + lane] - d);
      cl_[s] = cl;
      f = fma(cl, cl, f);
    }
    return 0.5 * quad_sum(has_node ? f : 0.0);
  }

  // egrad at the point whose rows are in sh_P (lgrad / jgrad, costs.py:98-123, 20-35) and the
  // per-slot constants of the Hessian there.  No cross-lane step: may be called by some slots only.
  // The clamped residuals are those cost() formed for this point (cl_: the same bits as recomputing them, which
  // until round 5 cost a squared distance, a target read and two clamps per slot a second time).
  __device__ inline void commit(double &g0, double &g1) {
    const double2 o = sh_P[own];
    double G0 = 0.0, G1 = 0.0;
#pragma unroll
    for (int s = 0; s < DEG; ++s) {
      const double2 r = row(sh_P, s);
      const double a = o.x - r.x, b = o.y - r.y;
      const double cl = cl_[s];
      // active: an equality always, a hinge iff its clamped residual is non-zero
      const bool act = ((sl[s] & 0x1800u) == 0x1800u) || (cl != 0.0);
      const double c = -cl;
      ys0[s] = act ? a + a : 0.0;
      ys1[s] = act ? b + b : 0.0;
      cc[s] = c + c;
      G0 = fma(c, a, G0);
      G1 = fma(c, b, G1);
    }
    g0 = G0 + G0;
    g1 = G1 + G1;
  }

  // ehess(Y, W) (lhess / jhess, costs.py:175-207, 39-58) at the last commit():
  //   H_i = sum_j [ 4 a (y.w) y + 2 c w ],  y = Y_i - Y_j,  w = W_i - W_j     (4 a y y^T = ys ys^T)
  __device__ inline void ehess(double w0, double w1, double &h0, double &h1) {
    __builtin_amdgcn_wave_barrier();
    sh_W[own] = make_double2(w0, w1);
    __builtin_amdgcn_wave_barrier();
    double a0 = 0.0, a1 = 0.0;
#pragma unroll
    for (int s = 0; s < DEG; ++s) {
      const double2 r = row(sh_W, s);
      const double u0 = w0 - r.x, u1 = w1 - r.y;
      const double t = fma(ys1[s], u1, ys0[s] * u0);
      a0 = fma(t, ys0[s], fma(cc[s], u0, a0));
      a1 = fma(t, ys1[s], fma(cc[s], u1, a1));
    }
    h0 = a0;
    h1 = a1;
  }

  // Horizontal-space projector at x (PSDFixedRank.proj, fixed_rank_psd_sym.py:91-113), k = 2: the
  // literal 4 x 4 matrix of :107-110 solved for the right-hand side [0, 1, -1, 0] (see
  // WaveCtx::proj_setup).  A function of x alone: slots whose point did not change get the same
  // values again, bit for bit.
  __device__ inline void proj_setup(double x0, double x1, int planar_proj_exact) {
    const double hm = has_node ? 1.0 : 0.0;
    const double X00 = quad_sum(hm * x0 * x0), X01 = quad_sum(hm * x0 * x1), X11 = quad_sum(hm * x1 * x1);
    double u0, u1, u2, u3;
    if (planar_proj_exact) {
      const double it = 1.0 / (X00 + X11);
      u0 = 0.0; u1 = it; u2 = -it; u3 = 0.0;
    } else {
      // The literal system of :107-110 (its [1][1] entry is X01 + X00) for the right-hand side [0, 1, -1, 0],
      //   [2a  b    b    0 ] u0    0          a = X00, b = X01, c = X11
      //   [b   a+b  0    b ] u1 =  1
      //   [b   0    a+c  b ] u2   -1
      //   [0   b    b    2c] u3    0
      // solved by substitution instead of WaveCtx::proj_setup's elimination with pivoting (250 instructions, a
      // tenth of this kernel's pass): rows 0 and 3 give u0 = -b s / 2a, u3 = -b s / 2c with s = u1 + u2, rows 1
      // and 2 then u1 = (1 + k s) / (a + b), u2 = (k s - 1) / (a + c), k = b^2 (a + c) / (2 a c) <= (a + c) / 2
      // (Cauchy-Schwarz), and their sum fixes s.  Same solution to round-off -- except where the literal entry
      // a + b is small against a + c (b < 0): the substitution divides by it while the system as a whole stays
      // well conditioned, so there (|a + b| < (a + c) / 20: a few per cent of the points) the elimination runs,
      // for the whole wavefront under a uniform branch, and the slot concerned takes its result.
      const double a = X00, b = X01, c = X11;
      const double iab = 1.0 / (a + b), iac = 1.0 / (a + c), i2a = 0.5 / a, i2c = 0.5 / c;
      const double k = b * b * (i2a + i2c);
      const double s = (iab - iac) / (1.0 - k * (iab + iac));
      u1 = (1.0 + k * s) * iab;
      u2 = (k * s - 1.0) * iac;
      u0 = -b * s * i2a;
      u3 = -b * s * i2c;
      const bool risky = !(fabs(a + b) >= 0.05 * (a + c));
      if (quad_any(risky)) {
        const Omega4 e = planar_omega_by_elimination(X00, X01, X11);
        u0 = risky ? e.u0 : u0;
        u1 = risky ? e.u1 : u1;
        u2 = risky ? e.u2 : u2;
        u3 = risky ? e.u3 : u3;
      }
    }
    pk[0] = -hm * x1;
    pk[1] = hm * x0;
    pk2[0] = hm * (x0 * u0 + x1 * u2);
    pk2[1] = hm * (x0 * u1 + x1 * u3);
    G2 = quad_sum(fma(pk2[1], pk2[1], pk2[0] * pk2[0]));
  }
};

// what a slot hands back when its problem meets a stopping rule
struct QuadStats {
  double f, gradnorm, Delta;
  int iterations, inner_total, stop, n_accept;
};

}  // namespace gik
