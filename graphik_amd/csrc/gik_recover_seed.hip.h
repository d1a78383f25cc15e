// graphik_amd/csrc/gik_recover_seed.hip.h -- joint angles out of a point matrix, and a point matrix out of joint angles.
//
//   recover_kernel   : one thread per goal: joint_variables (graph_revolute.py:251-318 /
//       graph_planar.py:147-176) + forward kinematics of the recovered angles -> EE pose error.  An end effector of
//       PipeConst::pos_goal_mask is a position goal: no T_final correction, its rotation error is not counted (0.0).
//   seed_kernel      : one wavefront per goal: the targets of a goal and the realization of q_init (see below).
// Plain kernels, defined where GIK_DEFINE_PLAIN_KERNELS is set (gik_k_prep.hip); every other unit sees prototypes.
#pragma once

#include <hip/hip_runtime.h>

#include "gik_args.h"
#include "gik_goal.hip.h"

namespace gik {

__device__ inline void mat4_mul(const double *A, const double *B, double *C) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      double s = (j == 3) ? A[i * 4 + 3] : 0.0;
      for (int t = 0; t < 3; ++t) s += A[i * 4 + t] * B[t * 4 + j];
      C[i * 4 + j] = s;
    }
  C[12] = C[13] = C[14] = 0.0;
  C[15] = 1.0;
}
__device__ inline void mat4_inv_rigid(const double *A, double *C) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) C[i * 4 + j] = A[j * 4 + i];
    C[i * 4 + 3] = -(A[0 * 4 + i] * A[3] + A[1 * 4 + i] * A[7] + A[2 * 4 + i] * A[11]);
  }
  C[12] = C[13] = C[14] = 0.0;
  C[15] = 1.0;
}
__device__ inline double wrap_pi(double e) {
  const double twopi = 6.283185307179586;
  double m = fmod(e + 3.141592653589793, twopi);
  if (m < 0.0) m += twopi;  // numpy mod takes the sign of the divisor
  return m - 3.141592653589793;
}

// (launched with 64 threads per block; without the bound the compiler budgets for 1024 and 128 VGPRs: 252 B of scratch)
__global__ void __launch_bounds__(64) recover_kernel(RecoverArgs a)
#ifndef GIK_DEFINE_PLAIN_KERNELS
    ;      // (defined in gik_k_prep.hip)
#else
{
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.B) return;
  const PipeConst &pc = a.pc;
  const int N = pc.N, K = pc.K, n = pc.n_joints;
  const double *P = a.Y + (size_t)b * N * K;
  double *q = a.q + (size_t)b * n;
  if (K == 3) {
    const double *p0 = P + pc.p_idx[0] * 3;
    // base frame from the recovered anchors: R = [x^, -y^, z^]  (graph_revolute.py:263-279)
    double R[9];
    const int src[3] = {pc.x_idx, pc.y_idx, pc.q_idx[0]};
    for (int c = 0; c < 3; ++c) {
      double v[3], nr = 0.0;
      for (int t = 0; t < 3; ++t) {
        v[t] = P[src[c] * 3 + t] - p0[t];
        nr += v[t] * v[t];
      }
      nr = sqrt(nr);
      const double sc = (nr == 0.0 ? 1.0 : 1.0 / nr) * (c == 1 ? -1.0 : 1.0);
      for (int t = 0; t < 3; ++t) R[t * 3 + c] = v[t] * sc;
    }
    double worst_p = 0.0, worst_r = 0.0;
    // one walk from the root per end effector (graph_revolute.py:285-316; joints shared by several
    // paths get the same angle from each)
    for (int e = 0; e < pc.n_ee; ++e) {
      const double *Tg = a.T_goal + ((size_t)b * pc.n_ee + e) * 16;
      const int *path = pc.ee_path + e * (n + 1);
      double Tp[16], Trel[16], tmp[16], inv[16];
      for (int t = 0; t < 16; ++t) Tp[t] = pc.T0[t];  // T[ROOT] = robot.T_base
      double th = 0.0;
      int cur = 0, last = 0;
      for (int k = 1; k <= n && path[k] >= 0; ++k) last = k;
      for (int k = 1; k <= last; ++k) {
        const int pred = path[k - 1];
        cur = path[k];
        mat4_inv_rigid(pc.T0 + pred * 16, inv);
        mat4_mul(inv, pc.T0 + cur * 16, Trel);  // T_rel = T_prev_0^-1 T_0
        // qs_0 = (T_prev_0^-1 T_0 trans_z(a)).trans
        double qs0[2];
        for (int t = 0; t < 2; ++t) qs0[t] = Trel[t * 4 + 3] + Trel[t * 4 + 2] * pc.axis_length;
        if (k == last && ((pc.pos_qs0_mask >> e) & 1)) {      // (a position goal behind a link along z: see PipeConst)
          qs0[0] = pc.pos_qs0[e][0];
          qs0[1] = pc.pos_qs0[e][1];
        }
        const double *pc_ = P + pc.p_idx[cur] * 3, *qc = P + pc.q_idx[cur] * 3;
        double dq[3], nr = 0.0;
        for (int t = 0; t < 3; ++t) {
          dq[t] = qc[t] - pc_[t];
          nr += dq[t] * dq[t];
        }
        nr = sqrt(nr);
        double qn[3], qb[3];
        for (int t = 0; t < 3; ++t) qn[t] = pc_[t] + dq[t] / nr - p0[t];
        for (int t = 0; t < 3; ++t) qb[t] = R[0 * 3 + t] * qn[0] + R[1 * 3 + t] * qn[1] + R[2 * 3 + t] * qn[2];
        double qs[2];
        for (int t = 0; t < 2; ++t)
          qs[t] = Tp[0 * 4 + t] * (qb[0] - Tp[3]) + Tp[1 * 4 + t] * (qb[1] - Tp[7]) +
                  Tp[2 * 4 + t] * (qb[2] - Tp[11]);
        th = atan2(qs0[0] * qs[1] - qs0[1] * qs[0], qs0[0] * qs[0] + qs0[1] * qs[1]);  // :308
        q[cur - 1] = th;
        if (k == last) break;  // keep T_prev of the last joint for the T_final correction
        const double c = cos(th), s = sin(th);
        double Rz[16] = {c, -s, 0, 0, s, c, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        mat4_mul(Tp, Rz, tmp);
        mat4_mul(tmp, Trel, Tp);  // :310
      }
      // T[ee] with the uncorrected last angle
      double Tee[16];
      {
        const double c = cos(th), s = sin(th);
        double Rz[16] = {c, -s, 0, 0, s, c, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        mat4_mul(Tp, Rz, tmp);
        mat4_mul(tmp, Trel, Tee);
      }
      const bool pos_goal = (pc.pos_goal_mask >> e) & 1;   // a position goal: no T_final, no rotation error
      if (((pc.last_along_z >> e) & 1) && !pos_goal) {  // :314-316
        // T_final expressed in the recovered base frame is the goal itself (T_base = identity
        // re-basing happened at load time); T_th = T[ee]^-1 T_final
        mat4_inv_rigid(Tee, inv);
        mat4_mul(inv, Tg, tmp);
        th = wrap_pi(th + atan2(tmp[4], tmp[0]));
        q[cur - 1] = th;
        const double c = cos(th), s = sin(th);
        double Rz[16] = {c, -s, 0, 0, s, c, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        mat4_mul(Tp, Rz, tmp);
        mat4_mul(tmp, Trel, Tee);
      }
      // pose error of FK(q) = T[ee] against the goal
      double dp = 0.0, tr = 0.0;
      for (int t = 0; t < 3; ++t) {
        const double df = Tg[t * 4 + 3] - Tee[t * 4 + 3];
        dp += df * df;
        for (int u = 0; u < 3; ++u) tr += Tg[t * 4 + u] * Tee[t * 4 + u];  // trace(Rg Rs^T)
      }
      worst_p = fmax(worst_p, sqrt(dp));
      if (!pos_goal) worst_r = fmax(worst_r, acos(fmin(1.0, fmax(-1.0, 0.5 * tr - 0.5))));
    }
    a.pos_err[b] = worst_p;     // (several end effectors: the worst of them)
    a.rot_err[b] = worst_r;
  } else {
    const double *Tg = a.T_goal + (size_t)b * 9 * pc.n_ee;
    // best_fit_transform of (p0, x, y) onto ((0,0), (-1,0), (0,1)) without reflection handling
    const double *A0 = P + pc.p_idx[0] * 2, *A1 = P + pc.x_idx * 2, *A2 = P + pc.y_idx * 2;
    const double ca[2] = {(A0[0] + A1[0] + A2[0]) / 3.0, (A0[1] + A1[1] + A2[1]) / 3.0};
    const double Bp[3][2] = {{0, 0}, {-1, 0}, {0, 1}};
    const double cb[2] = {-1.0 / 3.0, 1.0 / 3.0};
    const double *Ap[3] = {A0, A1, A2};
    double H[4] = {0, 0, 0, 0};  // H = AA^T BB
    for (int t = 0; t < 3; ++t)
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) H[i * 2 + j] += (Ap[t][i] - ca[i]) * (Bp[t][j] - cb[j]);
    // R = V U^T (H = U S V^T) = orthogonal polar factor of H^T; M = H^T
    const double M00 = H[0], M01 = H[2], M10 = H[1], M11 = H[3];
    const double det = M00 * M11 - M01 * M10;
    double Rm[4];
    if (det >= 0.0) {
      const double ang = atan2(M10 - M01, M00 + M11);
      Rm[0] = cos(ang); Rm[1] = -sin(ang); Rm[2] = sin(ang); Rm[3] = cos(ang);
    } else {
      const double ang = atan2(M10 + M01, M00 - M11);
      Rm[0] = cos(ang); Rm[1] = sin(ang); Rm[2] = sin(ang); Rm[3] = -cos(ang);
    }
    // One walk from the root per end effector (a chain: the one path 0, 1, ..., n; planar trees, round 6: joints shared
    // by several paths get the same angle from each -- graph_planar.py:147-176 walks the structure edges with R[u] per
    // node, which along a path is the running product kept here).  FK of the recovered angles along the same path:
    // T_i = T_{i-1} Rz(q_i) T0_{i-1}^-1 T0_i  (robot_planar.py:62-80); pose error: the worst end effector's.
    double worst_p = 0.0, worst_r = 0.0;
    for (int e = 0; e < pc.n_ee; ++e) {
      const double *Te = Tg + (size_t)e * 9;
      const int *path = pc.ee_path + e * (n + 1);
      double Rc[4] = {1, 0, 0, 1};
      double Fr[4] = {pc.T0[0], pc.T0[1], pc.T0[3], pc.T0[4]}, Ft[2] = {pc.T0[2], pc.T0[5]};
      for (int k = 1; k <= n && path[k] >= 0; ++k) {
        const int pred = path[k - 1], i = path[k];
        const double *pu = P + pc.p_idx[pred] * 2, *pv = P + pc.p_idx[i] * 2;
        const double d0 = pv[0] - pu[0], d1 = pv[1] - pu[1];
        double f0 = Rm[0] * d0 + Rm[1] * d1, f1 = Rm[2] * d0 + Rm[3] * d1;
        const double len = sqrt(f0 * f0 + f1 * f1);
        f0 /= len;
        f1 /= len;
        const double s0 = Rc[0] * f0 + Rc[2] * f1, s1 = Rc[1] * f0 + Rc[3] * f1;  // R[u]^T f
        const double th = atan2(s1, s0);
        q[i - 1] = wrap_pi(th);
        const double c = cos(th), s = sin(th);
        const double n0 = Rc[0] * c + Rc[1] * s, n1 = -Rc[0] * s + Rc[1] * c;
        const double n2 = Rc[2] * c + Rc[3] * s, n3 = -Rc[2] * s + Rc[3] * c;
        Rc[0] = n0; Rc[1] = n1; Rc[2] = n2; Rc[3] = n3;
        // T_rel = T0_pred^-1 T0_i
        const double *Ta = pc.T0 + pred * 9, *Tb = pc.T0 + i * 9;
        const double a00 = Ta[0], a01 = Ta[1], a10 = Ta[3], a11 = Ta[4];
        const double dxr = Tb[2] - Ta[2], dyr = Tb[5] - Ta[5];
        const double rr[4] = {a00 * Tb[0] + a10 * Tb[3], a00 * Tb[1] + a10 * Tb[4],
                              a01 * Tb[0] + a11 * Tb[3], a01 * Tb[1] + a11 * Tb[4]};
        const double rt[2] = {a00 * dxr + a10 * dyr, a01 * dxr + a11 * dyr};
        const double cq = cos(q[i - 1]), sq = sin(q[i - 1]);
        // F <- F * Rz(q) * T_rel
        const double g0 = Fr[0] * cq + Fr[1] * sq, g1 = -Fr[0] * sq + Fr[1] * cq;
        const double g2 = Fr[2] * cq + Fr[3] * sq, g3 = -Fr[2] * sq + Fr[3] * cq;
        Ft[0] += g0 * rt[0] + g1 * rt[1];
        Ft[1] += g2 * rt[0] + g3 * rt[1];
        Fr[0] = g0 * rr[0] + g1 * rr[2]; Fr[1] = g0 * rr[1] + g1 * rr[3];
        Fr[2] = g2 * rr[0] + g3 * rr[2]; Fr[3] = g2 * rr[1] + g3 * rr[3];
      }
      const double px = Ft[0], py = Ft[1], phi = atan2(Fr[2], Fr[0]);
      const double dx = Te[2] - px, dy = Te[5] - py;
      worst_p = fmax(worst_p, sqrt(dx * dx + dy * dy));
      const double gphi = atan2(Te[3], Te[0]);
      if (!((pc.pos_goal_mask >> e) & 1)) worst_r = fmax(worst_r, fabs(wrap_pi(gphi - phi)));   // (a position goal has none)
    }
    a.pos_err[b] = worst_p;
    a.rot_err[b] = worst_r;
  }
}
#endif

// ---------------------------------------------------------------------------------------------
// seed_kernel: joint-configuration warm start.  One wavefront per goal:
//   targets [T]  -- exactly the prepare kernels' rule (goal_distance, src >= 0 ? g*g : term_static)
//   Y_init [N*K] -- graph.realization(q_init) in node order (graph_base.py:112-120 through _pose_goal,
//                   graph_revolute.py:243-249 / graph_planar.py:136-145): the frames of q_init by
//                   F_j = F_parent(j) Rz(q_j) T0_parent^-1 T0_j (recover_kernel's walk, each joint once),
//                   then row i = trans(F_f) + coef * axis(F_f) for its recipe (f, coef), or anchor_pos.
// Lane 0 walks the frames into LDS (a handful of 4x4 products per joint); the rows and targets are
// written by all lanes, consecutive lanes on consecutive doubles.
__global__ void __launch_bounds__(WAVE) seed_kernel(SeedArgs a)
#ifndef GIK_DEFINE_PLAIN_KERNELS
    ;      // (defined in gik_k_prep.hip)
#else
{
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const PipeConst &pc = a.pc;
  const SeedConst &sc = a.sc;
  const int N = pc.N, K = pc.K, D = K + 1, DD = D * D, n = pc.n_joints, lane = threadIdx.x;
  const int axis = (K == 3) ? 2 : 0;
  double *F = smem;   // [n+1][DD] frames of this goal's q_init
  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const double *Tg = a.T_goal + (size_t)b * DD * pc.n_ee;
    for (int t = lane; t < pc.T; t += WAVE) {
      const int src = pc.term_src[t];
      double g = 0.0;
      if (src >= 0) {
        int an, gn;
        g = goal_distance(pc, Tg, src, an, gn);
      }
      a.targets[(size_t)b * pc.T + t] = src >= 0 ? g * g : pc.term_static[t];
    }
    if (lane == 0) {
      const double *q = a.q_init + (size_t)b * n;
      for (int o = 0; o < sc.n_fk; ++o) {
        const int j = sc.fk_order[o], p = sc.fk_parent[j];
        double *Fj = F + j * DD;
        if (p < 0) {
          for (int e = 0; e < DD; ++e) Fj[e] = pc.T0[j * DD + e];
          continue;
        }
        const double *Fp = F + p * DD, *R = sc.Trel + j * DD;
        const double c = cos(q[j - 1]), s = sin(q[j - 1]);
        for (int r = 0; r < K; ++r) {
          // row r of Fp Rz(q): columns 0, 1 rotate, the rest stay
          double m[4];
          m[0] = Fp[r * D + 0] * c + Fp[r * D + 1] * s;
          m[1] = Fp[r * D + 1] * c - Fp[r * D + 0] * s;
          for (int cc = 2; cc < D; ++cc) m[cc] = Fp[r * D + cc];
          for (int cc = 0; cc < D; ++cc) {
            double acc = (cc == K) ? m[K] : 0.0;
            for (int t = 0; t < K; ++t) acc += m[t] * R[t * D + cc];
            Fj[r * D + cc] = acc;
          }
        }
        for (int cc = 0; cc < D; ++cc) Fj[K * D + cc] = (cc == K) ? 1.0 : 0.0;
      }
    }
    __syncthreads();
    double *Y = a.Y_init + (size_t)b * N * K;
    for (int e = lane; e < N * K; e += WAVE) {
      const int node = e / K, c = e - node * K, f = sc.node_frame[node];
      Y[e] = f >= 0 ? F[f * DD + c * D + K] + sc.node_coef[node] * F[f * DD + c * D + axis]
                    : pc.anchor_pos[sc.node_anchor[node] * K + c];
    }
    __syncthreads();   // (F is rewritten by the next goal)
  }
}
#endif

}  // namespace gik
