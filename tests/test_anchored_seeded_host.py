"""The fixed-anchor solve from joint-configuration seeds, host side (CPU only): AnchoredProblem.seed_points against
the reference-pinned realization of tests/golden/seeded.npz, and the CPU twin of the device feature -- the oracle's
anchored trust-region solve started from seed_points(q_prev) -- on the two inputs of tests/test_anchored_seeded_gpu.py
with the bars that file holds the device to: the evidence that the formulation tracks a path among the obstacles and
pushes a seed out of the spheres."""
import functools

import numpy as np

from conftest import make_graph
from test_seeded_host import _fixture

N_PATHS, N_WAYPOINTS, STEP = 64, 8, 0.02


@functools.lru_cache(maxsize=None)
def host_problem():
    from graphik_amd.solvers.riemannian_solver import AnchoredProblem
    robot, graph = make_graph("ur10_table")
    return robot, graph, AnchoredProblem(graph, host_only=True)


def fk_clearance(robot, ap, Q):
    """min over (p1 .. p_{n-1}, sphere) of |p - centre| - radius of the configurations Q [..., n]: the clearance of
    AnchoredProblem.clearance(include_goal=False) computed from forward kinematics."""
    Q = np.asarray(Q, dtype=float)
    flat = Q.reshape(-1, robot.n)
    P = np.stack([robot.fk_batch(flat, i)[:, :3, 3] for i in range(1, robot.n)], axis=1)
    d = np.linalg.norm(P[:, :, None, :] - ap.obstacles[None, None, :, :3], axis=-1) - ap.obstacles[None, None, :, 3]
    return d.min(axis=(1, 2)).reshape(Q.shape[:-1])


@functools.lru_cache(maxsize=None)
def tracking_input():
    """Input (a): 64 collision-free paths of 8 waypoints, 0.02 rad per joint per waypoint.  Returns (Q [64,8,n],
    T [64,8,4,4])."""
    robot, graph, ap = host_problem()
    rng = np.random.RandomState(21)
    lb, ub = robot.limits_arrays()
    q0 = rng.uniform(0.6 * lb, 0.6 * ub, size=(4000, robot.n))
    sign = rng.choice([-1.0, 1.0], size=(4000, robot.n))
    Q = q0[:, None] + STEP * sign[:, None] * np.arange(N_WAYPOINTS)[None, :, None]
    keep = np.flatnonzero(fk_clearance(robot, ap, Q).min(axis=1) > 0.05)
    assert len(keep) >= N_PATHS
    Q = Q[keep[:N_PATHS]]
    T = robot.fk_batch(Q.reshape(-1, robot.n)).reshape(N_PATHS, N_WAYPOINTS, 4, 4)
    return Q, T


@functools.lru_cache(maxsize=None)
def collision_input():
    """Input (b): (seeds [64,n] in collision by more than 0.02 m, goal configurations [64,n] clear by more than
    0.05 m)."""
    robot, graph, ap = host_problem()
    rng = np.random.RandomState(22)
    lb, ub = robot.limits_arrays()
    Q = rng.uniform(lb, ub, size=(20000, robot.n))
    c = fk_clearance(robot, ap, Q)
    seeds, goals = Q[c < -0.02][:64], Q[c > 0.05][:64]
    assert len(seeds) == 64 and len(goals) == 64
    return seeds, goals


def free_matrices(ap):
    """Dense free-free matrices (D, omega, psi_L, psi_U) of the oracle's anchored solve."""
    ti, tj, tk, target = ap.free_terms
    Nf = len(ap.free)
    D, om, pL, pU = (np.zeros((Nf, Nf)) for _ in range(4))
    for i, j, k, t in zip(ti, tj, tk, target):
        if k == 1:
            om[i, j] = om[j, i] = 1.0
            D[i, j] = D[j, i] = t
        elif k == 2:
            pL[i, j] = pL[j, i] = t
        else:
            pU[i, j] = pU[j, i] = t
    return D, om, pL, pU


def full_points(ap, x_free, goal_anchor):
    """Free rows + anchors -> the robot graph's point matrix [N_robot, 3] (anch_gather_kernel on the host)."""
    Y = np.zeros((ap.base.N, 3))
    Y[ap.free] = x_free
    nb = len(ap.anchors) - 2
    Y[ap.anchors[:nb]] = ap.base.anchor_pos
    Y[ap.anchors[nb:]] = np.asarray(goal_anchor).reshape(2, 3)
    return Y


def twin_solve(ap, T, q_seed, **kw):
    """The CPU twin of gik_anchored_ik_batch_seeded: per goal the oracle's anchored solve from
    seed_points(q_seed).  Returns (oracle results, Y_full [B,N_robot,3], q [B,n])."""
    from oracle import c_oracle as co
    from parity_util import anchored_terms
    D, om, pL, pU = free_matrices(ap)
    ga = ap.goal_anchors(T)
    Y0 = ap.seed_points(q_seed)
    res, Y = [], []
    for b in range(len(T)):
        node, pos, tgt, kind = anchored_terms(ap, ga[b])
        res.append(co.rtr_solve_anchored(Y0[b], D, om, pL, pU, node, pos, tgt, kind, **kw))
        Y.append(full_points(ap, res[-1]["x"], ga[b]))
    Y = np.stack(Y)
    return res, Y, ap.base.joint_variables(Y, T)


def test_seed_points_are_the_free_rows_of_the_reference_realization():
    robot, graph, ap = host_problem()
    d = _fixture("ur10_table")
    Y = ap.seed_points(d["q_init"])
    assert Y.shape == (len(d["q_init"]), len(ap.free), 3)
    # (the fixture's graph carries the obstacle nodes behind the robot's; the robot graph's rows come first)
    assert list(graph.node_ids[:ap.base.N]) == list(ap.base.graph.node_ids)
    assert np.abs(Y - d["Y_init"][:, ap.free]).max() < 1e-12
    assert np.array_equal(ap.seed_points(d["q_init"][2]), Y[2:3])


def test_cpu_twin_tracks_paths_among_the_obstacles():
    """Input (a), each waypoint seeded by the previous answer: the bars of the device tracking test."""
    from parity_util import wrap_abs
    robot, graph, ap = host_problem()
    Q, T = tracking_input()
    q_prev, f, its, clear, pos, qs = Q[:, 0], [], [], [], [], []
    for l in range(N_WAYPOINTS):
        res, Y, q_prev = twin_solve(ap, T[:, l], q_prev)
        f.append([r["f(x)"] for r in res])
        its.append([r["iterations"] for r in res])
        clear.append(ap.clearance(Y))
        pos.append(ap.base.pose_errors(q_prev, T[:, l])[0])
        qs.append(q_prev)
    f, its, clear, pos, qs = (np.stack(a, axis=1) for a in (f, its, clear, pos, qs))
    conv = f < 1e-9
    print("twin tracking: converged", conv.sum(), "of", conv.size, "iterations median", np.median(its), "max", its.max(),
          "min clearance", clear[conv].min())
    assert conv.mean() >= 0.99
    assert np.all(clear[conv] > -1e-4)
    assert np.all(pos[conv] < 2e-2) and np.median(pos[conv]) < 1e-3
    assert np.mean(wrap_abs(qs[:, 1:] - qs[:, :-1]).max(axis=2) < 0.2) >= 0.99


def test_cpu_twin_pushes_colliding_seeds_out_of_the_spheres():
    """Input (b): collision-free goals started from seeds in collision."""
    robot, graph, ap = host_problem()
    seeds, goals = collision_input()
    res, Y, q = twin_solve(ap, robot.fk_batch(goals), seeds)
    conv = np.array([r["f(x)"] for r in res]) < 1e-9
    clear = ap.clearance(Y)
    print("twin collision input: converged", conv.sum(), "of 64, min clearance", clear[conv].min())
    assert conv.sum() >= 48
    assert np.all(clear[conv] > -1e-4)
