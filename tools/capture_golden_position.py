#!/usr/bin/env python3
"""Golden vectors for POSITION goals (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_position.py

A position goal pins the point of an end effector and leaves its orientation free: the reference's
graph.from_pos({"p6": xyz}) (graph_base.py:146-165), then distance_matrix_from_graph, adjacency_matrix_from_graph,
bound_smoothing, RiemannianSolver.solve and joint_variables(G_sol) with a T_final entry only for the end effectors
whose goal is a pose -- the flow of the reference's own tests (tests/test_bound_smoothing.py:85-89,
tests/test_adjacency_matrix.py:478-480, 844-847).  Runs the reference with the stand-ins of tools/ref_shims and records,
per scenario (key prefix "<scenario>__"):

  ur10, lwa4d             4 goals each, the end effector by position
  planar10_limits_pi      4 goals, p10 by position
  planar_tree_y5          2 goals, both end effectors by position (the tree of tests/golden/planar_tree.npz)
  tree5                   2 goals, p4 by pose and p5 by position: from_pos({p4, q4, p5}) (the tree of tests/golden/tree5.npz)

per goal what capture_golden.run_scenario / solve_one record: the configuration, the goal poses (of a position end
effector only the translation is a goal), the goal positions, D_goal, omega, lb, ub, Y_init, the trust-region
trajectory prefix, Y_sol, f, gradnorm, iterations, q_sol and the worst position error of FK(q_sol); for the first two
goals of the 3-D chains the costs.py-loop path as well ("loop_*").  Only numbers and node names are written
(tests/golden/position_goals.npz).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import capture_golden as cg  # noqa: E402  (sets up the reference's import path and the stand-ins)
import numpy as np  # noqa: E402
from graphik.graphs import ProblemGraphPlanar, ProblemGraphRevolute  # noqa: E402
from graphik.robots import RobotPlanar, RobotRevolute  # noqa: E402
from graphik.solvers.riemannian_solver import RiemannianSolver  # noqa: E402
from graphik.utils.dgp import (adjacency_matrix_from_graph, bound_smoothing,  # noqa: E402
                               distance_matrix_from_graph, graph_from_pos)
from graphik.utils.roboturdf import load_schunk_lwa4d, load_ur10  # noqa: E402

from capture_golden_planar_tree import tree_params  # noqa: E402
from capture_golden_tree import TREE  # noqa: E402

TRAJ = 32      # outer iterations of the trajectory prefix kept
TRAJ_KEYS = ("Delta", "numit", "stop", "f_before", "gradnorm_after", "accept")


def solve_position(robot, graph, q_goal, kinds, jit):
    """One goal through the reference: kinds[e] in ("pose", "position") per robot.end_effectors."""
    ees = list(robot.end_effectors)
    T_goal = {ee: robot.pose(q_goal, ee) for ee in ees}
    pose_ees = {ee: T_goal[ee] for ee, kind in zip(ees, kinds) if kind == "pose"}
    P = dict(graph._pose_goal(pose_ees)) if pose_ees else {}
    for ee, kind in zip(ees, kinds):
        if kind == "position":
            P[ee] = T_goal[ee].trans
    G = graph.from_pos(P)
    D_goal = distance_matrix_from_graph(G)
    omega = adjacency_matrix_from_graph(G)
    lb, ub = bound_smoothing(G)
    psi_L, psi_U = graph.distance_bound_matrices()
    Y_init = RiemannianSolver.generate_initialization((lb, ub), graph.dim, omega, psi_L, psi_U)
    solver = RiemannianSolver(graph)
    rec = cg.Recorder(solver.solver)
    info = solver.solve(D_goal, omega, use_limits=True, Y_init=Y_init.copy(), jit=jit)
    traj = rec.arrays(info["x"])
    rec.restore()
    G_sol = graph_from_pos(info["x"], graph.node_ids)
    q_sol = graph.joint_variables(G_sol, pose_ees) if pose_ees else graph.joint_variables(G_sol)
    err = max(float(np.linalg.norm(robot.pose(q_sol, ee).trans - T_goal[ee].trans)) for ee in ees)
    joints = [f"p{i}" for i in range(1, robot.n + 1)]      # (column i - 1 = joint p_i, whatever the order of joint_ids)
    out = dict(q_goal=np.array([q_goal[j] for j in joints], dtype=float),
               T_goal=np.stack([T_goal[ee].as_matrix() for ee in ees]),
               goal_pos=np.stack([np.asarray(T_goal[ee].trans, dtype=float) for ee in ees]),
               D_goal=D_goal, omega=omega, lb=lb, ub=ub, Y_init=Y_init, Y_sol=info["x"], f=float(info["f(x)"]),
               gradnorm=float(info["gradnorm"]), iterations=int(info["iterations"]),
               q_sol=np.array([q_sol[j] for j in joints], dtype=float), pos_err=err)
    for key in TRAJ_KEYS:
        a = traj["traj_" + key][:TRAJ]
        pad = np.full(TRAJ, np.nan) if a.dtype.kind == "f" else np.full(TRAJ, -9, dtype=np.int32)
        pad[:len(a)] = a
        out["traj_" + key] = pad
    return out


def run(name, robot, graph, seeds, kinds, loop_goals=0):
    rows, loops = [], []
    for gi, seed in enumerate(seeds):
        np.random.seed(seed)
        q_goal = robot.random_configuration()
        r = solve_position(robot, graph, q_goal, kinds, jit=False)
        print(f"{name} goal {gi} seed {seed}: it={r['iterations']} f={r['f']:.2e} pos_err={r['pos_err']:.2e}", flush=True)
        assert r["f"] < 1e-9, "pick a seed on which the reference converges"
        rows.append(r)
        if gi < loop_goals:
            rl = solve_position(robot, graph, q_goal, kinds, jit=True)
            print(f"    loops: it={rl['iterations']} f={rl['f']:.2e} pos_err={rl['pos_err']:.2e}", flush=True)
            loops.append(rl)
    out = {"node_ids": np.array(list(graph.node_ids)), "end_effectors": np.array(list(robot.end_effectors)),
           "kinds": np.array(kinds), "seed": np.array(seeds), "omega": rows[0]["omega"]}
    for key in rows[0]:
        if key != "omega":
            out[key] = np.array([r[key] for r in rows])
    for key in ("Y_sol", "f", "gradnorm", "iterations", "q_sol", "pos_err") + tuple("traj_" + k for k in TRAJ_KEYS):
        if loops:
            out["loop_" + key] = np.array([r[key] for r in loops])
    return {f"{name}__{k}": v for k, v in out.items()}


if __name__ == "__main__":
    data = {}
    robot, graph = load_ur10()
    data.update(run("ur10", robot, graph, [0, 1, 2, 3], ["position"], loop_goals=2))
    robot, graph = load_schunk_lwa4d()
    data.update(run("lwa4d", robot, graph, [0, 1, 2, 3], ["position"], loop_goals=2))
    robot, graph = cg.planar_chain(10, np.pi)
    data.update(run("planar10_limits_pi", robot, graph, [21, 22, 23, 24], ["position"]))
    robot = RobotPlanar(tree_params("y5"))
    data.update(run("planar_tree_y5", robot, ProblemGraphPlanar(robot), [0, 1], ["position", "position"]))
    robot = RobotRevolute(dict(TREE))
    assert list(robot.end_effectors) == ["p4", "p5"]
    data.update(run("tree5", robot, ProblemGraphRevolute(robot), [0, 1], ["pose", "position"]))
    path = os.path.join(cg.REPO, "tests", "golden", "position_goals.npz")
    np.savez_compressed(path, **data)
    print("wrote", path, os.path.getsize(path) // 1024, "KiB")
    assert os.path.getsize(path) < 200 * 1024
