#!/usr/bin/env python3
"""Golden vectors for warm-started (seeded) solves, by RUNNING THE REFERENCE (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/capture_golden_seeded.py [graph ...]

The reference's own warm start is RiemannianSolver.solve(D_goal, omega, Y_init=..., bounds=None)
(riemannian_solver.py:178-218; with bounds=None the seed is used, :197-198), with the seed built as
its examples build it: Y_init = pos_from_graph(graph.realization(q_init))
(experiments/simple_ik_examples/test_chain_2d_new.py:46-59).  Here q_init = q_goal + U(-delta, delta)
per joint, 12 goals at each delta in {0.02, 0.2}, on

    lwa4d, ur10, planar10_limits_pi (planar chain, limits +-pi), tree5 (the 3-D tree of capture_golden_tree.py)
    ur10_table (UR10 + table_environment(): realization only, no solve -- N = 116)

Per goal: q_goal, T_goal ([n_ee, d+1, d+1]), q_init, Y_init, Y_sol, f, gradnorm, iterations, q_sol and the
48-iteration trajectory prefix (the Recorder of capture_golden.py), for the numpy closures (jit=False) and, under
"loop_" keys, for the costs.py loops (jit=True: what the oracle restates).  Keys are prefixed by the graph name.
Only numbers are written, to tests/golden/seeded.npz.
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import capture_golden as cg  # noqa: E402  (puts the reference and the shims on sys.path)
import capture_golden_tree as ct  # noqa: E402
import numpy as np  # noqa: E402
from graphik.graphs import ProblemGraphRevolute  # noqa: E402
from graphik.robots import RobotRevolute  # noqa: E402
from graphik.solvers.riemannian_solver import RiemannianSolver  # noqa: E402
from graphik.utils.dgp import (adjacency_matrix_from_graph, distance_matrix_from_graph,  # noqa: E402
                               graph_from_pos, pos_from_graph)
from graphik.utils.roboturdf import load_schunk_lwa4d, load_ur10  # noqa: E402
from graphik.utils.utils import table_environment  # noqa: E402

DELTAS = (0.02, 0.2)
GOALS_PER_DELTA = 12


def seeded_one(robot, graph, q_goal, q_init, use_limits=True, solve=True):
    ees = list(robot.end_effectors)
    joints = [f"p{i}" for i in range(1, robot.n + 1)]
    T_goal = {ee: robot.pose(q_goal, ee) for ee in ees}
    G = graph.from_pose(T_goal)
    D_goal = distance_matrix_from_graph(G)
    omega = adjacency_matrix_from_graph(G)
    Y_init = pos_from_graph(graph.realization(q_init), graph.node_ids)
    out = dict(T_goal=np.stack([T_goal[ee].as_matrix() for ee in ees]), Y_init=Y_init)
    if not solve:
        return out
    # the numpy closures (jit=False, what the reference's examples run) and the costs.py loops (jit=True, the
    # path the oracle restates operation by operation): "loop_" keys
    for pre, jit in (("", False), ("loop_", True)):
        solver = RiemannianSolver(graph)
        rec = cg.Recorder(solver.solver)
        info = solver.solve(D_goal, omega, use_limits=use_limits, Y_init=Y_init.copy(), bounds=None, jit=jit)
        traj = rec.arrays(info["x"])
        rec.restore()
        q_sol = graph.joint_variables(graph_from_pos(info["x"], graph.node_ids), T_goal)
        pos = max(np.linalg.norm(robot.pose(q_sol, ee).trans - T_goal[ee].trans) for ee in ees)
        res = dict(Y_sol=info["x"], f=float(info["f(x)"]), gradnorm=float(info["gradnorm"]),
                   iterations=int(info["iterations"]), q_sol=np.array([q_sol[j] for j in joints]), pos_err=pos)
        for key, v in traj.items():
            pad = np.full(cg.MAX_TRAJ, np.nan) if v.dtype.kind == "f" else np.full(cg.MAX_TRAJ, -9, dtype=np.int32)
            pad[:len(v)] = v
            res[key] = pad
        out.update({pre + key: v for key, v in res.items() if not (pre and key == "Y_sol")})   # (size)
    return out


def run(name, robot, graph, use_limits=True, solve=True, goals_per_delta=GOALS_PER_DELTA, seed0=100):
    joints = [f"p{i}" for i in range(1, robot.n + 1)]
    rows = {}
    for di, delta in enumerate(DELTAS):
        for g in range(goals_per_delta):
            seed = seed0 + 1000 * di + g
            np.random.seed(seed)
            q_goal = robot.random_configuration()
            qg = np.array([q_goal[j] for j in joints])
            qi = qg + np.random.RandomState(seed).uniform(-delta, delta, size=len(qg))
            t0 = time.time()
            r = seeded_one(robot, graph, q_goal, {j: qi[i] for i, j in enumerate(joints)}, use_limits, solve)
            r.update(q_goal=qg, q_init=qi, delta=delta)
            if solve:
                print(f"  {name} delta={delta} goal {g}: it={r['iterations']} f={r['f']:.2e} "
                      f"pos={r['pos_err']:.2e} max|q-qg|={np.max(np.abs(r['q_sol'] - qg)):.3f} "
                      f"t={time.time() - t0:.1f}s", flush=True)
            for key, v in r.items():
                rows.setdefault(key, []).append(v)
    out = {f"{name}__{key}": np.array(v) for key, v in rows.items()}
    out[f"{name}__use_limits"] = np.array(int(use_limits))
    return out


def tree5():
    robot = RobotRevolute(dict(ct.TREE))
    return robot, ProblemGraphRevolute(robot)


def ur10_table():
    robot, graph = load_ur10()
    for idx, obs in enumerate(table_environment()):
        graph.add_spherical_obstacle(f"o{idx}", obs[0], obs[1])
    return robot, graph


GRAPHS = {
    "lwa4d": lambda: run("lwa4d", *load_schunk_lwa4d()),
    "ur10": lambda: run("ur10", *load_ur10()),
    "planar10_limits_pi": lambda: run("planar10_limits_pi", *cg.planar_chain(10, np.pi)),
    "tree5": lambda: run("tree5", *tree5()),
    "ur10_table": lambda: run("ur10_table", *ur10_table(), solve=False, goals_per_delta=4),
}

if __name__ == "__main__":
    todo = sys.argv[1:] or list(GRAPHS)
    path = os.path.join(REPO, "tests", "golden", "seeded.npz")
    data = dict(np.load(path)) if os.path.exists(path) and sys.argv[1:] else {}
    for name in todo:
        data = {k: v for k, v in data.items() if not k.startswith(name + "__")}
        data.update(GRAPHS[name]())
    np.savez_compressed(path, **data)
    print(f"wrote {path} ({os.path.getsize(path) / 1024:.1f} KiB)", flush=True)
