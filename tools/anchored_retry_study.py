#!/usr/bin/env python3
"""tools/anchored_retry_study.py -- restarts with a clearance rule in the fixed-anchor solve, measured on the device
(a measurement tool; bench.py is the project's yardstick and is not touched by it).  docs/NOTEBOOK.md 19.

    python tools/anchored_retry_study.py [--paths 4096] [--waypoints 32] [--step 0.02] [--reps 3]
                                         [--baseline-tree DIR] [--out profiles/anchored_retry_study.json]

UR10 + table_environment() and the paths of tools/anchored_tracking_study.py (the same generator, the same seed).
  cold    : the 4096 goals of waypoint 0, AnchoredProblem.solve(T, retries=r) for r in {0, 1, 3}: how many goals fail the
            rule (stop, pos_err, rot_err, clearance), how many of attempt 0's failures the restarts rescue, ms per batch.
  tracked : AnchoredProblem.solve_trajectory on all paths, retries = 0 and retries = 1 with retry_spread in
            {0, 0.1, 0.3}: share converged (f < 1e-9), share with clearance >= -1e-4, share succeeding under the rule,
            share of consecutive-waypoint joint jumps < 0.2 rad, ms per waypoint.
  baseline: --baseline-tree DIR, a checkout of the parent commit with its library built: its solve_trajectory runs in a
            child process (another interpreter, that tree's package and library) on the same paths, alternated `reps`
            times with this tree's retries = 0 run; the two min .. max ranges must overlap, since retries = 0 queues
            the same work, and the answers are compared bit for bit.
Prints one JSON line and writes it to --out.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

TOL = dict(pos_tol=0.01, rot_tol=0.01, clear_tol=1e-4)

CHILD = r"""
import sys, numpy as np
tree, tpath, qpath, opath = sys.argv[1:5]
sys.path.insert(0, tree)
sys.path.insert(0, tree + "/tools")
from anchored_tracking_study import scene
robot, ap = scene()
T, q0 = np.load(tpath), np.load(qpath)
ap.solve_trajectory(T[:, :2], q0)
q, _, info = ap.solve_trajectory(T, q0)
np.savez(opath, q=q, time=info["solve_time"], clearance=info["clearance"])
"""


def baseline_run(tree, tpath, qpath):
    """One solve_trajectory of the baseline tree in a child process: (seconds, q, clearance)."""
    import numpy as np
    opath = tpath + ".out.npz"
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "GIK_LIB_PATH")}
    subprocess.run([sys.executable, "-c", CHILD, os.path.abspath(tree), tpath, qpath, opath], check=True, env=env,
                   cwd=os.path.abspath(tree), timeout=900)
    d = np.load(opath)
    return float(d["time"]), d["q"], d["clearance"]


def rng3(t, scale):
    import numpy as np
    return [round(scale * v, 4) for v in (float(np.median(t)), min(t), max(t))]


def measure(a):
    import numpy as np
    import torch
    from anchored_tracking_study import paths, scene
    from graphik_amd.solvers.riemannian_solver import anchored_retry_failed
    robot, ap = scene()
    Q, T, kept = paths(robot, ap, a.paths, a.waypoints, a.step, a.margin)
    B, L = T.shape[:2]
    res = {"workload": "ur10_table_anchored_retry", "paths": B, "waypoints": L, "step_rad": a.step, "margin_m": a.margin,
           "reps": a.reps, "tolerances": TOL, "cold": [], "tracked": []}

    def quad(r):
        return [r[k].cpu().numpy() for k in ("stop", "pos_err", "rot_err", "clearance")]

    # ---- cold goals
    T0 = T[:, 0]
    ap.solve(T0[:64], retries=1, **TOL)                      # warm-up: library, handles, code objects
    plain_failed = None
    for retries in (0, 1, 3):
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0[0].record()
            r = ap.solve(T0, clearance=True, retries=retries, retry_seed=1, **(TOL if retries else {}))
            t0[1].record()
            torch.cuda.synchronize()
            times.append(t0[0].elapsed_time(t0[1]) * 1e-3)
        failed = anchored_retry_failed(*quad(r), **TOL)
        if retries == 0:
            plain_failed = failed
        row = {"retries": retries, "ms_per_batch_median_min_max": rng3(times, 1e3),
               "converged_f_lt_1e-9": float((r["f"].cpu().numpy() < 1e-9).mean()), "failed_under_the_rule": int(failed.sum()),
               "rescued_of_attempt_0_failures": int((plain_failed & ~failed).sum()),
               "attempt_0_failures": int(plain_failed.sum())}
        if retries:
            row["attempt_histogram"] = np.bincount(r["attempt"].cpu().numpy(), minlength=retries + 1).tolist()
        res["cold"].append(row)

    # ---- tracked paths
    ap.solve_trajectory(T[:, :2], Q[:, 0], retries=1, **TOL)
    tmp = tempfile.mkdtemp(prefix="anch_retry_study_")
    tpath, qpath = os.path.join(tmp, "T.npy"), os.path.join(tmp, "q0.npy")
    np.save(tpath, T), np.save(qpath, Q[:, 0])
    t_here, t_base, same = [], [], None
    for _ in range(a.reps):                                  # alternated: both see the same machine
        q, _, info = ap.solve_trajectory(T, Q[:, 0])
        t_here.append(info["solve_time"])
        if a.baseline_tree:
            dt, q_b, cl_b = baseline_run(a.baseline_tree, tpath, qpath)
            t_base.append(dt)
            same = bool(np.array_equal(q, q_b, equal_nan=True) and np.array_equal(info["clearance"], cl_b, equal_nan=True))

    def tracked_row(label, q, info, times):
        dq = np.abs(np.mod(q[:, 1:] - q[:, :-1] + np.pi, 2 * np.pi) - np.pi).max(axis=2)
        failed = anchored_retry_failed(info["stop"], info["pos_err"], info["rot_err"], info["clearance"], **TOL)
        row = {"run": label, "ms_per_waypoint_median_min_max": rng3(times, 1e3 / L),
               "converged_f_lt_1e-9": float((info["f(x)"] < 1e-9).mean()),
               "clearance_ge_-1e-4": float((info["clearance"] >= -1e-4).mean()),
               "succeed_under_the_rule": float((~failed).mean()), "failed_waypoints": int(failed.sum()),
               "min_clearance": float(np.nanmin(info["clearance"])), "joint_jump_lt_0.2": float((dq < 0.2).mean())}
        if "attempt" in info:
            row["waypoints_replaced"] = int((info["attempt"] > 0).sum())
        return row

    shutil.rmtree(tmp, ignore_errors=True)
    res["tracked"].append(tracked_row("retries=0", q, info, t_here))
    if a.baseline_tree:
        res["baseline"] = {"ms_per_waypoint_median_min_max": rng3(t_base, 1e3 / L), "same_bits_as_retries_0": same,
                           "ranges_overlap": bool(min(t_here) <= max(t_base) and min(t_base) <= max(t_here))}
    for spread in (0.0, 0.1, 0.3):
        times = []
        for _ in range(a.reps):
            q, _, info = ap.solve_trajectory(T, Q[:, 0], retries=1, retry_seed=1, retry_spread=spread, **TOL)
            times.append(info["solve_time"])
        res["tracked"].append(tracked_row(f"retries=1 spread={spread}", q, info, times))
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--paths", type=int, default=4096)
    p.add_argument("--waypoints", type=int, default=32)
    p.add_argument("--step", type=float, default=0.02)
    p.add_argument("--margin", type=float, default=0.05)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--baseline-tree", default=None)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "anchored_retry_study.json"))
    a = p.parse_args()
    res = measure(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
