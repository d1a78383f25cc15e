#!/usr/bin/env python3
"""tools/track_bench.py -- path tracking on the device: warm-started waypoint solves (a measurement tool; bench.py is
the project's yardstick and is not touched by it).

    python tools/track_bench.py [--paths 4096] [--waypoints 32] [--step 0.02] [--no-rocprof]

LWA4D, `paths` trajectories of `waypoints` goal poses, every joint moving `step` rad per waypoint (a random sign per
path and joint, from a random start inside 60 % of the joint range).  solve_trajectory seeds waypoint 0 with the
start configuration and waypoint l with the answer of waypoint l - 1, all on the device.  Prints one JSON line:
ms per waypoint, waypoint solves per second, outer iterations (median / max over all waypoint solves), and, for
comparison, the cold solve_batch (bound smoothing + MDS start) of the middle waypoints' goals.  Unless --no-rocprof,
the same run is repeated under `rocprofv3 --kernel-trace --stats` in a child process and seed_kernel's time and
share of the kernel time are added.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)


def paths(B, L, step, seed=11):
    import numpy as np
    from graphik_amd.utils.roboturdf import load_schunk_lwa4d
    robot, graph = load_schunk_lwa4d()
    rng = np.random.RandomState(seed)
    lb, ub = robot.limits_arrays()
    q0 = rng.uniform(0.6 * lb, 0.6 * ub, size=(B, robot.n))
    sign = rng.choice([-1.0, 1.0], size=(B, robot.n))
    Q = q0[:, None] + step * sign[:, None] * np.arange(L)[None, :, None]
    return robot, graph, Q, robot.fk_batch(Q.reshape(-1, robot.n)).reshape(B, L, 4, 4)


def measure(a):
    import numpy as np
    from graphik_amd.solvers.riemannian_solver import solve_batch, solve_trajectory
    robot, graph, Q, T = paths(a.paths, a.waypoints, a.step)
    solve_trajectory(graph, T[:, :2], Q[:, 0])                  # warm-up: library, handles, buffers
    q, _, info = solve_trajectory(graph, T, Q[:, 0])
    dq = np.abs(np.mod(q[:, 1:] - q[:, :-1] + np.pi, 2 * np.pi) - np.pi).max(axis=2)
    solve_batch(graph, T[:8, a.waypoints // 2])
    _, _, cold = solve_batch(graph, T[:, a.waypoints // 2])
    its = info["iterations"]
    return {"workload": "lwa4d_track", "paths": a.paths, "waypoints": a.waypoints, "step_rad": a.step,
            "ms_per_waypoint": 1e3 * info["solve_time"] / a.waypoints,
            "waypoint_solves_per_s": a.paths * a.waypoints / info["solve_time"],
            "iterations_median": float(np.median(its)), "iterations_max": int(its.max()),
            "pos_err_lt_1e-3": float(np.mean(info["pos_err"] < 1e-3)),
            "stop_normal": float(np.mean(info["stop"] == 0)),
            "joint_jump_lt_0.2": float(np.mean(dq < 0.2)),
            "cold_ms_per_batch": 1e3 * cold["solve_time"],
            "cold_iterations_median": float(np.median(cold["iterations"])),
            "cold_iterations_max": int(cold["iterations"].max())}


def kernel_stats(a):
    """seed_kernel's time under rocprofv3 --kernel-trace --stats (a child process: the profiler wraps a fresh
    interpreter)."""
    prof = shutil.which("rocprofv3")
    if not prof:
        return {"seed_kernel": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="track_prof_")
    cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "r1", "--",
           sys.executable, os.path.abspath(__file__), "--no-rocprof", "--paths", str(a.paths),
           "--waypoints", str(a.waypoints), "--step", str(a.step)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    files = glob.glob(os.path.join(out, "**", "r1_kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return {"seed_kernel": f"rocprofv3 run failed ({r.returncode})"}
    rows = list(csv.DictReader(open(files[0])))
    total = sum(float(x["TotalDurationNs"]) for x in rows)
    seed = [x for x in rows if "seed_kernel" in x["Name"]]
    res = {"kernel_ms_total": total / 1e6}
    if seed:
        calls, ns = int(seed[0]["Calls"]), float(seed[0]["TotalDurationNs"])
        res.update(seed_kernel_calls=calls, seed_kernel_us_avg=ns / calls / 1e3, seed_kernel_share=ns / total)
    shutil.rmtree(out, ignore_errors=True)
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--paths", type=int, default=4096)
    p.add_argument("--waypoints", type=int, default=32)
    p.add_argument("--step", type=float, default=0.02)
    p.add_argument("--no-rocprof", action="store_true")
    a = p.parse_args()
    res = measure(a)
    if not a.no_rocprof:
        res.update(kernel_stats(a))
    print(json.dumps(res))
