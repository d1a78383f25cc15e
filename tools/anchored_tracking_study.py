#!/usr/bin/env python3
"""tools/anchored_tracking_study.py -- path tracking among obstacles through the fixed-anchor solve, measured on the
device (a measurement tool; bench.py is the project's yardstick and is not touched by it).  docs/NOTEBOOK.md 17.

    python tools/anchored_tracking_study.py [--paths 4096] [--waypoints 32] [--step 0.02] [--reps 3] [--no-rocprof]

UR10 + table_environment(), `paths` trajectories of `waypoints` goal poses, every joint moving `step` rad per waypoint
(a random sign per path and joint, from a random start inside 60 % of the joint range); only paths whose p-nodes
p1 .. p5 stay more than `margin` outside every sphere at every waypoint are kept.  Two ways to solve the same goals,
alternated `reps` times in one process, each timed by the host clock around work that ends in a synchronise:
  tracked : AnchoredProblem.solve_trajectory -- waypoint 0 seeded by the start configuration, waypoint l by the answer
            of waypoint l - 1 (gik_anchored_ik_batch_seeded with the clearance), all on the device;
  cold    : gik_anchored_ik_batch per waypoint (bound smoothing + MDS start), buffers and poses resident as above.
Prints one JSON line: ms per waypoint (median and range over the repetitions), outer iterations, the share of
waypoints converged (f < 1e-9), clearances.  Unless --no-rocprof the tracked run is repeated under
`rocprofv3 --kernel-trace --stats` in a child process and the share of kernel time in seed_kernel +
anch_scatter_kernel + anch_clearance_kernel is added.
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
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)

GLUE = ("seed_kernel", "anch_scatter_kernel", "anch_clearance_kernel")


def scene():
    from graphik_amd.solvers.riemannian_solver import AnchoredProblem
    from graphik_amd.utils import table_environment
    from graphik_amd.utils.roboturdf import load_ur10
    robot, graph = load_ur10()
    for idx, obs in enumerate(table_environment()):
        graph.add_spherical_obstacle(f"o{idx}", obs[0], obs[1])
    return robot, AnchoredProblem(graph)


def fk_clearance(robot, ap, Q, chunk=16384):
    """min over (p1 .. p_{n-1}, sphere) of |p - centre| - radius of the configurations Q [M, n]."""
    import numpy as np
    C, r = ap.obstacles[:, :3], ap.obstacles[:, 3]
    out = np.empty(len(Q))
    for s in range(0, len(Q), chunk):
        q = Q[s:s + chunk]
        P = np.stack([robot.fk_batch(q, i)[:, :3, 3] for i in range(1, robot.n)], axis=1).reshape(-1, 3)
        d2 = (P * P).sum(1)[:, None] + (C * C).sum(1)[None] - 2.0 * P @ C.T
        out[s:s + chunk] = (np.sqrt(np.maximum(d2, 0.0)) - r[None]).reshape(len(q), -1).min(axis=1)
    return out


def paths(robot, ap, B, L, step, margin, seed=21):
    import numpy as np
    rng = np.random.RandomState(seed)
    lb, ub = robot.limits_arrays()
    kept, drawn = [], 0
    while sum(len(k) for k in kept) < B:
        q0 = rng.uniform(0.6 * lb, 0.6 * ub, size=(B, robot.n))
        sign = rng.choice([-1.0, 1.0], size=(B, robot.n))
        Q = q0[:, None] + step * sign[:, None] * np.arange(L)[None, :, None]
        ok = fk_clearance(robot, ap, Q.reshape(-1, robot.n)).reshape(B, L).min(axis=1) > margin
        kept.append(Q[ok])
        drawn += B
    Q = np.concatenate(kept)[:B]
    return Q, robot.fk_batch(Q.reshape(-1, robot.n)).reshape(B, L, 4, 4), sum(len(k) for k in kept) / drawn


def cold_run(ap, Tw, out):
    """One gik_anchored_ik_batch per waypoint into resident buffers; (seconds, f [L,B], iterations [L,B], Y of each)."""
    import torch
    tpl, base = ap.template, ap.base.template
    f, its, clear = [], [], []
    torch.cuda.synchronize()
    t0 = time.time()
    for l in range(len(Tw)):
        r = tpl.anchored_ik(base, Tw[l], out=out[l], clearance=True)
        f.append(r["f"]), its.append(r["iterations"]), clear.append(r["clearance"])
    torch.cuda.synchronize()
    dt = time.time() - t0
    return dt, torch.stack(f).cpu().numpy(), torch.stack(its).cpu().numpy(), torch.stack(clear).cpu().numpy()


def measure(a):
    import numpy as np
    import torch
    robot, ap = scene()
    Q, T, kept = paths(robot, ap, a.paths, a.waypoints, a.step, a.margin)
    B, L = T.shape[:2]
    tpl, base = ap.template, ap.base.template
    Tw = torch.from_numpy(np.ascontiguousarray(np.swapaxes(T, 0, 1))).to(tpl.device)
    out = [tpl.alloc_anchored_buffers(base, B, clearance=True) for _ in range(L)]
    for o in out[1:]:
        o["ws"] = out[0]["ws"]
    ap.solve_trajectory(T[:, :2], Q[:, 0])                  # warm-up: library, handles, code objects
    cold_run(ap, Tw[:2], out)
    if a.child:                                             # under the profiler: the tracked run alone
        ap.solve_trajectory(T, Q[:, 0])
        return {}
    t_track, t_cold = [], []
    for _ in range(a.reps):                                 # alternated: both see the same machine
        q, _, info = ap.solve_trajectory(T, Q[:, 0])
        t_track.append(info["solve_time"])
        dt, f_c, its_c, clear_c = cold_run(ap, Tw, out)
        t_cold.append(dt)
    conv, conv_c = info["f(x)"] < 1e-9, f_c < 1e-9
    dq = np.abs(np.mod(q[:, 1:] - q[:, :-1] + np.pi, 2 * np.pi) - np.pi).max(axis=2)
    ms = lambda t: [round(1e3 * v / L, 4) for v in (np.median(t), min(t), max(t))]      # noqa: E731
    return {"workload": "ur10_table_anchored_track", "paths": B, "waypoints": L, "step_rad": a.step, "margin_m": a.margin,
            "candidates_kept": round(kept, 4), "reps": a.reps,
            "tracked_ms_per_waypoint_median_min_max": ms(t_track),
            "tracked_waypoint_solves_per_s": B * L / float(np.median(t_track)),
            "tracked_iterations_median": float(np.median(info["iterations"])), "tracked_iterations_max": int(info["iterations"].max()),
            "tracked_converged": float(conv.mean()),
            "tracked_min_clearance_converged": float(info["clearance"][conv].min()),
            "tracked_min_clearance_all": float(np.nanmin(info["clearance"])),
            "tracked_pos_err_lt_1e-3": float(np.mean(info["pos_err"] < 1e-3)),
            "tracked_joint_jump_lt_0.2": float(np.mean(dq < 0.2)),
            "cold_ms_per_waypoint_median_min_max": ms(t_cold),
            "cold_iterations_median": float(np.median(its_c)), "cold_iterations_max": int(its_c.max()),
            "cold_converged": float(conv_c.mean()),
            "cold_min_clearance_converged": float(clear_c[conv_c].min())}


def kernel_stats(a):
    """Kernel times of the tracked run under rocprofv3 --kernel-trace --stats (a child process: the profiler wraps a
    fresh interpreter)."""
    prof = shutil.which("rocprofv3")
    if not prof:
        return {"kernel_shares": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="anch_track_prof_")
    cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "r1", "--",
           sys.executable, os.path.abspath(__file__), "--child", "--paths", str(a.paths),
           "--waypoints", str(a.waypoints), "--step", str(a.step), "--margin", str(a.margin)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    files = glob.glob(os.path.join(out, "**", "r1_kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return {"kernel_shares": f"rocprofv3 run failed ({r.returncode})"}
    rows = list(csv.DictReader(open(files[0])))
    total = sum(float(x["TotalDurationNs"]) for x in rows)
    res = {"kernel_ms_total": total / 1e6, "kernel_share": {}, "kernel_us_avg": {}}
    for x in sorted(rows, key=lambda x: -float(x["TotalDurationNs"]))[:8]:
        name = x["Name"].split("(")[0].split("::")[-1]
        res["kernel_share"][name] = round(float(x["TotalDurationNs"]) / total, 5)
        res["kernel_us_avg"][name] = round(float(x["TotalDurationNs"]) / int(x["Calls"]) / 1e3, 2)
    glue = [x for x in rows if any(g in x["Name"] for g in GLUE)]
    res["glue_kernels_found"] = sorted({g for g in GLUE for x in glue if g in x["Name"]})
    res["glue_share"] = sum(float(x["TotalDurationNs"]) for x in glue) / total
    res["glue_us_avg"] = {g: round(sum(float(x["TotalDurationNs"]) for x in glue if g in x["Name"]) /
                                   max(sum(int(x["Calls"]) for x in glue if g in x["Name"]), 1) / 1e3, 2) for g in GLUE}
    shutil.rmtree(out, ignore_errors=True)
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--paths", type=int, default=4096)
    p.add_argument("--waypoints", type=int, default=32)
    p.add_argument("--step", type=float, default=0.02)
    p.add_argument("--margin", type=float, default=0.05)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--no-rocprof", action="store_true")
    p.add_argument("--child", action="store_true", help="(internal) the run the profiler wraps")
    a = p.parse_args()
    res = measure(a)
    if not a.child:
        if not a.no_rocprof:
            res.update(kernel_stats(a))
        print(json.dumps(res))
