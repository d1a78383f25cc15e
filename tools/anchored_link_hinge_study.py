#!/usr/bin/env python3
"""tools/anchored_link_hinge_study.py -- link hinges in the fixed-anchor solve, measured on the device with link_hinges off
and on alternated (a measurement tool; bench.py is the project's yardstick and is not touched by it).  docs/NOTEBOOK.md 22.

    python tools/anchored_link_hinge_study.py [--paths 4096] [--waypoints 32] [--step 0.02] [--reps 3] [--sweep 4]
                                              [--no-rocprof] [--out profiles/anchored_link_hinge_study.json]

The workload, the generator and the seeds of tools/anchored_link_study.py (NOTEBOOK 20): UR10 + table_environment(), the
paths of tools/anchored_tracking_study.py.  The link_hinges=False rows are the code path NOTEBOOK 20 measured.
  (a) cold  : the goals of waypoint 0, AnchoredProblem.solve(T, clearance_mode="links"): converged answers (f < 1e-9), how
              many of them have link clearance < -1e-4, ms per batch; and the batch again with every walk visiting every
              obstacle (debug_flags 128): what an outer iteration costs with and without culling.
  (b) rule  : the same goals with retries=3, clearance_mode="links".
  (c) track : solve_trajectory(..., sweep=S): ms per waypoint, waypoints whose swept clearance is < -1e-4; and, unless
              --no-rocprof, the link_hinges=True run repeated under `rocprofv3 --kernel-trace --stats` in a child process:
              the share of kernel time per kernel.
Prints one JSON line and writes it to --out, with the digest of the library the numbers were taken on.
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
sys.path.insert(0, HERE)

TOL = dict(pos_tol=0.01, rot_tol=0.01, clear_tol=1e-4)


def rng3(t, scale):
    import numpy as np
    return [round(scale * v, 4) for v in (float(np.median(t)), min(t), max(t))]


def scene(link_hinges, params=None):
    from graphik_amd.solvers.riemannian_solver import AnchoredProblem
    from graphik_amd.utils import table_environment
    from graphik_amd.utils.roboturdf import load_ur10
    robot, graph = load_ur10()
    for idx, obs in enumerate(table_environment()):
        graph.add_spherical_obstacle(f"o{idx}", obs[0], obs[1])
    return robot, AnchoredProblem(graph, link_hinges=link_hinges, params=params)


def measure(a):
    import numpy as np
    import torch
    from anchored_tracking_study import paths
    from graphik_amd import _ffi
    from graphik_amd.solvers.riemannian_solver import anchored_retry_failed
    robot, on = scene(True)
    Q, T, kept = paths(robot, on, a.paths, a.waypoints, a.step, a.margin)
    B, L = T.shape[:2]
    if a.child:                                              # under the profiler: the tracked run on the hinge problem alone
        on.solve_trajectory(T[:, :2], Q[:, 0], sweep=a.sweep, clearance_mode="links")
        on.solve_trajectory(T, Q[:, 0], sweep=a.sweep, clearance_mode="links")
        return {}
    _, off = scene(False)
    _, on_full = scene(True, {"debug_flags": 128})
    probs = (("off", off), ("on", on))
    digest = open(_ffi.LIB_PATH + ".digest").read().strip() if os.path.exists(_ffi.LIB_PATH + ".digest") else None
    res = {"workload": "ur10_table_anchored_link_hinges", "paths": B, "waypoints": L, "step_rad": a.step, "margin_m": a.margin,
           "reps": a.reps, "tolerances": TOL, "library_digest": digest, "links": [list(l) for l in on.link_names],
           "link_radius": on.link_radius.tolist(),
           "template_info": {name: {k: int(p.template.info[k]) for k in ("anchored", "lds_bytes", "waves_per_cu")} for name, p in probs}}
    ct = TOL["clear_tol"]

    def timed(fn):
        e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e[0].record()
        r = fn()
        e[1].record()
        torch.cuda.synchronize()
        return r, e[0].elapsed_time(e[1]) * 1e-3

    T0 = T[:, 0]
    for _, p in probs + (("full", on_full),):                # warm-up: library, handles, code objects
        p.solve(T0[:64], retries=1, clearance_mode="links", **TOL)

    # ---- (a) cold answers; the cost of an outer iteration with and without culling
    rows = {name: {"t": []} for name in ("off", "on", "on_no_culling")}
    for _ in range(a.reps):                                  # alternated: all see the same machine
        for name, p in probs + (("on_no_culling", on_full),):
            r, dt = timed(lambda: p.solve(T0, clearance=True, clearance_mode="links"))
            rows[name]["t"].append(dt)
            rows[name]["r"] = r
    res["cold"] = []
    for name, p in probs + (("on_no_culling", on_full),):
        r = rows[name]["r"]
        link = r["clearance"].cpu().numpy()
        node = p.template.anchored_clearance(r["x"]).cpu().numpy()
        conv = r["f"].cpu().numpy() < 1e-9
        its = int(r["iterations"].cpu().numpy().sum())
        stop, pe, re = (r[k].cpu().numpy() for k in ("stop", "pos_err", "rot_err"))
        res["cold"].append({
            "link_hinges": name, "ms_per_batch_median_min_max": rng3(rows[name]["t"], 1e3), "converged": int(conv.sum()),
            "of_them_link_clearance_lt_-1e-4": int((conv & (link < -ct)).sum()),
            "of_them_link_clearance_lt_-1cm": int((conv & (link < -0.01)).sum()),
            "of_them_node_clearance_lt_-1e-4": int((conv & (node < -ct)).sum()),
            "median_depth": float(np.median(-link[conv & (link < -ct)])) if (conv & (link < -ct)).any() else None,
            "fail_the_link_rule": int(anchored_retry_failed(stop, pe, re, link, **TOL).sum()),
            "outer_iterations": its, "inner_iterations": int(r["inner_total"].cpu().numpy().sum()),
            "batch_us_per_outer_iteration": round(float(np.median(rows[name]["t"])) * 1e6 / max(its, 1), 4)})

    # ---- (b) restarts under the link rule
    rows = {name: {"t": []} for name, _ in probs}
    for _ in range(a.reps):
        for name, p in probs:
            r, dt = timed(lambda: p.solve(T0, retries=3, retry_seed=1, clearance_mode="links", **TOL))
            rows[name]["t"].append(dt)
            rows[name]["r"] = r
    res["rule"] = []
    for name, p in probs:
        r = rows[name]["r"]
        link = r["clearance"].cpu().numpy()
        stop, pe, re = (r[k].cpu().numpy() for k in ("stop", "pos_err", "rot_err"))
        conv = r["f"].cpu().numpy() < 1e-9
        att = r["attempt"].cpu().numpy()
        res["rule"].append({
            "link_hinges": name, "retries": 3, "clearance_mode": "links",
            "ms_per_batch_median_min_max": rng3(rows[name]["t"], 1e3), "converged": int(conv.sum()),
            "of_them_link_clearance_lt_-1e-4": int((conv & (link < -ct)).sum()),
            "fail_the_link_rule": int(anchored_retry_failed(stop, pe, re, link, **TOL).sum()),
            "miss_their_pose": int(((stop != 0) | ~(pe <= TOL["pos_tol"]) | ~(re <= TOL["rot_tol"])).sum()),
            "attempt_histogram": np.bincount(att, minlength=4).tolist()})

    # ---- (c) the tracking workload with the sweep
    res["tracked"] = []
    times = {name: [] for name, _ in probs}
    infos = {}
    for _, p in probs:
        p.solve_trajectory(T[:, :2], Q[:, 0], sweep=a.sweep, clearance_mode="links")
    for _ in range(a.reps):
        for name, p in probs:
            q, _, info = p.solve_trajectory(T, Q[:, 0], sweep=a.sweep, clearance_mode="links")
            times[name].append(info["solve_time"])
            infos[name] = info
    for name, _ in probs:
        info = infos[name]
        sw, cl = info["sweep_clearance"], info["clearance"]
        conv = info["f(x)"] < 1e-9
        ok = (info["stop"] == 0) & (info["pos_err"] <= TOL["pos_tol"]) & (info["rot_err"] <= TOL["rot_tol"])
        res["tracked"].append({
            "link_hinges": name, "sweep": a.sweep, "ms_per_waypoint_median_min_max": rng3(times[name], 1e3 / L),
            "waypoints": int(sw.size), "converged": float(conv.mean()), "on_their_pose": float(ok.mean()),
            "link_clearance_lt_-1e-4": int((cl < -ct).sum()), "sweep_clearance_lt_-1e-4": int((sw < -ct).sum()),
            "sweep_clearance_lt_-1cm": int((sw < -0.01).sum()), "min_sweep_clearance": float(np.nanmin(sw)),
            "nan_sweeps": int(np.isnan(sw).sum()), "outer_iterations": int(info["iterations"].sum())})
    return res


def kernel_stats(a):
    """Kernel times of the tracked run on the hinge problem under rocprofv3 --kernel-trace --stats (a child process: the
    profiler wraps a fresh interpreter)."""
    prof = shutil.which("rocprofv3")
    if not prof:
        return {"kernel_shares": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="anch_link_hinge_prof_")
    cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "r1", "--",
           sys.executable, os.path.abspath(__file__), "--child", "--paths", str(a.paths), "--waypoints", str(a.waypoints),
           "--step", str(a.step), "--margin", str(a.margin), "--sweep", str(a.sweep)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    files = glob.glob(os.path.join(out, "**", "r1_kernel_stats.csv"), recursive=True)
    if r.returncode != 0 or not files:
        return {"kernel_shares": f"rocprofv3 run failed ({r.returncode})"}
    rows = list(csv.DictReader(open(files[0])))
    total = sum(float(x["TotalDurationNs"]) for x in rows)
    res = {"kernel_ms_total": total / 1e6, "kernel_share": {}, "kernel_us_avg": {}, "kernel_calls": {}}
    for x in sorted(rows, key=lambda x: -float(x["TotalDurationNs"]))[:10]:
        name = x["Name"].split("(")[0].split("::")[-1]
        res["kernel_share"][name] = round(float(x["TotalDurationNs"]) / total, 6)
        res["kernel_us_avg"][name] = round(float(x["TotalDurationNs"]) / int(x["Calls"]) / 1e3, 2)
        res["kernel_calls"][name] = int(x["Calls"])
    shutil.rmtree(out, ignore_errors=True)
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--paths", type=int, default=4096)
    p.add_argument("--waypoints", type=int, default=32)
    p.add_argument("--step", type=float, default=0.02)
    p.add_argument("--margin", type=float, default=0.05)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--sweep", type=int, default=4)
    p.add_argument("--no-rocprof", action="store_true")
    p.add_argument("--child", action="store_true", help="(internal) the run the profiler wraps")
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "anchored_link_hinge_study.json"))
    a = p.parse_args()
    res = measure(a)
    if not a.child:
        if not a.no_rocprof:
            res.update(kernel_stats(a))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res))
