#!/usr/bin/env python3
"""tools/anchored_link_study.py -- clearance of whole links in the fixed-anchor solve, measured on the device (a
measurement tool; bench.py is the project's yardstick and is not touched by it).  docs/NOTEBOOK.md 20.

    python tools/anchored_link_study.py [--paths 4096] [--waypoints 32] [--step 0.02] [--reps 3] [--sweep 4] [--no-rocprof]
                                        [--out profiles/anchored_link_study.json]

UR10 + table_environment() and the paths of tools/anchored_tracking_study.py (the same generator, the same seed).
  (a) blind : the 4096 goals of waypoint 0, AnchoredProblem.solve(T) cold: of the converged answers (f < 1e-9) whose
              joint points are clear (node clearance >= -1e-4), the share with a link inside a sphere (link clearance
              < -1e-4), and how deep.
  (b) rule  : the same goals with retries=3, clearance_mode="nodes" and "links", alternated `reps` times: what the link
              rule leaves of (a)'s answers, how many goals fail each rule after the restarts, ms per batch.
  (c) share : solve_trajectory on all paths with sweep=S and without, alternated: ms per waypoint, the swept clearance
              between waypoints; and, unless --no-rocprof, the sweep run repeated under `rocprofv3 --kernel-trace --stats`
              in a child process: the share of kernel time in the kernels this feature adds.
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
NEW = ("anch_link_clearance_kernel", "anch_sweep_interp_kernel", "anch_sweep_min_kernel")


def rng3(t, scale):
    import numpy as np
    return [round(scale * v, 4) for v in (float(np.median(t)), min(t), max(t))]


def measure(a):
    import numpy as np
    import torch
    from anchored_tracking_study import paths, scene
    from graphik_amd import _ffi
    from graphik_amd.solvers.riemannian_solver import anchored_retry_failed
    robot, ap = scene()
    Q, T, kept = paths(robot, ap, a.paths, a.waypoints, a.step, a.margin)
    B, L = T.shape[:2]
    if a.child:                                              # under the profiler: the tracked run with the sweep alone
        ap.solve_trajectory(T[:, :2], Q[:, 0], sweep=a.sweep)
        ap.solve_trajectory(T, Q[:, 0], sweep=a.sweep)
        return {}
    digest = open(_ffi.LIB_PATH + ".digest").read().strip() if os.path.exists(_ffi.LIB_PATH + ".digest") else None
    res = {"workload": "ur10_table_anchored_links", "paths": B, "waypoints": L, "step_rad": a.step, "margin_m": a.margin,
           "reps": a.reps, "tolerances": TOL, "library_digest": digest, "links": [list(l) for l in ap.link_names],
           "link_radius": ap.link_radius.tolist()}
    tpl = ap.template
    ct = TOL["clear_tol"]

    def timed(fn):
        e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e[0].record()
        r = fn()
        e[1].record()
        torch.cuda.synchronize()
        return r, e[0].elapsed_time(e[1]) * 1e-3

    # ---- (a) what the node clearance misses on converged cold answers
    T0 = T[:, 0]
    ap.solve(T0[:64], retries=1, clearance_mode="links", **TOL)      # warm-up: library, handles, code objects
    r0 = ap.solve(T0, clearance=True)
    node0 = r0["clearance"].cpu().numpy()
    link0 = tpl.anchored_link_clearance(r0["x"]).cpu().numpy()
    conv0 = r0["f"].cpu().numpy() < 1e-9
    called_free = conv0 & (node0 >= -ct)
    blind = called_free & (link0 < -ct)
    res["blind"] = {"converged": int(conv0.sum()), "converged_and_node_clear": int(called_free.sum()),
                    "of_them_link_colliding": int(blind.sum()), "share": float(blind.sum() / max(called_free.sum(), 1)),
                    "deeper_than_1cm": int((called_free & (link0 < -0.01)).sum()),
                    "deepest_link_clearance": float(link0[blind].min()) if blind.any() else None,
                    "median_depth": float(np.median(-link0[blind])) if blind.any() else None}

    # ---- (b) restarts under either rule
    rows = {"nodes": {"t": []}, "links": {"t": []}}
    for _ in range(a.reps):                                  # alternated: both see the same machine
        for mode in ("nodes", "links"):
            r, dt = timed(lambda: ap.solve(T0, retries=3, retry_seed=1, clearance_mode=mode, **TOL))
            rows[mode]["t"].append(dt)
            rows[mode]["r"] = r
    res["rule"] = []
    for mode in ("nodes", "links"):
        r = rows[mode]["r"]
        node = tpl.anchored_clearance(r["x"]).cpu().numpy()
        link = tpl.anchored_link_clearance(r["x"]).cpu().numpy()
        stop, pe, re = (r[k].cpu().numpy() for k in ("stop", "pos_err", "rot_err"))
        conv = r["f"].cpu().numpy() < 1e-9
        att = r["attempt"].cpu().numpy()
        free = conv & (node >= -ct)
        res["rule"].append({
            "clearance_mode": mode, "retries": 3, "ms_per_batch_median_min_max": rng3(rows[mode]["t"], 1e3),
            "converged": int(conv.sum()), "converged_and_node_clear": int(free.sum()),
            "of_them_link_colliding": int((free & (link < -ct)).sum()),
            "of_the_blind_goals_still_link_colliding": int((blind & (link < -ct)).sum()),
            "of_the_blind_goals_replaced": int((blind & (att > 0)).sum()),
            "fail_the_node_rule": int(anchored_retry_failed(stop, pe, re, node, **TOL).sum()),
            "fail_the_link_rule": int(anchored_retry_failed(stop, pe, re, link, **TOL).sum()),
            "attempt_histogram": np.bincount(att, minlength=4).tolist()})

    # ---- (c) the tracking workload with and without the sweep
    ap.solve_trajectory(T[:, :2], Q[:, 0], sweep=a.sweep)
    t_plain, t_sweep = [], []
    for _ in range(a.reps):
        q, _, info = ap.solve_trajectory(T, Q[:, 0])
        t_plain.append(info["solve_time"])
        q, _, info = ap.solve_trajectory(T, Q[:, 0], sweep=a.sweep)
        t_sweep.append(info["solve_time"])
    sw, cl = info["sweep_clearance"], info["clearance"]
    conv = info["f(x)"] < 1e-9
    res["tracked"] = {"sweep": a.sweep, "ms_per_waypoint_plain_median_min_max": rng3(t_plain, 1e3 / L),
                      "ms_per_waypoint_sweep_median_min_max": rng3(t_sweep, 1e3 / L),
                      "waypoints": int(sw.size), "converged": float(conv.mean()),
                      "node_clearance_ge_-1e-4": float((cl >= -ct).mean()),
                      "sweep_clearance_lt_-1e-4": int((sw < -ct).sum()), "sweep_clearance_lt_-1cm": int((sw < -0.01).sum()),
                      "min_sweep_clearance": float(np.nanmin(sw)), "nan_sweeps": int(np.isnan(sw).sum())}
    return res


def kernel_stats(a):
    """Kernel times of the tracked run with the sweep under rocprofv3 --kernel-trace --stats (a child process: the
    profiler wraps a fresh interpreter)."""
    prof = shutil.which("rocprofv3")
    if not prof:
        return {"kernel_shares": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="anch_link_prof_")
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
    new = [x for x in rows if any(g in x["Name"] for g in NEW)]
    res["new_kernels_found"] = sorted({g for g in NEW for x in new if g in x["Name"]})
    res["new_kernels_share"] = sum(float(x["TotalDurationNs"]) for x in new) / total
    res["new_kernels_us_avg"] = {g: round(sum(float(x["TotalDurationNs"]) for x in new if g in x["Name"]) /
                                          max(sum(int(x["Calls"]) for x in new if g in x["Name"]), 1) / 1e3, 2) for g in NEW}
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
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "anchored_link_study.json"))
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
