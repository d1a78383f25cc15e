#!/usr/bin/env python3
"""tools/anchored_self_study.py -- self-collision clearance (link against link) in the fixed-anchor solve, measured on the
device (a measurement tool; bench.py is the project's yardstick and is not touched by it).  docs/NOTEBOOK.md 37.

    python tools/anchored_self_study.py [--paths 4096] [--waypoints 32] [--step 0.02] [--reps 3] [--sweep 4] [--no-rocprof]
                                        [--out profiles/anchored_self_study.json]

UR10 + table_environment() and the paths of tools/anchored_link_study.py (the same generator, the same seed), the
skeleton links as capsules of 3 cm and the ten "auto" pairs.  Nothing here is gated: nobody has measured these numbers.
  (a) blind : the goals of waypoint 0, AnchoredProblem.solve(T) cold: of the converged answers (f < 1e-9), how many
              self-collide (self clearance < -1e-4), how many of those are clear of the table by the link clearance, how deep.
  (b) rule  : the same goals with retries=3, clearance_mode="links" and "links+self", alternated `reps` times: ms per
              batch, how many of (a) are left, how many goals then miss their pose.
  (c) track : solve_trajectory(sweep=S) on all paths in both modes, alternated: ms per waypoint, swept self-collisions;
              and, unless --no-rocprof, the "links+self" run repeated under `rocprofv3 --kernel-trace --stats` in a child
              process: the share of kernel time in the kernel this feature adds.
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
RHO = 0.03
NEW = ("anch_self_clearance_kernel",)
MODES = ("links", "links+self")


def scene():
    from graphik_amd.solvers.riemannian_solver import AnchoredProblem
    from graphik_amd.utils import table_environment
    from graphik_amd.utils.roboturdf import load_ur10
    robot, graph = load_ur10()
    for idx, obs in enumerate(table_environment()):
        graph.add_spherical_obstacle(f"o{idx}", obs[0], obs[1])
    return robot, AnchoredProblem(graph, link_radius=RHO, self_pairs="auto")


def rng3(t, scale):
    import numpy as np
    return [round(scale * v, 4) for v in (float(np.median(t)), min(t), max(t))]


def measure(a):
    import numpy as np
    import torch
    from anchored_tracking_study import paths
    from graphik_amd import _ffi
    robot, ap = scene()
    Q, T, kept = paths(robot, ap, a.paths, a.waypoints, a.step, a.margin)
    B, L = T.shape[:2]
    if a.child:                                              # under the profiler: the tracked run in the new mode alone
        ap.solve_trajectory(T[:, :2], Q[:, 0], sweep=a.sweep, clearance_mode="links+self")
        ap.solve_trajectory(T, Q[:, 0], sweep=a.sweep, clearance_mode="links+self")
        return {}
    digest = open(_ffi.LIB_PATH + ".digest").read().strip() if os.path.exists(_ffi.LIB_PATH + ".digest") else None
    res = {"workload": "ur10_table_anchored_self", "paths": B, "waypoints": L, "step_rad": a.step, "margin_m": a.margin,
           "reps": a.reps, "tolerances": TOL, "library_digest": digest, "links": [list(l) for l in ap.link_names],
           "link_radius": ap.link_radius.tolist(), "self_pairs": ap.self_pairs.tolist()}
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

    # ---- (a) converged cold answers that self-collide
    T0 = T[:, 0]
    ap.solve(T0[:64], retries=1, clearance_mode="links+self", **TOL)      # warm-up: library, handles, code objects
    r0 = ap.solve(T0, clearance=True, clearance_mode="links")
    link0 = r0["clearance"].cpu().numpy()
    self0 = tpl.anchored_self_clearance(r0["x"]).cpu().numpy()
    conv0 = r0["f"].cpu().numpy() < 1e-9
    blind = conv0 & (self0 < -ct)
    res["blind"] = {"converged": int(conv0.sum()), "of_them_self_colliding": int(blind.sum()),
                    "share": float(blind.sum() / max(conv0.sum(), 1)),
                    "self_colliding_and_link_clear": int((blind & (link0 >= -ct)).sum()),
                    "deeper_than_1cm": int((conv0 & (self0 < -0.01)).sum()),
                    "deepest_self_clearance": float(self0[blind].min()) if blind.any() else None,
                    "median_depth": float(np.median(-self0[blind])) if blind.any() else None}

    # ---- (b) restarts under either rule
    rows = {mode: {"t": []} for mode in MODES}
    for _ in range(a.reps):                                  # alternated: both see the same machine
        for mode in MODES:
            r, dt = timed(lambda: ap.solve(T0, retries=3, retry_seed=1, clearance_mode=mode, **TOL))
            rows[mode]["t"].append(dt)
            rows[mode]["r"] = r
    res["rule"] = []
    for mode in MODES:
        r = rows[mode]["r"]
        link = tpl.anchored_link_clearance(r["x"]).cpu().numpy()
        own = tpl.anchored_self_clearance(r["x"]).cpu().numpy()
        stop, pe, re = (r[k].cpu().numpy() for k in ("stop", "pos_err", "rot_err"))
        att = r["attempt"].cpu().numpy()
        off_pose = (stop != 0) | ~(pe <= TOL["pos_tol"]) | ~(re <= TOL["rot_tol"])
        res["rule"].append({
            "clearance_mode": mode, "retries": 3, "ms_per_batch_median_min_max": rng3(rows[mode]["t"], 1e3),
            "self_colliding": int((own < -ct).sum()), "link_colliding": int((link < -ct).sum()),
            "of_the_blind_goals_still_self_colliding": int((blind & (own < -ct)).sum()),
            "of_the_blind_goals_replaced": int((blind & (att > 0)).sum()),
            "miss_their_pose": int(off_pose.sum()), "of_the_blind_goals_miss_their_pose": int((blind & off_pose).sum()),
            "attempt_histogram": np.bincount(att, minlength=4).tolist()})

    # ---- (c) the tracking workload with the sweep, in either mode
    track = {mode: {"t": []} for mode in MODES}
    ap.solve_trajectory(T[:, :2], Q[:, 0], sweep=a.sweep, clearance_mode="links+self")
    for _ in range(a.reps):
        for mode in MODES:
            q, _, info = ap.solve_trajectory(T, Q[:, 0], sweep=a.sweep, clearance_mode=mode)
            track[mode]["t"].append(info["solve_time"])
            track[mode]["info"] = info
    info = track["links+self"]["info"]
    sw = info["sweep_self_clearance"]
    res["tracked"] = {"sweep": a.sweep, "waypoints": int(sw.size),
                      "ms_per_waypoint_links_median_min_max": rng3(track["links"]["t"], 1e3 / L),
                      "ms_per_waypoint_links_self_median_min_max": rng3(track["links+self"]["t"], 1e3 / L),
                      "converged": float((info["f(x)"] < 1e-9).mean()),
                      "waypoints_link_or_self_colliding": int((info["clearance"] < -ct).sum()),
                      "sweep_self_clearance_lt_-1e-4": int((sw < -ct).sum()), "sweep_self_clearance_lt_-1cm": int((sw < -0.01).sum()),
                      "min_sweep_self_clearance": float(np.nanmin(sw)), "nan_sweeps": int(np.isnan(sw).sum()),
                      "same_link_sweep_in_both_modes": bool(np.array_equal(info["sweep_clearance"],
                                                                           track["links"]["info"]["sweep_clearance"]))}
    return res


def kernel_stats(a):
    """Kernel times of the tracked "links+self" run under rocprofv3 --kernel-trace --stats (a child process: the profiler
    wraps a fresh interpreter)."""
    prof = shutil.which("rocprofv3")
    if not prof:
        return {"kernel_shares": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="anch_self_prof_")
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
    res["new_kernels_calls"] = sum(int(x["Calls"]) for x in new)
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
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "anchored_self_study.json"))
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
