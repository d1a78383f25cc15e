#!/usr/bin/env python3
"""tools/anchored_self_hinge_study.py -- self hinges in the fixed-anchor solve, measured on the device with self_hinges off
and on alternated (a measurement tool; bench.py is the project's yardstick and is not touched by it).  docs/NOTEBOOK.md 39.

    python tools/anchored_self_hinge_study.py [--goals 4096] [--waypoints 32] [--step 0.02] [--reps 3] [--sweep 4]
                                              [--robots kuka,ur10] [--out profiles/anchored_self_hinge_study.json]

Per robot (KUKA, and UR10 for comparison with NOTEBOOK 37's table) + table_environment(), the skeleton as capsules of 3 cm,
the "auto" pairs (15 / 10), `goals` goals; the paths are those of tools/anchored_tracking_study.py (its generator and seed).
Nothing here is gated.
  (a) cold  : the goals of waypoint 0, AnchoredProblem.solve(T, clearance_mode="links+self"): ms per batch, converged
              answers (f < 1e-9), of them self-colliding (self clearance < -1e-4) and deeper than 1 cm.
  (b) rule  : the same goals with retries=3, clearance_mode="links+self".
  (c) track : solve_trajectory(sweep=S) on goals x waypoints: swept self-collisions with hinges on against off -- the
              ones restarts cannot touch.
  (d) price : ms per batch of the self build with link_radius = 0 (no pair can be active) against the plain anchored build
              on the same goals: what the pass costs when nothing is active, against the parent's kernel.
Prints one JSON line and writes it to --out, with the digest of the library the numbers were taken on.
"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

TOL = dict(pos_tol=0.01, rot_tol=0.01, clear_tol=1e-4)
RHO = 0.03
MODE = "links+self"


def rng3(t, scale):
    import numpy as np
    return [round(scale * v, 4) for v in (float(np.median(t)), min(t), max(t))]


def scene(name, self_hinges, rho=RHO, self_pairs="auto"):
    from graphik_amd.solvers.riemannian_solver import AnchoredProblem
    from graphik_amd.utils import table_environment
    from graphik_amd.utils.roboturdf import load_kuka, load_ur10
    robot, graph = {"kuka": load_kuka, "ur10": load_ur10}[name]()
    for idx, obs in enumerate(table_environment()):
        graph.add_spherical_obstacle(f"o{idx}", obs[0], obs[1])
    return robot, AnchoredProblem(graph, link_radius=rho, self_pairs=self_pairs, self_hinges=self_hinges)


def measure_robot(name, a):
    import numpy as np
    import torch
    from anchored_tracking_study import paths
    robot, on = scene(name, True)
    _, off = scene(name, False)
    _, zero_on = scene(name, True, rho=0.0)
    _, plain = scene(name, False, rho=0.0, self_pairs=None)
    Q, T, kept = paths(robot, on, a.goals, a.waypoints, a.step, a.margin)
    B, L = T.shape[:2]
    probs = (("off", off), ("on", on))
    ct = TOL["clear_tol"]
    res = {"robot": name, "goals": B, "waypoints": L, "pairs": int(len(on.self_pairs)), "link_radius": RHO,
           "template_info": {n: {k: int(p.template.info[k]) for k in ("anchored", "lds_bytes", "waves_per_cu")}
                             for n, p in probs + (("zero_radius_on", zero_on), ("plain", plain))}}

    def timed(fn):
        e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e[0].record()
        r = fn()
        e[1].record()
        torch.cuda.synchronize()
        return r, e[0].elapsed_time(e[1]) * 1e-3

    T0 = T[:, 0]
    for p in (off, on, zero_on, plain):                      # warm-up: library, handles, code objects
        p.solve(T0[:64], clearance=True)

    def self_depth(p, r):
        return p.template.anchored_self_clearance(r["x"]).cpu().numpy()

    # ---- (a) cold, (b) the rule
    for key, kw in (("cold", dict(clearance=True, clearance_mode=MODE)), ("rule", dict(retries=3, retry_seed=1, clearance_mode=MODE, **TOL))):
        rows = {n: {"t": []} for n, _ in probs}
        for _ in range(a.reps):                              # alternated: both see the same machine
            for n, p in probs:
                r, dt = timed(lambda: p.solve(T0, **kw))
                rows[n]["t"].append(dt)
                rows[n]["r"] = r
        res[key] = []
        for n, p in probs:
            r = rows[n]["r"]
            sc = self_depth(p, r)
            conv = r["f"].cpu().numpy() < 1e-9
            stop, pe, re = (r[k].cpu().numpy() for k in ("stop", "pos_err", "rot_err"))
            row = {"self_hinges": n, "ms_per_batch_median_min_max": rng3(rows[n]["t"], 1e3), "converged": int(conv.sum()),
                   "of_them_self_colliding": int((conv & (sc < -ct)).sum()), "of_them_deeper_than_1cm": int((conv & (sc < -0.01)).sum()),
                   "self_colliding_of_all": int((sc < -ct).sum()),
                   "miss_their_pose": int(((stop != 0) | ~(pe <= TOL["pos_tol"]) | ~(re <= TOL["rot_tol"])).sum()),
                   "outer_iterations": int(r["iterations"].cpu().numpy().sum())}
            if "attempt" in r:
                row["attempt_histogram"] = np.bincount(r["attempt"].cpu().numpy(), minlength=4).tolist()
            res[key].append(row)

    # ---- (c) the tracking workload with the sweep
    res["tracked"] = []
    times, infos = {n: [] for n, _ in probs}, {}
    for _, p in probs:
        p.solve_trajectory(T[:, :2], Q[:, 0], sweep=a.sweep, clearance_mode=MODE)
    for _ in range(a.reps):
        for n, p in probs:
            q, _, info = p.solve_trajectory(T, Q[:, 0], sweep=a.sweep, clearance_mode=MODE)
            times[n].append(info["solve_time"])
            infos[n] = info
    for n, _ in probs:
        info = infos[n]
        sw = info["sweep_self_clearance"]
        ok = (info["stop"] == 0) & (info["pos_err"] <= TOL["pos_tol"]) & (info["rot_err"] <= TOL["rot_tol"])
        res["tracked"].append({"self_hinges": n, "sweep": a.sweep, "ms_per_waypoint_median_min_max": rng3(times[n], 1e3 / L),
                               "waypoints": int(sw.size), "converged": float((info["f(x)"] < 1e-9).mean()), "on_their_pose": float(ok.mean()),
                               "swept_self_collisions": int((sw < -ct).sum()), "deeper_than_1cm": int((sw < -0.01).sum()),
                               "min_sweep_self_clearance": float(np.nanmin(sw)), "outer_iterations": int(info["iterations"].sum())})

    # ---- (d) the price of the pass with nothing active
    rows = {"plain": [], "zero_radius_on": []}
    its = {}
    for _ in range(a.reps):
        for n, p in (("plain", plain), ("zero_radius_on", zero_on)):
            r, dt = timed(lambda: p.solve(T0))
            rows[n].append(dt)
            its[n] = (int(r["iterations"].cpu().numpy().sum()), r["x"].cpu().numpy())
    res["price_inactive"] = {n: rng3(t, 1e3) for n, t in rows.items()}
    res["price_inactive"]["ratio_of_medians"] = round(float(np.median(rows["zero_radius_on"]) / np.median(rows["plain"])), 4)
    res["price_inactive"]["same_answers"] = bool(its["plain"][0] == its["zero_radius_on"][0] and np.array_equal(its["plain"][1], its["zero_radius_on"][1]))
    res["price_inactive"]["outer_iterations"] = its["plain"][0]
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--goals", type=int, default=4096)
    p.add_argument("--waypoints", type=int, default=32)
    p.add_argument("--step", type=float, default=0.02)
    p.add_argument("--margin", type=float, default=0.05)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--sweep", type=int, default=4)
    p.add_argument("--robots", default="kuka,ur10")
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "anchored_self_hinge_study.json"))
    a = p.parse_args()
    from graphik_amd import _ffi
    digest = open(_ffi.LIB_PATH + ".digest").read().strip() if os.path.exists(_ffi.LIB_PATH + ".digest") else None
    res = {"workload": "table_anchored_self_hinges", "reps": a.reps, "tolerances": TOL, "step_rad": a.step, "margin_m": a.margin,
           "library_digest": digest, "robots": [measure_robot(name, a) for name in a.robots.split(",")]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
