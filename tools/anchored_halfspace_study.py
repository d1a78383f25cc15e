#!/usr/bin/env python3
"""tools/anchored_halfspace_study.py -- half-space obstacles (a floor) in the fixed-anchor solve, measured on the device with
halfspaces off and on alternated (a measurement tool; bench.py is the project's yardstick and is not touched by it).
docs/NOTEBOOK.md 42.

    python tools/anchored_halfspace_study.py [--goals 4096] [--waypoints 8] [--step 0.02] [--reps 3] [--robots ur10,kuka]
                                             [--off-only] [--parent parent.json] [--out profiles/anchored_halfspace_study.json]

Per robot (UR10, KUKA), without obstacles and with table_environment(), the skeleton as capsules of 3 cm, a floor at
z = -0.1 with the default margins (the radius at every masked node), `goals` goals; the paths are those of
tools/anchored_tracking_study.py (its generator and seed).  Nothing here is gated.
  (a) cold  : the goals of waypoint 0, AnchoredProblem.solve(T, clearance_mode="links"), retries 0 and 3: ms per batch,
              converged answers (f < 1e-9), of them with a joint point / a link's capsule more than 1e-4 below the floor
              (plain numpy on the answer's point matrix, the same for both problems).
  (b) track : solve_trajectory on goals x waypoints, retries 0 and 3: waypoints per second, the same counts per waypoint.
  (c) price : ms per batch of the half-space build with a floor at z = -10 (never active) against the build without
              half-spaces on the same goals, and whether the answers are the same numbers.
--off-only measures the problems without half-spaces alone and touches no keyword this commit adds: run on the parent
commit it gives the figures `--parent` compares this commit's `off` rows with.
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
FLOOR = (0.0, 0.0, 1.0, -0.1)
MODE = "links"


def rng3(t, scale):
    import numpy as np
    return [round(scale * v, 4) for v in (float(np.median(t)), min(t), max(t))]


def scene(name, table, planes=None, margin=None):
    from graphik_amd.solvers.riemannian_solver import AnchoredProblem
    from graphik_amd.utils import table_environment
    from graphik_amd.utils.roboturdf import load_kuka, load_ur10
    robot, graph = {"kuka": load_kuka, "ur10": load_ur10}[name]()
    if table:
        for idx, obs in enumerate(table_environment()):
            graph.add_spherical_obstacle(f"o{idx}", obs[0], obs[1])
    kw = {} if planes is None else dict(halfspaces=[list(p) for p in planes], halfspace_margin=margin)
    return robot, AnchoredProblem(graph, link_radius=RHO, **kw)


def below_floor(Y_full, ap):
    """Per point matrix (numpy [B, N, 3]): (a joint point p1 .. p(n-1) below the floor, a link's capsule below it), in
    plain numpy, so that it also runs where the library has no half-space kernel."""
    import numpy as np
    g = ap.base.graph
    z = Y_full[:, [g.index(f"p{i}") for i in range(1, ap.robot.n)], 2]
    ends = Y_full[:, np.asarray(ap.link_rows).reshape(-1), 2]
    ct = TOL["clear_tol"]
    return (z.min(axis=1) - FLOOR[3]) < -ct, (ends.min(axis=1) - FLOOR[3] - RHO) < -ct


_PATHS = {}


def measure(name, table, a):
    import numpy as np
    import torch
    from anchored_tracking_study import paths
    robot, off = scene(name, table)
    probs = [("off", off)]
    if not a.off_only:
        probs.append(("on", scene(name, table, (FLOOR,))[1]))
        far = scene(name, table, ((0.0, 0.0, 1.0, -10.0),))[1]
    if name not in _PATHS:      # (the generator keeps paths that clear the table: drawn on the table scene, used on both)
        assert table, "the table scene of a robot is measured first"
        _PATHS[name] = paths(robot, off, a.goals, a.waypoints, a.step, a.margin)
    Q, T, kept = _PATHS[name]
    B, L = T.shape[:2]
    res = {"robot": name, "table": bool(table), "goals": B, "waypoints": L, "link_radius": RHO, "floor": list(FLOOR),
           "template_info": {n: {k: int(p.template.info[k]) for k in ("anchored", "lds_bytes", "waves_per_cu")} for n, p in probs}}

    def timed(fn):
        e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e[0].record()
        r = fn()
        e[1].record()
        torch.cuda.synchronize()
        return r, e[0].elapsed_time(e[1]) * 1e-3

    T0 = T[:, 0]
    for _, p in probs:                                       # warm-up: library, handles, code objects
        p.solve(T0[:64], retries=1, clearance_mode=MODE, **TOL)

    # ---- (a) cold, retries 0 and 3
    res["cold"] = []
    for retries in (0, 3):
        kw = dict(clearance=True, clearance_mode=MODE) if not retries else dict(retries=3, retry_seed=1, clearance_mode=MODE, **TOL)
        rows = {n: {"t": []} for n, _ in probs}
        for _ in range(a.reps):                              # alternated: both see the same machine
            for n, p in probs:
                r, dt = timed(lambda: p.solve(T0, **kw))
                rows[n]["t"].append(dt)
                rows[n]["r"] = r
        for n, p in probs:
            r = rows[n]["r"]
            node, link = below_floor(r["x"].cpu().numpy(), p)
            conv = r["f"].cpu().numpy() < 1e-9
            stop, pe, re = (r[k].cpu().numpy() for k in ("stop", "pos_err", "rot_err"))
            row = {"halfspaces": n, "retries": retries, "ms_per_batch_median_min_max": rng3(rows[n]["t"], 1e3),
                   "converged": int(conv.sum()), "of_them_joint_point_below_floor": int((conv & node).sum()),
                   "of_them_link_below_floor": int((conv & link).sum()), "link_below_floor_of_all": int(link.sum()),
                   "miss_their_pose": int(((stop != 0) | ~(pe <= TOL["pos_tol"]) | ~(re <= TOL["rot_tol"])).sum()),
                   "outer_iterations": int(r["iterations"].cpu().numpy().sum())}
            if "attempt" in r:
                row["attempt_histogram"] = np.bincount(r["attempt"].cpu().numpy(), minlength=4).tolist()
            res["cold"].append(row)

    # ---- (b) tracked, retries 0 and 3
    res["tracked"] = []
    for _, p in probs:
        p.solve_trajectory(T[:, :2], Q[:, 0], clearance_mode=MODE)
    for retries in (0, 3):
        kw = {} if not retries else dict(retries=3, retry_seed=1, retry_spread=0.5, **TOL)
        times, infos = {n: [] for n, _ in probs}, {}
        for _ in range(a.reps):
            for n, p in probs:
                q, Y, info = p.solve_trajectory(T, Q[:, 0], clearance_mode=MODE, return_Y=True, **kw)
                times[n].append(info["solve_time"])
                infos[n] = (info, np.asarray(Y))
        for n, p in probs:
            info, Y = infos[n]
            node, link = below_floor(Y.reshape(B * L, -1, 3), p)
            conv = (info["f(x)"] < 1e-9).reshape(-1)
            ok = (info["stop"] == 0) & (info["pos_err"] <= TOL["pos_tol"]) & (info["rot_err"] <= TOL["rot_tol"])
            res["tracked"].append({"halfspaces": n, "retries": retries, "ms_per_waypoint_median_min_max": rng3(times[n], 1e3 / L),
                                   "waypoints_per_s": round(B * L / float(np.median(times[n])), 1), "waypoints": int(B * L),
                                   "converged": int(conv.sum()), "on_their_pose": float(ok.mean()),
                                   "of_the_converged_joint_point_below_floor": int((conv & node).sum()),
                                   "of_the_converged_link_below_floor": int((conv & link).sum()),
                                   "link_below_floor_of_all": int(link.sum()), "outer_iterations": int(info["iterations"].sum())})

    # ---- (c) the price of the pass with nothing active
    if not a.off_only:
        far.solve(T0[:64])
        rows, its = {"off": [], "floor_at_-10": []}, {}
        for _ in range(a.reps):
            for n, p in (("off", off), ("floor_at_-10", far)):
                r, dt = timed(lambda: p.solve(T0))
                rows[n].append(dt)
                its[n] = (int(r["iterations"].cpu().numpy().sum()), r["x"].cpu().numpy())
        res["price_inactive"] = {n: rng3(t, 1e3) for n, t in rows.items()}
        res["price_inactive"]["ratio_of_medians"] = round(float(np.median(rows["floor_at_-10"]) / np.median(rows["off"])), 4)
        res["price_inactive"]["same_answers"] = bool(its["off"][0] == its["floor_at_-10"][0] and np.array_equal(its["off"][1], its["floor_at_-10"][1]))
        res["price_inactive"]["outer_iterations"] = its["off"][0]
    return res


def against_parent(res, parent):
    """This commit's `off` batch times over the parent commit's (its --off-only run), per (robot, table, retries)."""
    key = lambda r: (r["robot"], r["table"])      # noqa: E731
    theirs = {key(r): r for r in parent["robots"]}
    out = []
    for r in res["robots"]:
        p = theirs.get(key(r))
        if p is None:
            continue
        for mine, old in zip([c for c in r["cold"] if c["halfspaces"] == "off"], [c for c in p["cold"] if c["halfspaces"] == "off"]):
            out.append({"robot": r["robot"], "table": r["table"], "retries": mine["retries"],
                        "off_ms_this_commit": mine["ms_per_batch_median_min_max"], "off_ms_parent": old["ms_per_batch_median_min_max"],
                        "ratio_of_medians": round(mine["ms_per_batch_median_min_max"][0] / old["ms_per_batch_median_min_max"][0], 4),
                        "same_outer_iterations": mine["outer_iterations"] == old["outer_iterations"]})
    return out


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--goals", type=int, default=4096)
    p.add_argument("--waypoints", type=int, default=8)
    p.add_argument("--step", type=float, default=0.02)
    p.add_argument("--margin", type=float, default=0.05)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--robots", default="ur10,kuka")
    p.add_argument("--off-only", action="store_true", help="the problems without half-spaces alone (runs on the parent commit too)")
    p.add_argument("--parent", default=None, help="the JSON of an --off-only run on the parent commit, to compare the off rows with")
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "anchored_halfspace_study.json"))
    a = p.parse_args()
    from graphik_amd import _ffi
    digest = open(_ffi.LIB_PATH + ".digest").read().strip() if os.path.exists(_ffi.LIB_PATH + ".digest") else None
    res = {"workload": "anchored_halfspaces_floor", "reps": a.reps, "tolerances": TOL, "step_rad": a.step, "margin_m": a.margin,
           "off_only": a.off_only, "library_digest": digest,
           "robots": [measure(name, table, a) for name in a.robots.split(",") for table in (True, False)]}
    if a.parent:
        res["against_parent"] = against_parent(res, json.load(open(a.parent)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
