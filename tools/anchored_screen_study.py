#!/usr/bin/env python3
"""tools/anchored_screen_study.py -- screened restart seeds in the fixed-anchor solve, measured on the device with
retry_candidates 1, 4 and 8 alternated (a measurement tool; bench.py is the project's yardstick and is not touched by it).
docs/NOTEBOOK.md 45.

    python tools/anchored_screen_study.py [--goals 4096] [--waypoints 8] [--step 0.02] [--reps 3] [--robots ur10,kuka]
                                          [--unscreened-only] [--parent parent.json] [--out profiles/anchored_screen_study.json]

The cells of NOTEBOOK 42: per robot (UR10, KUKA), with table_environment() and without, the skeleton as capsules of 3 cm, a
floor at z = -0.1 with the default margins, clearance_mode="links", `goals` goals; the paths are those of
tools/anchored_tracking_study.py (its generator and seed).  Nothing here is gated.
  (a) cold  : the goals of waypoint 0, AnchoredProblem.solve(T, retries=3), per retry_candidates: ms per batch, converged
              answers (f < 1e-9), goals on their pose, converged answers with a joint point / a link's capsule more than 1e-4
              below the floor (plain numpy on the answer's point matrix), the attempt histogram.
  (b) track : solve_trajectory on goals x waypoints, retries=3, retry_spread=0.5, per retry_candidates: the same per waypoint.
  (c) seeds : the stand-alone step (gik_anchored_retry_seeds_screened) on the goals that fail attempt 0, attempt 1: the share
              of slots whose picked seed is clear (d_pick_clearance >= -clear_tol), and the step's own time -- two events around the C
              entry, every buffer allocated and uploaded before -- beside the solve kernel's time of a restart of the same
              slots from the picked seeds (gik_anchored_last_solve_ms).
--unscreened-only runs retry_candidates=1 alone through the call without the keyword and skips (c): it touches nothing this
commit adds, so run on the parent commit it gives the figures `--parent` compares this commit's one-candidate rows with.
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
RETRIES, SEED, SPREAD = 3, 1, 0.5


def rng3(t, scale):
    import numpy as np
    return [round(scale * v, 4) for v in (float(np.median(t)), min(t), max(t))]


def scene(name, table):
    from graphik_amd.solvers.riemannian_solver import AnchoredProblem
    from graphik_amd.utils import table_environment
    from graphik_amd.utils.roboturdf import load_kuka, load_ur10
    robot, graph = {"kuka": load_kuka, "ur10": load_ur10}[name]()
    if table:
        for idx, obs in enumerate(table_environment()):
            graph.add_spherical_obstacle(f"o{idx}", obs[0], obs[1])
    return robot, AnchoredProblem(graph, link_radius=RHO, halfspaces=[list(FLOOR)])


def below_floor(Y_full, ap):
    """Per point matrix (numpy [B, N, 3]): (a joint point p1 .. p(n-1) below the floor, a link's capsule below it)."""
    import numpy as np
    g = ap.base.graph
    z = Y_full[:, [g.index(f"p{i}") for i in range(1, ap.robot.n)], 2]
    ends = Y_full[:, np.asarray(ap.link_rows).reshape(-1), 2]
    ct = TOL["clear_tol"]
    return (z.min(axis=1) - FLOOR[3]) < -ct, (ends.min(axis=1) - FLOOR[3] - RHO) < -ct


def counts(f, stop, pe, re, Y, ap):
    import numpy as np
    node, link = below_floor(Y, ap)
    conv = f < 1e-9
    ok = (stop == 0) & (pe <= TOL["pos_tol"]) & (re <= TOL["rot_tol"])
    return {"converged": int(conv.sum()), "on_their_pose": int(ok.sum()), "of_the_converged_joint_point_below_floor": int((conv & node).sum()),
            "of_the_converged_link_below_floor": int((conv & link).sum()), "of": int(np.size(f))}


_PATHS = {}


def measure(name, table, a):
    import numpy as np
    import torch
    from anchored_tracking_study import paths
    from graphik_amd.solvers import riemannian_solver as rs
    robot, ap = scene(name, table)
    if name not in _PATHS:      # (the generator keeps paths that clear the table: drawn on the table scene, used on both)
        assert table, "the table scene of a robot is measured first"
        _PATHS[name] = paths(robot, ap, a.goals, a.waypoints, a.step, a.margin)
    Q, T, kept = _PATHS[name]
    B, L = T.shape[:2]
    cands = [None] if a.unscreened_only else [1, 4, 8]      # None: the call without the keyword
    kw_of = lambda c: {} if c is None else dict(retry_candidates=c)      # noqa: E731
    label = lambda c: 1 if c is None else c      # noqa: E731
    res = {"robot": name, "table": bool(table), "goals": B, "waypoints": L, "link_radius": RHO, "floor": list(FLOOR)}
    tpl, base = ap.template, ap.base.template

    def timed(fn):
        e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e[0].record()
        r = fn()
        e[1].record()
        torch.cuda.synchronize()
        return r, e[0].elapsed_time(e[1]) * 1e-3

    T0 = T[:, 0]
    for c in cands:                                          # warm-up: library, handles, code objects
        ap.solve(T0[:64], retries=1, clearance_mode=MODE, **TOL, **kw_of(c))

    # ---- (a) cold, retries = 3
    cold = dict(retries=RETRIES, retry_seed=SEED, clearance_mode=MODE, **TOL)
    rows = {c: {"t": [], "solve_ms": []} for c in cands}
    for _ in range(a.reps):                                  # alternated: every count sees the same machine
        for c in cands:
            r, dt = timed(lambda: ap.solve(T0, **cold, **kw_of(c)))
            rows[c]["t"].append(dt)
            rows[c]["solve_ms"].append(float(tpl.lib.gik_anchored_last_solve_ms(tpl._h)))
            rows[c]["r"] = r
    res["cold"] = []
    for c in cands:
        r = rows[c]["r"]
        f, stop, pe, re = (r[k].cpu().numpy() for k in ("f", "stop", "pos_err", "rot_err"))
        res["cold"].append({"retry_candidates": label(c), "retries": RETRIES, "ms_per_batch_median_min_max": rng3(rows[c]["t"], 1e3),
                            **counts(f, stop, pe, re, r["x"].cpu().numpy(), ap),
                            "attempt_histogram": np.bincount(r["attempt"].cpu().numpy(), minlength=RETRIES + 1).tolist(),
                            "last_restart_solve_kernel_ms_median_min_max": rng3(rows[c]["solve_ms"], 1.0),
                            "outer_iterations": int(r["iterations"].cpu().numpy().sum())})

    # ---- (b) tracked, local restarts
    track = dict(retries=RETRIES, retry_seed=SEED, retry_spread=SPREAD, clearance_mode=MODE, **TOL)
    for c in cands:
        ap.solve_trajectory(T[:, :2], Q[:, 0], **track, **kw_of(c))
    times, infos = {c: [] for c in cands}, {}
    for _ in range(a.reps):
        for c in cands:
            q, Y, info = ap.solve_trajectory(T, Q[:, 0], return_Y=True, **track, **kw_of(c))
            times[c].append(info["solve_time"])
            infos[c] = (info, np.asarray(Y))
    res["tracked"] = []
    for c in cands:
        info, Y = infos[c]
        flat = lambda k: info[k].reshape(-1)      # noqa: E731
        res["tracked"].append({"retry_candidates": label(c), "retries": RETRIES, "retry_spread": SPREAD,
                               "ms_per_waypoint_median_min_max": rng3(times[c], 1e3 / L),
                               "waypoints_per_s": round(B * L / float(np.median(times[c])), 1),
                               **counts(flat("f(x)"), flat("stop"), flat("pos_err"), flat("rot_err"), Y.reshape(B * L, -1, 3), ap),
                               "attempt_histogram": np.bincount(flat("attempt"), minlength=RETRIES + 1).tolist(),
                               "outer_iterations": int(info["iterations"].sum())})

    # ---- (c) the seeds themselves: the stand-alone step on the goals that fail attempt 0
    if not a.unscreened_only:
        lo, hi = robot.limits_arrays()
        res["seeds"] = []
        for kind, q_init, centre, spread in (("cold", None, None, 0.0), ("tracked_waypoint_0", Q[:, 0], Q[:, 0], SPREAD)):
            r0 = ap.solve(T0, q_init=q_init, clearance=True, clearance_mode=MODE)
            failed = rs.anchored_retry_failed(*(r0[k].cpu().numpy() for k in ("stop", "pos_err", "rot_err", "clearance")), **TOL)
            idx = np.flatnonzero(failed).astype(np.int32)
            # everything the entry reads or writes is on the device before the clock starts: the events enclose the C call alone
            import ctypes as C
            from graphik_amd import _ffi
            f64 = dict(dtype=torch.float64, device=tpl.device)
            count, n = len(idx), robot.n
            d_T = torch.from_numpy(np.ascontiguousarray(T0.reshape(B, 16))).to(tpl.device)
            d_idx = torch.from_numpy(idx).to(tpl.device)
            d_lo, d_hi = (torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(tpl.device) for v in (lo, hi))
            d_c = None if centre is None else torch.from_numpy(np.ascontiguousarray(centre)).to(tpl.device)
            T_out, q_out, cl_out = torch.empty(count, 16, **f64), torch.empty(count, n, **f64), torch.empty(count, **f64)
            pick_out = torch.empty(count, dtype=torch.int32, device=tpl.device)
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            for c in (1, 4, 8):
                ws = torch.empty(int(tpl.lib.gik_anchored_retry_seeds_screened_ws_bytes(tpl._h, base._h, count, c)) // 8 + 1, **f64)
                run = lambda: _ffi.check(tpl.lib.gik_anchored_retry_seeds_screened(      # noqa: E731
                    tpl._h, base._h, d_T.data_ptr(), d_idx.data_ptr(), count, SEED, 1, d_lo.data_ptr(), d_hi.data_ptr(),
                    None if d_c is None else d_c.data_ptr(), spread, c, _ffi.CLEARANCE_MODES[MODE], TOL["clear_tol"], None, ws.data_ptr(),
                    T_out.data_ptr(), q_out.data_ptr(), pick_out.data_ptr(), cl_out.data_ptr(), stream))
                run()
                ts = [timed(run)[1] for _ in range(max(a.reps, 5))]
                cl, pick = cl_out.cpu().numpy(), pick_out.cpu().numpy()
                # the restart this step feeds: one seeded solve of the same slots from the picked seeds, its solve kernel alone
                solve_ms = []
                for _ in range(max(a.reps, 3)):
                    ap.solve(T0[idx], q_init=q_out.cpu().numpy(), clearance=True, clearance_mode=MODE)
                    solve_ms.append(float(tpl.lib.gik_anchored_last_solve_ms(tpl._h)))
                res["seeds"].append({"kind": kind, "failed_attempt_0": int(count), "retry_candidates": c,
                                     "picked_seed_clear": int((cl >= -TOL["clear_tol"]).sum()),
                                     "share_clear": round(float((cl >= -TOL["clear_tol"]).mean()), 4) if count else None,
                                     "pick_histogram": np.bincount(pick, minlength=c).tolist(),
                                     "step_ms_median_min_max": rng3(ts, 1e3),
                                     "restart_solve_kernel_ms_median_min_max": rng3(solve_ms, 1.0),
                                     "workspace_bytes": int(ws.numel() * 8)})
    return res


def against_parent(res, parent):
    """This commit's one-candidate rows over the parent commit's (its --unscreened-only run), per (robot, table, workload)."""
    key = lambda r: (r["robot"], r["table"])      # noqa: E731
    theirs = {key(r): r for r in parent["robots"]}
    out = []
    for r in res["robots"]:
        p = theirs.get(key(r))
        if p is None:
            continue
        for work, field in (("cold", "ms_per_batch_median_min_max"), ("tracked", "ms_per_waypoint_median_min_max")):
            mine = [c for c in r[work] if c["retry_candidates"] == 1][0]
            old = p[work][0]
            same = all(mine[k] == old[k] for k in ("converged", "on_their_pose", "attempt_histogram", "outer_iterations"))
            out.append({"robot": r["robot"], "table": r["table"], "workload": work, "ms_this_commit": mine[field], "ms_parent": old[field],
                        "ratio_of_medians": round(mine[field][0] / old[field][0], 4), "same_counts_and_iterations": same})
    return out


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--goals", type=int, default=4096)
    p.add_argument("--waypoints", type=int, default=8)
    p.add_argument("--step", type=float, default=0.02)
    p.add_argument("--margin", type=float, default=0.05)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--robots", default="ur10,kuka")
    p.add_argument("--unscreened-only", action="store_true", help="one candidate through the call without the keyword (runs on the parent commit too)")
    p.add_argument("--parent", default=None, help="the JSON of an --unscreened-only run on the parent commit, to compare the one-candidate rows with")
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "anchored_screen_study.json"))
    a = p.parse_args()
    from graphik_amd import _ffi
    digest = open(_ffi.LIB_PATH + ".digest").read().strip() if os.path.exists(_ffi.LIB_PATH + ".digest") else None
    res = {"workload": "anchored_screened_restart_seeds", "reps": a.reps, "tolerances": TOL, "step_rad": a.step, "margin_m": a.margin,
           "unscreened_only": a.unscreened_only, "library_digest": digest,
           "robots": [measure(name, table, a) for name in a.robots.split(",") for table in (True, False)]}
    if a.parent:
        res["against_parent"] = against_parent(res, json.load(open(a.parent)))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
