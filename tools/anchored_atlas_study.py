#!/usr/bin/env python3
"""tools/anchored_atlas_study.py -- goal-aware seeds from a configuration atlas in the fixed-anchor solve, measured on the
device beside the blind starts (a measurement tool; bench.py is the project's yardstick and is not touched by it).
docs/NOTEBOOK.md 46.

    python tools/anchored_atlas_study.py [--goals 4096] [--reps 3] [--robots ur10,kuka] [--draws 16384,65536,262144]
                                         [--out profiles/anchored_atlas_study.json]

The cells of NOTEBOOK 42 and 45: per robot (UR10, KUKA), with table_environment() and without, the skeleton as capsules of
3 cm, a floor at z = -0.1 with the default margins, clearance_mode="links", `goals` goals: waypoint 0 of the paths of
tools/anchored_tracking_study.py (its generator and seed).  Nothing here is gated.
  (a) cold : AnchoredProblem.solve(T, ...) with no atlas at retries 0 and 3 (the rows of NOTEBOOK 45, in the same job) and,
             per atlas size, atlas= with retries 0 and with retries 3 x atlas_candidates 1 and 4; all alternated, `reps`
             repetitions: ms per batch, converged answers (f < 1e-9), goals on their pose, converged answers with a joint
             point / a link's capsule more than 1e-4 below the floor, the attempt histogram, the median outer iterations.
  (b) the atlas: draws, rows kept, the host build's seconds, the median key distance of the nearest row.
  (c) the nearest step alone: gik_atlas_nearest for goals x 65536 rows x K in {1, 8, 32}, two events around the C entry with
             every buffer allocated and uploaded before, beside the solve kernel's time of the batch it feeds
             (gik_anchored_last_solve_ms).
Prints one JSON line and writes it to --out, with the digest of the library the numbers were taken on.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)

from anchored_screen_study import MODE, RETRIES, SEED, TOL, counts, rng3, scene      # noqa: E402

ATLAS_SEED = 11
_PATHS = {}


def measure(name, table, a):
    import numpy as np
    import torch
    from anchored_tracking_study import paths
    from graphik_amd.solvers import riemannian_solver as rs
    robot, ap = scene(name, table)
    if name not in _PATHS:      # (the generator keeps paths that clear the table: drawn on the table scene, used on both)
        assert table, "the table scene of a robot is measured first"
        _PATHS[name] = paths(robot, ap, a.goals, 1, 0.02, 0.05)
    Q, T, kept = _PATHS[name]
    T0 = np.ascontiguousarray(T[:, 0])
    B = len(T0)
    tpl, base = ap.template, ap.base.template
    res = {"robot": name, "table": bool(table), "goals": B}

    # ---- (b) the atlases: the largest is built once, a smaller one is its rows among the first `draws` draws
    sizes = sorted(int(s) for s in a.draws.split(","))
    lo, hi = robot.limits_arrays()
    t0 = time.time()
    draws = rs.retry_seeds_host(ATLAS_SEED, np.arange(sizes[-1]), 0, lo, hi)
    big = rs.SeedAtlas.from_configurations(ap, draws, clearance_mode=MODE, clear_tol=TOL["clear_tol"])      # (unfiltered: the filter is per row)
    build_s = time.time() - t0
    clear = big.clearance >= -TOL["clear_tol"]
    atlases, res["atlas"] = {}, []
    for size in sizes:
        keep = clear[:size]
        A = rs.SeedAtlas(big.q[:size][keep], big.keys[:size][keep], big.clearance[:size][keep], device=tpl.device)
        atlases[size] = A
        nbr, dist = ap.atlas_nearest(T0, A, 1)
        res["atlas"].append({"draws": size, "rows": A.count, "share_kept": round(A.count / size, 4),
                             "host_build_seconds": round(build_s * size / sizes[-1], 2),
                             "median_nearest_key_distance_m": round(float(np.median(np.sqrt(dist.cpu().numpy()[:, 0]))), 4)})

    def timed(fn):
        e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e[0].record()
        r = fn()
        e[1].record()
        torch.cuda.synchronize()
        return r, e[0].elapsed_time(e[1]) * 1e-3

    # ---- (a) cold
    configs = [("none", None, 0, 1), ("none", None, RETRIES, 1)]
    for size in sizes:
        configs += [(size, atlases[size], 0, 1), (size, atlases[size], RETRIES, 1), (size, atlases[size], RETRIES, 4)]

    def kw_of(cfg):
        label, A, R, C = cfg
        kw = dict(clearance=True, clearance_mode=MODE)
        if R:
            kw.update(retries=R, retry_seed=SEED, **TOL)
        if A is not None:
            kw.update(atlas=A, atlas_candidates=C, **({} if R else TOL))
        return kw

    for cfg in configs:                                          # warm-up: library, handles, code objects
        ap.solve(T0[:64], **kw_of(cfg))
    rows = {i: {"t": [], "solve_ms": []} for i in range(len(configs))}
    for _ in range(a.reps):                                      # alternated: every configuration sees the same machine
        for i, cfg in enumerate(configs):
            r, dt = timed(lambda: ap.solve(T0, **kw_of(cfg)))
            rows[i]["t"].append(dt)
            rows[i]["solve_ms"].append(float(tpl.lib.gik_anchored_last_solve_ms(tpl._h)))
            rows[i]["r"] = r
    res["cold"] = []
    for i, (label, A, R, C) in enumerate(configs):
        r = rows[i]["r"]
        f, stop, pe, re, its = (r[k].cpu().numpy() for k in ("f", "stop", "pos_err", "rot_err", "iterations"))
        att = r["attempt"].cpu().numpy() if "attempt" in r else np.zeros(B, dtype=np.int64)
        res["cold"].append({"atlas_draws": label, "atlas_rows": None if A is None else A.count, "retries": R, "atlas_candidates": C if A is not None else None,
                            "ms_per_batch_median_min_max": rng3(rows[i]["t"], 1e3), **counts(f, stop, pe, re, r["x"].cpu().numpy(), ap),
                            "attempt_histogram": np.bincount(att, minlength=R + 1).tolist(),
                            "median_outer_iterations": float(np.median(its)),
                            "last_solve_kernel_ms_median_min_max": rng3(rows[i]["solve_ms"], 1.0)})

    # ---- (c) the nearest step alone, on a table of exactly 65536 rows (unfiltered draws: only the keys matter)
    import ctypes as C_
    from graphik_amd import _ffi
    M = min(65536, sizes[-1])
    K65 = rs.SeedAtlas(big.q[:M], big.keys[:M], big.clearance[:M], device=tpl.device)
    d_T = torch.from_numpy(np.ascontiguousarray(T0.reshape(B, 16))).to(tpl.device)
    stream = C_.c_void_p(torch.cuda.current_stream().cuda_stream)
    res["nearest"] = []
    for K in (1, 8, 32):
        nbr = torch.empty(B, K, dtype=torch.int32, device=tpl.device)
        dist = torch.empty(B, K, dtype=torch.float64, device=tpl.device)
        run = lambda: _ffi.check(tpl.lib.gik_atlas_nearest(base._h, K65.d_keys.data_ptr(), M, d_T.data_ptr(), None, B, K,      # noqa: E731
                                                           nbr.data_ptr(), dist.data_ptr(), stream))
        run()
        ts = [timed(run)[1] for _ in range(max(a.reps, 7))]
        res["nearest"].append({"goals": B, "rows": M, "K": K, "ms_median_min_max": rng3(ts, 1e3)})
    ap.solve(T0, atlas=K65, clearance_mode=MODE, **TOL)
    res["solve_kernel_ms_of_the_batch_it_feeds"] = round(float(tpl.lib.gik_anchored_last_solve_ms(tpl._h)), 3)
    return res


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--goals", type=int, default=4096)
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--robots", default="ur10,kuka")
    p.add_argument("--draws", default="16384,65536,262144")
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "anchored_atlas_study.json"))
    a = p.parse_args()
    from graphik_amd import _ffi
    digest = open(_ffi.LIB_PATH + ".digest").read().strip() if os.path.exists(_ffi.LIB_PATH + ".digest") else None
    res = {"workload": "anchored_atlas_seeds", "reps": a.reps, "tolerances": TOL, "clearance_mode": MODE, "atlas_seed": ATLAS_SEED,
           "library_digest": digest, "robots": []}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for name in a.robots.split(","):
        for table in (True, False):
            res["robots"].append(measure(name, table, a))
            with open(a.out, "w") as f:      # (after every cell: a run that is cut short keeps what it measured)
                json.dump(res, f, indent=1)
                f.write("\n")
    print(json.dumps(res))
