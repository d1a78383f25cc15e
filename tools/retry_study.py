#!/usr/bin/env python3
"""tools/retry_study.py -- what restarts from random joint seeds buy (a measurement tool; bench.py is the project's
yardstick and is not touched by it).

    python tools/retry_study.py [--goals 4096] [--robots lwa4d kuka ur10_table] [--repeat 3]
                                [--baseline-tree DIR] [--out profiles/retry_study.json]

For each robot, on the goals bench.py itself draws (Bench.goals, seed 0): solve_batch with retries in {0, 1, 3}
at the default outer-iteration budget (maxiter 3000) and at a short first budget (maxiter 300) -- success rate
(stop == 0, pos_err <= 0.01 m, rot_err <= 0.01 rad), goals at maxiter, goals whose answer comes from a restart,
and ms per batch (median of --repeat calls after one warm-up; solve_batch's own solve_time: the device pipeline
including the host synchronisations between attempts, without the copies of the results).

--baseline-tree DIR: a checkout of the commit to compare with (its library built).  Its plain default
solve_batch runs in a child process -- another interpreter, that tree's package and library -- on the same goals,
and its success rate and time are the "baseline" row; the answers of this tree's retries = 0 call are compared
with it bit for bit.  Prints a table and writes everything as JSON.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

POS_TOL, ROT_TOL = 0.01, 0.01
CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import bench
from graphik_amd.solvers.riemannian_solver import solve_batch
robot, graph = bench.build_graph(sys.argv[2])
T = np.load(sys.argv[3])
repeat = int(sys.argv[4])
solve_batch(graph, T[:64])
times = []
for _ in range(repeat + 1):
    q, Y, info = solve_batch(graph, T)
    times.append(info["solve_time"])
np.savez(sys.argv[5], q=q, stop=info["stop"], pos_err=info["pos_err"], rot_err=info["rot_err"],
         iterations=info["iterations"], times=np.array(times[1:]))
"""


def goals(robot_name, total, seed=0):
    """bench.py's own goal stream for one rank."""
    import bench
    from graphik_amd import distributed as gd
    robot, graph = bench.build_graph(robot_name)
    me = types.SimpleNamespace(gd=gd, rank=0, world=1)
    T, B = bench.Bench.goals(me, robot, total, seed)
    assert B == total
    return robot, graph, T


def summary(info, maxiter):
    import numpy as np
    ok = (info["stop"] == 0) & (info["pos_err"] <= POS_TOL) & (info["rot_err"] <= ROT_TOL)
    out = {"success": float(ok.mean()), "failed": int((~ok).sum()),
           "at_maxiter": int((info["stop"] == 1).sum())}
    if "attempt" in info:
        out["from_a_restart"] = int((info["attempt"] > 0).sum())
    return out


def run(graph, T, maxiter, retries, repeat):
    import numpy as np
    from graphik_amd.solvers.riemannian_solver import solve_batch
    params = None if maxiter == 3000 else {"maxiter": maxiter}
    kw = dict(params=params, retries=retries, retry_seed=0, pos_tol=POS_TOL, rot_tol=ROT_TOL)
    solve_batch(graph, T[:64], **kw)            # warm-up: handles, buffers
    times = []
    for _ in range(repeat + 1):
        q, Y, info = solve_batch(graph, T, **kw)
        times.append(info["solve_time"])
    row = {"maxiter": maxiter, "retries": retries, "ms_per_batch": 1e3 * float(np.median(times[1:])),
           "ms_runs": [1e3 * t for t in times[1:]]}
    row.update(summary(info, maxiter))
    return row, q, info


def baseline(tree, robot_name, T, repeat):
    import numpy as np
    tmp = tempfile.mkdtemp(prefix="retry_study_")
    gpath, opath = os.path.join(tmp, "goals.npy"), os.path.join(tmp, "out.npz")
    np.save(gpath, T)
    env = {k: v for k, v in os.environ.items() if k not in ("PYTHONPATH", "GIK_LIB_PATH")}
    subprocess.run([sys.executable, "-c", CHILD, os.path.abspath(tree), robot_name, gpath, str(repeat), opath],
                   check=True, env=env, cwd=os.path.abspath(tree), timeout=1500)
    d = dict(np.load(opath))
    row = {"maxiter": 3000, "retries": "baseline", "ms_per_batch": 1e3 * float(np.median(d["times"])),
           "ms_runs": [1e3 * float(t) for t in d["times"]]}
    row.update(summary(d, 3000))
    return row, d


def main():
    import numpy as np
    p = argparse.ArgumentParser()
    p.add_argument("--goals", type=int, default=4096)
    p.add_argument("--robots", nargs="+", default=["lwa4d", "kuka", "ur10_table"])
    p.add_argument("--repeat", type=int, default=3)
    p.add_argument("--baseline-tree", default=None)
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "retry_study.json"))
    a = p.parse_args()
    sys.path.insert(0, REPO)
    report = {"goals": a.goals, "pos_tol": POS_TOL, "rot_tol": ROT_TOL, "repeat": a.repeat, "robots": {}}
    for name in a.robots:
        robot, graph, T = goals(name, a.goals)
        rows = []
        base = None
        if a.baseline_tree:
            row, base = baseline(a.baseline_tree, name, T, a.repeat)
            rows.append(row)
        for maxiter in (3000, 300):
            for retries in (0, 1, 3):
                row, q, info = run(graph, T, maxiter, retries, a.repeat)
                if base is not None and maxiter == 3000 and retries == 0:
                    row["bit_identical_to_baseline"] = bool(
                        np.array_equal(q.view(np.int64), base["q"].view(np.int64)) and
                        np.array_equal(info["iterations"], base["iterations"]))
                rows.append(row)
                print(name, json.dumps(row), flush=True)
        report["robots"][name] = rows
        with open(a.out, "w") as f:          # (after every robot: a long run leaves what it has)
            json.dump(report, f, indent=1)
    print()
    print("| robot | maxiter | retries | success | failed | at maxiter | from a restart | ms per batch |")
    print("|---|---|---|---|---|---|---|---|")
    for name, rows in report["robots"].items():
        for r in rows:
            print(f"| {name} | {r['maxiter']} | {r['retries']} | {100 * r['success']:.2f} % | {r['failed']} | "
                  f"{r['at_maxiter']} | {r.get('from_a_restart', '-')} | {r['ms_per_batch']:.1f} |")


if __name__ == "__main__":
    main()
