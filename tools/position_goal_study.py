#!/usr/bin/env python3
"""tools/position_goal_study.py -- what position goals (goal="position") cost and buy next to pose goals of the same
configurations (a measurement tool; bench.py is the project's yardstick and is not touched by it).

    python tools/position_goal_study.py [--repeat 5] [--baseline-tree DIR] [--out profiles/position_goal_study.json]

1. solve_batch on random configurations (seed 0) of planar-10 (65536 goals), LWA4D and UR10 (4096 each), once with the
   poses and once with the positions of the same configurations: ms per batch (median of --repeat calls after one
   warm-up; solve_batch's own solve_time, as tools/retry_study.py times), median outer iterations, share converged
   (stop == 0 and pos_err <= 0.01 m).
2. The prepare kernel alone on the position templates of planar-10 (65536 goals) and UR10 (4096): four goals per
   wavefront against one (GIK_NO_PREP_QUAD, read at attach: a child process each), device events around
   Template.prepare, --repeat runs after a warm-up.
3. The regression check of the inert-slot test in prep_quad_kernel<13>: the same measurement on 65536 planar-10 POSE
   goals, on this tree and, with --baseline-tree DIR (a checkout of the commit to compare with, its library built),
   on that one: both lists of --repeat runs, their medians and spreads (max - min).
Prints a table and writes everything as JSON.
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

# argv: tree, robot, goal poses (.npy), repeat, goal kind ("pose": also what a tree without the keyword runs), output
PREP_CHILD = r"""
import json, sys
import numpy as np, torch
tree, name, poses, repeat, kind, out = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), sys.argv[5], sys.argv[6]
sys.path.insert(0, tree)
import bench
from graphik_amd.solvers.riemannian_solver import BatchProblem
robot, graph = bench.build_graph(name)
prob = BatchProblem(graph) if kind == "pose" else BatchProblem(graph, goal=kind)
T = torch.from_numpy(np.load(poses)).cuda()
tpl = prob.template
tpl.prepare(T)
torch.cuda.synchronize()
ms = []
for _ in range(repeat):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    tpl.prepare(T)
    b.record()
    torch.cuda.synchronize()
    ms.append(a.elapsed_time(b))
json.dump({"ms": ms, "goals_per_wave": int(tpl.info["goals_per_wave"])}, open(out, "w"))
"""


def goal_poses(name, B):
    """B random configurations (seed 0) of a bench.py robot -> (robot, graph, poses [B, d+1, d+1])."""
    import numpy as np
    import bench
    robot, graph = bench.build_graph(name)
    lb, ub = robot.limits_arrays()
    return robot, graph, robot.fk_batch(np.random.RandomState(0).uniform(lb, ub, size=(B, robot.n)))


def prepare_ms(tree, name, T, repeat, kind, no_quad=False):
    """Device milliseconds of `repeat` Template.prepare calls on the poses T, in a child process on `tree`."""
    import numpy as np
    env = dict(os.environ, **({"GIK_NO_PREP_QUAD": "1"} if no_quad else {}))
    with tempfile.TemporaryDirectory() as tmp:
        out, poses = os.path.join(tmp, "prep.json"), os.path.join(tmp, "poses.npy")
        np.save(poses, T)
        subprocess.run([sys.executable, "-c", PREP_CHILD, tree, name, poses, str(repeat), kind, out], check=True, env=env,
                       timeout=300)
        r = json.load(open(out))
    r.update(median=float(np.median(r["ms"])), spread=float(max(r["ms"]) - min(r["ms"])))
    return r


def solve_rows(graph, T, repeat):
    import numpy as np
    from graphik_amd.solvers.riemannian_solver import solve_batch
    d = graph.dim
    rows = {}
    for kind, goals in (("pose", T), ("position", T[:, :d, d])):
        solve_batch(graph, goals[:64], goal=kind)      # warm-up: handles, buffers
        times = []
        for _ in range(repeat + 1):
            q, Y, info = solve_batch(graph, goals, goal=kind)
            times.append(info["solve_time"])
        ok = (info["stop"] == 0) & (info["pos_err"] <= 0.01)
        rows[kind] = {"ms": float(np.median(times[1:]) * 1e3), "ms_runs": [t * 1e3 for t in times[1:]],
                      "outer_median": float(np.median(info["iterations"])), "converged": float(ok.mean()),
                      "pos_err_median": float(np.median(info["pos_err"]))}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "position_goal_study.json"))
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    res = {"solve": {}, "prepare": {}, "regression": {}}
    poses = {}
    for name, B in (("planar10_limits_pi", 65536), ("lwa4d", 4096), ("ur10", 4096)):
        robot, graph, poses[name] = goal_poses(name, B)
        res["solve"][name] = dict(goals=B, **solve_rows(graph, poses[name], args.repeat))
        for kind, r in res["solve"][name].items():
            if kind != "goals":
                print(f"{name:20s} B={B:6d} {kind:9s} {r['ms']:9.2f} ms  outer median {r['outer_median']:6.1f}  "
                      f"converged {r['converged']:.4f}", flush=True)
    for name, B in (("planar10_limits_pi", 65536), ("ur10", 4096)):
        res["prepare"][name] = {"goals": B, "quad": prepare_ms(REPO, name, poses[name], args.repeat, "position"),
                                "wave": prepare_ms(REPO, name, poses[name], args.repeat, "position", no_quad=True)}
        q, w = res["prepare"][name]["quad"], res["prepare"][name]["wave"]
        assert q["goals_per_wave"] == 4 and w["goals_per_wave"] == 1
        print(f"{name:20s} B={B:6d} position prepare: quad {q['median']:.3f} ms, wave {w['median']:.3f} ms", flush=True)
    reg = res["regression"]
    planar = poses["planar10_limits_pi"]
    reg["this"] = prepare_ms(REPO, "planar10_limits_pi", planar, args.repeat, "pose")
    print("prep_quad_kernel<13>, 65536 planar-10 pose goals, this tree:", reg["this"], flush=True)
    if args.baseline_tree:
        reg["baseline"] = prepare_ms(os.path.abspath(args.baseline_tree), "planar10_limits_pi", planar, args.repeat, "pose")
        print("... baseline tree:", reg["baseline"], flush=True)
        reg["this_again"] = prepare_ms(REPO, "planar10_limits_pi", planar, args.repeat, "pose")
        print("... this tree again:", reg["this_again"], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
