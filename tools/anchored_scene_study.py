#!/usr/bin/env python3
"""tools/anchored_scene_study.py -- what per-goal obstacle scenes cost in the fixed-anchor solve, measured on the device
(a measurement tool; bench.py is the project's yardstick and is not touched by it).  docs/NOTEBOOK.md 29.

    python tools/anchored_scene_study.py [--goals 4096] [--batches 5] [--warmup 2] [--plain-only]
                                         [--out profiles/anchored_scene_study.json]

UR10 + table_environment(), `--goals` cold goals (forward kinematics of uniform joint angles, RandomState(0)), the solve
kernel's own duration (gik_anchored_last_solve_ms): median, min and max of `--batches` batches after `--warmup`.
  plain   AnchoredProblem.solve(T): the call every earlier commit has (--plain-only stops here: run it from a checkout of
          another commit to compare; it uses nothing this feature adds)
  one     the scene call with ONE scene equal to the template's spheres: the price of the scene build itself (a restage
          at a wave's first problem, a scalar compare per problem after it)
  mixed   the scene call with three scenes -- the table, the table 0.2 m further in x, empty -- and scene_id = b % 3, so
          that nearly every problem a wave claims names another scene than the one it holds: a 3.2 KB restage per problem
Also checks, on the way, that `one` returns the plain call's bits.  Prints one JSON line and writes it to --out."""
import argparse
import ctypes as C
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--goals", type=int, default=4096)
    ap_.add_argument("--batches", type=int, default=5)
    ap_.add_argument("--warmup", type=int, default=2)
    ap_.add_argument("--plain-only", action="store_true")
    ap_.add_argument("--out", default=os.path.join(REPO, "profiles", "anchored_scene_study.json"))
    a = ap_.parse_args()
    import numpy as np
    import torch
    from graphik_amd import _ffi
    from graphik_amd.solvers.riemannian_solver import AnchoredProblem
    from graphik_amd.utils import table_environment
    from graphik_amd.utils.roboturdf import load_ur10
    robot, graph = load_ur10()
    for idx, obs in enumerate(table_environment()):
        graph.add_spherical_obstacle(f"o{idx}", obs[0], obs[1])
    ap = AnchoredProblem(graph)
    lib = ap.template.lib
    lib.gik_anchored_last_solve_ms.restype = C.c_double
    lb, ub = robot.limits_arrays()
    T = robot.fk_batch(np.random.RandomState(0).uniform(lb, ub, size=(a.goals, robot.n)))

    def timed(fn):
        ms, last = [], None
        for i in range(a.warmup + a.batches):
            last = fn()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms.append(float(lib.gik_anchored_last_solve_ms(ap.template._h)))
        return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}, last

    digest = open(_ffi.LIB_PATH + ".digest").read().strip() if os.path.exists(_ffi.LIB_PATH + ".digest") else None
    res = {"workload": "ur10_table_anchored_scenes", "goals": a.goals, "batches": a.batches, "warmup": a.warmup,
           "library_digest": digest, "template_info": {k: int(ap.template.info[k]) for k in ("anchored", "lds_bytes", "waves_per_cu", "n_cu")}}
    res["plain"], plain = timed(lambda: ap.solve(T))
    res["iterations_total"] = int(plain["iterations"].sum().item())
    if not a.plain_only:
        table = ap.obstacles
        one = ap.scene_set([table])
        res["one"], r1 = timed(lambda: ap.solve(T, scenes=one))
        res["one_equals_plain_bits"] = bool(torch.equal(r1["x"].view(torch.int64), plain["x"].view(torch.int64)))
        three = ap.scene_set([table, table + np.array([0.2, 0.0, 0.0, 0.0]), np.zeros((0, 4))])
        ids = torch.arange(a.goals, device=ap.template.device, dtype=torch.int32) % 3
        res["mixed"], r3 = timed(lambda: ap.solve(T, scenes=three, scene_id=ids))
        res["mixed_iterations_total"] = int(r3["iterations"].sum().item())
        # the same three scenes, goals sorted by scene: the restages go away, the work stays
        order = torch.argsort(ids, stable=True)
        Ts = T[order.cpu().numpy()]
        ids_s = ids[order].contiguous()
        res["mixed_sorted"], _ = timed(lambda: ap.solve(Ts, scenes=three, scene_id=ids_s))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
