"""The claim-order part of the launch plan (graphik_amd/csrc/gik_plan.h) without a device, by the stand-alone program
tests/host/claim_order_plan.cpp: which batch sizes order their claims, the sizing and layout of the key and order
buffers in the leased workspace, an unchanged plan for templates without a key, and the keys that are refused.  Built
plain and with the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def _build(tmp_path, name, extra):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler (c++, g++, clang++) on this machine")
    exe = str(tmp_path / name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-I" + os.path.join(REPO, "graphik_amd", "csrc")] + extra +
                       [os.path.join(REPO, "tests", "host", "claim_order_plan.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, r


def test_claim_order_plan(tmp_path):
    exe, r = _build(tmp_path, "claim_order_plan", [])
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert " 0 failures" in run.stdout


def test_claim_order_plan_under_the_sanitizers(tmp_path):
    exe, r = _build(tmp_path, "claim_order_plan_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0:
        pytest.skip("the sanitizers' runtime does not link here: " + r.stderr[-300:])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "Sanitizer" not in run.stderr, run.stdout[-3000:] + run.stderr[-3000:]
    assert " 0 failures" in run.stdout


def test_robot_data_names_the_key_only_where_the_study_supports_it():
    """lwa4d.json carries claim_key = reach (tools/claim_order_study.py, NOTEBOOK 21); the other packaged robots stay on
    index order.  The terms BatchProblem hands over are the (p0, p_e) equality terms: their target is the squared reach."""
    import numpy as np
    from conftest import make_graph
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    for name, want in (("lwa4d", "reach"), ("kuka", None), ("ur10", None)):
        robot, graph = make_graph(name)
        assert getattr(robot, "claim_key", None) == want, name
        prob = BatchProblem(graph, use_limits=True, host_only=True)
        terms = prob.claim_key_terms()
        assert len(terms) == 1
        ti, tj, tk, _ = prob.terms
        t = terms[0]
        assert tk[t] == 1 and {graph.node_ids[ti[t]], graph.node_ids[tj[t]]} == {"p0", f"p{robot.n}"}
        # the term's target IS the squared distance of the goal position from the base origin
        rs = np.random.RandomState(5)
        lb, ub = robot.limits_arrays()
        T_goal = robot.fk_batch(lb + (ub - lb) * rs.rand(16, robot.n))
        tg, _ = prob.prepare(T_goal)
        assert np.allclose(tg[:, t], (T_goal[:, :3, 3] ** 2).sum(1), rtol=1e-12, atol=1e-15)
