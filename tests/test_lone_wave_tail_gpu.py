"""The lone wavefront's tCG step after its reduction-to-branch tail was shortened (docs/NOTEBOOK.md 23): |Hdelta|^2 formed on
the distributed sum, the exit test accumulated in EXEC (plain_in_exec, gik_rtr.hip.h).  Both touch only the SPLIT builds
of the per-edge kernel -- one wave per SIMD -- and change no bit of any output.

* Build equality: the same batch through the SPLIT build (the default plan of a batch this size) and through the
  tail-spreading one-piece build (a template created under GIK_WAVES_PER_CU=8), whose source path is the old one.
  The spread build only runs when the batch is larger than the launch (gik_plan.h: 8 waves on each CU), so the batch
  is twice that, not the 256 problems that would do for the SPLIT build alone; the test checks that problems
  were in fact handed over, which only that build does.  A hand-over drops the tCG checkpoint, so inner_executed of the
  problems that moved may be larger (include/graphik_amd.h); everything else, and inner_executed of the others, is equal
  byte for byte.
* Cold-path coverage: 64 problems with mininner / maxinner / kappa / theta off their defaults, so that every exit of
  the cold block runs.  All six tCG exit codes have to occur in the traces (checked on the CPU oracle for these inputs:
  mininner4 gives 0 1 2 3 5, mix gives 0 1 2 3 4); the first outer iterations agree with the oracle decision for
  decision; every output equals the parent library's, recorded in tests/golden/solve_digest_parent.json.
* Retrace: with debug_flags = 16 every output equals the default run's.
* Digests: tools/solve_digest.py's hash on 512 problems of the three 3-D goldens against the parent library's."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden, make_graph

pytestmark = pytest.mark.gpu

FIELDS = ("x", "f", "gradnorm", "iterations", "inner_total", "inner_executed", "stop", "n_accept")
DIGEST_FIELDS = ("x", "f", "gradnorm", "iterations", "inner_total", "stop", "n_accept")      # tools/solve_digest.py
COLD_SETS = {"mininner4": {"mininner": 4}, "mix": {"mininner": 3, "maxinner": 12, "kappa": 0.3},
             "maxinner5": {"maxinner": 5}, "theta2": {"theta": 2.0, "kappa": 0.5}}
TRACE_CAP = 3000      # maxiter: whole trajectories ("model increased" exits come late in a solve)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module")
def parent():
    with open(os.path.join(GOLDEN, "solve_digest_parent.json")) as f:
        return json.load(f)


def golden_batch(name, B, params=None):
    """(template, start points, targets) as tools/solve_digest.py forms them: the golden start points, jittered."""
    import torch
    from graphik_amd.engine import Template
    d = load_golden(name)
    T = Template.from_matrices(d["omega"], d["psi_L"], d["psi_U"], k=int(d["dim"]), use_limits=bool(int(d["use_limits"])),
                               params=params)
    tg = T.targets_from_D(d["D_goal"])
    idx = np.arange(B) % len(d["Y_init"])
    Y0 = d["Y_init"][idx] + 1e-3 * np.random.RandomState(0).randn(B, *d["Y_init"].shape[1:])
    return T, Y0, tg[torch.as_tensor(idx, device=tg.device)]


def ten_slot_batch(B, params=None):
    """UR10 + one spherical obstacle: the only packaged graph with ten terms on a node (rtr_wave_kernel<3, 10, ...>)."""
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    robot, graph = make_graph("ur10")
    graph.add_spherical_obstacle("o0", np.array([0.6, 0.1, 0.4]), 0.15)
    prob = BatchProblem(graph, use_limits=True, params=params)
    assert prob.template.info["max_terms_per_node"] == 10 and prob.template.info["hessian_form"] == 1
    lb, ub = robot.limits_arrays()
    Tg = robot.fk_batch(lb + (ub - lb) * np.random.RandomState(11).rand(64, robot.n))[np.arange(B) % 64]
    targets, Y0 = prob.prepare(Tg)
    Y0 = np.asarray(Y0) + 1e-3 * np.random.RandomState(0).randn(*np.asarray(Y0).shape)
    return prob.template, Y0, targets


def solved(torch, T, Y0, tg, trace_cap=0):
    r = T.solve(Y0, tg, trace_cap=trace_cap)
    torch.cuda.synchronize()
    out = {k: r[k].cpu().numpy() for k in FIELDS + ("flags",)}
    if trace_cap:
        out["trace"] = {k: v.cpu().numpy() for k, v in r["trace"].items()}
    return out


def digest(out):
    h = hashlib.sha256()
    for k in DIGEST_FIELDS:
        h.update(out[k].tobytes())
    return h.hexdigest()[:16]


@pytest.mark.parametrize("case", ["lwa4d", "kuka", "ur10-ten-slots"])
def test_split_build_equals_the_one_piece_build(torch_cuda, monkeypatch, case):
    make = (lambda B: ten_slot_batch(B)) if case == "ur10-ten-slots" else (lambda B: golden_batch(case, B))
    T, _, _ = make(1)
    B = 2 * 8 * T.info["n_cu"]
    T, Y0, tg = make(B)
    assert T.info["hessian_form"] == 1 and T.info["problems_per_wave"] == 1
    assert B <= 6 * 4 * T.info["n_cu"]      # gik_plan.h: the default plan of this batch is one wave per SIMD
    split = solved(torch_cuda, T, Y0, tg)
    assert not (split["flags"] & 2).any()   # nothing paused: the plain kernel
    monkeypatch.setenv("GIK_WAVES_PER_CU", "8")      # (read once, at creation)
    Ts, _, _ = make(1)
    monkeypatch.delenv("GIK_WAVES_PER_CU")
    spread = solved(torch_cuda, Ts, Y0, tg)
    moved = (spread["flags"] & 2) != 0
    print(case, "B", B, "moved", int(moved.sum()), "hand-overs", int((spread["flags"] >> 8).sum()),
          "iterations", int(split["iterations"].sum()), "maxiter problems", int((split["stop"] == 1).sum()))
    assert moved.any(), "no problem was handed over: the batch did not run on the tail-spreading build"
    assert int(split["iterations"].min()) >= 1
    for k in FIELDS:
        if k == "inner_executed":
            assert np.array_equal(split[k][~moved], spread[k][~moved]), k
            assert np.all(spread[k][moved] >= split[k][moved]), k
        else:
            assert split[k].tobytes() == spread[k].tobytes(), k


_cold = {}


def cold_run(torch, name, flags=0):
    if (name, flags) not in _cold:
        T, Y0, tg = golden_batch("lwa4d", 64, dict(COLD_SETS[name], debug_flags=flags))
        _cold[name, flags] = solved(torch, T, Y0, tg, trace_cap=TRACE_CAP)
    return _cold[name, flags]


def test_cold_block_exits_all_occur(torch_cuda):
    """mininner4 and mix run the theta = 1 builds -- the ones with the hand-written test: between them every exit."""
    seen = {}
    for name in COLD_SETS:
        out = cold_run(torch_cuda, name)
        codes = set()
        for g in range(64):
            codes.update(out["trace"]["stop"][g, :min(TRACE_CAP, int(out["iterations"][g]))].tolist())
        seen[name] = codes
    print({k: sorted(v) for k, v in seen.items()})
    assert seen["mininner4"] | seen["mix"] == {0, 1, 2, 3, 4, 5}, seen
    assert 4 in seen["maxinner5"] and 5 in seen["theta2"], seen


@pytest.mark.parametrize("name", sorted(COLD_SETS))
def test_cold_block_against_the_oracle_and_the_parent(torch_cuda, parent, name):
    from oracle import c_oracle as co
    d = load_golden("lwa4d")
    kw = COLD_SETS[name]
    out = cold_run(torch_cuda, name)
    idx = np.arange(64) % len(d["Y_init"])
    Y0 = d["Y_init"][idx] + 1e-3 * np.random.RandomState(0).randn(64, *d["Y_init"].shape[1:])
    for g in range(0, 64, 4):
        o = co.rtr_solve(Y0[g], d["D_goal"][idx[g]], d["omega"], d["psi_L"], d["psi_U"], True, traj_cap=12, **kw)
        m = min(5, int(out["iterations"][g]), o["iterations"])
        for key in ("numit", "stop", "accept"):
            assert np.array_equal(out["trace"][key][g][:m], o["traj"][key][:m]), (g, key)
    print(name, digest(out), "parent", parent["cold"][name])
    assert digest(out) == parent["cold"][name]["sha"]
    assert int(out["iterations"].sum()) == parent["cold"][name]["iterations"]


@pytest.mark.parametrize("name", ["default"] + sorted(COLD_SETS))
def test_retrace_off_changes_nothing(torch_cuda, name):
    if name == "default":
        T, Y0, tg = golden_batch("lwa4d", 64)
        a = solved(torch_cuda, T, Y0, tg)
        T, Y0, tg = golden_batch("lwa4d", 64, {"debug_flags": 16})
        b = solved(torch_cuda, T, Y0, tg)
    else:
        a, b = cold_run(torch_cuda, name), cold_run(torch_cuda, name, 16)
        for k in a["trace"]:
            assert a["trace"][k].tobytes() == b["trace"][k].tobytes(), k
    # inner_executed is what Retrace saves: the one field that has to differ
    assert np.all(b["inner_executed"] >= a["inner_executed"])
    if name == "default":
        assert (b["inner_executed"] > a["inner_executed"]).any(), "Retrace skipped no product: the flag did nothing"
    for k in FIELDS:
        if k != "inner_executed":
            assert a[k].tobytes() == b[k].tobytes(), k


@pytest.mark.parametrize("name", ["lwa4d", "kuka", "ur10"])
def test_digest_of_512_problems_is_the_parents(torch_cuda, parent, name):
    T, Y0, tg = golden_batch(name, 512)
    out = solved(torch_cuda, T, Y0, tg)
    print(name, digest(out), int(out["iterations"].sum()), "parent", parent["digest_512"][name])
    assert digest(out) == parent["digest_512"][name]["sha"]
    assert int(out["iterations"].sum()) == parent["digest_512"][name]["iterations"]
