"""Position goals, host side (CPU only): BatchProblem(graph, goal=...) against the reference's graph.from_pos flow
(tests/golden/position_goals.npz, tools/capture_golden_position.py) -- the edge pattern, D_goal, bound smoothing, the
oracle's trust-region solves from the reference's Y_init, joint_variables without T_final, the pose errors -- the
argument checks of the goal= keyword, and plan_prepare's rule for templates whose inert goal slots are all position
goals (tests/host/prep_plan_position.cpp)."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_golden, make_graph, planar_tree

# scenario -> the goal= argument of its fixture
SCENARIOS = {"ur10": "position", "lwa4d": "position", "planar10_limits_pi": "position",
             "planar_tree_y5": ("position", "position"), "tree5": ("pose", "position")}


def position_graph(name):
    if name == "tree5":
        from test_host_layer import tree_robot
        return tree_robot()
    if name == "planar_tree_y5":
        return planar_tree("y5")
    return make_graph(name)


def position_fixture(name):
    d = load_golden("position_goals")
    return {k[len(name) + 2:]: d[k] for k in d.files if k.startswith(name + "__")}


def fixture_goals(name, d):
    """The goal array of a scenario as its entries take it: positions where every end effector is one, else poses."""
    if all(k == "position" for k in d["kinds"]):
        return d["goal_pos"][:, 0] if d["goal_pos"].shape[1] == 1 else d["goal_pos"]
    return d["T_goal"]


def _problem(name, **kw):
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    robot, graph = position_graph(name)
    return BatchProblem(graph, goal=SCENARIOS[name], host_only=True, **kw), graph


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_position_problem_matches_reference_goal_graph(name):
    """omega, D_goal and bound smoothing of from_pos({p_e: xyz}) (tree5: from_pos({p4, q4, p5}))."""
    from graphik_amd.utils import dgp
    d = position_fixture(name)
    bp, graph = _problem(name)
    assert list(d["node_ids"]) == list(graph.node_ids) and list(d["end_effectors"]) == list(bp.end_effectors)
    assert tuple(d["kinds"]) == bp.goal_kinds
    assert np.array_equal(bp.omega, d["omega"])
    T = bp.goal_poses(fixture_goals(name, d))
    D, lo, up = bp.assemble(T)
    assert np.abs(D - d["D_goal"]).max() < 1e-12
    lb, ub = dgp.floyd_warshall_bounds(lo, up)
    assert np.abs(lb - d["lb"]).max() < 1e-12 and np.abs(ub - d["ub"]).max() < 1e-12
    # positions and the poses they came from are the same goal
    assert np.array_equal(bp.assemble(d["T_goal"] if bp.multi_ee else d["T_goal"][:, 0])[0], D)


def test_ur10_position_template_has_four_terms_fewer():
    """The pose pattern minus the four anchor <-> q_n edges (50 edges against 54)."""
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    robot, graph = make_graph("ur10")
    pose, pos = BatchProblem(graph, host_only=True), BatchProblem(graph, goal="position", host_only=True)
    assert len(pose.terms[0]) - len(pos.terms[0]) == 4
    assert int(np.triu(pose.omega).sum()) == 54 and int(np.triu(pos.omega).sum()) == 50
    gone = np.argwhere(np.triu(pose.omega - pos.omega) != 0)
    q6 = graph.index("q6")
    assert len(gone) == 4 and all(q6 in pair for pair in gone.tolist())
    assert pos.goal_nodes == [graph.index("p6")] and pose.goal_nodes == [graph.index("p6"), q6]
    assert pos.claim_key_nodes() == pose.claim_key_nodes() == [graph.index("p6")]


@pytest.mark.parametrize("name", ["ur10", "lwa4d", "planar10_limits_pi", "planar_tree_y5", "tree5"])
def test_pose_is_the_default(name):
    """goal="pose", spelled out or per end effector, gives the arrays a problem without the argument has."""
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    robot, graph = position_graph(name)
    a = BatchProblem(graph, host_only=True)
    T = position_fixture(name)["T_goal"]
    T = T if a.multi_ee else T[:, 0]
    for goal in ("pose", ["pose"] * len(a.end_effectors)):
        b = BatchProblem(graph, goal=goal, host_only=True)
        assert b.goal_nodes == a.goal_nodes and b.anchor_nodes == a.anchor_nodes
        for key in ("omega", "base_D", "base_lower", "base_upper"):
            assert np.array_equal(getattr(a, key), getattr(b, key), equal_nan=True), key
        for x, y in zip(a.terms, b.terms):
            assert np.array_equal(x, y, equal_nan=True)
        assert np.array_equal(a.goal_positions(T), b.goal_positions(T))
        for x, y in zip(a.assemble(T), b.assemble(T)):
            assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_oracle_reproduces_reference_position_solves(name):
    """The oracle from the reference's Y_init on the position-goal problem, with the bars of test_oracle_golden.py:
    3-D -- the loop path's prefix over min(20, how long the reference's two paths agree) where both are recorded, the
    first five outer iterations of the numpy path everywhere; planar -- every decision but the last two iterations',
    f to 1e-7 and the point to 1e-9; and the same convergence class."""
    from oracle import c_oracle as co
    from parity_util import CONTRACT_K, TRAJ_KEYS, assert_prefix_equal, first_divergence, stable_prefix
    d = position_fixture(name)
    bp, graph = _problem(name)
    for g in range(len(d["seed"])):
        r = co.rtr_solve(d["Y_init"][g], d["D_goal"][g], bp.omega, bp.psi_L, bp.psi_U, True, traj_cap=32)
        npp = {k: d[f"traj_{k}"][g] for k in TRAJ_KEYS}
        assert (r["f(x)"] < 1e-9) == (d["f"][g] < 1e-9)
        if graph.dim == 3:
            assert_prefix_equal(r["traj"], npp, 5)
            if "loop_iterations" in d and g < len(d["loop_iterations"]):
                loop = {k: d[f"loop_traj_{k}"][g] for k in TRAJ_KEYS}
                n = min(32, r["iterations"], int(d["loop_iterations"][g]), int(d["iterations"][g]))
                m = max(5, min(CONTRACT_K, stable_prefix(npp, loop, n)))
                assert_prefix_equal(r["traj"], loop, m)
                assert first_divergence(r["traj"], npp, n) >= min(CONTRACT_K, first_divergence(loop, npp, n)) - 1, g
        else:
            n = int(d["iterations"][g])
            assert abs(r["iterations"] - n) <= 1
            m = min(n, r["iterations"]) - 2
            for key in ("numit", "stop", "accept", "Delta"):
                assert np.array_equal(r["traj"][key][:m], npp[key][:m]), (g, key)
            assert np.allclose(r["traj"]["f_before"][:m], npp["f_before"][:m], rtol=1e-7, atol=1e-24)
            assert np.abs(r["x"] - d["Y_sol"][g]).max() < 1e-9


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_joint_variables_and_pose_errors_without_t_final(name):
    """joint_variables of the reference's Y_sol: T_final only for the pose end effectors; rot_err 0 for position
    goals (tree5: the pose end effector's alone); pos_err the worst end effector's."""
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    from parity_util import wrap_abs
    d = position_fixture(name)
    bp, graph = _problem(name)
    T = d["T_goal"] if bp.multi_ee else d["T_goal"][:, 0]
    q = bp.joint_variables(d["Y_sol"], T)
    assert wrap_abs(q - d["q_sol"]).max() < 1e-9
    pos, rot = bp.pose_errors(q, T)
    assert np.abs(pos - d["pos_err"]).max() < 1e-9
    if name == "tree5":
        _, rot4 = BatchProblem._pose_err(bp.robot.fk_batch(q, 4), T[:, 0], 3)
        assert np.array_equal(rot, rot4)
        # p4's orientation counts, p5's does not: turn either goal frame by 0.3 rad about its z axis
        c, s = np.cos(0.3), np.sin(0.3)
        Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        for e, want in ((0, 0.3), (1, 0.0)):
            T2 = T.copy()
            T2[:, e, :3, :3] = T[:, e, :3, :3] @ Rz
            assert np.abs(bp.pose_errors(q, T2)[1] - (rot + want)).max() < 1e-7      # (acos near 1: sqrt of the round-off)
    else:
        assert rot.dtype == np.float64 and np.array_equal(rot, np.zeros(len(q)))
    # packed positions carry no orientation: the same answers
    if name != "tree5":
        Tp = bp.goal_poses(fixture_goals(name, d))
        assert np.array_equal(bp.joint_variables(d["Y_sol"], Tp), q)
        pos2, rot2 = bp.pose_errors(q, Tp)
        assert np.array_equal(pos2, pos) and np.array_equal(rot2, rot)


def test_goal_argument_errors():
    from graphik_amd.solvers.riemannian_solver import (AnchoredProblem, BatchProblem, goal_kinds, goal_poses, solve_batch,
                                                       solve_trajectory)
    robot, graph = make_graph("ur10")
    tree = position_graph("tree5")[1]
    with pytest.raises(ValueError, match="unknown goal kind"):
        BatchProblem(graph, goal="orientation", host_only=True)
    with pytest.raises(ValueError, match="unknown goal kind"):
        BatchProblem(tree, goal=("pose", "axis"), host_only=True)
    with pytest.raises(ValueError, match="unknown goal kind"):
        BatchProblem(graph, goal=[1], host_only=True)
    with pytest.raises(ValueError, match="2 entries for 1 end effector"):
        BatchProblem(graph, goal=("position", "position"), host_only=True)
    with pytest.raises(ValueError, match="1 entries for 2 end effectors"):
        BatchProblem(tree, goal=["position"], host_only=True)
    with pytest.raises(ValueError, match="sequence"):
        goal_kinds(None, 1)
    # goal arrays, checked before any device work
    P = np.zeros((4, 3))
    for bad in (np.zeros((4, 2)), np.zeros((4, 2, 3)), np.zeros((4, 3, 3)), np.zeros(3), np.zeros((4, 1, 1, 3))):
        with pytest.raises(ValueError, match="goal array of shape"):
            solve_batch(graph, bad, goal="position")
    with pytest.raises(ValueError, match="goal array of shape"):       # mixed kinds take poses
        solve_batch(tree, np.zeros((4, 2, 3)), goal=("pose", "position"))
    with pytest.raises(ValueError, match="goal array of shape"):
        solve_trajectory(graph, np.zeros((4, 3)), np.zeros(6), goal="position")      # (a path has a waypoint axis)
    with pytest.raises(ValueError, match="unknown goal kind"):
        solve_batch(graph, P, goal="point")
    # the seed rules are today's
    with pytest.raises(ValueError, match="not both"):
        solve_batch(graph, P, goal="position", Y_init=np.zeros((4, 16, 3)), q_init=np.zeros((4, 6)))
    with pytest.raises(ValueError, match="shape"):
        solve_batch(graph, P, goal="position", q_init=np.zeros((3, 6)))
    with pytest.raises(ValueError, match="cannot be combined with Y_init"):
        solve_batch(graph, P, goal="position", Y_init=np.zeros((4, 16, 3)), retries=1)
    # packing
    assert goal_poses(P, ("position",), 3).shape == (4, 4, 4)
    assert goal_poses(P[:, None], ("position",), 3).shape == (4, 1, 4, 4)
    assert goal_poses(np.zeros((4, 5, 2, 2)), ("position",) * 2, 2, lead=2).shape == (4, 5, 2, 3, 3)
    one = goal_poses(np.array([[1.0, 2.0, 3.0]]), ("position",), 3)[0]
    assert np.array_equal(one, [[1, 0, 0, 1], [0, 1, 0, 2], [0, 0, 1, 3], [0, 0, 0, 1]])
    with pytest.raises(NotImplementedError, match="pose goals"):
        AnchoredProblem(graph, goal="position", host_only=True)


def test_problem_cache_keeps_the_kinds_apart(monkeypatch):
    from graphik_amd.solvers import riemannian_solver as rs
    robot, graph = make_graph("ur10")
    made = []

    class Stub:
        def __init__(self, graph, use_limits, params, device, goal="pose"):
            made.append(goal)
            self.graph = graph

    monkeypatch.setattr(rs, "BatchProblem", Stub)
    monkeypatch.setattr(rs, "_PROBLEM_CACHE", type(rs._PROBLEM_CACHE)())
    a = rs._problem_for(graph)
    b = rs._problem_for(graph, goal="position")
    assert a is not b and made == [("pose",), ("position",)]
    assert rs._problem_for(graph, goal="pose") is a and rs._problem_for(graph, goal=["position"]) is b
    assert len(made) == 2


def test_prepare_plan_with_position_goals(tmp_path):
    """plan_prepare (gik_plan.h): inert slots that are all position goals keep the four-goals-per-wavefront kernel."""
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler (c++, g++, clang++) on this machine")
    exe = str(tmp_path / "prep_plan_position")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(REPO, "graphik_amd", "csrc"),
                    os.path.join(REPO, "tests", "host", "prep_plan_position.cpp"), "-o", exe], check=True)
    rows = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout)
    got = {(r["N"], r["inert"], r["position"], r["no_quad"]): r["variant"] for r in rows}
    assert got[(13, 1, 1, 0)] == "quad13" and got[(16, 1, 1, 0)] == "quad"
    assert got[(13, 1, 0, 0)] == got[(16, 1, 0, 0)] == "wave"
    assert got[(17, 1, 1, 0)] == got[(17, 1, 0, 0)] == got[(17, 0, 0, 0)] == "wave"
    assert got[(13, 0, 0, 0)] == "quad13" and got[(16, 0, 0, 0)] == "quad"      # (no inert slot: as before)
    assert got[(13, 1, 1, 1)] == got[(16, 1, 1, 1)] == "wave"                  # (GIK_NO_PREP_QUAD still wins)
    # the position flag changes nothing else of a plan
    by = {(r["N"], r["inert"], r["position"], r["no_quad"]): r for r in rows}
    for N in (13, 16):
        a, b = by[(N, 0, 0, 0)], by[(N, 1, 1, 0)]
        assert (a["lds"], a["wpc"], a["wave_lds"], a["wave_wpc"]) == (b["lds"], b["wpc"], b["wave_lds"], b["wave_wpc"])
