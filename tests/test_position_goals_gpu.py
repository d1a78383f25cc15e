"""Position goals on the MI355X (goal="position"): the device prepare (four goals per wavefront and one), recover and
solve against the reference's graph.from_pos flow (tests/golden/position_goals.npz) and the host mirror, the
combinations with q_init, retries and solve_trajectory, the refusals of the C ABI, and goal="pose" unchanged.
Batch sizes 1, 4, 5 and 67: one group of four, a group plus one, past one 64-thread recover block."""
import ctypes as C

import numpy as np
import pytest

from test_position_goals_host import SCENARIOS, position_fixture, position_graph

pytestmark = pytest.mark.gpu

SIZES = (1, 4, 5, 67)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_PROBLEMS = {}


def _problem(name, goal=None):
    """One BatchProblem (device template + pipeline) per (graph, kinds) for the whole module."""
    goal = SCENARIOS[name] if goal is None else goal
    key = (name, str(goal))
    if key not in _PROBLEMS:
        from graphik_amd.solvers.riemannian_solver import BatchProblem
        robot, graph = position_graph(name)
        bp = BatchProblem(graph, goal=goal)
        assert bp.device_pipeline
        _PROBLEMS[key] = (robot, graph, bp)
    return _PROBLEMS[key]


def _poses(name, B, seed=5):
    """B goal poses of a scenario ([B, d+1, d+1], trees [B, n_ee, d+1, d+1]): the fixture's, then random configurations."""
    robot, graph = position_graph(name)
    d = position_fixture(name)
    lb, ub = robot.limits_arrays()
    Q = np.random.RandomState(seed).uniform(lb, ub, size=(B, robot.n))
    ees = list(robot.end_effectors)
    T = np.stack([robot.fk_batch(Q, int(e[1:])) for e in ees], axis=1)
    n = min(B, len(d["T_goal"]))
    T[:n] = d["T_goal"][:n]
    return T if len(ees) > 1 else T[:, 0]


def _points(name, T):
    """... as the goal array of the scenario's entries: positions where every end effector is one."""
    if all(k == "position" for k in np.atleast_1d(SCENARIOS[name])):
        d = T.shape[-1] - 1
        return T[..., :d, d]
    return T


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_prepare_against_host_and_reference(torch_cuda, name):
    """Targets == the host's to 1e-12 at every batch size; bound smoothing (gik_prepare_batch_debug) == the
    reference's to 1e-12; the initial point classified as test_device_prepare_against_reference_fixtures does."""
    from test_hip_gpu import _classify_init
    from graphik_amd.utils import dgp
    robot, graph, bp = _problem(name)
    d = position_fixture(name)
    T = _poses(name, max(SIZES))
    want = bp.targets_from_D(bp.assemble(T)[0])
    for B in SIZES:
        tg, Y = bp.template.prepare(T[:B])
        assert np.abs(tg.cpu().numpy() - want[:B]).max() < 1e-12, B
        assert np.all(np.isfinite(Y.cpu().numpy())), B
        # positions and the poses they were cut from are the same goals
        tg2, _ = bp.template.prepare(bp.goal_poses(_points(name, T[:B])))
        assert torch_cuda.equal(tg, tg2)
    Tf = d["T_goal"] if bp.multi_ee else d["T_goal"][:, 0]
    r = bp.template.prepare_debug(Tf)
    assert np.abs(r["lb"].cpu().numpy() - d["lb"]).max() < 1e-12 and np.abs(r["ub"].cpu().numpy() - d["ub"]).max() < 1e-12
    Y_ref, info_ref = dgp.generate_initialization_batch(d["lb"], d["ub"], graph.dim, d["omega"], canonical=False,
                                                        return_info=True)
    assert np.abs(Y_ref @ np.swapaxes(Y_ref, 1, 2) - d["Y_init"] @ np.swapaxes(d["Y_init"], 1, 2)).max() < 1e-8
    Y_d, K_d = r["Y_init"].cpu().numpy(), r["K"].cpu().numpy()
    cls = _classify_init(Y_d, K_d, d["Y_init"], info_ref)
    mask = cls.pop("mask_identical")
    print(name, cls)
    assert cls["unexplained"] == 0, cls
    near = np.any((info_ref["ev_rank"] > 0.25e-8) & (info_ref["ev_rank"] < 4e-8), axis=1)
    assert np.all((mask | near)[K_d == info_ref["K"]])


@pytest.mark.parametrize("name", ["ur10", "planar10_limits_pi"])
def test_quad_prepare_kernel_takes_position_goals(torch_cuda, monkeypatch, name):
    """UR10 (N = 16) and planar-10 (N = 13) with a position goal have an inert odd slot and still run four goals per
    wavefront; against prep_wave_kernel (GIK_NO_PREP_QUAD at attach): targets bit for bit, initial points to 1e-12."""
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    robot, graph = position_graph(name)
    quad = BatchProblem(graph, goal="position")
    monkeypatch.setenv("GIK_NO_PREP_QUAD", "1")
    wave = BatchProblem(graph, goal="position")
    assert quad.template.info["goals_per_wave"] == 4 and wave.template.info["goals_per_wave"] == 1
    T = _poses(name, max(SIZES))
    for B in SIZES:
        tq, Yq = [x.cpu().numpy() for x in quad.template.prepare(T[:B])]
        tw, Yw = [x.cpu().numpy() for x in wave.template.prepare(T[:B])]
        assert np.array_equal(tq, tw), B
        print(name, B, "max |Y_quad - Y_wave|", np.abs(Yq - Yw).max())
        assert np.abs(Yq - Yw).max() < 1e-12, B


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_recover_without_t_final(torch_cuda, name):
    """recover_kernel on the reference's Y_sol: q == joint_variables(G_sol) with T_final for the pose end effectors only,
    pos_err == the fixture's, rot_err exactly 0.0 (tree5: the pose end effector's alone), 67 rows."""
    from parity_util import wrap_abs
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    robot, graph, bp = _problem(name)
    d = position_fixture(name)
    n = len(d["Y_sol"])
    rows = np.arange(67) % n
    T = (d["T_goal"] if bp.multi_ee else d["T_goal"][:, 0])[rows]
    q, pos, rot = (x.cpu().numpy() for x in bp.template.recover(d["Y_sol"][rows], T))
    print(name, "max |q - q_sol|", wrap_abs(q - d["q_sol"][rows]).max(), "max |pos_err - ref|", np.abs(pos - d["pos_err"][rows]).max())
    assert wrap_abs(q - d["q_sol"][rows]).max() < 1e-9
    assert np.abs(pos - d["pos_err"][rows]).max() < 1e-9
    if name == "tree5":
        # (acos near 1 takes the square root of the round-off of its argument: a few ulp of 1 are up to 3e-8 rad)
        _, rot4 = BatchProblem._pose_err(robot.fk_batch(q, 4), T[:, 0], 3)
        assert np.abs(rot - rot4).max() < 1e-7
        c, s = np.cos(0.3), np.sin(0.3)
        T3 = T.copy()
        T3[:, 0, :3, :3] = T[:, 0, :3, :3] @ np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
        rot3 = bp.template.recover(d["Y_sol"][rows], T3)[2].cpu().numpy()
        assert np.abs(rot3 - (rot4 + 0.3)).max() < 1e-7      # (p4's orientation counts ...)
        # the position end effector's orientation plays no part: turn its goal frame upside down
        T2 = T.copy()
        T2[:, 1, :3, :3] = np.diag([1.0, -1.0, -1.0])
        q2, pos2, rot2 = (x.cpu().numpy() for x in bp.template.recover(d["Y_sol"][rows], T2))
        assert np.array_equal(q2, q) and np.array_equal(pos2, pos) and np.array_equal(rot2, rot)
    else:
        assert rot.dtype == np.float64 and np.array_equal(rot, np.zeros(67)) and not np.signbit(rot).any()
    for B in (1, 4, 5):
        qb, pb, rb = (x.cpu().numpy() for x in bp.template.recover(d["Y_sol"][rows[:B]], T[:B]))
        assert np.array_equal(qb, q[:B]) and np.array_equal(pb, pos[:B]) and np.array_equal(rb, rot[:B])


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_solve_against_oracle_and_reference(torch_cuda, name):
    """The device solve from the device's own start against the oracle from the same point (the rule of
    test_seeded_host.assert_seeded_prefix); solve_batch(goal=...) converges exactly where the reference does, and the
    position errors stay under the bars of test_seeded_gpu.py."""
    from oracle import c_oracle as co
    from test_seeded_host import _above_floor, assert_seeded_prefix
    from graphik_amd.solvers.riemannian_solver import solve_batch
    robot, graph, bp = _problem(name)
    d = position_fixture(name)
    Tf = d["T_goal"] if bp.multi_ee else d["T_goal"][:, 0]
    tg, Y0 = bp.template.prepare(Tf)
    r = bp.template.solve(Y0, tg, trace_cap=48)
    tr = {k: v.cpu().numpy() for k, v in r["trace"].items()}
    its = r["iterations"].cpu().numpy()
    Y0 = Y0.cpu().numpy()
    for g in range(len(Tf)):
        o = co.rtr_solve(Y0[g], d["D_goal"][g], bp.omega, bp.psi_L, bp.psi_U, True, traj_cap=48)
        m = min(_above_floor(o["traj"]["f_before"], graph.dim), int(its[g]), o["iterations"])
        assert_seeded_prefix({k: tr[k][g] for k in tr}, o["traj"], m, graph.dim)
    bar = 5e-3 if graph.dim == 3 else 1e-5
    for B in SIZES:
        T = _poses(name, B)
        q, Y, info = solve_batch(graph, _points(name, T), goal=SCENARIOS[name])
        n = min(B, len(Tf))
        conv = d["f"][:n] < 1e-9
        print(name, B, "f", info["f(x)"][:n], "pos_err", info["pos_err"][:n], "rot_err max", info["rot_err"].max())
        assert np.array_equal(info["f(x)"][:n] < 1e-9, conv)
        assert np.all(info["pos_err"][:n][conv] < bar)
        if name != "tree5":
            assert np.array_equal(info["rot_err"], np.zeros(B))
        assert q.shape == (B, robot.n) and Y.shape == (B, bp.N, graph.dim)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_seed_targets_equal_prepare_targets(torch_cuda, name):
    robot, graph, bp = _problem(name)
    T = _poses(name, 67)
    lb, ub = robot.limits_arrays()
    Q = np.random.RandomState(2).uniform(lb, ub, size=(67, robot.n))
    tg_seed, Y = bp.template.seed(T, Q)
    tg_prep, _ = bp.template.prepare(T)
    assert torch_cuda.equal(tg_seed, tg_prep)
    assert np.abs(Y.cpu().numpy() - bp.seed_points(Q)).max() < 1e-12      # (the seed places every node, q_e included)


def test_retries_on_lwa4d_position_goals(torch_cuda):
    """retries=2 on 67 goals: a goal that did not fail keeps attempt 0 and is bit for bit the retries=0 run's; the failure
    rule's numpy mirror (rot_err = 0 never fails it) agrees on every goal."""
    from test_retry_gpu import ROW_KEYS, _failed, _rows, _same_rows, _triple
    from graphik_amd.solvers.riemannian_solver import solve_batch
    robot, graph = position_graph("lwa4d")
    P_goal = _points("lwa4d", _poses("lwa4d", 67, seed=9))
    params = {"maxiter": 150}      # (a short budget: some goals fail the first attempt)
    P = solve_batch(graph, P_goal, params=params, goal="position")
    R = solve_batch(graph, P_goal, params=params, goal="position", retries=2, retry_seed=3)
    att = R[2]["attempt"]
    failed_P = _failed(*_triple(P[2]))
    print("failed at first", int(failed_P.sum()), "attempts", np.bincount(att, minlength=3).tolist())
    assert np.array_equal(P[2]["rot_err"], np.zeros(67)) and np.array_equal(R[2]["rot_err"], np.zeros(67))
    assert np.array_equal(failed_P, (P[2]["stop"] != 0) | ~(P[2]["pos_err"] <= 0.01))      # (the rotation term dropped out)
    assert att.dtype == np.int32 and not np.any(att[~failed_P]) and att.max() <= 2
    assert _same_rows(_rows(R, att == 0), _rows(P, att == 0))
    assert np.sum(~_failed(*_triple(R[2]))) >= np.sum(~failed_P)
    assert set(ROW_KEYS) <= set(R[2])


def test_trajectory_equals_the_waypoint_loop(torch_cuda):
    """solve_trajectory(goal="position") on 5 paths of 3 waypoints == solve_batch(q_init=previous angles) per waypoint."""
    from graphik_amd.solvers.riemannian_solver import solve_batch, solve_trajectory
    robot, graph = position_graph("lwa4d")
    rng = np.random.RandomState(4)
    lb, ub = robot.limits_arrays()
    q0 = rng.uniform(0.6 * lb, 0.6 * ub, size=(5, robot.n))
    Qp = q0[:, None] + 0.02 * np.arange(3)[None, :, None]
    Pp = robot.fk_batch(Qp.reshape(-1, robot.n)).reshape(5, 3, 4, 4)[..., :3, 3]      # [5, 3, 3] positions
    q, Y, info = solve_trajectory(graph, Pp, q0, return_Y=True, goal="position")
    assert q.shape == (5, 3, robot.n) and np.array_equal(info["rot_err"], np.zeros((5, 3)))
    q_prev = q0
    for l in range(3):
        ql, Yl, il = solve_batch(graph, Pp[:, l], q_init=q_prev, goal="position")
        assert np.array_equal(ql, q[:, l]) and np.array_equal(Yl, Y[:, l]), l
        assert np.array_equal(il["iterations"], info["iterations"][:, l]) and np.array_equal(il["pos_err"], info["pos_err"][:, l])
        q_prev = ql
    assert np.all(info["pos_err"] < 5e-3)


def _attach_arguments(monkeypatch, graph, goal):
    """The keyword arguments BatchProblem hands to Template.attach_pipeline, and a fresh template of the same terms."""
    from graphik_amd import engine
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    seen = {}
    orig = engine.Template.attach_pipeline

    def spy(self, **kw):
        seen.update(kw)
        return orig(self, **kw)

    monkeypatch.setattr(engine.Template, "attach_pipeline", spy)
    bp = BatchProblem(graph, goal=goal)
    monkeypatch.setattr(engine.Template, "attach_pipeline", orig)
    fresh = lambda: engine.Template.from_matrices(bp.omega, bp.psi_L, bp.psi_U, k=graph.dim, use_limits=True)   # noqa: E731
    return bp, seen, fresh


def test_attach_refusals(torch_cuda, monkeypatch):
    """gik_pipeline_attach: a set bit with a non-negative odd slot, a bit at or beyond n_ee, a bit that
    last_link_along_z also has -- each its own message; the same descriptor without the fault attaches."""
    from graphik_amd import _ffi
    robot, graph = position_graph("ur10")
    bp, kw, fresh = _attach_arguments(monkeypatch, graph, "position")
    assert kw["position_goal_mask"] == 1 and kw["goal_nodes"][1] == -1 and kw["last_link_along_z"] == 0
    fresh().attach_pipeline(**kw)
    q6 = graph.index("q6")
    for bad, msg in ((dict(goal_nodes=[kw["goal_nodes"][0], q6]), "must be -1"),
                     (dict(position_goal_mask=2), "at or beyond n_ee"),
                     (dict(position_goal_mask=3), "at or beyond n_ee"),
                     (dict(position_goal_mask=-1), "at or beyond n_ee"),
                     (dict(last_link_along_z=1), "last_link_along_z")):
        with pytest.raises(_ffi.GikError, match=msg):
            fresh().attach_pipeline(**dict(kw, **bad))
    # several end effectors: the odd slot of the position end effector, the bit beyond the last one
    tree = position_graph("tree5")[1]
    bp, kw, fresh = _attach_arguments(monkeypatch, tree, ("pose", "position"))
    assert kw["position_goal_mask"] == 2 and list(kw["ee_goal_nodes"])[3] == -1
    fresh().attach_pipeline(**kw)
    slots = list(kw["ee_goal_nodes"])
    with pytest.raises(_ffi.GikError, match="must be -1"):
        fresh().attach_pipeline(**dict(kw, ee_goal_nodes=slots[:3] + [tree.index("q5")]))
    with pytest.raises(_ffi.GikError, match="at or beyond n_ee"):
        fresh().attach_pipeline(**dict(kw, position_goal_mask=4))
    with pytest.raises(_ffi.GikError, match="bad ee_goal_nodes"):      # (a -1 odd slot without the bit: the old message)
        fresh().attach_pipeline(**dict(kw, position_goal_mask=0))
    # the point-axis setter: only for an end effector with a position goal
    t = fresh()
    t.attach_pipeline(**kw)
    lib = _ffi.lib()
    assert lib.gik_pipeline_set_point_axis(t._h, 0, 0.0, 1.0) != 0 and "position goal" in lib.gik_last_error().decode()
    assert lib.gik_pipeline_set_point_axis(t._h, 1, float("nan"), 1.0) != 0 and "finite" in lib.gik_last_error().decode()
    assert lib.gik_pipeline_set_point_axis(t._h, 1, 0.0, 1.0) == 0


def test_anchored_entry_refuses_a_position_base(torch_cuda):
    """gik_anchored_ik_batch with a base template that has position goals: non-zero, its message, nothing queued."""
    import torch
    from conftest import make_graph
    from graphik_amd import _ffi
    from graphik_amd.solvers.riemannian_solver import AnchoredProblem
    robot, graph = make_graph("ur10")
    graph.add_spherical_obstacle("o0", np.array([0.4, 0.3, 0.5]), 0.1)
    ap = AnchoredProblem(graph)
    base = _problem("ur10")[2].template      # the same robot graph, position goals
    B = 4
    out = ap.template.alloc_anchored_buffers(ap.base.template, B)
    for v in out.values():
        v.view(torch.uint8).fill_(0xA5)
    before = {k: v.clone() for k, v in out.items()}
    T = torch.from_numpy(np.ascontiguousarray(_poses("ur10", B))).cuda()
    lib = _ffi.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (T.data_ptr(), B, out["ws"].data_ptr(), out["Y"].data_ptr(), out["stats"].data_ptr(), out["q"].data_ptr(),
            out["pos_err"].data_ptr(), out["rot_err"].data_ptr(), stream)
    assert lib.gik_anchored_ik_batch(ap.template._h, base._h, *args) != 0
    assert "position goals" in lib.gik_last_error().decode()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k].view(torch.uint8), before[k].view(torch.uint8)) for k in out)
    assert lib.gik_anchored_ik_batch(ap.template._h, ap.base.template._h, *args) == 0      # (its own base: runs)
    torch.cuda.synchronize()
    assert not torch.equal(out["q"].view(torch.uint8), before["q"].view(torch.uint8))


@pytest.mark.parametrize("name", ["ur10", "lwa4d", "planar10_limits_pi", "tree5"])
def test_pose_goals_are_unchanged(torch_cuda, name):
    """goal="pose" at B = 5: q, Y and the statistics bit for bit those of a call without the argument."""
    from graphik_amd.solvers.riemannian_solver import BatchProblem, clear_problem_cache, solve_batch
    robot, graph = position_graph(name)
    T = _poses(name, 5)
    clear_problem_cache()
    a = solve_batch(graph, T)
    for goal in ("pose", ["pose"] * len(robot.end_effectors)):
        b = solve_batch(graph, T, goal=goal)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        for key in ("f(x)", "gradnorm", "iterations", "inner_iterations", "stop", "pos_err", "rot_err", "attempt"):
            assert np.array_equal(a[2][key], b[2][key]), key
    # ... and a problem built with the keyword runs the kernels of one built without it
    p0, p1 = BatchProblem(graph), BatchProblem(graph, goal="pose")
    assert p0.template.info == p1.template.info
    r0, r1 = p0.template.ik(T), p1.template.ik(T)
    for key in ("x", "q", "pos_err", "rot_err", "f", "iterations"):
        assert torch_cuda.equal(r0[key], r1[key]), key
