"""Joint-configuration warm starts, host side (CPU only): the batched realization BatchProblem.seed_points
against the reference's pos_from_graph(graph.realization(q_init)), the oracle's seeded trust-region solves
against the reference's RiemannianSolver.solve(..., Y_init=..., bounds=None), and solve_batch's argument
checks.  Fixture: tests/golden/seeded.npz (tools/capture_golden_seeded.py)."""
import numpy as np
import pytest

from conftest import load_golden, make_graph

GRAPHS = ["lwa4d", "ur10", "planar10_limits_pi", "tree5"]


def _graph(name):
    if name == "tree5":
        from test_host_layer import tree_robot
        return tree_robot()
    return make_graph(name)


def _fixture(name):
    d = load_golden("seeded")
    return {k[len(name) + 2:]: d[k] for k in d.files if k.startswith(name + "__")}


@pytest.mark.parametrize("name", GRAPHS + ["ur10_table"])
def test_seed_points_match_reference_realization(name):
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    d = _fixture(name)
    robot, graph = _graph(name)
    bp = BatchProblem(graph, host_only=True)
    Y = bp.seed_points(d["q_init"])
    assert Y.shape == d["Y_init"].shape
    assert np.abs(Y - d["Y_init"]).max() < 1e-12
    # one seed for every goal broadcasts; a single configuration is a batch of one
    assert np.array_equal(bp.seed_points(d["q_init"][3]), Y[3:4])


def _above_floor(f_before, dim):
    """Leading outer iterations whose f is still above the level at which the iterate's round-off decides f's
    leading digits: a seeded solve starts near the solution, where f ~ |Y - Y*|^2 and a 1e-13 difference in Y
    is already a 1e-4 relative difference in f = 1e-10 (3-D; planar chains hold 1e-7 down to f = 1e-10)."""
    floor = 1e-8 if dim == 3 else 1e-10
    below = np.flatnonzero(~(np.asarray(f_before) >= floor))
    return int(below[0]) if len(below) else len(f_before)


def assert_seeded_prefix(t, o, m, dim):
    """Trajectory prefix of a seeded solve: decisions (inner iterations, tCG stop reason, acceptance, radius)
    identical over the first m outer iterations, f before each to 1e-8 (planar 1e-7) and |grad| after each
    step but the last to 1e-8 (planar 1e-6).  3-D: the first outer iteration only.  Started near the solution,
    the tCG calls run ~20-60 inner iterations on a nearly singular Hessian: from the second call on, the
    reference's own costs.py loops and the oracle, which restates them, can end one inner iteration apart and
    differ at 5e-4 relative in |grad| (LWA4D, UR10), so nothing further can be promised step by step -- 3-D is
    pinned by its answers.  Planar: the rule of the cold-start planar tests above the floor."""
    assert m >= 1
    if dim == 3:
        m = min(m, 1)
    for key in ("numit", "stop", "accept", "Delta"):
        assert np.array_equal(t[key][:m], o[key][:m]), (key, t[key][:m], o[key][:m])
    rtol = 1e-8 if dim == 3 else 1e-7
    assert np.allclose(t["f_before"][:m], o["f_before"][:m], rtol=rtol, atol=0), (t["f_before"][:m], o["f_before"][:m])
    assert np.allclose(t["gradnorm_after"][:m - 1], o["gradnorm_after"][:m - 1], rtol=rtol if dim == 3 else 1e-6,
                       atol=0), (t["gradnorm_after"][:m - 1], o["gradnorm_after"][:m - 1])


@pytest.mark.parametrize("name", GRAPHS)
def test_oracle_reproduces_reference_seeded_solves(name):
    """The oracle from the reference's seed against the reference's costs.py-loop path (the one the oracle
    restates): the trajectory prefix (assert_seeded_prefix, over the iterations above the round-off floor),
    and the same answers."""
    from oracle import c_oracle as co
    from parity_util import TRAJ_KEYS, wrap_abs
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    d = _fixture(name)
    robot, graph = _graph(name)
    bp = BatchProblem(graph, host_only=True)
    D = bp.assemble(d["T_goal"])[0]
    use_lim = bool(int(d["use_limits"]))
    for g in range(len(d["q_init"])):
        o = co.rtr_solve(d["Y_init"][g], D[g], bp.omega, bp.psi_L, bp.psi_U, use_lim, traj_cap=48)
        ref = {k: d[f"loop_traj_{k}"][g] for k in TRAJ_KEYS}
        its = int(d["loop_iterations"][g])
        assert_seeded_prefix(o["traj"], ref, min(_above_floor(ref["f_before"], graph.dim), its), graph.dim)
        assert (o["f(x)"] < 1e-9) == (d["f"][g] < 1e-9)
        if robot.n == 6 or name == "tree5":       # isolated solutions: the same joint angles
            q = bp.joint_variables(o["x"][None], d["T_goal"][g:g + 1] if name == "tree5" else d["T_goal"][g:g + 1, 0])
            assert wrap_abs(q[0] - d["q_sol"][g]).max() < 5e-3, g


def test_solve_batch_rejects_bad_seeds():
    """Checked before any device work: Y_init together with q_init, a wrong shape, a non-finite angle."""
    from graphik_amd.solvers.riemannian_solver import solve_batch, solve_trajectory
    robot, graph = make_graph("lwa4d")
    d = _fixture("lwa4d")
    T = d["T_goal"][:4, 0]
    q = d["q_init"][:4]
    with pytest.raises(ValueError, match="not both"):
        solve_batch(graph, T, Y_init=d["Y_init"][:4], q_init=q)
    for bad in (q[:3], q[:, :6], np.zeros(6), np.zeros((4, 7, 1))):
        with pytest.raises(ValueError, match="shape"):
            solve_batch(graph, T, q_init=bad)
    nan = q.copy()
    nan[2, 3] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        solve_batch(graph, T, q_init=nan)
    inf = q[0].copy()
    inf[0] = np.inf
    with pytest.raises(ValueError, match="non-finite"):
        solve_batch(graph, T, q_init=inf)
    with pytest.raises(ValueError, match="q_start"):
        solve_trajectory(graph, np.stack([T, T], axis=1), q[:, :5])
