"""Joint-configuration warm starts on the MI355X: seed_kernel (gik_seed_batch) against the reference's
realization of the seed, the seeded device solve against the oracle and the reference, gik_ik_batch_seeded's
error paths, and path tracking (solve_trajectory).  Fixture: tests/golden/seeded.npz."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_graph
from test_seeded_host import GRAPHS, _above_floor, _fixture, _graph, assert_seeded_prefix

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _problem(name):
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    robot, graph = _graph(name)
    bp = BatchProblem(graph)
    assert bp.device_pipeline
    return robot, graph, bp


def _poses(d):
    T = d["T_goal"]
    return T[:, 0] if T.shape[1] == 1 else T      # chains [B, d+1, d+1], trees [B, n_ee, 4, 4]


@pytest.mark.parametrize("name", GRAPHS + ["ur10_table"])
def test_seed_matches_reference_and_prepare_targets(torch_cuda, name):
    """Y_init = the reference's pos_from_graph(graph.realization(q_init)) to 1e-12; targets bit-identical to
    gik_prepare_batch's (the same goal_distance helper and rule)."""
    d = _fixture(name)
    robot, graph, bp = _problem(name)
    tg, Y = bp.template.seed(_poses(d), d["q_init"])
    assert np.abs(Y.cpu().numpy() - d["Y_init"]).max() < 1e-12
    tg_prep, _ = bp.template.prepare(_poses(d))
    assert torch_cuda.equal(tg, tg_prep)
    # one seed broadcast to every goal
    _, Y1 = bp.template.seed(_poses(d), d["q_init"][0])
    assert np.abs(Y1.cpu().numpy() - d["Y_init"][0][None]).max() < 1e-12


@pytest.mark.parametrize("name", GRAPHS)
def test_seeded_solve_against_oracle_and_reference(torch_cuda, name):
    """The device solve from the device seed against the oracle from the same point: the trajectory prefix
    (test_seeded_host.assert_seeded_prefix: 3-D the first two outer iterations to 1e-8, planar decision for
    decision while f is above the round-off floor).  The answers (solve_batch(q_init=...)) within the bars of
    the drop-in tests: isolated solutions (UR10, the tree) in joint angles, redundant ones in end-effector
    position."""
    from oracle import c_oracle as co
    from parity_util import wrap_abs
    from graphik_amd.solvers.riemannian_solver import solve_batch
    d = _fixture(name)
    robot, graph, bp = _problem(name)
    T = _poses(d)
    tg, Y0 = bp.template.seed(T, d["q_init"])
    r = bp.template.solve(Y0, tg, trace_cap=48)
    tr = {k: v.cpu().numpy() for k, v in r["trace"].items()}
    its = r["iterations"].cpu().numpy()
    D = bp.assemble(d["T_goal"])[0]
    Y0 = Y0.cpu().numpy()
    for g in range(len(d["q_init"])):
        o = co.rtr_solve(Y0[g], D[g], bp.omega, bp.psi_L, bp.psi_U, True, traj_cap=48)
        m = min(_above_floor(o["traj"]["f_before"], graph.dim), int(its[g]), o["iterations"])
        assert_seeded_prefix({k: tr[k][g] for k in tr}, o["traj"], m, graph.dim)
    q, Y, info = solve_batch(graph, T, q_init=d["q_init"])
    conv = d["f"] < 1e-9
    assert np.array_equal(info["f(x)"] < 1e-9, conv)
    if name in ("ur10", "tree5"):
        assert np.all(wrap_abs(q - d["q_sol"])[conv].max(axis=1) < 5e-3)
    else:
        assert np.all(info["pos_err"][conv] < (5e-3 if graph.dim == 3 else 1e-5))


def test_seed_at_the_answer_stops_at_once(torch_cuda):
    """q_init = q_goal: the seed is a solution -- at most one outer iteration, and the recovered angles are the
    goal's (wrapped) to 1e-6."""
    from parity_util import wrap_abs
    from graphik_amd.solvers.riemannian_solver import solve_batch
    robot, graph = make_graph("lwa4d")
    rng = np.random.RandomState(3)
    lb, ub = robot.limits_arrays()
    Q = rng.uniform(lb, ub, size=(64, robot.n))
    q, Y, info = solve_batch(graph, robot.fk_batch(Q), q_init=Q)
    assert info["iterations"].max() <= 1
    assert wrap_abs(q - Q).max() < 1e-6


def _lwa4d_paths(B, L, step=0.02, seed=11):
    from graphik_amd.utils.roboturdf import load_schunk_lwa4d
    robot, graph = load_schunk_lwa4d()
    rng = np.random.RandomState(seed)
    lb, ub = robot.limits_arrays()
    q0 = rng.uniform(0.6 * lb, 0.6 * ub, size=(B, robot.n))
    direction = rng.choice([-1.0, 1.0], size=(B, robot.n))
    Qp = q0[:, None] + step * direction[:, None] * np.arange(L)[None, :, None]     # [B, L, n]
    T = robot.fk_batch(Qp.reshape(-1, robot.n)).reshape(B, L, 4, 4)
    return robot, graph, Qp, T


def test_solve_trajectory_tracks_lwa4d_paths(torch_cuda):
    """256 LWA4D paths x 16 waypoints, 0.02 rad per joint per waypoint: the waypoints are reached, the joint
    motion between waypoints stays small (the seeded solve keeps the IK branch), and waypoint l is exactly
    solve_batch(T[:, l], q_init=q[:, l - 1])."""
    from parity_util import wrap_abs
    from graphik_amd.solvers.riemannian_solver import solve_batch, solve_trajectory
    robot, graph, Qp, T = _lwa4d_paths(256, 16)
    q, Y, info = solve_trajectory(graph, T, Qp[:, 0], return_Y=True)
    assert q.shape == (256, 16, robot.n) and Y.shape == (256, 16, 18, 3)
    for key in ("iterations", "stop", "f(x)", "gradnorm", "pos_err", "rot_err"):
        assert info[key].shape == (256, 16), key
    assert np.mean(info["pos_err"] < 1e-3) >= 0.99
    jump = wrap_abs(q[:, 1:] - q[:, :-1]).max(axis=2)
    assert np.mean(jump < 0.2) >= 0.99
    for l in (1, 9, 15):
        ql, Yl, il = solve_batch(graph, T[:, l], q_init=q[:, l - 1])
        assert np.array_equal(ql, q[:, l]) and np.array_equal(Yl, Y[:, l]), l
        assert np.array_equal(il["iterations"], info["iterations"][:, l])
    q0, _, i0 = solve_batch(graph, T[:, 0], q_init=Qp[:, 0])
    assert np.array_equal(q0, q[:, 0])
    # without return_Y the same answers
    q2, Y2, _ = solve_trajectory(graph, T, Qp[:, 0])
    assert Y2 is None and np.array_equal(q2, q)


def test_seed_may_alias_the_answer(torch_cuda):
    """gik_ik_batch_seeded with d_q_init == d_q: the seed is read before the answer is written."""
    import torch
    from graphik_amd.solvers.riemannian_solver import _problem_for
    robot, graph, Qp, T = _lwa4d_paths(64, 2)
    prob = _problem_for(graph)
    tpl = prob.template
    ref = tpl.ik(T[:, 1], q_init=Qp[:, 0])
    out = tpl.alloc_ik_buffers(64)
    out["q"].copy_(torch.from_numpy(Qp[:, 0]))
    res = tpl.ik(T[:, 1], out=out, q_init=out["q"])
    assert res["q"].data_ptr() == out["q"].data_ptr()
    assert torch.equal(res["q"], ref["q"]) and torch.equal(res["x"], ref["x"])


def test_host_seed_fallback_without_device_pipeline(torch_cuda, monkeypatch):
    """A graph the device pipeline does not take is seeded on the host (BatchProblem.seed_points) and solved on
    the device; the answers agree with the device-seeded ones and the reference's within the drop-in bar."""
    from parity_util import wrap_abs
    from graphik_amd.solvers import riemannian_solver as rs
    d = _fixture("ur10")
    robot, graph = make_graph("ur10")
    T = _poses(d)
    q_dev, _, i_dev = rs.solve_batch(graph, T, q_init=d["q_init"])
    prob = rs._problem_for(graph)
    calls = []
    orig = rs.BatchProblem.seed_points

    def spy(self, q):
        calls.append(len(q))
        return orig(self, q)

    monkeypatch.setattr(rs.BatchProblem, "seed_points", spy)
    monkeypatch.setattr(prob, "device_pipeline", False)
    q_host, _, i_host = rs.solve_batch(graph, T, q_init=d["q_init"])
    assert calls == [len(T)]
    conv = i_dev["f(x)"] < 1e-9
    assert np.array_equal(i_host["f(x)"] < 1e-9, conv)
    # the two starts agree to ~1e-15, which a 3-D solve amplifies to ~1e-3 in where it stops (the drop-in bar)
    assert wrap_abs(q_host - q_dev)[conv].max() < 5e-3
    assert np.all(wrap_abs(q_host - d["q_sol"])[conv].max(axis=1) < 5e-3)
    # path tracking falls back to one host-seeded solve_batch per waypoint
    qt, _, it = rs.solve_trajectory(graph, np.stack([T, T], axis=1), d["q_init"])
    assert len(calls) == 3 and it["iterations"].shape == (len(T), 2)


def _hip_runtime():
    """The HIP runtime this process (torch, libgraphik_amd) already has loaded."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            return C.CDLL(path)
    raise RuntimeError("libamdhip64 is not loaded")


def test_seeded_call_refuses_capture_and_null_seed(torch_cuda):
    import torch
    from graphik_amd import _ffi
    from graphik_amd.solvers.riemannian_solver import _problem_for
    robot, graph, Qp, T = _lwa4d_paths(8, 1)
    tpl = _problem_for(graph).template
    lib = _ffi.lib()
    out = tpl.alloc_ik_buffers(8)
    Tg = torch.from_numpy(np.ascontiguousarray(T[:, 0])).cuda()
    q0 = torch.from_numpy(Qp[:, 0].copy()).cuda()

    def call(q_ptr, stream):
        return lib.gik_ik_batch_seeded(tpl._h, Tg.data_ptr(), q_ptr, 8, out["targets"].data_ptr(),
                                       out["Y"].data_ptr(), out["stats"].data_ptr(), out["q"].data_ptr(),
                                       out["pos_err"].data_ptr(), out["rot_err"].data_ptr(), stream)

    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    assert call(None, C.c_void_p(s.cuda_stream)) != 0
    assert "q_init" in lib.gik_last_error().decode()
    assert lib.gik_seed_batch(tpl._h, Tg.data_ptr(), None, 8, out["targets"].data_ptr(), out["Y"].data_ptr(),
                              C.c_void_p(s.cuda_stream)) != 0
    assert "q_init" in lib.gik_last_error().decode()
    hip = _hip_runtime()
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    assert hip.hipStreamBeginCapture(C.c_void_p(s.cuda_stream), 2) == 0      # hipStreamCaptureModeRelaxed
    rc = call(q0.data_ptr(), C.c_void_p(s.cuda_stream))
    msg = lib.gik_last_error().decode()
    graph_h = C.c_void_p()
    assert hip.hipStreamEndCapture(C.c_void_p(s.cuda_stream), C.byref(graph_h)) == 0
    n_nodes = C.c_size_t(99)
    assert hip.hipGraphGetNodes(graph_h, None, C.byref(n_nodes)) == 0
    hip.hipGraphDestroy(graph_h)
    assert rc != 0 and "capturing" in msg
    assert n_nodes.value == 0
    # the same call on the same stream, not capturing, runs
    assert call(q0.data_ptr(), C.c_void_p(s.cuda_stream)) == 0
    s.synchronize()
