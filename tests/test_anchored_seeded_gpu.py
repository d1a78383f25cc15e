"""The fixed-anchor solve from joint-configuration seeds on the MI355X: anch_scatter_kernel (gik_anchored_seed_batch),
the seeded pipeline (gik_anchored_ik_batch_seeded) as the composition of its steps and against the oracle from the
device seed, anch_clearance_kernel (gik_anchored_clearance) at its edges, path tracking among the obstacles
(AnchoredProblem.solve_trajectory), aliasing and the refusals.  UR10 + table_environment() unless said.  The inputs
and the CPU twin's evidence for the bars: tests/test_anchored_seeded_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import make_graph
from test_anchored_seeded_host import collision_input, free_matrices, tracking_input
from test_seeded_host import _above_floor, assert_seeded_prefix

pytestmark = pytest.mark.gpu

STAT_KEYS = ("f", "gradnorm", "iterations", "inner_total", "stop", "n_accept")      # (the fields that timing cannot touch)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def _problem():
    from graphik_amd.solvers.riemannian_solver import AnchoredProblem
    robot, graph = make_graph("ur10_table")
    return robot, graph, AnchoredProblem(graph)


def _np(t):
    return t.cpu().numpy()


def test_scatter_is_exact(torch_cuda):
    """Y_free is the free rows of seed_kernel's realization, bit for bit; the goal anchors are the goal pose's."""
    robot, graph, ap = _problem()
    Q, T = tracking_input()
    tpl, base = ap.template, ap.base.template
    Yf, goal = tpl.anchored_seed(base, T[:, 3], Q[:, 0])
    assert Yf.shape == (64, len(ap.free), 3) and goal.shape == (64, 6)
    _, Y_full = base.seed(T[:, 3], Q[:, 0])
    assert torch_cuda.equal(Yf, Y_full[:, ap.free])
    assert np.abs(_np(goal) - ap.goal_anchors(T[:, 3])).max() < 1e-15
    # one seed for every goal
    Yf1, goal1 = tpl.anchored_seed(base, T[:, 3], Q[5, 0])
    assert torch_cuda.equal(Yf1, Yf[5:6].expand(64, -1, -1)) and torch_cuda.equal(goal1, goal)


def test_pipeline_is_the_composition_of_its_steps(torch_cuda):
    """anchored_ik(q_init=) = anchored_seed -> solve -> (gather) -> recover, bit for bit."""
    robot, graph, ap = _problem()
    Q, T = tracking_input()
    tpl, base = ap.template, ap.base.template
    Tg, q0 = T[:, 1], Q[:, 0]
    r = tpl.anchored_ik(base, Tg, q_init=q0)
    assert "clearance" not in r
    Yf, goal = tpl.anchored_seed(base, Tg, q0)
    s = tpl.solve(Yf, goal)
    x = r["x"]
    assert torch_cuda.equal(x[:, ap.free], s["x"])
    g = ap.base.graph
    xn = _np(x)
    assert np.abs(xn[:, g.index("p0")]).max() == 0.0
    assert np.abs(xn[:, g.index(f"p{robot.n}")] - Tg[:, :3, 3]).max() < 1e-15
    q, pe, re = base.recover(x, Tg)
    assert torch_cuda.equal(q, r["q"]) and torch_cuda.equal(pe, r["pos_err"]) and torch_cuda.equal(re, r["rot_err"])
    for key in STAT_KEYS:
        assert torch_cuda.equal(s[key], r[key]), key


def test_seeded_solve_against_oracle_from_the_device_seed(torch_cuda):
    """Input (b), collision-free goals from seeds in collision: the device solve from the device seed against the
    oracle's anchored solve from the same point -- trajectory prefix, convergence class on at least 54 of 64 (the
    one-in-six allowance of test_anchored_trajectory_against_oracle), at least 48 converge (the CPU twin: 58), and no
    converged answer is inside a sphere."""
    from oracle import c_oracle as co
    from parity_util import anchored_terms
    robot, graph, ap = _problem()
    seeds, goals = collision_input()
    Tg = robot.fk_batch(goals)
    tpl, base = ap.template, ap.base.template
    Yf, goal = tpl.anchored_seed(base, Tg, seeds)
    r = tpl.solve(Yf, goal, trace_cap=48)
    tr = {k: _np(v) for k, v in r["trace"].items()}
    its = _np(r["iterations"])
    D, om, pL, pU = free_matrices(ap)
    ga, Y0 = ap.goal_anchors(Tg), _np(Yf)
    f_oracle = np.empty(64)
    for b in range(64):
        node, pos, tgt, kind = anchored_terms(ap, ga[b])
        o = co.rtr_solve_anchored(Y0[b], D, om, pL, pU, node, pos, tgt, kind, traj_cap=48)
        m = min(_above_floor(o["traj"]["f_before"], 3), int(its[b]), o["iterations"])
        assert_seeded_prefix({k: tr[k][b] for k in tr}, o["traj"], m, 3)
        f_oracle[b] = o["f(x)"]
    res = ap.solve(Tg, q_init=seeds)
    f, clear = _np(res["f"]), _np(res["clearance"])
    conv = f < 1e-9
    print("same class", int((conv == (f_oracle < 1e-9)).sum()), "converged", int(conv.sum()), "oracle", int((f_oracle < 1e-9).sum()),
          "min clearance", clear[conv].min())
    assert (conv == (f_oracle < 1e-9)).sum() >= 54
    assert conv.sum() >= 48
    assert np.all(clear[conv] > -1e-4), clear[conv].min()


def test_seed_at_the_answer_stops_at_once(torch_cuda):
    """q_init = q_goal, collision free: at most one outer iteration, the goal's angles back, and the device clearance
    is the host's."""
    from parity_util import wrap_abs
    robot, graph, ap = _problem()
    _, goals = collision_input()
    res = ap.solve(robot.fk_batch(goals), q_init=goals)
    assert int(res["iterations"].max()) <= 1
    assert wrap_abs(_np(res["q"]) - goals).max() < 1e-6
    assert np.abs(_np(res["clearance"]) - ap.clearance(_np(res["x"]))).max() < 1e-12


def test_tracking_among_the_obstacles(torch_cuda):
    """Input (a) through solve_trajectory: the waypoints converge, stay out of the spheres and on their IK branch;
    waypoint l is exactly solve(T[:, l], q_init=q[:, l - 1])."""
    from parity_util import wrap_abs
    robot, graph, ap = _problem()
    Q, T = tracking_input()
    B, L = T.shape[:2]
    q, Y, info = ap.solve_trajectory(T, Q[:, 0], return_Y=True)
    assert q.shape == (B, L, robot.n) and Y.shape == (B, L, ap.base.N, 3)
    for key in ("iterations", "inner_iterations", "stop", "f(x)", "gradnorm", "pos_err", "rot_err", "clearance"):
        assert info[key].shape == (B, L), key
    assert info["solve_time"] > 0
    assert np.all((info["stop"] == 0) | (info["stop"] == 1))
    conv = info["f(x)"] < 1e-9
    jump = wrap_abs(q[:, 1:] - q[:, :-1]).max(axis=2)
    print("converged", conv.mean(), "iterations median", np.median(info["iterations"]), "min clearance",
          info["clearance"][conv].min(), "max pos_err", info["pos_err"][conv].max(), "jumps < 0.2", np.mean(jump < 0.2))
    assert conv.mean() >= 0.99
    assert np.all(info["clearance"][conv] > -1e-4)
    assert np.all(info["pos_err"][conv] < 2e-2) and np.median(info["pos_err"][conv]) < 1e-3
    assert np.mean(jump < 0.2) >= 0.99
    for l in (1, 4, 7):
        r = ap.solve(T[:, l], q_init=q[:, l - 1], clearance=True)
        assert np.array_equal(_np(r["q"]), q[:, l]) and np.array_equal(_np(r["x"]), Y[:, l]), l
        assert np.array_equal(_np(r["iterations"]), info["iterations"][:, l])
        assert np.array_equal(_np(r["clearance"]), info["clearance"][:, l])
        assert np.abs(info["clearance"][:, l] - ap.clearance(Y[:, l])).max() < 1e-12
    q2, Y2, info2 = ap.solve_trajectory(T, Q[:, 0])
    assert Y2 is None and np.array_equal(q2, q) and np.array_equal(info2["clearance"], info["clearance"])


@functools.lru_cache(maxsize=None)
def _scene(n_obs):
    """UR10 with the first n_obs spheres of the table (128: the table + 28 more, the limit)."""
    from graphik_amd.solvers.riemannian_solver import AnchoredProblem
    from graphik_amd.utils import table_environment
    robot, graph = make_graph("ur10")
    spheres = [(np.asarray(c, dtype=float), float(r)) for c, r in table_environment()]
    rng = np.random.RandomState(31)
    while len(spheres) < n_obs:
        spheres.append((rng.uniform(-1.0, 1.0, size=3), 0.05 + 0.1 * rng.rand()))
    for idx, (c, r) in enumerate(spheres[:n_obs]):
        graph.add_spherical_obstacle(f"o{idx}", c, r)
    ap = AnchoredProblem(graph)
    assert len(ap.obstacles) == n_obs and int(ap.obs_mask.sum()) == 5
    return ap


@pytest.mark.parametrize("n_obs", [0, 1, 13, 100, 128])
def test_clearance_kernel_at_its_edges(torch_cuda, n_obs):
    """No obstacle (+inf), one, 5 x 13 = 65 pairs (one past a wavefront), the table, the 128-obstacle limit; batches of
    1, 63 and 65; p-nodes inside spheres (negative values); a NaN row is NaN for its goal alone.  Host formula: 1e-12."""
    ap = _scene(n_obs)
    g = ap.base.graph
    masked = [ap.free[i] for i in np.flatnonzero(ap.obs_mask)]
    assert masked == [g.index(f"p{i}") for i in range(1, 6)]
    rng = np.random.RandomState(100 + n_obs)
    for B in (1, 63, 65):
        Y = 0.6 * rng.randn(B, ap.base.N, 3) + np.array([0.0, 0.0, 0.9])
        if n_obs:
            for b in range(B):
                for i in masked:
                    Y[b, i] = ap.obstacles[rng.randint(n_obs), :3] + 0.07 * rng.randn(3)
        c = _np(ap.template.anchored_clearance(Y))
        assert c.shape == (B,)
        if n_obs == 0:
            assert np.all(np.isposinf(c))
            continue
        ref = ap.clearance(Y)
        assert np.abs(c - ref).max() < 1e-12
        assert ref.min() < 0 or n_obs == 1      # (p-nodes inside spheres: negative values occur)
        bad = B // 2
        Y[bad, masked[2], 1] = np.nan
        c = _np(ap.template.anchored_clearance(Y))
        ok = np.arange(B) != bad
        assert np.isnan(c[bad]) and np.array_equal(c[ok], _np(ap.template.anchored_clearance(Y[ok])))
        assert B == 1 or np.abs(c[ok] - ref[ok]).max() < 1e-12


def _hip_runtime():
    """The HIP runtime this process (torch, libgraphik_amd) already has loaded."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            return C.CDLL(path)
    raise RuntimeError("libamdhip64 is not loaded")


def test_aliasing_and_refusals(torch_cuda):
    import torch
    from graphik_amd import _ffi
    robot, graph, ap = _problem()
    Q, T = tracking_input()
    tpl, base = ap.template, ap.base.template
    B = 64
    # the seed may be the answer's own buffer
    ref = tpl.anchored_ik(base, T[:, 1], q_init=Q[:, 0], clearance=True)
    out = tpl.alloc_anchored_buffers(base, B, clearance=True)
    out["q"].copy_(torch.from_numpy(Q[:, 0].copy()))
    res = tpl.anchored_ik(base, T[:, 1], q_init=out["q"], out=out, clearance=True)
    assert res["q"].data_ptr() == out["q"].data_ptr() and res["clearance"].data_ptr() == out["clearance"].data_ptr()
    for key in ("q", "x", "pos_err", "rot_err", "clearance"):
        assert torch.equal(res[key], ref[key]), key
    # refusals, each with its message and before anything is queued
    lib = _ffi.lib()
    Tg = torch.from_numpy(np.ascontiguousarray(T[:, 1])).cuda()
    q0 = torch.from_numpy(Q[:, 0].copy()).cuda()

    def call(anch, bs, q_ptr, stream, n=B):
        return lib.gik_anchored_ik_batch_seeded(anch, bs, Tg.data_ptr(), q_ptr, n, out["ws"].data_ptr(), out["Y"].data_ptr(),
                                                out["stats"].data_ptr(), out["q"].data_ptr(), out["pos_err"].data_ptr(),
                                                out["rot_err"].data_ptr(), out["clearance"].data_ptr(), stream)

    s = torch.cuda.Stream()
    stream = C.c_void_p(s.cuda_stream)
    torch.cuda.synchronize()
    for args, word in (((tpl._h, base._h, None, stream), "q_init"),
                       ((base._h, base._h, q0.data_ptr(), stream), "fixed-anchor"),
                       ((tpl._h, tpl._h, q0.data_ptr(), stream), "pipeline"),
                       ((tpl._h, base._h, q0.data_ptr(), stream, -1), "bad argument")):
        assert call(*args) != 0
        assert word in lib.gik_last_error().decode(), (word, lib.gik_last_error().decode())
    Yf = torch.empty(B, tpl.N * 3, dtype=torch.float64, device="cuda")
    goal = torch.empty(B, 6, dtype=torch.float64, device="cuda")
    assert lib.gik_anchored_seed_batch(tpl._h, base._h, Tg.data_ptr(), None, B, out["ws"].data_ptr(), Yf.data_ptr(),
                                       goal.data_ptr(), stream) != 0
    assert "q_init" in lib.gik_last_error().decode()
    assert lib.gik_anchored_clearance(base._h, out["Y"].data_ptr(), B, out["clearance"].data_ptr(), stream) != 0
    assert "fixed-anchor" in lib.gik_last_error().decode()
    assert lib.gik_anchored_clearance(tpl._h, None, B, out["clearance"].data_ptr(), stream) != 0
    assert "null buffer" in lib.gik_last_error().decode()
    # a capturing stream: refused, and the capture stays empty
    hip = _hip_runtime()
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    assert hip.hipStreamBeginCapture(stream, 2) == 0      # hipStreamCaptureModeRelaxed
    rcs, msgs = [], []
    for fn in (lambda: call(tpl._h, base._h, q0.data_ptr(), stream),
               lambda: lib.gik_anchored_seed_batch(tpl._h, base._h, Tg.data_ptr(), q0.data_ptr(), B, out["ws"].data_ptr(),
                                                   Yf.data_ptr(), goal.data_ptr(), stream),
               lambda: lib.gik_anchored_clearance(tpl._h, out["Y"].data_ptr(), B, out["clearance"].data_ptr(), stream)):
        rcs.append(fn())
        msgs.append(lib.gik_last_error().decode())
    graph_h = C.c_void_p()
    assert hip.hipStreamEndCapture(stream, C.byref(graph_h)) == 0
    n_nodes = C.c_size_t(99)
    assert hip.hipGraphGetNodes(graph_h, None, C.byref(n_nodes)) == 0
    hip.hipGraphDestroy(graph_h)
    assert all(rc != 0 for rc in rcs) and all("capturing" in m for m in msgs), (rcs, msgs)
    assert n_nodes.value == 0
    # the same call on the same stream, not capturing, runs
    assert call(tpl._h, base._h, q0.data_ptr(), stream) == 0
    s.synchronize()
    assert torch.equal(out["q"], ref["q"]) and torch.equal(out["clearance"], ref["clearance"])
    # B = 0
    r0 = ap.solve(T[:0, 1], q_init=Q[:0, 0])
    assert r0["x"].shape == (0, ap.base.N, 3) and r0["q"].shape == (0, robot.n) and r0["clearance"].shape == (0,)
    Yf0, goal0 = tpl.anchored_seed(base, T[:0, 1], Q[:0, 0])
    assert Yf0.shape == (0, tpl.N, 3) and goal0.shape == (0, 6)
    assert tpl.anchored_clearance(np.zeros((0, ap.base.N, 3))).shape == (0,)
    q_t, Y_t, info_t = ap.solve_trajectory(T[:0], Q[:0, 0])
    assert q_t.shape == (0, T.shape[1], robot.n) and info_t["clearance"].shape == (0, T.shape[1])


def test_cold_path_is_unchanged(torch_cuda):
    """solve(T) without a seed: the keys it always had, and the bits of a direct gik_anchored_ik_batch call."""
    import torch
    from graphik_amd import _ffi
    robot, graph, ap = _problem()
    _, goals = collision_input()
    Tg = robot.fk_batch(goals)
    tpl, base = ap.template, ap.base.template
    r = ap.solve(Tg)
    assert set(r) == {"x", "q", "pos_err", "rot_err", "_ws", "f", "gradnorm", "stepsize", "iterations", "inner_total",
                      "stop", "n_accept", "inner_executed", "flags"}
    B = len(Tg)
    out = tpl.alloc_anchored_buffers(base, B)
    Td = torch.from_numpy(np.ascontiguousarray(Tg)).cuda()
    lib = _ffi.lib()
    _ffi.check(lib.gik_anchored_ik_batch(tpl._h, base._h, Td.data_ptr(), B, out["ws"].data_ptr(), out["Y"].data_ptr(),
                                         out["stats"].data_ptr(), out["q"].data_ptr(), out["pos_err"].data_ptr(),
                                         out["rot_err"].data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert torch.equal(out["Y"].reshape(B, -1, 3), r["x"]) and torch.equal(out["q"], r["q"])
    assert torch.equal(out["pos_err"], r["pos_err"]) and torch.equal(out["rot_err"], r["rot_err"])
    from graphik_amd.engine import _decode_stats
    st = _decode_stats(out["stats"])
    for key in STAT_KEYS:
        assert torch.equal(st[key], r[key]), key
    # ... and with clearance=True the same answer plus the clearance of it
    rc = ap.solve(Tg, clearance=True)
    assert torch.equal(rc["x"], r["x"]) and np.abs(_np(rc["clearance"]) - ap.clearance(_np(r["x"]))).max() < 1e-12
