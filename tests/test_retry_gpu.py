"""Restarts from random joint seeds on the MI355X: the three kernels alone (gik_retry_select / _seeds / _merge)
against numpy, gik_ik_batch_retry end to end through solve_batch / solve_trajectory -- every row of the answer is
bit for bit either the plain call's or a seeded solve from the generator's angles -- and the driver's refusals."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden, make_graph

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1025]
POS_TOL, ROT_TOL = 0.01, 0.01


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_PROBLEMS = {}


def _problem(name):
    """One BatchProblem (device template + pipeline) per graph for the whole module."""
    if name not in _PROBLEMS:
        from graphik_amd.solvers.riemannian_solver import BatchProblem
        if name == "tree5":
            from test_host_layer import tree_robot
            robot, graph = tree_robot()
        else:
            robot, graph = make_graph(name)
        bp = BatchProblem(graph)
        assert bp.device_pipeline
        _PROBLEMS[name] = (robot, graph, bp)
    return _PROBLEMS[name]


def _lib():
    from graphik_amd import _ffi
    return _ffi.lib(), _ffi


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _failed(stop, pos, rot, pos_tol=POS_TOL, rot_tol=ROT_TOL):
    return (stop != 0) | ~(pos <= pos_tol) | ~(rot <= rot_tol)


def _score(pos, rot, pos_tol=POS_TOL, rot_tol=ROT_TOL):
    with np.errstate(invalid="ignore"):
        s = np.maximum(pos / pos_tol, rot / rot_tol)       # (np.maximum propagates NaN)
    return np.where(np.isnan(s), np.inf, s)


def _better(new, old, pos_tol=POS_TOL, rot_tol=ROT_TOL):
    """The merge order of include/graphik_amd.h: new / old = (stop, pos_err, rot_err) arrays."""
    ok_n, ok_o = ~_failed(*new, pos_tol, rot_tol), ~_failed(*old, pos_tol, rot_tol)
    return (ok_n & ~ok_o) | ((ok_n == ok_o) & (_score(*new[1:], pos_tol, rot_tol) < _score(*old[1:], pos_tol, rot_tol)))


def _stats_buffer(torch, stop, rng=None):
    """[B] gik_stats records as a [B, 6] fp64 device buffer with the given stop codes (and random payload)."""
    _, _ffi = _lib()
    B = len(stop)
    raw = np.zeros((B, _ffi.STATS_BYTES // 8))
    if rng is not None:
        raw[:] = rng.standard_normal(raw.shape)
    ints = raw.view(np.int32)
    ints[:, _ffi.STATS_I32["stop"]] = stop
    if rng is not None:
        ints[:, _ffi.STATS_I32["iterations"]] = rng.randint(0, 3000, B)
    return raw


# ---- 1. select ---------------------------------------------------------------------------------------------
def _select_patterns(B):
    rng = np.random.RandomState(B)
    ok = lambda: (np.zeros(B, dtype=np.int32), np.full(B, 1e-3), np.full(B, 2e-3))     # noqa: E731
    out = {}
    out["none"] = ok()
    s, p, r = ok(); p[:] = 1.0; out["all"] = (s, p, r)
    s, p, r = ok(); r[::2] = 0.5; out["every_other"] = (s, p, r)
    s, p, r = ok(); r[-1] = 1.0; out["last_only"] = (s, p, r)
    s, p, r = ok(); p[::3] = np.nan; out["nan_pos_err"] = (s, p, r)
    s, p, r = ok(); p[:] = POS_TOL; r[:] = ROT_TOL; out["at_the_tolerance"] = (s, p, r)
    s, p, r = ok(); p[:] = 0.0; r[:] = 0.0; s[1::2] = 1; s[0] = 2; out["stopped_with_zero_error"] = (s, p, r)
    s, p, r = ok()
    s[:] = rng.choice([0, 0, 0, 1, 2], B); p[:] = rng.choice([1e-3, POS_TOL, 0.011, np.nan], B, p=[.6, .2, .15, .05])
    r[:] = rng.choice([1e-3, ROT_TOL, np.nextafter(ROT_TOL, 1.0)], B)
    out["mixed"] = (s, p, r)
    return out


@pytest.mark.parametrize("B", SIZES)
def test_select_compacts_the_failed_goals(torch_cuda, B):
    torch = torch_cuda
    lib, _ffi = _lib()
    pats = _select_patterns(B)
    expect_any = {"none": False, "all": True, "at_the_tolerance": False, "stopped_with_zero_error": True, "last_only": True}
    for name, (stop, pos, rot) in pats.items():
        want = np.flatnonzero(_failed(stop, pos, rot))
        if name in expect_any:
            assert (len(want) > 0) == expect_any[name], name
        if name == "all":
            assert len(want) == B
        if name == "last_only":
            assert want.tolist() == [B - 1]
        stats = torch.from_numpy(_stats_buffer(torch, stop)).cuda()
        d_pos, d_rot = torch.from_numpy(pos).cuda(), torch.from_numpy(rot).cuda()
        idx = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")        # a guard entry on either side
        cnt = torch.tensor([-7, 12345, -7], dtype=torch.int32, device="cuda")    # (the call zeroes the count itself)
        _ffi.check(lib.gik_retry_select(stats.data_ptr(), d_pos.data_ptr(), d_rot.data_ptr(), B, POS_TOL, ROT_TOL,
                                        idx.data_ptr() + 4, cnt.data_ptr() + 4, _stream(torch)))
        torch.cuda.synchronize()
        idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
        assert cnt.tolist() == [-7, len(want), -7], name
        assert np.array_equal(np.sort(idx[1:1 + len(want)]), want), name
        assert np.all(idx[1 + len(want):] == -7) and idx[0] == -7, name


# ---- 2. seeds ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ur10", "lwa4d", "tree5"])
@pytest.mark.parametrize("B", SIZES)
def test_seeds_copy_poses_and_draw_the_mirrors_angles(torch_cuda, name, B):
    """n = 6 (UR10), n = 7 (LWA4D), and a tree with two end effectors (pose rows of 2 x 16 doubles)."""
    torch = torch_cuda
    from graphik_amd.solvers.riemannian_solver import retry_seeds_host
    lib, _ffi = _lib()
    robot, graph, bp = _problem(name)
    tpl = bp.template
    n, pose_w = robot.n, tpl.n_ee * 16
    assert n == {"ur10": 6, "lwa4d": 7, "tree5": 5}[name] and tpl.n_ee == (2 if name == "tree5" else 1)
    rng = np.random.RandomState(100 + B)
    T = rng.standard_normal((B, pose_w))             # (the kernel copies rows: any bits will do)
    count = B if B < 64 else B - 3                   # a shuffled subset: slots and goals differ
    idx = rng.permutation(B)[:count].astype(np.int32)
    lo, hi = robot.limits_arrays()
    seed, attempt = 0xDEADBEEFCAFEF00D, 1 + B % 63
    d_T, d_idx = torch.from_numpy(T).cuda(), torch.from_numpy(idx).cuda()
    d_lo, d_hi = torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()
    T_out = torch.full((count + 2, pose_w), -7.0, dtype=torch.float64, device="cuda")
    q_out = torch.full((count + 2, n), -7.0, dtype=torch.float64, device="cuda")
    _ffi.check(lib.gik_retry_seeds(tpl._h, d_T.data_ptr(), d_idx.data_ptr(), count, seed, attempt, d_lo.data_ptr(),
                                   d_hi.data_ptr(), T_out.data_ptr() + 8 * pose_w, q_out.data_ptr() + 8 * n,
                                   _stream(torch)))
    torch.cuda.synchronize()
    T_out, q_out = T_out.cpu().numpy(), q_out.cpu().numpy()
    assert np.array_equal(T_out[1:-1].view(np.int64), T[idx].view(np.int64))
    want = retry_seeds_host(seed, idx, attempt, lo, hi)
    assert np.array_equal(q_out[1:-1].view(np.int64), want.view(np.int64))
    assert np.all(q_out[1:-1] >= lo) and np.all(q_out[1:-1] <= hi)
    for buf in (T_out, q_out):
        assert np.all(buf[0] == -7.0) and np.all(buf[-1] == -7.0)


# ---- 3. merge ----------------------------------------------------------------------------------------------
def _merge_cases(count, seed=5):
    """(stop, pos_err, rot_err) of incumbents and retries over a small set of values, so that every cell --
    success class x success class, strictly better / equal / worse, NaN on either side -- occurs many times."""
    rng = np.random.RandomState(seed)
    pos_vals = np.array([0.002, 0.005, POS_TOL, 0.02, 0.05, np.nan])
    rot_vals = np.array([0.001, 0.005, ROT_TOL, 0.02, 0.05, np.nan])
    p = [.19, .19, .19, .19, .19, .05]

    def draw():
        return (rng.choice([0, 0, 1, 2], count).astype(np.int32), rng.choice(pos_vals, count, p=p),
                rng.choice(rot_vals, count, p=p))

    return draw(), draw()


def _merge_cells(old, new):
    ok_o, ok_n = ~_failed(*old), ~_failed(*new)
    so, sn = _score(*old[1:]), _score(*new[1:])
    rel = np.where(sn < so, "better", np.where(sn == so, "equal", "worse"))
    nan_n = np.isnan(new[1]) | np.isnan(new[2])
    nan_o = np.isnan(old[1]) | np.isnan(old[2])
    return ok_o, ok_n, rel, nan_n, nan_o


def test_merge_keeps_the_better_answer(torch_cuda):
    torch = torch_cuda
    lib, _ffi = _lib()
    robot, graph, bp = _problem("lwa4d")
    tpl = bp.template
    row, n = tpl.N * tpl.k, robot.n
    B, count = 3000, 2500                     # more slots than resident wavefronts: the grid-stride loop runs
    rng = np.random.RandomState(9)
    old, new = _merge_cases(count)
    ok_o, ok_n, rel, nan_n, nan_o = _merge_cells(old, new)
    for a in (False, True):                    # every cell of the table is in the draw
        for b in (False, True):
            for r in ("better", "equal", "worse"):
                assert np.any((ok_o == a) & (ok_n == b) & (rel == r) & ~nan_n & ~nan_o), (a, b, r)
    assert np.any(nan_n & ok_o) and np.any(nan_n & ~ok_o & ~nan_o) and np.any(nan_n & nan_o) and np.any(nan_o & ~nan_n)
    idx = rng.permutation(B)[:count].astype(np.int32)
    # incumbents [B] (goals outside idx: arbitrary), with one guard row before and after every buffer
    inc_stop = rng.choice([0, 1], B).astype(np.int32)
    inc_pos, inc_rot = rng.uniform(0, 0.02, B), rng.uniform(0, 0.02, B)
    inc_stop[idx], inc_pos[idx], inc_rot[idx] = old

    def guarded(a):
        g = np.full((1,) + a.shape[1:], -7, dtype=a.dtype)
        return np.concatenate([g, a, g])

    host = {"Y": guarded(rng.standard_normal((B, row))), "stats": guarded(_stats_buffer(torch, inc_stop, rng)),
            "q": guarded(rng.standard_normal((B, n))), "pos": guarded(inc_pos), "rot": guarded(inc_rot),
            "attempt": guarded(rng.randint(0, 3, B).astype(np.int32))}
    retry = {"Y": rng.standard_normal((count, row)), "stats": _stats_buffer(torch, new[0], rng),
             "q": rng.standard_normal((count, n)), "pos": new[1].copy(), "rot": new[2].copy()}
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    dre = {k: torch.from_numpy(v).cuda() for k, v in retry.items()}
    d_idx = torch.from_numpy(idx).cuda()
    ATTEMPT = 5

    def ptr(k):      # past the guard row
        t = dev[k]
        return t.data_ptr() + t.element_size() * (t.numel() // t.shape[0])

    _ffi.check(lib.gik_retry_merge(tpl._h, d_idx.data_ptr(), count, ATTEMPT, POS_TOL, ROT_TOL, dre["Y"].data_ptr(),
                                   dre["stats"].data_ptr(), dre["q"].data_ptr(), dre["pos"].data_ptr(),
                                   dre["rot"].data_ptr(), ptr("Y"), ptr("stats"), ptr("q"), ptr("pos"), ptr("rot"),
                                   ptr("attempt"), _stream(torch)))
    torch.cuda.synchronize()
    take = _better(new, old)
    assert 0.2 < take.mean() < 0.8
    assert not np.any(take & nan_n)                               # a NaN never wins
    assert not np.any(take & (rel == "equal") & (ok_o == ok_n))   # a tie keeps the incumbent
    assert np.all(take[ok_n & ~ok_o]) and not np.any(take[~ok_n & ok_o])
    for k in host:
        want = host[k].copy()
        if k == "attempt":
            want[1 + idx[take]] = ATTEMPT
        else:
            want[1 + idx[take]] = retry[k][take]
        got = dev[k].cpu().numpy()
        bits = np.int64 if want.dtype == np.float64 else np.int32
        assert np.array_equal(got.view(bits), want.view(bits)), k


# ---- 4-6. end to end -----------------------------------------------------------------------------------------
def _goals(robot, B, seed):
    rng = np.random.RandomState(seed)
    lb, ub = robot.limits_arrays()
    return robot.fk_batch(rng.uniform(lb, ub, size=(B, robot.n)))


ROW_KEYS = ("stop", "iterations", "pos_err", "rot_err")


def _same_rows(a, b):
    """(q, Y, info) triples: bit-identical in q, Y, stop, iterations, pos_err, rot_err?"""
    def bits(x):
        x = np.ascontiguousarray(x)
        return x.view(np.int64) if x.dtype == np.float64 else x
    return (np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and
            all(np.array_equal(bits(a[2][k]), bits(b[2][k])) for k in ROW_KEYS))


def _rows(res, sel):
    q, Y, info = res
    return q[sel], Y[sel], {k: info[k][sel] for k in ROW_KEYS}


def _triple(info):
    return info["stop"], info["pos_err"], info["rot_err"]


def _check_identities(graph, T, params, retries, seed, exact=True):
    """The contract of a solve with restarts against the plain call P on the same goals.  Returns (P, R)."""
    from graphik_amd.solvers.riemannian_solver import retry_seeds_host, solve_batch
    lo, hi = graph.robot.limits_arrays()
    P = solve_batch(graph, T, params=params)
    R = solve_batch(graph, T, params=params, retries=retries, retry_seed=seed, pos_tol=POS_TOL, rot_tol=ROT_TOL)
    att = R[2]["attempt"]
    assert att.dtype == np.int32 and att.shape == (len(T),)
    assert att.min() >= 0 and att.max() <= retries
    failed_P = _failed(*_triple(P[2]))
    assert not np.any(att[~failed_P]), "a goal that succeeded at once was retried"
    # no goal is worse than in P, and no success is lost
    assert not np.any(_better(_triple(P[2]), _triple(R[2])))
    assert np.sum(~_failed(*_triple(R[2]))) >= np.sum(~failed_P)
    if not exact:
        return P, R
    first = att == 0
    assert _same_rows(_rows(R, first), _rows(P, first))
    if not failed_P.any():                      # the early exit: nothing was queued after the first attempt
        assert not att.any() and _same_rows(R, P)
    for g in np.flatnonzero(att > 0):
        q0 = retry_seeds_host(seed, [g], int(att[g]), lo, hi)
        S = solve_batch(graph, T[g:g + 1], q_init=q0, params=params)
        assert _same_rows(_rows(R, slice(g, g + 1)), S), (g, att[g])
        # an answer that replaced another one is strictly better than what the plain call had
        assert _better(tuple(x[g:g + 1] for x in _triple(R[2])), tuple(x[g:g + 1] for x in _triple(P[2])))[0]
    return P, R


def test_end_to_end_every_goal_fails_the_first_attempt(torch_cuda):
    """LWA4D, 256 goals, maxiter = 5: from the MDS start every goal stops at maxiter, so every goal is retried."""
    from graphik_amd.solvers.riemannian_solver import solve_batch
    robot, graph = make_graph("lwa4d")
    T = _goals(robot, 256, seed=21)
    params = {"maxiter": 5}
    P, R = _check_identities(graph, T, params, retries=2, seed=77)
    failed_P = _failed(*_triple(P[2]))
    assert failed_P.any(), "no goal failed the first attempt: the test would check nothing"
    att = R[2]["attempt"]
    print("attempt histogram", np.bincount(att, minlength=3).tolist(), "successes", int(np.sum(~failed_P)), "->",
          int(np.sum(~_failed(*_triple(R[2])))))
    assert (att > 0).any(), "no retry improved on any of 256 five-iteration answers"
    # the same seed: the same bits; another seed: other seeds, so some seeded row differs
    R2 = solve_batch(graph, T, params=params, retries=2, retry_seed=77)
    assert _same_rows(R2, R) and np.array_equal(R2[2]["attempt"], att)
    R3 = solve_batch(graph, T, params=params, retries=2, retry_seed=78)
    seeded = (att > 0) | (R3[2]["attempt"] > 0)
    assert not _same_rows(_rows(R3, seeded), _rows(R, seeded))


@pytest.mark.parametrize("name,B", [("lwa4d", 128), ("ur10", 64)])
def test_end_to_end_default_budget(torch_cuda, name, B):
    robot, graph = make_graph(name)
    T = _goals(robot, B, seed=22)
    P, R = _check_identities(graph, T, None, retries=1, seed=3)
    print(name, "failed in P", int(_failed(*_triple(P[2])).sum()), "rescued or improved", int((R[2]["attempt"] > 0).sum()))


def test_end_to_end_seeded_first_attempt(torch_cuda):
    """q_init + retries: the first attempt is the seeded solve, the later ones are random."""
    from graphik_amd.solvers.riemannian_solver import retry_seeds_host, solve_batch
    robot, graph = make_graph("lwa4d")
    T = _goals(robot, 64, seed=23)
    lo, hi = robot.limits_arrays()
    q_init = np.random.RandomState(4).uniform(lo, hi, size=(64, robot.n))
    params = {"maxiter": 5}
    P = solve_batch(graph, T, q_init=q_init, params=params)
    R = solve_batch(graph, T, q_init=q_init, params=params, retries=1, retry_seed=9)
    att = R[2]["attempt"]
    assert _failed(*_triple(P[2])).any()
    assert _same_rows(_rows(R, att == 0), _rows(P, att == 0))
    for g in np.flatnonzero(att > 0)[:16]:
        S = solve_batch(graph, T[g:g + 1], q_init=retry_seeds_host(9, [g], 1, lo, hi), params=params)
        assert _same_rows(_rows(R, slice(g, g + 1)), S)
    assert not np.any(_better(_triple(P[2]), _triple(R[2])))


def test_planar_chain_is_never_worse(torch_cuda):
    """Planar-10, 64 goals: properties only (planar bits may depend on the batch size)."""
    robot, graph = make_graph("planar10_limits_pi")
    T = _goals(robot, 64, seed=24)
    _check_identities(graph, T, {"maxiter": 20}, retries=1, seed=5, exact=False)
    _check_identities(graph, T, None, retries=1, seed=5, exact=False)


# ---- 7. path tracking ------------------------------------------------------------------------------------------
def test_solve_trajectory_with_retries(torch_cuda):
    from graphik_amd.solvers.riemannian_solver import solve_batch, solve_trajectory
    robot, graph = make_graph("lwa4d")
    rng = np.random.RandomState(31)
    lb, ub = robot.limits_arrays()
    Bp, L = 8, 3
    Q = rng.uniform(0.6 * lb, 0.6 * ub, size=(Bp, 1, robot.n)) + 0.05 * np.arange(L)[None, :, None]
    T = robot.fk_batch(Q.reshape(-1, robot.n)).reshape(Bp, L, 4, 4)
    q_start = rng.uniform(lb, ub, size=(Bp, robot.n))       # far from the paths: short solves from it fail
    params = {"maxiter": 5}
    kw = dict(params=params, retries=1, retry_seed=13)
    q, Y, info = solve_trajectory(graph, T, q_start, return_Y=True, **kw)
    assert info["attempt"].shape == (Bp, L) and info["attempt"].dtype == np.int32
    assert info["attempt"].min() >= 0 and info["attempt"].max() <= 1
    prev = q_start
    for l in range(L):
        S = solve_batch(graph, T[:, l], q_init=prev, **kw)
        way = (q[:, l], Y[:, l], {k: info[k][:, l] for k in ROW_KEYS})
        assert _same_rows(way, S), l
        assert np.array_equal(info["attempt"][:, l], S[2]["attempt"]), l
        prev = q[:, l]                                       # rescued angles seed the next waypoint
    print("trajectory attempts", info["attempt"].tolist())


# ---- 8. refusals -------------------------------------------------------------------------------------------------
def _hip_runtime():
    """The HIP runtime this process (torch, libgraphik_amd) already has loaded."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            return C.CDLL(path)
    raise RuntimeError("libamdhip64 is not loaded")


def test_driver_refusals_leave_the_outputs_alone(torch_cuda):
    torch = torch_cuda
    from graphik_amd.engine import Template
    lib, _ffi = _lib()
    robot, graph, bp = _problem("lwa4d")
    tpl = bp.template
    B = 8
    T = torch.from_numpy(np.ascontiguousarray(_goals(robot, B, seed=41))).cuda()
    lo, hi = (torch.from_numpy(a).cuda() for a in robot.limits_arrays())
    out = tpl.alloc_ik_buffers(B)
    out["attempt"] = torch.empty(B, dtype=torch.int32, device="cuda")
    for v in out.values():
        v.view(torch.int32).fill_(-7)
    before = {k: v.clone() for k, v in out.items()}
    ws = torch.empty(int(lib.gik_retry_ws_bytes(tpl._h, B)) // 8 + 1, dtype=torch.float64, device="cuda")
    assert lib.gik_retry_ws_bytes(tpl._h, B) > 0
    d = load_golden("lwa4d")
    bare = Template.from_matrices(d["omega"], d["psi_L"], d["psi_U"], k=3, use_limits=True, device="cuda:0")   # no pipeline
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def call(handle=None, retries=1, q_lo=lo.data_ptr(), q_hi=hi.data_ptr(), stream=None):
        opts = _ffi.RetryOpts(retries=retries, seed=1, pos_tol=POS_TOL, rot_tol=ROT_TOL, d_q_lo=q_lo, d_q_hi=q_hi)
        rc = lib.gik_ik_batch_retry(handle or tpl._h, T.data_ptr(), None, B, C.byref(opts), ws.data_ptr(),
                                    out["targets"].data_ptr(), out["Y"].data_ptr(), out["stats"].data_ptr(),
                                    out["q"].data_ptr(), out["pos_err"].data_ptr(), out["rot_err"].data_ptr(),
                                    out["attempt"].data_ptr(), stream or C.c_void_p(s.cuda_stream))
        return rc, lib.gik_last_error().decode()

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(out[k].view(torch.int32), before[k].view(torch.int32)) for k in out)

    rc, msg = call(handle=bare._h)
    assert rc != 0 and "pipeline" in msg and untouched()
    assert lib.gik_retry_ws_bytes(bare._h, B) == 0
    rc, msg = call(retries=64)
    assert rc != 0 and "retries" in msg and "63" in msg and untouched()
    rc, msg = call(retries=-1)
    assert rc != 0 and "retries" in msg and untouched()
    rc, msg = call(q_lo=None)
    assert rc != 0 and "limits" in msg and untouched()
    rc, msg = call(q_hi=None)
    assert rc != 0 and "limits" in msg and untouched()
    hip = _hip_runtime()
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    assert hip.hipStreamBeginCapture(C.c_void_p(s.cuda_stream), 2) == 0      # hipStreamCaptureModeRelaxed
    rc, msg = call()
    rc0, msg0 = call(retries=0)                                              # ... also without retries
    graph_h = C.c_void_p()
    assert hip.hipStreamEndCapture(C.c_void_p(s.cuda_stream), C.byref(graph_h)) == 0
    n_nodes = C.c_size_t(99)
    assert hip.hipGraphGetNodes(graph_h, None, C.byref(n_nodes)) == 0
    hip.hipGraphDestroy(graph_h)
    assert rc != 0 and "capturing" in msg and rc0 != 0 and "capturing" in msg0
    assert n_nodes.value == 0 and untouched()
    # the same call on the same stream, not capturing, runs; with retries = 0 it is the plain call
    rc, msg = call(retries=0)
    assert rc == 0, msg
    s.synchronize()
    ref = tpl.ik(T)
    torch.cuda.synchronize()
    assert torch.equal(out["q"], ref["q"]) and torch.equal(out["Y"].reshape(ref["x"].shape), ref["x"])
    assert not out["attempt"].any()
    rc, msg = call(retries=2)
    assert rc == 0, msg
    s.synchronize()
    assert int(out["attempt"].max()) <= 2 and int(out["attempt"].min()) >= 0
