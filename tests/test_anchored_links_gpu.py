"""Clearance of whole links in the fixed-anchor solve on the MI355X: anch_link_clearance_kernel at its edges against the
numpy mirror, gik_anchored_sweep_clearance against two plain calls (bit for bit) and the mirror, the restart rule
reading the link clearance (clearance_mode="links") on configurations whose joint points are clear and whose links are
not, solve_trajectory(sweep=), and the refusals of the new entry points.  UR10 + table_environment() unless said.
The inputs and the mirror's own tests: tests/test_anchored_links_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import make_graph
from test_anchored_links_host import _Cell, node_clear_link_colliding, sweep_colliding_pairs, uniform_pairs
from test_anchored_retry_gpu import KEYS, TOL, _bits, _host, _same_rows
from test_anchored_seeded_host import tracking_input
from test_retry_gpu import _hip_runtime, _stats_buffer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _np(t):
    return t.detach().cpu().numpy()


def _rs():
    from graphik_amd.solvers import riemannian_solver as rs
    return rs


def _lib():
    from graphik_amd import _ffi
    return _ffi.lib(), _ffi


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _problem(links="skeleton"):
    """UR10 + table for the whole module: with the default skeleton, or built with links=[] (none attached)."""
    robot, graph = make_graph("ur10_table")
    return robot, graph, _rs().AnchoredProblem(graph, links=None if links == "skeleton" else [])


@functools.lru_cache(maxsize=None)
def _scene(n_obs, rho):
    """UR10 with the first n_obs spheres of the table (128: the table + 28 more, the limit), skeleton links of radius rho."""
    from graphik_amd.utils import table_environment
    robot, graph = make_graph("ur10")
    spheres = [(np.asarray(c, dtype=float), float(r)) for c, r in table_environment()]
    rng = np.random.RandomState(31)
    while len(spheres) < n_obs:
        spheres.append((rng.uniform(-1.0, 1.0, size=3), 0.05 + 0.1 * rng.rand()))
    for idx, (c, r) in enumerate(spheres[:n_obs]):
        graph.add_spherical_obstacle(f"o{idx}", c, r)
    ap = _rs().AnchoredProblem(graph, link_radius=rho)
    assert len(ap.obstacles) == n_obs and len(ap.link_rows) == 6
    return ap


# ---- 1. the kernel -------------------------------------------------------------------------------------------------
def _planted(ap, B, rng):
    """[B, N, 3] random point matrices with four links planted around one sphere (centre c) of every goal: p0->p1 has
    length zero; p2->p3 starts 30 cm beside c and points away from it (nearest point: end a); p3->p4 comes half way back
    (nearest point: end b); p4->p5 passes 5 cm beside c at its middle (nearest point: in the interior, inside the
    sphere, both ends 30 cm away)."""
    g = ap.base.graph
    p = [g.index(f"p{i}") for i in range(7)]
    Y = 0.6 * rng.randn(B, ap.base.N, 3) + np.array([0.0, 0.0, 0.9])
    for b in range(B):
        c = ap.obstacles[rng.randint(len(ap.obstacles)), :3] if len(ap.obstacles) else np.zeros(3)
        Y[b, p[1]] = Y[b, p[0]]
        Y[b, p[2]] = c + np.array([0.3, 0.05, 0.0])
        Y[b, p[3]] = Y[b, p[2]] + (Y[b, p[2]] - c)
        Y[b, p[4]] = Y[b, p[3]] + 0.5 * (c - Y[b, p[3]])
        Y[b, p[5]] = 2.0 * (c + np.array([0.0, 0.05, 0.0])) - Y[b, p[4]]
    return Y


def _clamp_cases(ap, Y):
    """Per goal: does a (link, sphere) pair with t <= 0, with t >= 1, with 0 < t < 1 and a zero-length link occur?"""
    a, b = Y[:, ap.link_rows[:, 0], None, :], Y[:, ap.link_rows[:, 1], None, :]
    d, u = b - a, ap.obstacles[None, None, :, :3] - a
    L2, ud = (d * d).sum(-1), (u * d).sum(-1)
    pos = L2 > 0
    return ((pos & (ud <= 0)).any(axis=(1, 2)), (pos & (ud >= L2)).any(axis=(1, 2)),
            (pos & (ud > 0) & (ud < L2)).any(axis=(1, 2)), (~pos).any(axis=(1, 2)))


@pytest.mark.parametrize("rho", [0.0, 0.03])
@pytest.mark.parametrize("n_obs", [0, 1, 11, 100, 128])
def test_link_kernel_at_its_edges(torch_cuda, n_obs, rho):
    """No obstacle (+inf), one, 6 x 11 = 66 pairs (one past a wavefront), the table, the 128-obstacle limit; batches of
    1, 63 and 65; every clamp case and a zero-length link in every goal; links through spheres (negative values); thin
    and 3 cm links; a NaN row is NaN for its goal alone.  Against the numpy mirror to 1e-12, the bar the node kernel is
    held to on such points."""
    ap = _scene(n_obs, rho)
    g = ap.base.graph
    assert ap.link_rows.tolist() == [[g.index(f"p{i}"), g.index(f"p{i + 1}")] for i in range(6)]
    assert np.all(ap.link_radius == rho)
    rng = np.random.RandomState(100 + n_obs)
    for B in (1, 63, 65):
        Y = _planted(ap, B, rng)
        c = _np(ap.template.anchored_link_clearance(Y))
        assert c.shape == (B,)
        if n_obs == 0:
            assert np.all(np.isposinf(c))
            continue
        for case in _clamp_cases(ap, Y):
            assert case.all()
        ref = ap.link_clearance(Y)
        assert np.abs(c - ref).max() < 1e-12
        assert np.all(ref < 0.05 - ap.obstacles[:, 3].min() + 1e-9)      # (the planted link passes 5 cm from a centre)
        assert np.all(ref <= ap.clearance(Y, include_goal=True) - rho + 1e-12)
        bad = B // 2
        Yn = Y.copy()
        Yn[bad, g.index("p3"), 1] = np.nan
        cn = _np(ap.template.anchored_link_clearance(Yn))
        ok = np.arange(B) != bad
        assert np.isnan(cn[bad]) and np.array_equal(_bits(cn[ok]), _bits(_np(ap.template.anchored_link_clearance(Y[ok]))))
        assert np.array_equal(_bits(cn[ok]), _bits(c[ok]))
        # the end effector's row alone (the end of the last link, a row the node clearance never reads)
        Yn = Y.copy()
        Yn[bad, g.index("p6"), 0] = np.nan
        cn = _np(ap.template.anchored_link_clearance(Yn))
        assert np.isnan(cn[bad]) and np.array_equal(_bits(cn[ok]), _bits(c[ok]))


# ---- 2. the sweep --------------------------------------------------------------------------------------------------
def _device_link_clearance_of(torch, ap, q):
    """Link clearance of the device realization of joint angles q [B, n] (gik_seed_batch; the goal poses play no part)."""
    T = np.broadcast_to(np.eye(4), (len(q), 4, 4)).copy()
    _, Y = ap.base.template.seed(T, q)
    return _np(ap.template.anchored_link_clearance(Y))


@pytest.mark.parametrize("B", [1, 65])
def test_sweep_against_two_plain_calls_and_the_mirror(torch_cuda, B):
    """S = 1 is the minimum of the link clearances of the two ends' device realizations, bit for bit.  S = 1 and 7 against
    the numpy mirror to 1e-11: the device realization is held to the host's to 1e-12 per coordinate
    (tests/test_seeded_gpu.py), so a point moves by at most sqrt(3) 1e-12 and the clearance by no more; the rest is
    margin."""
    torch = torch_cuda
    robot, graph, ap = _problem()
    u = uniform_pairs()
    qa, qb = u["qa"][100:100 + B].copy(), u["qb"][100:100 + B].copy()
    one = _np(ap.sweep_clearance(qa, qb, 1))
    ends = np.minimum(_device_link_clearance_of(torch, ap, qa), _device_link_clearance_of(torch, ap, qb))
    assert one.shape == (B,) and np.array_equal(_bits(one), _bits(ends))
    for S in (1, 7):
        got = _np(ap.sweep_clearance(qa, qb, S))
        want = ap.sweep_clearance_host(qa, qb, S)
        assert np.abs(got - want).max() < 1e-11, S
        assert np.all(got <= one)
    # a NaN angle: NaN for that pair alone, whichever sample it reaches
    if B > 1:
        qn = qb.copy()
        qn[B // 2, 3] = np.nan
        got = _np(ap.sweep_clearance(qa, qn, 7))
        ok = np.arange(B) != B // 2
        assert np.isnan(got[B // 2]) and np.array_equal(_bits(got[ok]), _bits(_np(ap.sweep_clearance(qa, qb, 7))[ok]))
    # device tensors are taken as they are
    assert np.array_equal(_bits(_np(ap.sweep_clearance(torch.from_numpy(qa).cuda(), torch.from_numpy(qb).cuda(), 1))), _bits(one))


def test_sweep_finds_the_pairs_the_ends_miss(torch_cuda):
    """The pairs the CPU found: both ends link-clear by more than 1 cm, more than 1 cm inside a sphere on the way."""
    torch = torch_cuda
    robot, graph, ap = _problem()
    pairs, _ = sweep_colliding_pairs()
    u = uniform_pairs()
    qa, qb = u["qa"][pairs], u["qb"][pairs]
    assert len(pairs) >= 10
    sw = _np(ap.sweep_clearance(qa, qb, 8))
    print("sweep-colliding pairs:", len(pairs), "deepest", sw.min(), "shallowest", sw.max())
    assert np.all(sw < -0.01)
    assert np.all(_device_link_clearance_of(torch, ap, qa) > 0.01) and np.all(_device_link_clearance_of(torch, ap, qb) > 0.01)
    assert np.all(_np(ap.sweep_clearance(qa, qb, 1)) > 0.01)


# ---- 3. the rule -----------------------------------------------------------------------------------------------------
def _selected(torch, h, tol):
    """The goals gik_anchored_retry_select compacts from a host result: the set a restart attempt solves again."""
    lib, _ffi = _lib()
    B = len(h["stop"])
    stats = torch.from_numpy(_stats_buffer(torch, h["stop"])).cuda()
    d = [torch.from_numpy(np.ascontiguousarray(h[k])).cuda() for k in ("pos_err", "rot_err", "clearance")]
    idx = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    _ffi.check(lib.gik_anchored_retry_select(stats.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), B,
                                             tol["pos_tol"], tol["rot_tol"], tol["clear_tol"], idx.data_ptr(), cnt.data_ptr(),
                                             _stream(torch)))
    torch.cuda.synchronize()
    return np.sort(idx.cpu().numpy()[:int(cnt.item())])


def test_the_rule_reads_the_link_clearance(torch_cuda):
    """16 configurations whose joint points are clear by more than 1 cm and whose links are more than 1 cm inside a
    sphere, each asked for its own pose from itself: the solve stops at once.  The node rule sees nothing to retry; the
    link rule sends every one of them back, and what it keeps is, bit for bit, either attempt 0's answer or the seeded
    solve from the generator's angles with the link clearance of that answer."""
    torch = torch_cuda
    rs = _rs()
    robot, graph, ap = _problem()
    q = uniform_pairs()["qa"][node_clear_link_colliding()[:16]]
    assert len(q) == 16
    T = robot.fk_batch(q)
    lo, hi = robot.limits_arrays()
    seed = 41
    # attempt 0 in either mode: the same answer, its node and its link clearance
    P = _host(ap.solve(T, q_init=q))
    P_nodes = _host(ap.solve(T, q_init=q, clearance_mode="nodes"))
    P_links = _host(ap.solve(T, q_init=q, clearance_mode="links"))
    assert _same_rows(P_nodes, P)
    assert all(np.array_equal(_bits(P_links[k]), _bits(P[k])) for k in KEYS if k != "clearance")
    assert int(P["iterations"].max()) <= 1 and np.all(P["stop"] == 0)
    assert np.array_equal(_bits(P_links["clearance"]), _bits(_np(ap.template.anchored_link_clearance(P["x"]))))
    assert np.abs(P_links["clearance"] - ap.link_clearance(P["x"])).max() < 1e-12
    print("attempt 0: node clearance", P["clearance"].min(), "..", P["clearance"].max(), "link clearance",
          P_links["clearance"].min(), "..", P_links["clearance"].max())
    assert np.all(P["clearance"] > 0.0) and np.all(P_links["clearance"] < -0.005)
    assert len(_selected(torch, P, TOL)) == 0 and np.array_equal(_selected(torch, P_links, TOL), np.arange(16))
    # nodes: nothing is retried, and the word changes nothing
    N = _host(ap.solve(T, q_init=q, retries=2, retry_seed=seed, clearance_mode="nodes", **TOL))
    D = _host(ap.solve(T, q_init=q, retries=2, retry_seed=seed, **TOL))
    assert not N["attempt"].any() and _same_rows(N, P)
    assert _same_rows(N, D) and np.array_equal(N["attempt"], D["attempt"])
    # links
    R = _host(ap.solve(T, q_init=q, retries=2, retry_seed=seed, clearance_mode="links", **TOL))
    att = R["attempt"]
    assert att.min() >= 0 and att.max() <= 2
    print("links: attempt histogram", np.bincount(att, minlength=3).tolist(), "link clearance after", R["clearance"].min(), "..",
          R["clearance"].max(), "clear after", int((R["clearance"] >= -TOL["clear_tol"]).sum()), "of 16")
    first = att == 0
    assert _same_rows(R, P_links, first, first)
    for g in np.flatnonzero(att > 0):
        q0 = rs.retry_seeds_host(seed, [g], int(att[g]), lo, hi)
        S = _host(ap.solve(T[g:g + 1], q_init=q0, clearance_mode="links"))
        assert _same_rows(R, S, slice(g, g + 1)), (g, att[g])
        assert np.array_equal(_bits(S["clearance"]), _bits(_np(ap.template.anchored_link_clearance(S["x"]))))
        quad = lambda h, sel: (h["stop"][sel], h["pos_err"][sel], h["rot_err"][sel], h["clearance"][sel])      # noqa: E731
        assert rs.anchored_retry_better(quad(R, slice(g, g + 1)), quad(P_links, slice(g, g + 1)), **TOL)[0]
    assert np.abs(R["clearance"] - ap.link_clearance(R["x"])).max() < 1e-12
    # a cold batch in link mode: attempt 0 is the cold call, then the link clearance of its answer
    cold = ap.solve(T)
    Cl = _host(ap.solve(T, clearance=True, clearance_mode="links"))
    assert np.array_equal(_bits(_np(cold["x"])), _bits(Cl["x"]))
    assert np.array_equal(_bits(Cl["clearance"]), _bits(_np(ap.template.anchored_link_clearance(cold["x"]))))
    C0 = _host(ap.solve(T, retries=1, retry_seed=seed, clearance_mode="links", **TOL))
    keep = C0["attempt"] == 0
    assert _same_rows(C0, Cl, keep, keep)


# ---- 4. path tracking ----------------------------------------------------------------------------------------------
def test_solve_trajectory_sweep(torch_cuda):
    robot, graph, ap = _problem()
    Q, T = tracking_input()
    Bp, L = 8, 3
    T, q_start = T[:Bp, :L], Q[:Bp, 0]
    q0, Y0, info0 = ap.solve_trajectory(T, q_start, return_Y=True)
    q1, Y1, info1 = ap.solve_trajectory(T, q_start, return_Y=True, sweep=2)
    assert "sweep_clearance" not in info0 and info1["sweep_clearance"].shape == (Bp, L)
    assert np.array_equal(_bits(q0), _bits(q1)) and np.array_equal(_bits(Y0), _bits(Y1))
    assert set(info1) == set(info0) | {"sweep_clearance"}
    for k in info0:
        if k != "solve_time":
            assert np.array_equal(_bits(info0[k]), _bits(info1[k])), k
    prev = q_start
    for l in range(L):
        want = _np(ap.sweep_clearance(prev, q1[:, l], 2))
        assert np.array_equal(_bits(info1["sweep_clearance"][:, l]), _bits(want)), l
        prev = q1[:, l]
    # link mode: the same answers, the link clearance in info["clearance"]; with restarts the sweep is still reported
    q2, Y2, info2 = ap.solve_trajectory(T, q_start, return_Y=True, clearance_mode="links", sweep=2)
    assert np.array_equal(_bits(q2), _bits(q1)) and np.array_equal(_bits(info2["sweep_clearance"]), _bits(info1["sweep_clearance"]))
    for l in range(L):
        assert np.array_equal(_bits(info2["clearance"][:, l]), _bits(_np(ap.template.anchored_link_clearance(Y2[:, l]))))
    assert np.all(info2["clearance"] <= info1["clearance"] + 1e-12)    # (links are nearer than joint points)
    q3, Y3, info3 = ap.solve_trajectory(T, q_start, retries=1, retry_seed=3, clearance_mode="links", sweep=2, **TOL)
    assert info3["sweep_clearance"].shape == (Bp, L) and info3["attempt"].shape == (Bp, L)
    prev = q_start
    for l in range(L):
        assert np.array_equal(_bits(info3["sweep_clearance"][:, l]), _bits(_np(ap.sweep_clearance(prev, q3[:, l], 2)))), l
        prev = q3[:, l]


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_come_with_a_message_and_queue_nothing(torch_cuda):
    torch = torch_cuda
    lib, _ffi = _lib()
    robot, graph, ap = _problem()
    _, _, bare = _problem("none")
    tpl, base = ap.template, ap.base.template
    assert bare.template.n_link is None and tpl.n_link == 6
    B, n = 8, robot.n
    u = uniform_pairs()
    qa, qb = torch.from_numpy(u["qa"][:B].copy()).cuda(), torch.from_numpy(u["qb"][:B].copy()).cuda()
    T = torch.from_numpy(np.ascontiguousarray(robot.fk_batch(u["qa"][:B]))).cuda()
    lo, hi = (torch.from_numpy(a).cuda() for a in robot.limits_arrays())
    Y = torch.from_numpy(u["Ya"][:B].reshape(B, -1).copy()).cuda()
    out = tpl.alloc_anchored_buffers(base, B, clearance=True)
    del out["ws"]
    out["attempt"] = torch.empty(B, dtype=torch.int32, device="cuda")
    out["sweep"] = torch.empty(B, dtype=torch.float64, device="cuda")
    rws = torch.empty(int(lib.gik_anchored_retry_ws_bytes(tpl._h, base._h, B)) // 8 + 1, dtype=torch.float64, device="cuda")
    nbytes = int(lib.gik_anchored_sweep_ws_bytes(tpl._h, base._h, B, 4))
    assert nbytes == 8 * B * 5 * (n + 16 + base.T + tpl.full_N * 3 + 1)
    sws = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
    for v in out.values():
        v.view(torch.int32).fill_(-7)
    before = {k: v.clone() for k, v in out.items()}
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    st = C.c_void_p(s.cuda_stream)

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(out[k].view(torch.int32), before[k].view(torch.int32)) for k in out)

    def retry(anch=tpl, mode=0, retries=1, n_goals=B):
        opts = _ffi.AnchoredRetryOpts(retries=retries, clearance_mode=mode, seed=1, pos_tol=0.01, rot_tol=0.01,
                                      d_q_lo=lo.data_ptr(), d_q_hi=hi.data_ptr(), clear_tol=1e-4, spread=0.0)
        rc = lib.gik_anchored_ik_batch_retry(anch._h, base._h, T.data_ptr(), qa.data_ptr(), n_goals, C.byref(opts),
                                             rws.data_ptr(), out["Y"].data_ptr(), out["stats"].data_ptr(), out["q"].data_ptr(),
                                             out["pos_err"].data_ptr(), out["rot_err"].data_ptr(), out["clearance"].data_ptr(),
                                             out["attempt"].data_ptr(), st)
        return rc, lib.gik_last_error().decode()

    def link(anch=tpl._h, y=Y.data_ptr(), o=out["clearance"].data_ptr(), n_goals=B):
        return lib.gik_anchored_link_clearance(anch, y, n_goals, o, st), lib.gik_last_error().decode()

    def sweep(anch=tpl._h, bs=base._h, a=qa.data_ptr(), b=qb.data_ptr(), S=4, ws=sws.data_ptr(), o=out["sweep"].data_ptr(), n_goals=B):
        return lib.gik_anchored_sweep_clearance(anch, bs, a, b, n_goals, S, ws, o, st), lib.gik_last_error().decode()

    calls = [
        (lambda: retry(anch=bare.template, mode=1), "no links attached"), (lambda: retry(anch=bare.template, mode=1, retries=0), "no links attached"),
        (lambda: retry(mode=2), "clearance_mode"), (lambda: retry(mode=-1, retries=0), "clearance_mode"),
        (lambda: link(anch=bare.template._h), "no links attached"), (lambda: link(anch=base._h), "fixed-anchor"),
        (lambda: link(y=None), "null buffer"), (lambda: link(o=None), "null buffer"), (lambda: link(n_goals=-1), "bad argument"),
        (lambda: sweep(anch=bare.template._h), "no links attached"), (lambda: sweep(anch=base._h), "fixed-anchor"),
        (lambda: sweep(bs=tpl._h), "pipeline"), (lambda: sweep(S=0), "samples"), (lambda: sweep(a=None), "null buffer"),
        (lambda: sweep(b=None), "null buffer"), (lambda: sweep(ws=None), "null buffer"), (lambda: sweep(o=None), "null buffer"),
        (lambda: sweep(n_goals=-1), "bad argument"), (lambda: sweep(S=2 ** 31 - 1), "fit an int"),
    ]
    for call, word in calls:
        rc, msg = call()
        assert rc != 0 and word in msg and "gik_anchored_" in msg, (word, msg)
        assert untouched(), word
    assert lib.gik_anchored_sweep_ws_bytes(base._h, base._h, B, 4) == 0 and lib.gik_anchored_sweep_ws_bytes(tpl._h, base._h, B, 0) == 0
    # attach: a second one, and on a template of its own a bad row, a bad radius, a non-anchored handle -- then a good one
    rows = np.array([0, 4], dtype=np.int32)

    def attach(h, a, b, r):
        a, b, r = np.asarray(a, dtype=np.int32), np.asarray(b, dtype=np.int32), np.asarray(r, dtype=np.float64)
        d = _ffi.LinkDesc(n_link=len(a), link_a=a.ctypes.data_as(C.POINTER(C.c_int32)),
                          link_b=b.ctypes.data_as(C.POINTER(C.c_int32)), link_radius=r.ctypes.data_as(C.POINTER(C.c_double)))
        return lib.gik_anchored_attach_links(h, C.byref(d)), lib.gik_last_error().decode()

    robot2, graph2 = make_graph("ur10_table")
    fresh = _rs().AnchoredProblem(graph2, links=[]).template
    N = fresh.full_N
    for (a, b, r), word in ((([0, N], rows, [0.0, 0.0]), "outside"), ((rows, [4, -1], [0.0, 0.0]), "outside"),
                            ((rows, rows, [0.0, -1e-3]), "link_radius"), ((rows, rows, [np.nan, 0.0]), "link_radius"),
                            ((np.zeros(65), np.zeros(65), np.zeros(65)), "n_link")):
        rc, msg = attach(fresh._h, a, b, r)
        assert rc != 0 and word in msg and "gik_anchored_attach_links" in msg, msg
    rc, msg = attach(base._h, rows, rows, [0.0, 0.0])
    assert rc != 0 and "fixed-anchor" in msg
    rc, msg = link(anch=fresh._h)
    assert rc != 0 and "no links attached" in msg            # (a refused attach attaches nothing)
    rc, msg = attach(fresh._h, rows, [4, N - 1], [0.0, 0.02])
    assert rc == 0, msg
    rc, msg = attach(fresh._h, rows, rows, [0.0, 0.0])
    assert rc != 0 and "already attached" in msg
    rc, msg = attach(tpl._h, rows, rows, [0.0, 0.0])
    assert rc != 0 and "already attached" in msg
    assert untouched()
    # a capturing stream: refused, and the capture stays empty
    hip = _hip_runtime()
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    assert hip.hipStreamBeginCapture(st, 2) == 0      # hipStreamCaptureModeRelaxed
    got = [link(), sweep(), retry(mode=1), retry(mode=1, retries=0)]
    graph_h = C.c_void_p()
    assert hip.hipStreamEndCapture(st, C.byref(graph_h)) == 0
    n_nodes = C.c_size_t(99)
    assert hip.hipGraphGetNodes(graph_h, None, C.byref(n_nodes)) == 0
    hip.hipGraphDestroy(graph_h)
    assert all(rc != 0 and "capturing" in msg for rc, msg in got), got
    assert n_nodes.value == 0 and untouched()
    # B == 0 returns 0 and queues nothing
    for rc, msg in (link(n_goals=0), sweep(n_goals=0), retry(mode=1, n_goals=0)):
        assert rc == 0, msg
    assert untouched()
    # the same calls on the same stream, not capturing, run: the answers of the Python layer
    rc, msg = link()
    assert rc == 0, msg
    rc, msg = sweep()
    assert rc == 0, msg
    s.synchronize()
    assert torch.equal(out["clearance"], tpl.anchored_link_clearance(Y.reshape(B, -1, 3)))
    assert torch.equal(out["sweep"], ap.sweep_clearance(qa, qb, 4))
    rc, msg = retry(mode=1, retries=2)
    assert rc == 0, msg
    s.synchronize()
    ref = ap.solve(_np(T).reshape(B, 4, 4), q_init=_np(qa), retries=2, retry_seed=1, clearance_mode="links", **TOL)
    torch.cuda.synchronize()
    assert torch.equal(out["q"], ref["q"]) and torch.equal(out["attempt"], ref["attempt"])
    assert torch.equal(out["clearance"], ref["clearance"])
    # the link set of the fresh template is its own: two links, the second 2 cm thick
    want = _Cell([[0, 4], [4, N - 1]], ap.obstacles, [0.0, 0.02])(u["Ya"][:B])
    assert np.abs(_np(fresh.anchored_link_clearance(u["Ya"][:B].copy())) - want).max() < 1e-12
