"""Self-collision clearance (link against link) in the fixed-anchor solve on the MI355X: anch_self_clearance_kernel in both
of its lane maps against the numpy mirror, the merged clearance of clearance_mode="links+self", the restart rule reading
it on configurations that every other measure calls clear, the two-output sweep, and the refusals of the new entry
points.  UR10 + table_environment().  The inputs and the mirror's own tests: tests/test_anchored_self_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import make_graph
from test_anchored_retry_gpu import KEYS, TOL, _bits, _host, _same_rows
from test_anchored_seeded_host import tracking_input
from test_anchored_self_host import RHO, _Cell, uniform_configurations, world_clear_self_colliding
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
def _problem(self_pairs="auto", links="skeleton"):
    """UR10 + table, skeleton capsules of 3 cm: with the ten "auto" pairs, without self pairs, or without links at all."""
    robot, graph = make_graph("ur10_table")
    if links != "skeleton":
        return robot, graph, _rs().AnchoredProblem(graph, links=[])
    return robot, graph, _rs().AnchoredProblem(graph, link_radius=RHO, self_pairs=self_pairs)


# ---- 1. the kernel -------------------------------------------------------------------------------------------------
N_ROWS = 16      # UR10's robot graph


def _link_set(n_link, rng):
    """n_link distinct links over the 16 rows: eight with rows of their own -- (0, 1), (2, 3), (4, 5), (6, 7) are the
    planted ones --, eight that join them into a ring, the rest drawn."""
    links = ([(2 * i, 2 * i + 1) for i in range(8)] + [(2 * i + 1, (2 * i + 2) % N_ROWS) for i in range(8)])[:n_link]
    every = [(a, b) for a in range(N_ROWS) for b in range(N_ROWS) if a != b and (a, b) not in links and (b, a) not in links]
    links += [every[i] for i in rng.permutation(len(every))[:n_link - len(links)]]
    return np.array(links, dtype=np.int32)


def _pair_list(links, n_pair, rng):
    """n_pair pairs of the links: every pair, or (0, 1), (1, 2), (2, 3) first (the planted ones) and the rest drawn from
    the pairs that share no row, some turned round.  (Among every pair of 64 links over 16 rows some share a row, and
    their value -rho_l - rho_m is the minimum whatever the points: that case tests the stride over 2016 pairs and the
    NaN, the others the geometry.)"""
    n_link = len(links)
    every = [(l, m) for l in range(n_link) for m in range(l + 1, n_link)]
    if n_pair == len(every):
        return np.array(every, dtype=np.int32)
    head = [(0, 1), (1, 2), (2, 3)][:n_pair]
    rest = [(l, m) for l, m in every if (l, m) not in head and not set(links[l].tolist()) & set(links[m].tolist())]
    pairs = head + [rest[i] if k % 3 else rest[i][::-1] for k, i in enumerate(rng.permutation(len(rest))[:n_pair - len(head)])]
    return np.array(pairs, dtype=np.int32).reshape(-1, 2)


def _points(B, rng):
    """[B, 16, 3] random point matrices; by goal % 4: 1 -- link 0 has length zero; 2 -- link 2 passes through a point of
    link 1 (crossing); 3 -- link 3 is parallel to link 2, 5 cm beside it."""
    Y = 0.5 * rng.randn(B, N_ROWS, 3)
    for b in range(B):
        if b % 4 == 1:
            Y[b, 1] = Y[b, 0]
        if b % 4 == 2:
            p, w = Y[b, 2] + 0.3 * (Y[b, 3] - Y[b, 2]), rng.randn(3)
            Y[b, 4], Y[b, 5] = p - 0.4 * w, p + 0.6 * w
        if b % 4 == 3:
            d = Y[b, 5] - Y[b, 4]
            Y[b, 6] = Y[b, 4] + 0.25 * d + np.array([0.05, 0.0, 0.0])
            Y[b, 7] = Y[b, 6] + 0.7 * d
    return Y


def _device_self(torch, tpl, Y, pad=3):
    """gik_anchored_self_clearance on Y [B, 16, 3] through the library, into a buffer of B + pad: the B values, after
    checking that the entries beyond B are untouched."""
    lib, _ffi = _lib()
    B = len(Y)
    y = torch.from_numpy(np.ascontiguousarray(Y).reshape(B, -1)).cuda()
    out = torch.full((B + pad,), -7.0, dtype=torch.float64, device="cuda")
    _ffi.check(lib.gik_anchored_self_clearance(tpl._h, y.data_ptr(), B, out.data_ptr(), _stream(torch)))
    torch.cuda.synchronize()
    got = _np(out)
    assert np.all(got[B:] == -7.0)
    return got[:B]


BATCHES = (1, 3, 4, 5, 63, 65)


@pytest.mark.parametrize("n_pair,n_link,rho", [(1, 16, "mixed"), (10, 16, "mixed"), (10, 16, 0.0), (10, 16, 0.03), (16, 16, "mixed"),
                                               (17, 16, "mixed"), (64, 16, "mixed"), (65, 16, "mixed"), (65, 16, 0.0),
                                               (65, 16, 0.03), (2016, 64, "mixed"), (0, 16, "mixed")])
def test_self_kernel_in_both_lane_maps(torch_cuda, n_pair, n_link, rho):
    """Up to 16 pairs four goals share a wavefront (1, 10, 16 pairs), beyond that a goal has its own (17, 64, 65 and the
    2016 pairs of 64 links); batches that fill a packed wavefront partly and that stride the grid; radii 0, 3 cm and
    mixed; zero-length, crossing and parallel links planted.  Against the numpy mirror to 1e-12.  A NaN goal is NaN
    alone; a goal's bits do not depend on its batch; nothing is written beyond B; no pair: +inf."""
    torch = torch_cuda
    rng = np.random.RandomState(1000 + 7 * n_pair + n_link)
    links = _link_set(n_link, rng)
    pairs = _pair_list(links, n_pair, rng)
    radius = np.where(np.arange(n_link) % 2, 0.03, 0.0) if rho == "mixed" else np.full(n_link, rho)
    assert len(pairs) == n_pair and len(set(map(tuple, links.tolist()))) == n_link
    robot, graph = make_graph("ur10_table")
    tpl = _rs().AnchoredProblem(graph, links=[]).template
    assert tpl.full_N == N_ROWS and tpl.n_self is None
    tpl.attach_links(links[:, 0], links[:, 1], radius)
    tpl.attach_self_pairs(pairs[:, 0], pairs[:, 1])
    assert tpl.n_self == n_pair
    mirror = _Cell(links, pairs, radius)
    Y = _points(65, rng)
    full = _device_self(torch, tpl, Y)
    if n_pair == 0:
        assert np.all(np.isposinf(full)) and np.all(np.isposinf(mirror(Y)))
        return
    want = mirror(Y)
    print("n_pair", n_pair, "worst", np.abs(full - want).max(), "min", want.min(), "max", want.max())
    assert np.all(np.isfinite(want)) and np.abs(full - want).max() < 1e-12
    assert np.array_equal(_bits(_np(tpl.anchored_self_clearance(Y))), _bits(full))      # the Python layer's call
    for B in BATCHES:
        got = _device_self(torch, tpl, Y[:B])
        assert np.array_equal(_bits(got), _bits(full[:B])), B
    # a NaN in one goal of a four-goal wavefront, in an end pair 0 reads: the others are what they are alone
    for B, bad in ((4, 1), (5, 4), (65, 62)):
        Yn = Y[:B].copy()
        Yn[bad, links[pairs[0, 0], 1], 2] = np.nan
        got = _device_self(torch, tpl, Yn)
        ok = np.arange(B) != bad
        assert np.isnan(got[bad]) and np.array_equal(_bits(got[ok]), _bits(full[:B][ok])), (B, bad)
        assert np.isnan(mirror(Yn)[bad])
        for g in np.flatnonzero(ok)[:3]:
            assert np.array_equal(_bits(_device_self(torch, tpl, Yn[g:g + 1])), _bits(got[g:g + 1]))


# ---- 2. the merge ----------------------------------------------------------------------------------------------------
def test_mode_links_self_is_the_minimum_of_the_two_device_clearances(torch_cuda):
    """65 goals, each asked for its own pose from itself.  "links+self": the clearance is np.minimum of the device link
    clearance and the device self clearance of the returned points, bit for bit -- with the problem's own spheres and with
    two scenes.  "nodes" and "links" return what they return on a problem built without self_pairs."""
    robot, graph, ap = _problem()
    _, _, plain = _problem(None)
    assert plain.self_pairs is None and plain.template.n_self is None and ap.template.n_self == 10
    u = uniform_configurations()
    q = u["q"][:65].copy()
    T = robot.fk_batch(q)
    tpl = ap.template
    R = ap.solve(T, q_init=q, clearance=True, clearance_mode="links+self")
    assert "attempt" not in R
    link, own = _np(tpl.anchored_link_clearance(R["x"])), _np(tpl.anchored_self_clearance(R["x"]))
    assert np.array_equal(_bits(_np(R["clearance"])), _bits(np.minimum(link, own)))
    assert (own < link).sum() >= 3 and (link < own).sum() >= 3           # both sides of the minimum are taken
    assert np.abs(own - ap.self_clearance(_np(R["x"]))).max() < 1e-12
    cold = ap.solve(T[:9], clearance=True, clearance_mode="links+self")
    assert np.array_equal(_bits(_np(cold["x"])), _bits(_np(plain.solve(T[:9])["x"])))
    assert np.array_equal(_bits(_np(cold["clearance"])), _bits(np.minimum(_np(tpl.anchored_link_clearance(cold["x"])),
                                                                        _np(tpl.anchored_self_clearance(cold["x"])))))
    # two scenes
    S = ap.scene_set([ap.obstacles[:60], ap.obstacles[40:] + np.array([0.0, 0.0, 0.05, 0.0])])
    ids = np.arange(65) % 2
    Rs = ap.solve(T, q_init=q, clearance=True, clearance_mode="links+self", scenes=S, scene_id=ids)
    link_s = _np(tpl.anchored_link_clearance(Rs["x"], scenes=S, scene_id=ids))
    assert np.array_equal(_bits(_np(Rs["clearance"])), _bits(np.minimum(link_s, _np(tpl.anchored_self_clearance(Rs["x"])))))
    assert not np.array_equal(link_s, link)
    # the other modes do not see the pairs
    for mode in ("nodes", "links"):
        a = _host(ap.solve(T, q_init=q, clearance=True, clearance_mode=mode))
        b = _host(plain.solve(T, q_init=q, clearance=True, clearance_mode=mode))
        assert _same_rows(a, b), mode
        a = _host(ap.solve(T, q_init=q, retries=1, retry_seed=5, clearance_mode=mode, **TOL))
        b = _host(plain.solve(T, q_init=q, retries=1, retry_seed=5, clearance_mode=mode, **TOL))
        assert _same_rows(a, b) and np.array_equal(a["attempt"], b["attempt"]), mode


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


def test_the_rule_reads_the_self_clearance(torch_cuda):
    """16 configurations whose joint points and links are more than 1 cm clear of the table and whose own capsules are
    more than 1 cm inside each other, each asked for its own pose from itself: the solve stops at once.  The link rule
    sees nothing to retry; "links+self" sends every one of them back, and what it keeps is, bit for bit, either attempt
    0's answer or the seeded solve from the generator's angles with the merged clearance of that answer."""
    torch = torch_cuda
    rs = _rs()
    robot, graph, ap = _problem()
    q = uniform_configurations()["q"][world_clear_self_colliding()[:16]]
    assert len(q) == 16
    T = robot.fk_batch(q)
    lo, hi = robot.limits_arrays()
    seed = 43
    P = {mode: _host(ap.solve(T, q_init=q, clearance_mode=mode)) for mode in ("nodes", "links", "links+self")}
    for mode, h in P.items():
        assert int(h["iterations"].max()) <= 1 and np.all(h["stop"] == 0), mode
        assert h["pos_err"].max() <= TOL["pos_tol"] and h["rot_err"].max() <= TOL["rot_tol"], mode
        assert all(np.array_equal(_bits(h[k]), _bits(P["nodes"][k])) for k in KEYS if k != "clearance"), mode
    both = P["links+self"]
    assert np.all(P["nodes"]["clearance"] > 0.005) and np.all(P["links"]["clearance"] > 0.005) and np.all(both["clearance"] < -0.005)
    assert len(_selected(torch, P["links"], TOL)) == 0 and np.array_equal(_selected(torch, both, TOL), np.arange(16))
    L = _host(ap.solve(T, q_init=q, retries=2, retry_seed=seed, clearance_mode="links", **TOL))
    assert not L["attempt"].any() and _same_rows(L, P["links"])
    R = _host(ap.solve(T, q_init=q, retries=2, retry_seed=seed, clearance_mode="links+self", **TOL))
    att = R["attempt"]
    assert att.min() >= 0 and att.max() <= 2
    print("links+self: attempt histogram", np.bincount(att, minlength=3).tolist(), "clearance after", R["clearance"].min(), "..",
          R["clearance"].max(), "; self-clear after:", int((ap.self_clearance(R["x"]) >= -TOL["clear_tol"]).sum()), "of 16; on their pose:",
          int(((R["pos_err"] <= TOL["pos_tol"]) & (R["rot_err"] <= TOL["rot_tol"])).sum()))
    first = att == 0
    assert _same_rows(R, both, first, first)
    for g in np.flatnonzero(att > 0):
        q0 = rs.retry_seeds_host(seed, [g], int(att[g]), lo, hi)
        S = _host(ap.solve(T[g:g + 1], q_init=q0, clearance_mode="links+self"))
        assert _same_rows(R, S, slice(g, g + 1)), (g, att[g])
        quad = lambda h, sel: (h["stop"][sel], h["pos_err"][sel], h["rot_err"][sel], h["clearance"][sel])      # noqa: E731
        assert rs.anchored_retry_better(quad(R, slice(g, g + 1)), quad(both, slice(g, g + 1)), **TOL)[0]
    want = np.minimum(ap.link_clearance(R["x"]), ap.self_clearance(R["x"]))
    assert np.abs(R["clearance"] - want).max() < 1e-12


# ---- 4. the sweep ----------------------------------------------------------------------------------------------------
def _realization(ap, q):
    T = np.broadcast_to(np.eye(4), (len(q), 4, 4)).copy()
    return ap.base.template.seed(T, q)[1]


@pytest.mark.parametrize("B", [1, 65])
def test_sweep_self_against_two_plain_calls_and_the_mirror(torch_cuda, B):
    """S = 1 is the minimum of the self clearances of the two ends' device realizations, bit for bit.  S = 1 and 7 against
    the numpy mirror to 1e-11, the existing sweep's bar.  With both outputs the link output is
    gik_anchored_sweep_clearance's."""
    robot, graph, ap = _problem()
    tpl, base = ap.template, ap.base.template
    u = uniform_configurations()
    qa, qb = u["q"][200:200 + B].copy(), u["q"][300:300 + B].copy()
    qb = qa + 0.3 * (qb - qa)
    one = _np(ap.sweep_self_clearance(qa, qb, 1))
    ends = np.minimum(_np(tpl.anchored_self_clearance(_realization(ap, qa))), _np(tpl.anchored_self_clearance(_realization(ap, qb))))
    assert one.shape == (B,) and np.array_equal(_bits(one), _bits(ends))
    for S in (1, 7):
        link, own = tpl.anchored_sweep_clearances(base, qa, qb, S)
        assert np.abs(_np(own) - ap.sweep_self_clearance_host(qa, qb, S)).max() < 1e-11, S
        assert np.all(_np(own) <= one)
        assert np.array_equal(_bits(_np(link)), _bits(_np(ap.sweep_clearance(qa, qb, S)))), S
        assert np.array_equal(_bits(_np(own)), _bits(_np(ap.sweep_self_clearance(qa, qb, S)))), S
        only_link, none = tpl.anchored_sweep_clearances(base, qa, qb, S, self_=False)
        assert none is None and np.array_equal(_bits(_np(only_link)), _bits(_np(link)))


def test_solve_trajectory_sweep_self(torch_cuda):
    robot, graph, ap = _problem()
    Q, T = tracking_input()
    Bp, L = 8, 3
    T, q_start = T[:Bp, :L], Q[:Bp, 0]
    q1, Y1, info1 = ap.solve_trajectory(T, q_start, return_Y=True, clearance_mode="links", sweep=2)
    q2, Y2, info2 = ap.solve_trajectory(T, q_start, return_Y=True, clearance_mode="links+self", sweep=2)
    assert "sweep_self_clearance" not in info1 and set(info2) == set(info1) | {"sweep_self_clearance"}
    assert np.array_equal(_bits(q1), _bits(q2)) and np.array_equal(_bits(Y1), _bits(Y2))
    assert np.array_equal(_bits(info1["sweep_clearance"]), _bits(info2["sweep_clearance"]))
    assert info2["sweep_self_clearance"].shape == (Bp, L)
    prev = q_start
    for l in range(L):
        assert np.array_equal(_bits(info2["sweep_clearance"][:, l]), _bits(_np(ap.sweep_clearance(prev, q2[:, l], 2)))), l
        assert np.array_equal(_bits(info2["sweep_self_clearance"][:, l]), _bits(_np(ap.sweep_self_clearance(prev, q2[:, l], 2)))), l
        merged = np.minimum(_np(ap.template.anchored_link_clearance(Y2[:, l])), _np(ap.template.anchored_self_clearance(Y2[:, l])))
        assert np.array_equal(_bits(info2["clearance"][:, l]), _bits(merged)), l
        prev = q2[:, l]
    q3, _, info3 = ap.solve_trajectory(T, q_start, retries=1, retry_seed=3, clearance_mode="links+self", sweep=2, **TOL)
    assert info3["sweep_self_clearance"].shape == (Bp, L) and info3["attempt"].shape == (Bp, L)
    prev = q_start
    for l in range(L):
        assert np.array_equal(_bits(info3["sweep_self_clearance"][:, l]), _bits(_np(ap.sweep_self_clearance(prev, q3[:, l], 2)))), l
        prev = q3[:, l]


# ---- 5. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_come_with_a_message_and_queue_nothing(torch_cuda):
    torch = torch_cuda
    lib, _ffi = _lib()
    robot, graph, ap = _problem()
    _, _, plain = _problem(None)              # links, no self pairs
    _, _, bare = _problem(None, "none")       # no links
    tpl, base = ap.template, ap.base.template
    B = 8
    u = uniform_configurations()
    qa, qb = torch.from_numpy(u["q"][:B].copy()).cuda(), torch.from_numpy(u["q"][B:2 * B].copy()).cuda()
    T = torch.from_numpy(np.ascontiguousarray(robot.fk_batch(u["q"][:B]))).cuda()
    lo, hi = (torch.from_numpy(a).cuda() for a in robot.limits_arrays())
    Y = torch.from_numpy(u["Y"][:B].reshape(B, -1).copy()).cuda()
    out = tpl.alloc_anchored_buffers(base, B, clearance=True)
    out["attempt"] = torch.empty(B, dtype=torch.int32, device="cuda")
    out["sweep_link"] = torch.empty(B, dtype=torch.float64, device="cuda")
    out["sweep_self"] = torch.empty(B, dtype=torch.float64, device="cuda")
    rws = torch.empty(int(lib.gik_anchored_retry_ws_bytes(tpl._h, base._h, B)) // 8 + B + 1, dtype=torch.float64, device="cuda")
    sws = torch.empty(int(lib.gik_anchored_sweep_ws_bytes(tpl._h, base._h, B, 4)) // 8, dtype=torch.float64, device="cuda")
    for v in out.values():
        v.view(torch.int32).fill_(-7)
    before = {k: v.clone() for k, v in out.items()}
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    st = C.c_void_p(s.cuda_stream)
    scenes = ap.scene_set([ap.obstacles[:10]])
    sc = scenes.desc(None)
    answer = [out[k].data_ptr() for k in ("Y", "stats", "q", "pos_err", "rot_err")]

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(out[k].view(torch.int32), before[k].view(torch.int32)) for k in out)

    def err(rc):
        return rc, lib.gik_last_error().decode()

    def opts(retries, mode=2):
        return _ffi.AnchoredRetryOpts(retries=retries, clearance_mode=mode, seed=1, pos_tol=0.01, rot_tol=0.01, d_q_lo=lo.data_ptr(),
                                      d_q_hi=hi.data_ptr(), clear_tol=1e-4, spread=0.0)

    def retry(anch=tpl, retries=1, n_goals=B, mode=2):
        return err(lib.gik_anchored_ik_batch_retry(anch._h, base._h, T.data_ptr(), qa.data_ptr(), n_goals, C.byref(opts(retries, mode)),
                                                   rws.data_ptr(), *answer, out["clearance"].data_ptr(), out["attempt"].data_ptr(), st))

    def retry_scenes(anch=tpl, retries=1):
        return err(lib.gik_anchored_ik_batch_retry_scenes(anch._h, base._h, T.data_ptr(), qa.data_ptr(), B, C.byref(opts(retries)),
                                                          C.byref(sc), rws.data_ptr(), *answer, out["clearance"].data_ptr(),
                                                          out["attempt"].data_ptr(), st))

    def ik_scenes(anch=tpl):
        return err(lib.gik_anchored_ik_batch_scenes(anch._h, base._h, T.data_ptr(), qa.data_ptr(), B, C.byref(sc), out["ws"].data_ptr(),
                                                    *answer, out["clearance"].data_ptr(), 2, st))

    def own(anch=tpl._h, y=Y.data_ptr(), o=out["clearance"].data_ptr(), n_goals=B):
        return err(lib.gik_anchored_self_clearance(anch, y, n_goals, o, st))

    def sweep(anch=tpl._h, bs=base._h, a=qa.data_ptr(), b=qb.data_ptr(), S=4, ws=sws.data_ptr(), o1=out["sweep_link"].data_ptr(),
              o2=out["sweep_self"].data_ptr(), n_goals=B):
        return err(lib.gik_anchored_sweep_clearances(anch, bs, a, b, n_goals, S, ws, o1, o2, st))

    calls = [
        (lambda: retry(anch=plain.template), "clearance_mode"), (lambda: retry(anch=plain.template, retries=0), "clearance_mode"),
        (lambda: retry(anch=bare.template), "clearance_mode"), (lambda: retry(mode=3), "GIK_CLEARANCE_LINKS_SELF (2)"),
        (lambda: retry_scenes(anch=plain.template), "clearance_mode"),
        (lambda: ik_scenes(anch=plain.template), "clearance_mode"),
        (lambda: own(anch=plain.template._h), "no self pairs attached"), (lambda: own(anch=bare.template._h), "no links attached"),
        (lambda: own(anch=base._h), "fixed-anchor"), (lambda: own(y=None), "null buffer"), (lambda: own(o=None), "null buffer"),
        (lambda: own(n_goals=-1), "bad argument"),
        (lambda: sweep(anch=bare.template._h), "no links attached"), (lambda: sweep(anch=base._h), "fixed-anchor"),
        (lambda: sweep(bs=tpl._h), "pipeline"), (lambda: sweep(S=0), "samples"), (lambda: sweep(a=None), "null buffer"),
        (lambda: sweep(b=None), "null buffer"), (lambda: sweep(ws=None), "null buffer"), (lambda: sweep(n_goals=-1), "bad argument"),
        (lambda: sweep(S=2 ** 31 - 1), "fit an int"), (lambda: sweep(o1=None, o2=None), "both outputs"),
        (lambda: sweep(anch=plain.template._h), "no self pairs attached"),
    ]
    for call, word in calls:
        rc, msg = call()
        assert rc != 0 and word in msg and "gik_anchored_" in msg, (word, msg)
        assert untouched(), word
    for call, name in ((retry, "gik_anchored_ik_batch_retry:"), (retry_scenes, "gik_anchored_ik_batch_retry_scenes:"),
                       (ik_scenes, "gik_anchored_ik_batch_scenes:")):
        assert call(anch=plain.template)[1].startswith(name)
    # attach: on a template of its own every refusal, then a good one, then a second one
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)      # noqa: E731

    def attach(h, l, m, n=None):
        l, m = (None if a is None else i32(a) for a in (l, m))
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))      # noqa: E731
        return err(lib.gik_anchored_attach_self_pairs(h, len(l) if n is None else n, ptr(l), ptr(m)))

    robot2, graph2 = make_graph("ur10_table")
    fresh = _rs().AnchoredProblem(graph2, link_radius=RHO).template      # six links, no pairs yet
    for args, word in (((base._h, [0], [2]), "fixed-anchor"), ((bare.template._h, [0], [2]), "no links attached"),
                       ((tpl._h, [0], [2]), "already attached"), ((fresh._h, [0], [2], -1), "n_pair"),
                       ((fresh._h, [0], [2], 2017), "n_pair"), ((fresh._h, None, [2], 1), "null pair array"),
                       ((fresh._h, [0], None, 1), "null pair array"), ((fresh._h, [0, 6], [2, 1]), "outside"),
                       ((fresh._h, [0, 1], [2, -1]), "outside"), ((fresh._h, [0, 3], [2, 3]), "twice")):
        rc, msg = attach(*args)
        assert rc != 0 and word in msg and "gik_anchored_attach_self_pairs" in msg, (word, msg)
    rc, msg = own(anch=fresh._h)
    assert rc != 0 and "no self pairs attached" in msg            # (a refused attach attaches nothing)
    rc, msg = attach(fresh._h, [0, 1], [1, 5])                    # (links 0 and 1 share a row: legal here)
    assert rc == 0, msg
    rc, msg = attach(fresh._h, [0], [2])
    assert rc != 0 and "already attached" in msg
    assert untouched()
    # a capturing stream: refused, and the capture stays empty
    hip = _hip_runtime()
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    assert hip.hipStreamBeginCapture(st, 2) == 0      # hipStreamCaptureModeRelaxed
    got = [own(), sweep(), retry(), retry(retries=0)]
    graph_h = C.c_void_p()
    assert hip.hipStreamEndCapture(st, C.byref(graph_h)) == 0
    n_nodes = C.c_size_t(99)
    assert hip.hipGraphGetNodes(graph_h, None, C.byref(n_nodes)) == 0
    hip.hipGraphDestroy(graph_h)
    assert all(rc != 0 and "capturing" in msg for rc, msg in got), got
    assert n_nodes.value == 0 and untouched()
    # B == 0 returns 0 and queues nothing
    for rc, msg in (own(n_goals=0), sweep(n_goals=0), retry(n_goals=0)):
        assert rc == 0, msg
    assert untouched()
    # the same calls on the same stream, not capturing, run: the answers of the Python layer
    rc, msg = own()
    assert rc == 0, msg
    rc, msg = sweep()
    assert rc == 0, msg
    s.synchronize()
    assert torch.equal(out["clearance"], tpl.anchored_self_clearance(Y.reshape(B, -1, 3)))
    assert torch.equal(out["sweep_link"], ap.sweep_clearance(qa, qb, 4)) and torch.equal(out["sweep_self"], ap.sweep_self_clearance(qa, qb, 4))
    rc, msg = sweep(o1=None)
    assert rc == 0, msg
    s.synchronize()
    assert torch.equal(out["sweep_self"], ap.sweep_self_clearance(qa, qb, 4))
    rc, msg = retry(retries=2)
    assert rc == 0, msg
    s.synchronize()
    ref = ap.solve(_np(T).reshape(B, 4, 4), q_init=_np(qa), retries=2, retry_seed=1, clearance_mode="links+self", **TOL)
    torch.cuda.synchronize()
    assert torch.equal(out["q"], ref["q"]) and torch.equal(out["attempt"], ref["attempt"])
    assert torch.equal(out["clearance"], ref["clearance"])
    # the pairs of the fresh template are its own: (0, 1) shares a row, so its value is -2 rho whatever the points
    want = _Cell(plain.link_rows, [(0, 1), (1, 5)], RHO)(u["Y"][:B])
    assert np.abs(_np(fresh.anchored_self_clearance(u["Y"][:B].copy())) - want).max() < 1e-12 and np.all(want <= -2 * RHO + 1e-15)
