"""Per-goal obstacle scenes in the fixed-anchor solve on the MI355X: a goal solved under scene s equals, BIT FOR BIT, the
same goal solved through the existing entry points on a template (or AnchoredProblem) created with scene s's spheres.
References are built on the same device, one per scene, each solving the WHOLE batch (so that restart seeds, a function
of the goal's index, agree); row b is compared against the reference of scene_id[b].

  1  template level, the synthetic scenes of tests/synth_anchored_scenes.py (9- and 20-slot scene builds, near lists on
     and off), anchored outside the kernels by the numpy reference of the first cost
  2  4096 problems with scene_id = b % 3: more problems than resident waves, so a wave changes scene between problems
  3  UR10, 64 goals, table / table shifted by 0.2 m / empty: cold and seeded, node and link clearance, link hinges
  4  restarts        5  tracking with a scene per waypoint        6  refusals"""
import ctypes as C
import functools

import numpy as np
import pytest

import synth_anchored as sa
import synth_anchored_scenes as ss
from conftest import make_graph
from parity_util import anchored_numpy_terms
from test_anchored_seeded_gpu import _hip_runtime
from test_anchored_seeded_host import collision_input

pytestmark = pytest.mark.gpu

STATS = ("f", "gradnorm", "iterations", "inner_total", "stop", "n_accept")
KEYS = ("x", "q", "pos_err", "rot_err") + STATS
TOL = dict(pos_tol=0.01, rot_tol=0.01, clear_tol=1e-4)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _np(t):
    return t.detach().cpu().numpy()


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64) if x.dtype == np.float64 else x


def _rs():
    from graphik_amd.solvers import riemannian_solver as rs
    return rs


def _host(res, keys):
    return {k: _np(res[k]) for k in keys}


def _assert_rows(got, refs, ids, keys, what=""):
    """row b of every array of `got` is row b of refs[ids[b]], bit for bit"""
    for k in keys:
        want = np.stack([refs[int(s)][k][b] for b, s in enumerate(ids)])
        assert np.array_equal(_bits(got[k]), _bits(want)), (what, k, np.flatnonzero((_bits(got[k]) != _bits(want)).reshape(len(ids), -1).any(1)))


# ---- 1, 2. template level ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _template(cid, s, dbg=0):
    """The template of a case created with scene s's spheres (s None: with the case's own)."""
    from graphik_amd.engine import Template
    sc = ss.build(cid)
    p = sc.p if s is None else ss.with_scene(sc.p, sc.scenes[s])
    return Template(p.N, 3, p.ti, p.tj, p.tk, None, params={"debug_flags": dbg} if dbg else None, anchored=sa.anchored_desc(p))


@functools.lru_cache(maxsize=None)
def _scene_set(cid):
    """The case's scenes with the module's own stride and NaN padding rows, on the device."""
    import torch
    from graphik_amd.engine import SceneSet
    sc = ss.build(cid)
    S = SceneSet(sc.scenes, torch.device(f"cuda:{torch.cuda.current_device()}"), stride=sc.stride)
    assert np.array_equal(S.obs_host, sc.obs, equal_nan=True) and S.counts.tolist() == sc.counts.tolist()
    return S


def _solve_host(r):
    out = {k: _np(r[k]) for k in ("x",) + STATS}
    out.update({"trace_" + k: _np(v) for k, v in r["trace"].items()})
    return out


@functools.lru_cache(maxsize=None)
def _references(cid, dbg=0):
    """Per scene: the WHOLE batch of 8 solved on the template created with that scene (gik_solve_batch), on the host."""
    sc = ss.build(cid)
    return [_solve_host(_template(cid, s, dbg).solve(sc.Y0, sc.p.goal.copy(), trace_cap=32)) for s in range(ss.N_SCENE)]


@pytest.mark.parametrize("dbg", [0, 128])
@pytest.mark.parametrize("cid", sorted(ss.CASES))
def test_template_level_bit_identity(torch_cuda, cid, dbg):
    """B = 8, scene_id = [0,1,2,0,1,2,0,1]: x, the statistics and the whole trace equal the per-scene templates', with near
    lists (dbg 0) and with every walk visiting every sphere (debug_flags 128); the first cost is the numpy reference's of
    that scene to 1e-12.  The call runs on the template created with the case's OWN spheres, which must play no part."""
    sc = ss.build(cid)
    refs = _references(cid, dbg)
    T = _template(cid, None, dbg)
    assert T.info["max_terms_per_node"] == sa.CASES[cid]["slots"]
    got = _solve_host(T.solve(sc.Y0, sc.p.goal.copy(), trace_cap=32, scenes=_scene_set(cid), scene_id=ss.SCENE_ID))
    keys = sorted(got)
    for k in keys:
        want = np.stack([refs[int(s)][k][b] for b, s in enumerate(ss.SCENE_ID)])
        assert np.array_equal(_bits(got[k]), _bits(want)), (cid, dbg, k)      # (trace rows beyond the last iteration: the fill)
    Z = np.zeros((sc.p.N, 3))
    for b, s in enumerate(ss.SCENE_ID):
        ref = anchored_numpy_terms(sa.free_terms(sc.p), ss.anchor_terms(cid, int(s), b), sc.Y0[b], Z)[0]
        f0 = got["trace_f_before"][b, 0]
        print(f"{cid} goal {b} scene {s}: f_before[0] {f0:.12e} numpy {ref:.12e} rel {abs(f0 - ref) / abs(ref):.1e}")
        assert abs(f0 - ref) <= 1e-12 * abs(ref), (cid, b, s, f0, ref)
    assert np.all(got["stop"] == 0) and np.all(got["f"] < 1e-9) and int(got["iterations"].min()) >= 1
    # near lists on and off give the same bits under scenes too
    if dbg == 128:
        other = _references(cid, 0)
        for k in ("x",) + STATS:
            for s in range(ss.N_SCENE):
                assert np.array_equal(_bits(refs[s][k]), _bits(other[s][k])), (cid, k, s)


def test_which_scene_builds_ran(torch_cuda):
    slots = {cid: _template(cid, None).info["max_terms_per_node"] for cid in ss.CASES}
    assert set(slots.values()) == {9, 20} and slots["a20_full"] == 20 and slots["near9"] == 9


@pytest.mark.parametrize("cid", ["near9", "a20_full"])
def test_a_wave_changes_scene_between_problems(torch_cuda, cid):
    """The 8 goals tiled to B = 4096 with scene_id = b % 3: every copy is the per-scene template's answer for its
    (goal, scene), bit for bit.  4096 problems on at most 1024 resident waves: every wave restages."""
    sc = ss.build(cid)
    refs = _references(cid)
    Bt = 4096
    goal_of = np.arange(Bt) % ss.B
    ids = (np.arange(Bt) % 3).astype(np.int32)
    T = _template(cid, None)
    assert T.info["n_cu"] * T.info["waves_per_cu"] < Bt
    r = T.solve(sc.Y0[goal_of], sc.p.goal[goal_of].copy(), scenes=_scene_set(cid), scene_id=ids)
    for k in ("x",) + STATS:
        got = _np(r[k])
        want = np.stack([refs[int(s)][k][g] for g, s in zip(goal_of, ids)])
        assert np.array_equal(_bits(got), _bits(want)), (cid, k)
    assert len({(int(g), int(s)) for g, s in zip(goal_of, ids)}) == 3 * ss.B      # every (goal, scene) pair occurs


# ---- 3 - 5. UR10 -----------------------------------------------------------------------------------------------------
def _table():
    from graphik_amd.utils import table_environment
    return np.array([[*np.asarray(o[0], dtype=float), float(o[1])] for o in table_environment()]).reshape(-1, 4)


def _spheres(shift):
    """The table's spheres moved by `shift` metres in x; None: no sphere."""
    return np.zeros((0, 4)) if shift is None else _table() + np.array([shift, 0.0, 0.0, 0.0])


@functools.lru_cache(maxsize=None)
def _problem(shift, hinges=False, maxiter=None):
    """UR10 among _spheres(shift), as an AnchoredProblem of its own: the reference of one scene."""
    robot, graph = make_graph("ur10")
    for k, o in enumerate(_spheres(shift)):
        graph.add_spherical_obstacle(f"o{k}", o[:3].copy(), float(o[3]))
    ap = _rs().AnchoredProblem(graph, link_hinges=hinges, params=None if maxiter is None else {"maxiter": maxiter})
    assert np.array_equal(ap.obstacles, _spheres(shift))
    return robot, ap


SHIFTS3 = (0.0, 0.2, None)          # table_environment(), the same table 0.2 m further in x, empty


@functools.lru_cache(maxsize=None)
def _goals64():
    """64 goals whose configurations have a joint point more than 2 cm inside the table's spheres, the seeds 0.05 rad
    (sigma) off them, and scene ids that mix the three scenes."""
    colliding, _ = collision_input()
    rng = np.random.RandomState(41)
    seeds = colliding + 0.05 * rng.randn(*colliding.shape)
    return colliding, seeds, rng.randint(0, 3, size=64).astype(np.int32)


@pytest.mark.parametrize("hinges", [False, True])
@pytest.mark.parametrize("mode", ["nodes", "links"])
@pytest.mark.parametrize("seeded", [False, True])
def test_ur10_three_scenes(torch_cuda, seeded, mode, hinges):
    """AnchoredProblem.solve with scenes, cold and with q_init, node and link clearance, without and with link hinges (the
    link scene build): x, q, errors, statistics and clearance equal three per-scene AnchoredProblems', bit for bit."""
    torch = torch_cuda
    colliding, seeds, ids = _goals64()
    robot, ap = _problem(0.0, hinges)
    T = robot.fk_batch(colliding)
    q_init = seeds if seeded else None
    refs = []
    for shift in SHIFTS3:
        _, ap_s = _problem(shift, hinges)
        refs.append(_host(ap_s.solve(T, q_init=q_init, clearance=True, clearance_mode=mode), KEYS + ("clearance",)))
    # non-vacuity, on the references alone: the table changes the answer of at least a quarter of the goals
    moved = np.abs(refs[0]["x"] - refs[2]["x"]).reshape(64, -1).max(1) > 1e-3
    print(f"seeded {seeded} mode {mode} hinges {hinges}: table and empty answers differ for {int(moved.sum())} of 64 goals")
    assert moved.sum() >= 16
    S = ap.scene_set([_spheres(s) for s in SHIFTS3])
    assert ap.template.info["anchored"] == (3 if hinges else 1)
    for scene_id in (ids, torch.from_numpy(ids).cuda(), torch.from_numpy(ids.astype(np.int64)).cuda()):
        got = _host(ap.solve(T, q_init=q_init, clearance=True, clearance_mode=mode, scenes=S, scene_id=scene_id), KEYS + ("clearance",))
        _assert_rows(got, refs, ids, KEYS + ("clearance",), (seeded, mode, hinges))
    assert np.all(np.isposinf(got["clearance"][ids == 2])) and np.all(np.isfinite(got["clearance"][ids != 2]))
    # the clearance entries on their own, and the numpy mirrors per scene
    x = got["x"]
    fn = ap.template.anchored_link_clearance if mode == "links" else ap.template.anchored_clearance
    assert np.array_equal(_bits(_np(fn(x, scenes=S, scene_id=ids))), _bits(got["clearance"]))
    mirror = ap.link_clearance if mode == "links" else ap.clearance
    for s in (0, 1):
        sel = ids == s
        assert np.abs(mirror(x[sel], obstacles=S.scenes[s]) - got["clearance"][sel]).max() < 1e-12
    # one scene, no ids: every goal in scene 0
    one = _host(ap.solve(T, q_init=q_init, clearance=True, clearance_mode=mode, scenes=ap.scene_set([_spheres(0.2)])), KEYS + ("clearance",))
    _assert_rows(one, refs, np.ones(64, dtype=int), KEYS + ("clearance",), "one scene")
    # device ids outside [0, S) are a ValueError (one reduction), nothing is queued
    bad = torch.from_numpy(ids).cuda().clone()
    bad[5] = 3
    with pytest.raises(ValueError, match=r"outside \[0, 3\)"):
        ap.solve(T, scenes=S, scene_id=bad)


@pytest.mark.parametrize("mode", ["nodes", "links"])
def test_restarts_with_scenes(torch_cuda, mode):
    """retries = 2 at maxiter = 5 from the colliding seeds (where attempt 0 fails): every output, `attempt` included, equals
    the per-scene problems' row for row -- the scene went through attempt 0, every compact batch and every clearance."""
    colliding, goals = collision_input()
    _, _, ids = _goals64()
    robot, ap = _problem(0.0, False, 5)
    T = robot.fk_batch(goals)
    keys = KEYS + ("clearance", "attempt")
    kw = dict(q_init=colliding, retries=2, retry_seed=77, clearance_mode=mode, **TOL)
    refs = [_host(_problem(shift, False, 5)[1].solve(T, **kw), keys) for shift in SHIFTS3]
    hist = [np.bincount(r["attempt"], minlength=3).tolist() for r in refs]
    print("attempt histograms per scene:", hist)
    assert sum(h[1] + h[2] for h in hist) > 0, "no restart replaced an answer in any scene: the test would check nothing"
    S = ap.scene_set([_spheres(s) for s in SHIFTS3])
    got = _host(ap.solve(T, scenes=S, scene_id=ids, **kw), keys)
    _assert_rows(got, refs, ids, keys, mode)
    # cold attempt 0, one restart
    kw = dict(retries=1, retry_seed=3, clearance_mode=mode, **TOL)
    refs = [_host(_problem(shift, False, 5)[1].solve(T, **kw), keys) for shift in SHIFTS3]
    _assert_rows(_host(ap.solve(T, scenes=S, scene_id=ids, **kw), keys), refs, ids, keys, "cold " + mode)


def test_tracking_with_a_scene_per_waypoint(torch_cuda):
    """16 paths x 4 waypoints, the table 5 cm further in x at every waypoint (and the paths out of step with each other):
    solve_trajectory with scene_id [B, L] equals a manual chain of per-scene seeded solves that takes, at every waypoint,
    each path's row from the problem of its scene."""
    torch = torch_cuda
    Bp, L = 16, 4
    shifts = (0.0, 0.05, 0.10, 0.15)
    robot, ap = _problem(0.0)
    colliding, _ = collision_input()
    rng = np.random.RandomState(8)
    q0 = colliding[:Bp]
    dq = 0.04 * rng.randn(Bp, 1, robot.n)
    Q = q0[:, None] + np.arange(1, L + 1)[None, :, None] * dq
    T = robot.fk_batch(Q.reshape(Bp * L, robot.n)).reshape(Bp, L, 4, 4)
    ids = ((np.arange(L)[None] + np.arange(Bp)[:, None]) % 4).astype(np.int32)      # [B, L]
    S = ap.scene_set([_spheres(s) for s in shifts])
    q, Y, info = ap.solve_trajectory(T, q0, return_Y=True, scenes=S, scene_id=ids)
    keys = KEYS + ("clearance",)
    q_prev = torch.from_numpy(q0).cuda()
    for l in range(L):
        refs = [_host(_problem(s)[1].solve(T[:, l], q_init=q_prev, clearance=True), keys) for s in shifts]
        row = {k: np.stack([refs[int(s)][k][b] for b, s in enumerate(ids[:, l])]) for k in keys}
        assert np.array_equal(_bits(q[:, l]), _bits(row["q"])), l
        assert np.array_equal(_bits(Y[:, l]), _bits(row["x"])), l
        for k_info, k in (("f(x)", "f"), ("gradnorm", "gradnorm"), ("iterations", "iterations"), ("stop", "stop"),
                          ("inner_iterations", "inner_total"), ("pos_err", "pos_err"), ("rot_err", "rot_err"), ("clearance", "clearance")):
            assert np.array_equal(_bits(info[k_info][:, l]), _bits(row[k])), (l, k)
        q_prev = torch.from_numpy(row["q"]).cuda()
    # a scene per path ([B]) is the same scene at every waypoint
    q1, _, info1 = ap.solve_trajectory(T, q0, scenes=S, scene_id=ids[:, 0])
    q2, _, info2 = ap.solve_trajectory(T, q0, scenes=S, scene_id=np.repeat(ids[:, :1], L, axis=1))
    assert np.array_equal(_bits(q1), _bits(q2)) and np.array_equal(_bits(info1["clearance"]), _bits(info2["clearance"]))
    with pytest.raises(ValueError, match="sweep= with scenes="):
        ap.solve_trajectory(T, q0, scenes=S, scene_id=ids, sweep=4)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------
def test_refusals(torch_cuda):
    torch = torch_cuda
    from graphik_amd import _ffi
    lib = _ffi.lib()
    robot, ap = _problem(0.0)
    tpl, base = ap.template, ap.base.template
    B = 8
    colliding, seeds, _ = _goals64()
    Tg = torch.from_numpy(robot.fk_batch(colliding[:B])).cuda().reshape(B, 16).contiguous()
    q0 = torch.from_numpy(seeds[:B]).cuda().contiguous()
    S = ap.scene_set([_spheres(0.0), _spheres(0.2)])
    ids = torch.zeros(B, dtype=torch.int32, device="cuda")
    out = tpl.alloc_anchored_buffers(base, B, clearance=True)
    for k in ("Y", "q", "pos_err", "rot_err", "clearance"):
        out[k].fill_(-7.0)
    answer = [out[k].data_ptr() for k in ("Y", "stats", "q", "pos_err", "rot_err")]
    s = torch.cuda.Stream()
    stream = C.c_void_p(s.cuda_stream)

    def scene(n_scene=2, stride=None, obs=True, n_obs=True, with_ids=True):
        return _ffi.SceneSet(n_scene=n_scene, stride=S.stride if stride is None else stride, d_obs=S.obs.data_ptr() if obs else None,
                             d_n_obs=S.n_obs.data_ptr() if n_obs else None, d_scene_id=ids.data_ptr() if with_ids else None)

    Yf, goal = tpl.anchored_seed(base, Tg, q0)
    Yf = Yf.reshape(B, -1).contiguous()
    Yo = torch.full_like(Yf, -7.0)
    stats = torch.zeros(B, _ffi.STATS_BYTES // 8, dtype=torch.float64, device="cuda")
    rws = torch.empty(tpl.anchored_retry_ws_bytes(base, B, scenes=True) // 8 + B + 2, dtype=torch.float64, device="cuda")
    attempt = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    lo, hi = (torch.from_numpy(a).cuda() for a in robot.limits_arrays())
    opts = _ffi.AnchoredRetryOpts(retries=1, clearance_mode=0, seed=1, pos_tol=0.01, rot_tol=0.01, d_q_lo=lo.data_ptr(),
                                  d_q_hi=hi.data_ptr(), clear_tol=1e-4, spread=0.0)

    def calls(sc, a=tpl):
        """every scene entry with the scene set sc on the handle a"""
        return [
            lambda: lib.gik_solve_batch_scenes(a._h, Yf.data_ptr(), goal.data_ptr(), B, Yo.data_ptr(), stats.data_ptr(), None,
                                               C.byref(sc), stream),
            lambda: lib.gik_anchored_ik_batch_scenes(a._h, base._h, Tg.data_ptr(), q0.data_ptr(), B, C.byref(sc),
                                                     out["ws"].data_ptr(), *answer, out["clearance"].data_ptr(), 0, stream),
            lambda: lib.gik_anchored_ik_batch_scenes(a._h, base._h, Tg.data_ptr(), None, B, C.byref(sc),
                                                     out["ws"].data_ptr(), *answer, out["clearance"].data_ptr(), 1, stream),
            lambda: lib.gik_anchored_clearance_scenes(a._h, out["Y"].data_ptr(), B, C.byref(sc), out["clearance"].data_ptr(), stream),
            lambda: lib.gik_anchored_link_clearance_scenes(a._h, out["Y"].data_ptr(), B, C.byref(sc), out["clearance"].data_ptr(),
                                                           stream),
            lambda: lib.gik_anchored_ik_batch_retry_scenes(a._h, base._h, Tg.data_ptr(), q0.data_ptr(), B, C.byref(opts), C.byref(sc),
                                                           rws.data_ptr(), *answer, out["clearance"].data_ptr(), attempt.data_ptr(),
                                                           stream)]

    def refused(fns, word):
        for fn in fns:
            assert fn() != 0
            msg = lib.gik_last_error().decode()
            assert word in msg, (word, msg)

    refused(calls(scene(n_scene=0)), "n_scene")
    refused(calls(scene(stride=129)), "stride")
    refused(calls(scene(with_ids=False)), "d_scene_id")
    refused(calls(scene(n_obs=False)), "d_n_obs")
    refused(calls(scene(obs=False)), "d_obs")
    refused(calls(scene(), base), "fixed-anchor")                     # a template that is not anchored
    assert lib.gik_solve_batch_scenes(tpl._h, Yf.data_ptr(), goal.data_ptr(), B, Yo.data_ptr(), stats.data_ptr(), None, None, stream) != 0
    assert "null scene set" in lib.gik_last_error().decode()
    assert lib.gik_anchored_ik_batch_scenes(tpl._h, base._h, Tg.data_ptr(), None, B, C.byref(scene()), out["ws"].data_ptr(), *answer,
                                            None, 2, stream) != 0
    assert "clearance_mode" in lib.gik_last_error().decode()
    # a capturing stream: every entry refuses, and the capture stays empty
    hip = _hip_runtime()
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    assert hip.hipStreamBeginCapture(stream, 2) == 0      # hipStreamCaptureModeRelaxed
    rcs, msgs = [], []
    for fn in calls(scene()):
        rcs.append(fn())
        msgs.append(lib.gik_last_error().decode())
    graph_h = C.c_void_p()
    assert hip.hipStreamEndCapture(stream, C.byref(graph_h)) == 0
    n_nodes = C.c_size_t(99)
    assert hip.hipGraphGetNodes(graph_h, None, C.byref(n_nodes)) == 0
    hip.hipGraphDestroy(graph_h)
    assert all(rc != 0 for rc in rcs) and all("capturing" in m for m in msgs), (rcs, msgs)
    assert n_nodes.value == 0
    # nothing was queued by any refusal: the outputs still hold their fill
    torch.cuda.synchronize()
    assert all(bool((out[k] == -7.0).all()) for k in ("Y", "q", "pos_err", "rot_err", "clearance"))
    assert bool((Yo == -7.0).all()) and bool((attempt == -7).all())
    # the same calls on the same stream, not capturing, run; B = 0 returns 0
    for fn in calls(scene()):
        assert fn() == 0, lib.gik_last_error().decode()
    s.synchronize()
    assert lib.gik_solve_batch_scenes(tpl._h, None, None, 0, None, None, None, C.byref(scene()), stream) == 0
    # the Python layer: sweep with scenes, scene ids without scenes, a scene set on a template that is not anchored
    T4 = robot.fk_batch(colliding[:B])
    with pytest.raises(ValueError, match="sweep= with scenes="):
        ap.solve_trajectory(T4[:, None], seeds[:B], scenes=S, scene_id=np.zeros(B, dtype=int), sweep=2)
    with pytest.raises(ValueError, match="scene_id needs scenes"):
        ap.solve(T4, scene_id=np.zeros(B, dtype=int))
    with pytest.raises(ValueError, match="scene_id is required"):
        ap.solve(T4, scenes=S)
    with pytest.raises(ValueError, match="not anchored"):
        base.solve(np.zeros((B, base.N, 3)), np.zeros((B, base.T)), scenes=S, scene_id=np.zeros(B, dtype=int))
