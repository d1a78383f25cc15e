"""Screened restart seeds of the fixed-anchor solve on the MI355X: the stand-alone step (gik_anchored_retry_seeds_screened)
against the numpy mirror -- the picked angles bit for bit, the pick, its clearance to 1e-11 --, the restart loop
(gik_anchored_ik_batch_retry_screened) end to end through AnchoredProblem.solve / solve_trajectory, and the refusals of
both entries.  UR10 with 3 cm capsules, every self pair and a floor at z = -0.1; the draws are those of
tests/test_anchored_screen_host.py: seed 7, goals 0 .. 511, attempt 1, limits +-pi.

The device and the host realize a configuration to 1e-11 of each other, not to the bit.  A pick can therefore differ only
where a candidate's clearance lies that close to -clear_tol, or where the two best clearances of a goal without a clear
candidate lie that close to each other: every comparison first asserts, on the mirror's values and for every goal it
compares, a margin of 1e-9 on both counts (pick_margins).  No goal is filtered out."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import make_graph
from test_anchored_screen_host import ATTEMPT, CLEAR_TOL, FLOOR, GOALS, RHO, SEED, pi_limits, pick_margins
from test_anchored_seeded_host import collision_input, tracking_input

pytestmark = pytest.mark.gpu

MODES = ("nodes", "links", "links+self")
KEYS = ("x", "q", "stop", "iterations", "pos_err", "rot_err", "clearance")
TOL = dict(pos_tol=0.01, rot_tol=0.01, clear_tol=CLEAR_TOL)
MARGIN = 1e-9
BAR = 1e-11          # device realization against BatchProblem.seed_points: the bar of the sphere sweep's test


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _rs():
    from graphik_amd.solvers import riemannian_solver as rs
    return rs


def _lib():
    from graphik_amd import _ffi
    return _ffi.lib(), _ffi


def _stream(torch):
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64) if x.dtype == np.float64 else x


@functools.lru_cache(maxsize=None)
def _room(maxiter=None):
    """UR10 + table_environment(), 3 cm capsules, every self pair, the floor: one problem per iteration budget."""
    robot, graph = make_graph("ur10_table")
    ap = _rs().AnchoredProblem(graph, params=None if maxiter is None else {"maxiter": maxiter}, link_radius=RHO,
                               self_pairs="auto", halfspaces=[list(FLOOR)])
    return robot, ap


@functools.lru_cache(maxsize=None)
def _ceiling():
    """The allowed side is z >= 10: no configuration of a robot that reaches 1.4 m is clear."""
    robot, graph = make_graph("ur10")
    return robot, _rs().AnchoredProblem(graph, link_radius=RHO, halfspaces=[[0.0, 0.0, 1.0, 10.0]])


@functools.lru_cache(maxsize=None)
def _bare(maxiter=5):
    """No sphere, no half-space, no links: nothing to measure."""
    robot, graph = make_graph("ur10")
    return robot, _rs().AnchoredProblem(graph, params={"maxiter": maxiter}, links=[])


def _two_scenes(ap):
    """The table's spheres split into two scenes, and the scene of goal g: the ids alternate."""
    return [ap.obstacles[:50].copy(), ap.obstacles[50:].copy()], (np.arange(GOALS) % 2).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _centres():
    lo, hi = pi_limits()
    return np.random.RandomState(41).uniform(0.8 * lo, 0.8 * hi, size=(GOALS, 6))


@functools.lru_cache(maxsize=None)
def _mirror(mode, scenes, spread):
    """The mirror's candidate table of all 512 goals, 16 candidates: (q_c [16, 512, n], clearance_c [16, 512]), computed
    once and shared.  scenes: goal g against scene g % 2 of _two_scenes, each scene's column taken from a call against
    that scene alone (tests/test_anchored_screen_host.py holds the per-goal form to that)."""
    robot, ap = _room()
    lo, hi = pi_limits()
    kw = dict(clearance_mode=mode, clear_tol=CLEAR_TOL)
    if spread:
        kw.update(center=_centres(), spread=spread)
    goals = np.arange(GOALS)
    if not scenes:
        ap.screened_seeds_host(SEED, goals, ATTEMPT, 16, lo, hi, **kw)
        q_c, cl_c = ap.last_screen
    else:
        sets, ids = _two_scenes(ap)
        tables = []
        for s in sets:
            ap.screened_seeds_host(SEED, goals, ATTEMPT, 16, lo, hi, obstacles=s, **kw)
            tables.append(ap.last_screen)
        q_c = tables[0][0]
        cl_c = np.where(ids[None, :] == 0, tables[0][1], tables[1][1])
    q_c.setflags(write=False)
    cl_c.setflags(write=False)
    return q_c, cl_c


def _expect(q_c, cl_c, idx, candidates):
    """What the device must write for the compact list idx with the first `candidates` rows of a mirror table, after the
    margins have been asserted on exactly those values."""
    cl = cl_c[:candidates][:, idx]
    near, gap = pick_margins(cl, CLEAR_TOL)
    assert near >= MARGIN and gap >= MARGIN, (near, gap)
    pick = _rs().retry_pick_host(cl, CLEAR_TOL)
    cols = np.arange(len(idx))
    return q_c[:candidates][:, idx][pick, cols], pick, cl[pick, cols]


def _subset(count):
    """A shuffled subset of the 512 goals: slot r is not goal r."""
    idx = np.random.RandomState(600 + count).permutation(GOALS)[:count].astype(np.int32)
    assert count == 1 or not np.array_equal(idx, np.arange(count))
    return idx


# ---- 1. the stand-alone step against the mirror ----------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 5, 65, 130])
def test_screened_step_matches_the_mirror(torch_cuda, count):
    """One slot, a partial wavefront, one more than a wavefront, two and a bit; 1, 2, 8 and 16 candidates; the three
    clearance modes with the floor, against the problem's own spheres and against two alternating scenes; uniform and
    local seeds."""
    torch = torch_cuda
    robot, ap = _room()
    tpl, base = ap.template, ap.base.template
    lo, hi = pi_limits()
    T = np.random.RandomState(7).standard_normal((GOALS, 4, 4))      # (the step copies pose rows: any bits will do)
    idx = _subset(count)
    sets, ids = _two_scenes(ap)
    ss = ap.scene_set(sets)
    picked_later = 0
    for mode in MODES:
        for scenes in (False, True):
            for spread in (0.0, 0.3):
                q_c, cl_c = _mirror(mode, scenes, spread)
                for cand in (1, 2, 8, 16):
                    q, pick, cl = _expect(q_c, cl_c, idx, cand)
                    res = tpl.anchored_retry_seeds_screened(
                        base, T, idx, SEED, ATTEMPT, cand, (lo, hi), center=_centres() if spread else None, spread=spread,
                        clearance_mode=mode, clear_tol=CLEAR_TOL, scenes=ss if scenes else None, scene_id=ids if scenes else None)
                    torch.cuda.synchronize()
                    case = (mode, scenes, spread, cand)
                    assert np.array_equal(res["pick"].cpu().numpy(), pick), case
                    assert np.array_equal(_bits(res["q"].cpu().numpy()), _bits(q)), case
                    assert np.array_equal(_bits(res["T"].cpu().numpy()), _bits(T[idx])), case
                    got = res["clearance"].cpu().numpy()
                    assert np.all(np.isfinite(got)) and np.abs(got - cl).max() < BAR, (case, np.abs(got - cl).max())
                    picked_later += int((pick > 0).sum())
    assert count < 5 or picked_later > 0      # (the screening chose something other than the blind seed)


def test_guard_rows_around_the_outputs(torch_cuda):
    """The raw entry on buffers with a guard row on either side: nothing outside [count] rows is written, and the
    optional outputs may be null."""
    torch = torch_cuda
    lib, _ffi = _lib()
    robot, ap = _room()
    tpl, base = ap.template, ap.base.template
    lo, hi = pi_limits()
    count, cand, n = 65, 8, 6
    idx = _subset(count)
    q_want, pick_want, cl_want = _expect(*_mirror("links+self", False, 0.0), idx, cand)
    d_T = torch.from_numpy(np.random.RandomState(7).standard_normal((GOALS, 16))).cuda()
    d_idx, d_lo, d_hi = (torch.from_numpy(a).cuda() for a in (idx, lo, hi))
    nbytes = int(lib.gik_anchored_retry_seeds_screened_ws_bytes(tpl._h, base._h, count, cand))
    assert nbytes > 0 and nbytes % 8 == 0
    ws = torch.full((nbytes // 8 + 2,), -7.0, dtype=torch.float64, device="cuda")
    for with_outputs in (True, False):
        T_out = torch.full((count + 2, 16), -7.0, dtype=torch.float64, device="cuda")
        q_out = torch.full((count + 2, n), -7.0, dtype=torch.float64, device="cuda")
        pick = torch.full((count + 2,), -7, dtype=torch.int32, device="cuda")
        cl = torch.full((count + 2,), -7.0, dtype=torch.float64, device="cuda")
        ws.fill_(-7.0)
        _ffi.check(lib.gik_anchored_retry_seeds_screened(
            tpl._h, base._h, d_T.data_ptr(), d_idx.data_ptr(), count, SEED, ATTEMPT, d_lo.data_ptr(), d_hi.data_ptr(), None, 0.0,
            cand, _ffi.CLEARANCE_LINKS_SELF, CLEAR_TOL, None, ws.data_ptr() + 8, T_out.data_ptr() + 8 * 16, q_out.data_ptr() + 8 * n,
            pick.data_ptr() + 4 if with_outputs else None, cl.data_ptr() + 8 if with_outputs else None, _stream(torch)))
        torch.cuda.synchronize()
        T_out, q_out, pick, cl, w = (t.cpu().numpy() for t in (T_out, q_out, pick, cl, ws))
        for buf in (T_out, q_out, pick, cl, w):
            assert np.all(buf[0] == -7) and np.all(buf[-1] == -7)
        assert np.array_equal(_bits(q_out[1:-1]), _bits(q_want))
        assert np.array_equal(_bits(T_out[1:-1]), _bits(d_T.cpu().numpy()[idx]))
        if with_outputs:
            assert np.array_equal(pick[1:-1], pick_want) and np.abs(cl[1:-1] - cl_want).max() < BAR
        else:
            assert np.all(pick == -7) and np.all(cl == -7.0)


def test_all_blocked_picks_the_largest_clearance(torch_cuda):
    """Under a ceiling at z >= 10 no candidate is clear and the pick is the largest clearance.  Where the whole arm is
    above its base the lowest link end is the base row itself, a constant no configuration moves -- the same bits on the
    device and in the mirror --, so such candidates tie exactly and the lowest c wins on both sides; every other pair of
    best clearances keeps the margin."""
    torch = torch_cuda
    robot, ap = _ceiling()
    lo, hi = pi_limits()
    idx = _subset(65)
    ap.screened_seeds_host(SEED, np.arange(GOALS), ATTEMPT, 8, lo, hi, clearance_mode="links")
    q_c, cl_c = ap.last_screen
    cl = cl_c[:, idx]
    assert np.all(cl_c < -8.0)                       # no candidate is clear, none is near the bar
    top = np.sort(cl, axis=0)
    gap = top[-1] - top[-2]
    base_row = -10.0 - RHO                           # the base, at z = 0, with its capsule radius
    assert np.all((gap >= MARGIN) | ((gap == 0.0) & (top[-1] == base_row))), gap.min()
    assert (gap >= MARGIN).any() and (gap == 0.0).any()
    pick = _rs().retry_pick_host(cl, CLEAR_TOL)
    assert np.array_equal(pick, cl.argmax(axis=0)) and len(set(pick.tolist())) > 4
    res = ap.template.anchored_retry_seeds_screened(ap.base.template, np.zeros((GOALS, 4, 4)), idx, SEED, ATTEMPT, 8, (lo, hi),
                                                    clearance_mode="links")
    torch.cuda.synchronize()
    cols = np.arange(len(idx))
    assert np.array_equal(res["pick"].cpu().numpy(), pick)
    assert np.array_equal(_bits(res["q"].cpu().numpy()), _bits(q_c[:, idx][pick, cols]))
    assert np.abs(res["clearance"].cpu().numpy() - cl[pick, cols]).max() < BAR


def test_nan_centre_gives_a_nan_seed_for_that_goal_alone(torch_cuda):
    torch = torch_cuda
    robot, ap = _room()
    lo, hi = pi_limits()
    idx = _subset(65)
    g = int(idx[17])
    centre = _centres().copy()
    centre[g] = np.nan
    q_c, cl_c = _mirror("links+self", False, 0.3)
    res = ap.template.anchored_retry_seeds_screened(ap.base.template, np.zeros((GOALS, 4, 4)), idx, SEED, ATTEMPT, 4, (lo, hi),
                                                    center=centre, spread=0.3, clearance_mode="links+self")
    torch.cuda.synchronize()
    got_q, got_pick, got_cl = (res[k].cpu().numpy() for k in ("q", "pick", "clearance"))
    assert np.isnan(got_q[17]).all() and got_pick[17] == 0 and np.isnan(got_cl[17])
    others = np.arange(65) != 17
    want_q, want_pick, want_cl = _expect(q_c, cl_c, idx[others], 4)
    assert np.array_equal(_bits(got_q[others]), _bits(want_q)) and np.array_equal(got_pick[others], want_pick)
    assert np.abs(got_cl[others] - want_cl).max() < BAR


@pytest.mark.parametrize("spread", [0.0, 0.3])
def test_one_candidate_writes_the_unscreened_bits(torch_cuda, spread):
    torch = torch_cuda
    lib, _ffi = _lib()
    robot, ap = _room()
    tpl, base = ap.template, ap.base.template
    lo, hi = pi_limits()
    count = 130
    idx = _subset(count)
    T = np.random.RandomState(8).standard_normal((GOALS, 4, 4))
    centre = _centres() if spread else None
    res = tpl.anchored_retry_seeds_screened(base, T, idx, SEED, 5, 1, (lo, hi), center=centre, spread=spread, clearance_mode="links")
    d_T, d_idx, d_lo, d_hi = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (T.reshape(GOALS, 16), idx, lo, hi))
    d_c = None if centre is None else torch.from_numpy(centre).cuda()
    T_ref = torch.empty(count, 16, dtype=torch.float64, device="cuda")
    q_ref = torch.empty(count, 6, dtype=torch.float64, device="cuda")
    _ffi.check(lib.gik_anchored_retry_seeds(base._h, d_T.data_ptr(), d_idx.data_ptr(), count, SEED, 5, d_lo.data_ptr(),
                                            d_hi.data_ptr(), None if d_c is None else d_c.data_ptr(), spread, T_ref.data_ptr(),
                                            q_ref.data_ptr(), _stream(torch)))
    torch.cuda.synchronize()
    assert torch.equal(res["q"], q_ref) and torch.equal(res["T"].reshape(count, 16), T_ref)
    assert not res["pick"].any()
    assert np.array_equal(_bits(q_ref.cpu().numpy()), _bits(_rs().retry_seeds_host(SEED, idx, 5, lo, hi, center=None if centre is None
                                                                                      else centre[idx], spread=spread)))


# ---- 2. end to end -----------------------------------------------------------------------------------------------------
def _host(res):
    out = {k: res[k].cpu().numpy() for k in KEYS}
    if "attempt" in res:
        out["attempt"] = res["attempt"].cpu().numpy()
    return out


def _same_rows(a, b, sel_a=slice(None), sel_b=slice(None)):
    return all(np.array_equal(_bits(a[k][sel_a]), _bits(b[k][sel_b])) for k in KEYS)


def _check_restarted_rows(ap, T, R, seed, candidates, mode, lo, hi, scene_kw=None, obstacles_of=None):
    """Every goal with attempt a > 0 holds, bit for bit, the one-goal seeded solve from the mirror's pick for
    (seed, g, a) -- after that pick's margins have been asserted.  Returns how many rows were compared."""
    att = R["attempt"]
    rows = np.flatnonzero(att > 0)
    for g in rows:
        obstacles = None if obstacles_of is None else obstacles_of(g)
        q0, pick, cl = ap.screened_seeds_host(seed, [g], int(att[g]), candidates, lo, hi, clearance_mode=mode,
                                              clear_tol=CLEAR_TOL, obstacles=obstacles)
        near, gap = pick_margins(ap.last_screen[1], CLEAR_TOL)
        assert near >= MARGIN and gap >= MARGIN, (g, near, gap)
        kw = {} if scene_kw is None else scene_kw(g)
        S = _host(ap.solve(T[g:g + 1], q_init=q0, clearance=True, clearance_mode=mode, **kw))
        assert _same_rows(R, S, slice(g, g + 1)), (g, att[g], int(pick[0]))
    return len(rows)


def test_end_to_end_restarts_start_from_the_mirrors_pick(torch_cuda):
    """64 goals from colliding seeds, the floor attached, five iterations, two restarts (the input of
    tests/test_anchored_retry_gpu.py's end-to-end test)."""
    robot, ap = _room(5)
    seeds, goals = collision_input()
    T = robot.fk_batch(goals)
    lo, hi = robot.limits_arrays()
    for mode in ("nodes", "links+self"):
        kw = dict(q_init=seeds, retries=2, retry_seed=77, clearance_mode=mode, **TOL)
        P = _host(ap.solve(T, **kw))
        R1 = _host(ap.solve(T, retry_candidates=1, **kw))
        assert _same_rows(R1, P) and np.array_equal(R1["attempt"], P["attempt"])      # 1: the call without the keyword
        R4 = _host(ap.solve(T, retry_candidates=4, **kw))
        first = R4["attempt"] == 0
        plain = _host(ap.solve(T, q_init=seeds, clearance=True, clearance_mode=mode))
        assert _same_rows(R4, plain, first, first)                                    # attempt 0 is the plain call's
        n = _check_restarted_rows(ap, T, R4, 77, 4, mode, lo, hi)
        print(mode, "attempts, 1 candidate:", np.bincount(P["attempt"], minlength=3).tolist(), "4 candidates:",
              np.bincount(R4["attempt"], minlength=3).tolist(), "rows compared:", n)
        assert n > 0, "no restart replaced any of 64 five-iteration answers: the test would check nothing"
        # the same call again: the same bits
        R4b = _host(ap.solve(T, retry_candidates=4, **kw))
        assert _same_rows(R4b, R4) and np.array_equal(R4b["attempt"], R4["attempt"])


def test_end_to_end_with_scenes(torch_cuda):
    robot, ap = _room(5)
    seeds, goals = collision_input()
    T = robot.fk_batch(goals)
    lo, hi = robot.limits_arrays()
    sets, ids = _two_scenes(ap)
    ids = ids[:len(T)]
    ss = ap.scene_set(sets)
    kw = dict(q_init=seeds, retries=2, retry_seed=77, clearance_mode="links", scenes=ss, scene_id=ids, **TOL)
    P = _host(ap.solve(T, **kw))
    R1 = _host(ap.solve(T, retry_candidates=1, **kw))
    assert _same_rows(R1, P) and np.array_equal(R1["attempt"], P["attempt"])
    R4 = _host(ap.solve(T, retry_candidates=4, **kw))
    n = _check_restarted_rows(ap, T, R4, 77, 4, "links", lo, hi, scene_kw=lambda g: dict(scenes=ss, scene_id=ids[g:g + 1]),
                              obstacles_of=lambda g: sets[ids[g]])
    print("scenes: attempts", np.bincount(R4["attempt"], minlength=3).tolist(), "rows compared:", n)
    assert n > 0


def test_nothing_to_measure_is_the_unscreened_call(torch_cuda):
    """No sphere, no half-space, no links: every clearance is +inf, every pick is candidate 0."""
    robot, ap = _bare()
    seeds, goals = collision_input()
    T = robot.fk_batch(goals)
    kw = dict(q_init=seeds, retries=2, retry_seed=77, **TOL)
    R1 = _host(ap.solve(T, retry_candidates=1, **kw))
    R8 = _host(ap.solve(T, retry_candidates=8, **kw))
    assert _same_rows(R8, R1) and np.array_equal(R8["attempt"], R1["attempt"])
    assert np.all(np.isposinf(R8["clearance"])) and (R8["attempt"] > 0).any()


def test_solve_trajectory_passes_the_candidates_on(torch_cuda):
    robot, ap = _room(5)
    Q, T = tracking_input()
    Bp, L = 8, 3
    T = T[:Bp, :L]
    lb, ub = robot.limits_arrays()
    q_start = np.random.RandomState(31).uniform(lb, ub, size=(Bp, robot.n))       # far from the paths
    kw = dict(retries=1, retry_seed=13, retry_spread=0.3, retry_candidates=4, clearance_mode="links+self", **TOL)
    q, Y, info = ap.solve_trajectory(T, q_start, return_Y=True, **kw)
    assert info["attempt"].shape == (Bp, L) and info["attempt"].max() <= 1
    prev = q_start
    for l in range(L):
        S = _host(ap.solve(T[:, l], q_init=prev, **kw))
        way = {"x": Y[:, l], "q": q[:, l], **{k: info[k][:, l] for k in ("stop", "iterations", "pos_err", "rot_err", "clearance")}}
        assert _same_rows(way, S), l
        assert np.array_equal(info["attempt"][:, l], S["attempt"]), l
        prev = q[:, l]
    print("trajectory attempts", info["attempt"].tolist())


# ---- 3. refusals of the two entries --------------------------------------------------------------------------------------
def _capture_refused(torch, s, call):
    """call() on the capturing stream s: refused, and the capture stays empty."""
    from test_retry_gpu import _hip_runtime
    hip = _hip_runtime()
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    assert hip.hipStreamBeginCapture(C.c_void_p(s.cuda_stream), 2) == 0      # hipStreamCaptureModeRelaxed
    rc, msg = call()
    graph_h = C.c_void_p()
    assert hip.hipStreamEndCapture(C.c_void_p(s.cuda_stream), C.byref(graph_h)) == 0
    n_nodes = C.c_size_t(99)
    assert hip.hipGraphGetNodes(graph_h, None, C.byref(n_nodes)) == 0
    hip.hipGraphDestroy(graph_h)
    assert rc != 0 and "capturing" in msg and n_nodes.value == 0


def test_step_refusals_leave_the_outputs_alone(torch_cuda):
    torch = torch_cuda
    lib, _ffi = _lib()
    robot, ap = _room()
    robot_c, ceiling = _ceiling()                       # a template without self pairs and without spheres
    tpl, base = ap.template, ap.base.template
    count, cand, n = 8, 4, 6
    d_T = torch.zeros(GOALS, 16, dtype=torch.float64, device="cuda")
    d_idx = torch.arange(count, dtype=torch.int32, device="cuda")
    lo, hi = (torch.from_numpy(a).cuda() for a in pi_limits())
    centre = torch.zeros(GOALS, n, dtype=torch.float64, device="cuda")
    ws = torch.empty(int(lib.gik_anchored_retry_seeds_screened_ws_bytes(tpl._h, base._h, count, 16)) // 8 + 1, dtype=torch.float64, device="cuda")
    out = {"T": torch.empty(count, 16, dtype=torch.float64, device="cuda"), "q": torch.empty(count, n, dtype=torch.float64, device="cuda"),
           "pick": torch.empty(count, dtype=torch.int32, device="cuda"), "cl": torch.empty(count, dtype=torch.float64, device="cuda")}
    for v in out.values():
        v.view(torch.int32).fill_(-7)
    before = {k: v.clone() for k, v in out.items()}
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    bad_scene = _ffi.SceneSet(n_scene=0, stride=0)
    DEFAULT = object()

    def call(anch=tpl._h, bs=base._h, cnt=count, attempt=1, q_lo=lo.data_ptr(), q_hi=hi.data_ptr(), ctr=None, spread=0.0,
             candidates=cand, mode=_ffi.CLEARANCE_NODES, clear_tol=CLEAR_TOL, scenes=None, d_ws=DEFAULT, q_out=DEFAULT):
        pick = lambda v, d: d if v is DEFAULT else v      # noqa: E731
        rc = lib.gik_anchored_retry_seeds_screened(anch, bs, d_T.data_ptr(), d_idx.data_ptr(), cnt, SEED, attempt, q_lo, q_hi, ctr,
                                                   spread, candidates, mode, clear_tol, scenes, pick(d_ws, ws.data_ptr()),
                                                   out["T"].data_ptr(), pick(q_out, out["q"].data_ptr()), out["pick"].data_ptr(),
                                                   out["cl"].data_ptr(), C.c_void_p(s.cuda_stream))
        return rc, lib.gik_last_error().decode()

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(out[k].view(torch.int32), before[k].view(torch.int32)) for k in out)

    for kw, word in ((dict(candidates=0), "candidates"), (dict(candidates=17), "candidates"), (dict(candidates=-1), "candidates"),
                     (dict(clear_tol=0.0), "clear_tol"), (dict(clear_tol=-1e-4), "clear_tol"), (dict(clear_tol=float("nan")), "clear_tol"),
                     (dict(d_ws=None), "workspace"), (dict(d_ws=ws.data_ptr() + 4), "aligned"),
                     (dict(attempt=64), "attempt"), (dict(attempt=-1), "attempt"), (dict(q_lo=None), "limits"), (dict(q_hi=None), "limits"),
                     (dict(spread=-0.1), "spread"), (dict(spread=float("nan")), "spread"), (dict(spread=0.1), "d_q_center"),
                     (dict(mode=3), "clearance_mode"), (dict(mode=-1), "clearance_mode"),
                     (dict(anch=ceiling.template._h, bs=ceiling.base.template._h, mode=_ffi.CLEARANCE_LINKS_SELF), "clearance_mode"),
                     (dict(scenes=C.byref(bad_scene)), "n_scene"), (dict(q_out=None), "null buffer"),
                     (dict(bs=tpl._h), "pipeline"), (dict(anch=base._h), "fixed-anchor"), (dict(cnt=-1), "bad argument")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg and "gik_anchored_retry_seeds_screened" in msg, (kw, msg)
        assert untouched(), kw
    assert lib.gik_anchored_retry_seeds_screened_ws_bytes(tpl._h, base._h, count, 0) == 0
    assert lib.gik_anchored_retry_seeds_screened_ws_bytes(tpl._h, base._h, count, 17) == 0
    assert lib.gik_anchored_retry_seeds_screened_ws_bytes(base._h, base._h, count, 4) == 0
    _capture_refused(torch, s, call)
    assert untouched()
    rc, msg = call(cnt=0)                                  # count = 0 returns 0 and queues nothing
    assert rc == 0 and untouched()
    rc, msg = call(ctr=centre.data_ptr(), spread=0.1)      # the same call, in order, runs
    assert rc == 0, msg
    s.synchronize()
    assert not untouched()


def test_loop_refusals_leave_the_outputs_alone(torch_cuda):
    torch = torch_cuda
    lib, _ffi = _lib()
    robot, ap = _room()
    tpl, base = ap.template, ap.base.template
    B, cand = 8, 4
    seeds, goals = collision_input()
    Tg = robot.fk_batch(goals[:B])
    T = torch.from_numpy(np.ascontiguousarray(Tg)).cuda()
    q0 = torch.from_numpy(seeds[:B].copy()).cuda()
    lo, hi = (torch.from_numpy(a).cuda() for a in robot.limits_arrays())
    out = tpl.alloc_anchored_buffers(base, B, clearance=True, ws=False)
    out["attempt"] = torch.empty(B, dtype=torch.int32, device="cuda")
    nbytes = int(lib.gik_anchored_ik_batch_retry_screened_ws_bytes(tpl._h, base._h, B, cand))
    plain = int(lib.gik_anchored_retry_ws_bytes(tpl._h, base._h, B))
    assert nbytes % 8 == 0 and nbytes > plain + 4 * B
    assert nbytes < int(lib.gik_anchored_ik_batch_retry_screened_ws_bytes(tpl._h, base._h, B, 16))
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    for v in out.values():
        v.view(torch.int32).fill_(-7)
    before = {k: v.clone() for k, v in out.items()}
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    bad_scene = _ffi.SceneSet(n_scene=0, stride=0)
    DEFAULT = object()

    def call(anch=tpl._h, bs=base._h, retries=1, q_lo=lo.data_ptr(), q_hi=hi.data_ptr(), clear_tol=CLEAR_TOL, spread=0.0, mode=0,
             candidates=cand, scenes=None, q_init=DEFAULT, clearance=DEFAULT, attempt=DEFAULT, d_ws=DEFAULT, n=B, pos_tol=0.01):
        opts = _ffi.AnchoredRetryOpts(retries=retries, clearance_mode=mode, seed=1, pos_tol=pos_tol, rot_tol=0.01, d_q_lo=q_lo,
                                      d_q_hi=q_hi, clear_tol=clear_tol, spread=spread)
        pick = lambda v, d: d if v is DEFAULT else v      # noqa: E731
        rc = lib.gik_anchored_ik_batch_retry_screened(anch, bs, T.data_ptr(), pick(q_init, q0.data_ptr()), n, C.byref(opts), candidates,
                                                      scenes, pick(d_ws, ws.data_ptr()), out["Y"].data_ptr(), out["stats"].data_ptr(),
                                                      out["q"].data_ptr(), out["pos_err"].data_ptr(), out["rot_err"].data_ptr(),
                                                      pick(clearance, out["clearance"].data_ptr()),
                                                      pick(attempt, out["attempt"].data_ptr()), C.c_void_p(s.cuda_stream))
        return rc, lib.gik_last_error().decode()

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(out[k].view(torch.int32), before[k].view(torch.int32)) for k in out)

    for kw, word in ((dict(candidates=0), "candidates"), (dict(candidates=17), "candidates"), (dict(candidates=-2), "candidates"),
                     (dict(clear_tol=0.0), "clear_tol"), (dict(clear_tol=float("nan")), "clear_tol"),
                     (dict(retries=0, clear_tol=0.0), "clear_tol"),
                     (dict(d_ws=None), "workspace"), (dict(d_ws=ws.data_ptr() + 4), "aligned"),
                     (dict(retries=64), "retries"), (dict(retries=-1), "retries"), (dict(q_lo=None), "limits"), (dict(q_hi=None), "limits"),
                     (dict(spread=-0.1), "spread"), (dict(spread=0.1, q_init=None), "d_q_init"), (dict(clearance=None), "d_clearance"),
                     (dict(attempt=None), "d_attempt"), (dict(pos_tol=0.0), "positive"), (dict(mode=3), "clearance_mode"),
                     (dict(scenes=C.byref(bad_scene)), "n_scene"),
                     (dict(bs=tpl._h), "pipeline"), (dict(anch=base._h), "fixed-anchor"), (dict(n=-1), "bad argument")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg and "gik_anchored_ik_batch_retry_screened" in msg, (kw, msg)
        assert untouched(), kw
    assert lib.gik_anchored_ik_batch_retry_screened_ws_bytes(tpl._h, base._h, B, 0) == 0
    assert lib.gik_anchored_ik_batch_retry_screened_ws_bytes(tpl._h, tpl._h, B, 4) == 0
    _capture_refused(torch, s, call)
    assert untouched()
    rc, msg = call(n=0)
    assert rc == 0 and untouched()
    # the same call on the same stream, not capturing, runs: the answer of the Python layer
    rc, msg = call(retries=2)
    assert rc == 0, msg
    s.synchronize()
    ref = ap.solve(Tg, q_init=seeds[:B], retries=2, retry_seed=1, retry_candidates=cand, **TOL)
    torch.cuda.synchronize()
    assert torch.equal(out["q"], ref["q"]) and torch.equal(out["Y"].reshape(ref["x"].shape), ref["x"])
    assert torch.equal(out["attempt"], ref["attempt"]) and torch.equal(out["clearance"], ref["clearance"])
