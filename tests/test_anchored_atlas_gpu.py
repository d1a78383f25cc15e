"""Goal-aware seeds from a configuration atlas on the MI355X (docs/NOTEBOOK.md 46): (a) atlas_nearest_kernel against the
numpy mirror, index and distance bits; (b) the candidate step (gik_anchored_atlas_seeds) against atlas_seeds_host -- the
picked angles bit for bit, the pick, its clearance to 1e-11; (c) gik_anchored_ik_batch_atlas end to end through
AnchoredProblem.solve; (d) the finding the feature stands on: more goals converged and clear from the nearest atlas row
than from the blind seed.

The device and the host realize a configuration to 1e-11 of each other, not to the bit: as in
tests/test_anchored_screen_gpu.py every comparison of a pick first asserts, on the mirror's values and for every slot it
compares, a margin of 1e-9 around the two places where a pick can turn (pick_margins).  No slot is filtered out."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import make_graph
from test_anchored_atlas_host import BLIND_ATTEMPT, BLIND_SEED, floor_problem, room_atlas, room_goals
from test_anchored_screen_gpu import BAR, KEYS, MARGIN, TOL, _bits, _capture_refused, _host, _room, _same_rows, _two_scenes
from test_anchored_screen_host import CLEAR_TOL, FLOOR, RHO, pi_limits, pick_margins
from test_anchored_seeded_host import collision_input

pytestmark = pytest.mark.gpu

MODES = ("nodes", "links", "links+self")
GOALS = 160          # goals of the nearest tables; the compact lists are subsets of them


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


# ---- (a) the nearest kernel against the mirror ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _base(W):
    """The UR10 robot graph's problem: pose goals (W = 6) or a position goal (W = 3)."""
    robot, graph = make_graph("ur10")
    rs = _rs()
    return rs.BatchProblem(graph) if W == 6 else rs.BatchProblem(graph, goal="position")


@functools.lru_cache(maxsize=None)
def _goal_poses():
    """160 goal poses: any bits will do for the key, so the rotation block is random; goals 0 .. 7 repeat goal 8 .. 15's
    position with another axis (equal in W = 3, different in W = 6)."""
    T = np.random.RandomState(50).uniform(-1.0, 1.0, (GOALS, 4, 4))
    T[:8, :3, 3] = T[8:16, :3, 3]
    return T


@functools.lru_cache(maxsize=None)
def _table(M, W):
    """M keys of width W around the goals' own keys: rows 10 .. 79 identical (where M allows: ties across more than one
    trip of 64 rows) and next to goal 5; a NaN row at 0 and at M - 1; row M // 2 IS goal 3's key; the rest uniform."""
    goal_keys = _base(W).goal_positions(_goal_poses()).reshape(GOALS, -1)
    assert goal_keys.shape == (GOALS, W)
    keys = np.random.RandomState(1000 + M).uniform(-1.5, 1.5, (M, W))
    if M >= 80:
        keys[10:80] = goal_keys[5] + 1e-3
    if M >= 3:
        keys[M // 2] = goal_keys[3]
    keys[0, W - 1] = np.nan
    keys[M - 1, 0] = np.nan
    keys.setflags(write=False)
    return keys, goal_keys


def _subset(count, seed=600):
    idx = np.random.RandomState(seed + count).permutation(GOALS)[:count].astype(np.int32)
    assert count == 1 or not np.array_equal(idx, np.arange(count))
    return idx


@pytest.mark.parametrize("W", [6, 3])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 200, 4097])
def test_nearest_kernel_matches_the_mirror(torch_cuda, M, W):
    """Every K in {1, 5, 64} x count in {1, 5, 65, 130} x (d_idx NULL, a shuffled subset): d_nbr equal and d_dist bit for
    bit.  The mirror's table of all 160 goals at K = 64 is computed once per (M, W); a smaller K is its prefix."""
    torch = torch_cuda
    rs = _rs()
    bp = _base(W)
    keys, goal_keys = _table(M, W)
    T = _goal_poses()
    atlas = rs.SeedAtlas(np.zeros((M, 6)), keys, np.zeros(M), device=bp.template.device)
    want_n, want_d = rs.atlas_nearest_host(keys, goal_keys, 64)
    assert np.array_equal(rs.atlas_nearest_host(keys, goal_keys[:7], 5)[0], want_n[:7, :5])      # (the prefix property)
    finite = min(max(M - 2, 0), 64) if M > 1 else 0                  # the two NaN rows are never listed
    assert np.all((want_n >= 0).sum(axis=1) == finite)
    if M >= 3:
        assert want_n[3, 0] == M // 2 and want_d[3, 0] == 0.0                                    # a goal that is itself a row
    if M >= 200:
        assert np.array_equal(want_n[5], np.arange(10, 74)) and len(set(want_d[5].tolist())) == 1   # ties: ascending rows
    for K in (1, 5, 64):
        for count in (1, 5, 65, 130):
            for idx in (None, _subset(count)):
                goals = np.arange(count) if idx is None else idx
                nbr, dist = bp.template.atlas_nearest(atlas, T[:count] if idx is None else T, K, idx=idx)
                torch.cuda.synchronize()
                case = (M, W, K, count, idx is not None)
                assert np.array_equal(nbr.cpu().numpy(), want_n[goals, :K]), case
                assert np.array_equal(_bits(dist.cpu().numpy()), _bits(want_d[goals, :K])), case
    # d_dist may be null
    nbr, dist = bp.template.atlas_nearest(atlas, T, 5, dist=False)
    torch.cuda.synchronize()
    assert dist is None and np.array_equal(nbr.cpu().numpy(), want_n[:, :5])


def test_nearest_guard_rows_and_refusals(torch_cuda):
    torch = torch_cuda
    lib, _ffi = _lib()
    rs = _rs()
    bp = _base(6)
    keys, goal_keys = _table(200, 6)
    want_n, want_d = rs.atlas_nearest_host(keys, goal_keys, 5)
    d_keys = torch.from_numpy(np.ascontiguousarray(keys.T)).cuda()
    d_T = torch.from_numpy(np.ascontiguousarray(_goal_poses().reshape(GOALS, 16))).cuda()
    count, K = 65, 5
    nbr = torch.full((count + 2, K), -7, dtype=torch.int32, device="cuda")
    dist = torch.full((count + 2, K), -7.0, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    torch.cuda.synchronize()

    def call(base=bp.template._h, k=d_keys.data_ptr(), M=200, cnt=count, kk=K, out=nbr.data_ptr() + 4 * K):
        rc = lib.gik_atlas_nearest(base, k, M, d_T.data_ptr(), None, cnt, kk, out, dist.data_ptr() + 8 * K, C.c_void_p(s.cuda_stream))
        return rc, lib.gik_last_error().decode()

    def untouched():
        torch.cuda.synchronize()
        return bool((nbr == -7).all()) and bool((dist == -7.0).all())

    robot, ap = _room()
    for kw, word in ((dict(kk=0), "1 .. 64"), (dict(kk=65), "1 .. 64"), (dict(M=0), "atlas_count"), (dict(k=None), "null atlas"),
                     (dict(cnt=-1), "bad argument"), (dict(out=None), "null buffer"), (dict(base=ap.template._h), "pipeline"),
                     (dict(cnt=2 ** 26, kk=64), "fit an int")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg and "gik_atlas_nearest" in msg, (kw, msg)
        assert untouched(), kw
    _capture_refused(torch, s, call)
    assert untouched()
    rc, msg = call(cnt=0)
    assert rc == 0 and untouched()
    rc, msg = call()
    assert rc == 0, msg
    s.synchronize()
    got_n, got_d = nbr.cpu().numpy(), dist.cpu().numpy()
    assert np.all(got_n[0] == -7) and np.all(got_n[-1] == -7) and np.all(got_d[0] == -7) and np.all(got_d[-1] == -7)
    assert np.array_equal(got_n[1:-1], want_n[:count]) and np.array_equal(_bits(got_d[1:-1]), _bits(want_d[:count]))


# ---- (b) the candidate step against atlas_seeds_host ---------------------------------------------------------------------
N_STEP = 130         # goals of the candidate step's tables


@functools.lru_cache(maxsize=None)
def _step_inputs():
    """UR10 + table_environment() with the floor; an atlas of 2048 uniform draws, NOT filtered (so that the pick has
    blocked candidates to pass over); 130 goals from the FK of other draws."""
    rs = _rs()
    robot, ap = _room()
    lo, hi = pi_limits()
    A = rs.SeedAtlas.from_configurations(ap, rs.retry_seeds_host(21, np.arange(2048), 0, lo, hi), clearance_mode="links+self")
    T = robot.fk_batch(rs.retry_seeds_host(22, np.arange(N_STEP), 0, lo, hi))
    return A, T


@functools.lru_cache(maxsize=None)
def _step_mirror(mode, scenes, C, first):
    """(q [130, n], pick [130], clearance [130], clearance_c [C, 130]) of atlas_seeds_host over all 130 goals; with scenes
    goal g is measured against scene g % 2 of _two_scenes."""
    robot, ap = _room()
    A, T = _step_inputs()
    obstacles = None
    if scenes:
        sets, ids = _two_scenes(ap)
        obstacles = [sets[i] for i in ids[:N_STEP]]
    q, pick, cl = ap.atlas_seeds_host(T, A, C, first=first, clearance_mode=mode, clear_tol=CLEAR_TOL, obstacles=obstacles)
    return q, pick, cl, ap.last_atlas[2]


@pytest.mark.parametrize("count", [1, 65])
def test_candidate_step_matches_the_mirror(torch_cuda, count):
    torch = torch_cuda
    robot, ap = _room()
    tpl, base = ap.template, ap.base.template
    A, T = _step_inputs()
    sets, ids = _two_scenes(ap)
    ids = ids[:N_STEP]
    ss = ap.scene_set(sets)
    idx = np.random.RandomState(700 + count).permutation(N_STEP)[:count].astype(np.int32)
    nbr, _ = ap.atlas_nearest(T, A, 32)
    passed_over, seen = 0, [np.inf, np.inf, 0.0]      # (smallest margins, largest clearance difference)
    for mode in MODES:
        for scenes in (False, True):
            for cand in (1, 4, 16):
                for first in (0, cand):
                    q, pick, cl, cl_c = _step_mirror(mode, scenes, cand, first)
                    near, gap = pick_margins(cl_c[:, idx], CLEAR_TOL)      # every compared slot, asserted, nothing filtered
                    assert near >= MARGIN and gap >= MARGIN, (mode, scenes, cand, first, near, gap)
                    res = tpl.anchored_atlas_seeds(base, A, T, nbr, cand, first=first, idx=idx, clearance_mode=mode,
                                                   clear_tol=CLEAR_TOL, scenes=ss if scenes else None, scene_id=ids if scenes else None)
                    torch.cuda.synchronize()
                    case = (mode, scenes, cand, first)
                    assert np.array_equal(res["pick"].cpu().numpy(), pick[idx]), case
                    assert np.array_equal(_bits(res["q"].cpu().numpy()), _bits(q[idx])), case
                    assert np.array_equal(_bits(res["T"].cpu().numpy()), _bits(T[idx])), case
                    got = res["clearance"].cpu().numpy()
                    assert np.all(np.isfinite(got)) and np.abs(got - cl[idx]).max() < BAR, (case, np.abs(got - cl[idx]).max())
                    passed_over += int((pick[idx] > 0).sum())
                    seen = [min(seen[0], near), min(seen[1], gap), max(seen[2], float(np.abs(got - cl[idx]).max()))]
    print("count", count, "smallest |clearance + clear_tol|:", seen[0], "smallest gap of a blocked slot:", seen[1],
          "largest |device - mirror| clearance:", seen[2], "picks that passed over a nearer row:", passed_over)
    assert count < 5 or passed_over > 0      # (some pick passed over a blocked nearer row)
    # idx NULL: slot r is goal r
    q, pick, cl, cl_c = _step_mirror("links", False, 4, 0)
    res = tpl.anchored_atlas_seeds(base, A, T[:count], nbr[:count].contiguous(), 4, clearance_mode="links")
    torch.cuda.synchronize()
    near, gap = pick_margins(cl_c[:, :count], CLEAR_TOL)
    assert near >= MARGIN and gap >= MARGIN
    assert np.array_equal(res["pick"].cpu().numpy(), pick[:count]) and np.array_equal(_bits(res["q"].cpu().numpy()), _bits(q[:count]))


def test_missing_neighbours_are_nan_candidates(torch_cuda):
    """An atlas of three rows: ranks 3 and up are -1.  Beside a real row a NaN candidate is never picked; where every
    candidate is one, that goal alone gets NaN angles, pick 0 and a NaN clearance."""
    torch = torch_cuda
    rs = _rs()
    robot, ap = _room()
    A, T = _step_inputs()
    T = T[:20]
    small = rs.SeedAtlas(A.q[:3], A.keys[:3], A.clearance[:3], device=ap.template.device)
    nbr, dist = ap.atlas_nearest(T, small, 6)
    torch.cuda.synchronize()
    assert bool((nbr[:, 3:] == -1).all()) and bool(torch.isposinf(dist[:, 3:]).all()) and bool((nbr[:, :3] >= 0).all())
    q, pick, cl = ap.atlas_seeds_host(T, small, 4, first=1, clearance_mode="links")      # ranks 1, 2 and two missing ones
    near, gap = pick_margins(ap.last_atlas[2][:2], CLEAR_TOL)
    assert near >= MARGIN and gap >= MARGIN
    res = ap.template.anchored_atlas_seeds(ap.base.template, small, T, nbr, 4, first=1, clearance_mode="links")
    torch.cuda.synchronize()
    assert np.array_equal(res["pick"].cpu().numpy(), pick) and np.all(pick < 2)
    assert np.array_equal(_bits(res["q"].cpu().numpy()), _bits(q)) and np.abs(res["clearance"].cpu().numpy() - cl).max() < BAR
    res = ap.template.anchored_atlas_seeds(ap.base.template, small, T, nbr, 2, first=3, clearance_mode="links")
    torch.cuda.synchronize()
    assert bool(torch.isnan(res["q"]).all()) and not bool(res["pick"].any()) and bool(torch.isnan(res["clearance"]).all())


# ---- (c) end to end ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _e2e_inputs():
    robot, ap = _room(5)
    A, _ = _step_inputs()
    seeds, goals = collision_input()
    return robot, ap, A, seeds, robot.fk_batch(goals)


def _check_atlas_rows(ap, A, T, R, cand, mode, scene_kw=None, obstacles=None):
    """Every goal holds, bit for bit, the one-goal seeded solve from the mirror's pick among ranks [a C, (a + 1) C) of
    its attempt a, and atlas_pick names that row -- after the pick's margins have been asserted.  Rows with atlas_pick
    -1 (they started from q_init) are the caller's to check.  Returns the attempts' histogram of the compared rows."""
    att, named = R["attempt"], R["atlas_pick"]
    compared = []
    for a in sorted(set(att.tolist())):
        q0, pick, cl = ap.atlas_seeds_host(T, A, cand, first=a * cand, clearance_mode=mode, clear_tol=CLEAR_TOL, obstacles=obstacles)
        rows, q_c, cl_c = ap.last_atlas
        for g in np.flatnonzero((att == a) & (named >= 0)):
            near, gap = pick_margins(cl_c[:, g:g + 1], CLEAR_TOL)
            assert near >= MARGIN and gap >= MARGIN, (g, a, near, gap)
            assert named[g] == rows[pick[g], g], (g, a)
            kw = {} if scene_kw is None else scene_kw(g)
            S = _host(ap.solve(T[g:g + 1], q_init=q0[g:g + 1], clearance=True, clearance_mode=mode, **kw))
            assert _same_rows(R, S, slice(g, g + 1)), (g, a, int(pick[g]))
            compared.append(a)
    return np.bincount(compared, minlength=3).tolist()


def _host_atlas(res):
    out = _host(res)
    out["atlas_pick"] = res["atlas_pick"].cpu().numpy()
    if "attempt" not in out:
        out["attempt"] = np.zeros(len(out["atlas_pick"]), dtype=np.int32)
    return out


def test_end_to_end_every_goal_starts_from_the_mirrors_pick(torch_cuda):
    robot, ap, A, seeds, T = _e2e_inputs()
    for mode in ("nodes", "links+self"):
        kw = dict(retries=2, clearance_mode=mode, **TOL)
        P = ap.solve(T, **kw)
        assert "atlas_pick" not in P
        N = ap.solve(T, atlas=None, **kw)                         # atlas=None: the call as it was, array for array
        assert sorted(N) == sorted(P) and _same_rows(_host(N), _host(P)) and np.array_equal(_host(N)["attempt"], _host(P)["attempt"])
        R = _host_atlas(ap.solve(T, atlas=A, atlas_candidates=2, **kw))
        assert np.all(R["atlas_pick"] >= 0) and R["attempt"].max() <= 2
        hist = _check_atlas_rows(ap, A, T, R, 2, mode)
        print(mode, "attempts of the compared rows:", hist)
        assert sum(hist) == len(T) and hist[1] + hist[2] > 0
        R2 = _host_atlas(ap.solve(T, atlas=A, atlas_candidates=2, **kw))      # the same call again: the same bits
        assert _same_rows(R2, R) and np.array_equal(R2["attempt"], R["attempt"]) and np.array_equal(R2["atlas_pick"], R["atlas_pick"])
    # retries = 0: attempt 0 alone, from the nearest clear row of four
    R0 = _host_atlas(ap.solve(T, atlas=A, atlas_candidates=4, clearance_mode="links"))
    assert _check_atlas_rows(ap, A, T, R0, 4, "links")[0] == len(T)


def test_end_to_end_with_scenes(torch_cuda):
    robot, ap, A, seeds, T = _e2e_inputs()
    sets, ids = _two_scenes(ap)
    ids = ids[:len(T)]
    ss = ap.scene_set(sets)
    R = _host_atlas(ap.solve(T, atlas=A, atlas_candidates=2, retries=2, clearance_mode="links", scenes=ss, scene_id=ids, **TOL))
    hist = _check_atlas_rows(ap, A, T, R, 2, "links", scene_kw=lambda g: dict(scenes=ss, scene_id=ids[g:g + 1]),
                             obstacles=[sets[i] for i in ids])
    print("scenes: attempts of the compared rows:", hist)
    assert sum(hist) == len(T) and hist[1] + hist[2] > 0


def test_end_to_end_with_q_init_the_restarts_alone_take_atlas_rows(torch_cuda):
    robot, ap, A, seeds, T = _e2e_inputs()
    mode = "links+self"
    R = _host_atlas(ap.solve(T, q_init=seeds, atlas=A, atlas_candidates=2, retries=2, clearance_mode=mode, **TOL))
    first = R["attempt"] == 0
    plain = _host(ap.solve(T, q_init=seeds, clearance=True, clearance_mode=mode))
    assert _same_rows(R, plain, first, first)                                  # attempt 0 is the call without an atlas
    assert np.all(R["atlas_pick"][first] == -1) and np.all(R["atlas_pick"][~first] >= 0)
    hist = _check_atlas_rows(ap, A, T, R, 2, mode)
    print("q_init: attempts", np.bincount(R["attempt"], minlength=3).tolist(), "compared:", hist)
    assert hist[0] == 0 and sum(hist) == int((~first).sum()) > 0


def test_batch_refusals_queue_nothing(torch_cuda):
    torch = torch_cuda
    lib, _ffi = _lib()
    rs = _rs()
    robot, ap, A, seeds, Tg = _e2e_inputs()
    tpl, base = ap.template, ap.base.template
    B, cand = 8, 2
    tiny = rs.SeedAtlas(A.q[:5], A.keys[:5], A.clearance[:5], device=tpl.device)
    with pytest.raises(ValueError, match="exceeds"):                               # the Python layer, before any device call
        ap.solve(Tg[:B], atlas=tiny, atlas_candidates=2, retries=2)
    T = torch.from_numpy(np.ascontiguousarray(Tg[:B])).cuda()
    out = tpl.alloc_anchored_buffers(base, B, clearance=True, ws=False)
    out["attempt"] = torch.empty(B, dtype=torch.int32, device="cuda")
    nbytes = int(lib.gik_anchored_ik_batch_atlas_ws_bytes(tpl._h, base._h, B, cand, 2))
    screened = int(lib.gik_anchored_ik_batch_retry_screened_ws_bytes(tpl._h, base._h, B, cand))
    assert nbytes % 8 == 0 and nbytes == screened + 4 * B * 6 + 8 * B * 6 + 4 * B * 3      # nbr, q0, rows (B = 8: no padding)
    assert int(lib.gik_anchored_retry_ws_bytes(tpl._h, base._h, B)) < screened
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    for v in out.values():
        v.view(torch.int32).fill_(-7)
    before = {k: v.clone() for k, v in out.items()}
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    DEFAULT = object()

    def call(anch=tpl._h, bs=base._h, retries=2, candidates=cand, spread=0.0, keys=A.d_keys.data_ptr(), q=A.d_q.data_ptr(),
             M=A.count, clear_tol=CLEAR_TOL, pos_tol=0.01, mode=0, d_ws=DEFAULT, n=B, clearance=DEFAULT):
        opts = _ffi.AnchoredRetryOpts(retries=retries, clearance_mode=mode, seed=1, pos_tol=pos_tol, rot_tol=0.01, clear_tol=clear_tol,
                                      spread=spread)      # (no limits: the entry draws nothing)
        pick = lambda v, d: d if v is DEFAULT else v      # noqa: E731
        rc = lib.gik_anchored_ik_batch_atlas(anch, bs, T.data_ptr(), None, n, C.byref(opts), candidates, keys, q, M, None,
                                             pick(d_ws, ws.data_ptr()), out["Y"].data_ptr(), out["stats"].data_ptr(), out["q"].data_ptr(),
                                             out["pos_err"].data_ptr(), out["rot_err"].data_ptr(),
                                             pick(clearance, out["clearance"].data_ptr()), out["attempt"].data_ptr(),
                                             C.c_void_p(s.cuda_stream))
        return rc, lib.gik_last_error().decode()

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(out[k].view(torch.int32), before[k].view(torch.int32)) for k in out)

    for kw, word in ((dict(M=5), "exceeds atlas_count"), (dict(retries=4, candidates=16), "1 .. 64"), (dict(candidates=0), "candidates"),
                     (dict(candidates=17), "candidates"), (dict(retries=64), "retries"), (dict(spread=0.1), "spread"),
                     (dict(keys=None), "null atlas"), (dict(q=None), "null atlas"), (dict(M=0), "atlas_count"),
                     (dict(clear_tol=0.0), "clear_tol"), (dict(pos_tol=0.0), "positive"), (dict(mode=3), "clearance_mode"),
                     (dict(d_ws=None), "workspace"), (dict(d_ws=ws.data_ptr() + 4), "aligned"), (dict(clearance=None), "d_clearance"),
                     (dict(bs=tpl._h), "pipeline"), (dict(anch=base._h), "fixed-anchor"), (dict(n=-1), "bad argument")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg and "gik_anchored_ik_batch_atlas" in msg, (kw, msg)
        assert untouched(), kw
    assert lib.gik_anchored_ik_batch_atlas_ws_bytes(tpl._h, base._h, B, 16, 4) == 0
    assert lib.gik_anchored_ik_batch_atlas_ws_bytes(tpl._h, tpl._h, B, 2, 2) == 0
    _capture_refused(torch, s, call)
    assert untouched()
    rc, msg = call(n=0)
    assert rc == 0 and untouched()
    rc, msg = call()                                       # the same call on the same stream, not capturing, runs
    assert rc == 0, msg
    s.synchronize()
    ref = ap.solve(Tg[:B], atlas=A, atlas_candidates=cand, retries=2, **TOL)
    torch.cuda.synchronize()
    assert torch.equal(out["q"], ref["q"]) and torch.equal(out["Y"].reshape(ref["x"].shape), ref["x"])
    assert torch.equal(out["attempt"], ref["attempt"]) and torch.equal(out["clearance"], ref["clearance"])


# ---- (d) the finding -----------------------------------------------------------------------------------------------------
def test_more_goals_converge_clear_from_the_nearest_row_than_from_the_blind_seed(torch_cuda):
    """The 256 goals and the 12370-row atlas of NOTEBOOK 46 on the device, default iteration budget, the floor alone:
    converged (f < 1e-9) and clear (halfspace_clearance of whole links >= -1e-4) from solve(T, atlas=A) against
    solve(T, q_init=blind).  The CPU twin's 232 against 192 is the expectation; the device's counts are printed and
    recorded in the NOTEBOOK, and only their order is asserted."""
    rs = _rs()
    robot, host_ap = floor_problem()
    q, T, blind = room_goals()
    A = room_atlas()
    robot_d, graph_d = make_graph("ur10")
    ap = rs.AnchoredProblem(graph_d, link_radius=RHO, self_pairs="auto", halfspaces=[FLOOR])

    def good(res):
        f = res["f"].cpu().numpy()
        x = res["x"].cpu().numpy()
        return int(((f < 1e-9) & (ap.halfspace_clearance(x, links=True) >= -CLEAR_TOL)).sum())

    from_atlas = good(ap.solve(T, atlas=A, clearance_mode="links+self"))
    from_blind = good(ap.solve(T, q_init=blind, clearance_mode="links+self"))
    print("converged and clear of", len(T), "-- from the nearest atlas row:", from_atlas, "from the blind seed:", from_blind)
    assert BLIND_SEED == 7 and BLIND_ATTEMPT == 1 and len(T) == 256 and A.count == 12370
    assert from_atlas > from_blind
