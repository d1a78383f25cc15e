"""Restarts with a clearance rule in the fixed-anchor solve on the MI355X: the three kernels alone
(gik_anchored_retry_select / _seeds / _merge) against numpy, gik_anchored_ik_batch_retry end to end through
AnchoredProblem.solve / solve_trajectory -- every row of the answer is bit for bit either the plain call's or a seeded
solve from the generator's angles -- local mode, and the driver's refusals.  UR10 + table_environment() unless said.
The inputs, the mirror and the CPU twin's evidence for the bars: tests/test_anchored_retry_host.py."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import make_graph
from test_anchored_seeded_gpu import _scene
from test_anchored_seeded_host import collision_input, tracking_input
from test_anchored_retry_host import TWIN_MAXITER, TWIN_SEED
from test_retry_gpu import _failed as plain_failed
from test_retry_gpu import _better as plain_better
from test_retry_gpu import _hip_runtime, _merge_cases, _select_patterns, _stats_buffer

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 1025]
POS_TOL, ROT_TOL, CLEAR_TOL = 0.01, 0.01, 1e-4
TOL = dict(pos_tol=POS_TOL, rot_tol=ROT_TOL, clear_tol=CLEAR_TOL)
KEYS = ("x", "q", "stop", "iterations", "pos_err", "rot_err", "clearance")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@functools.lru_cache(maxsize=None)
def _problem(maxiter=None):
    """One AnchoredProblem (UR10 + table) per iteration budget for the whole module."""
    from graphik_amd.solvers.riemannian_solver import AnchoredProblem
    robot, graph = make_graph("ur10_table")
    return robot, graph, AnchoredProblem(graph, params=None if maxiter is None else {"maxiter": maxiter})


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


def _host(res):
    """A result of AnchoredProblem.solve -> numpy, the fields the identities compare (+ attempt if there)."""
    out = {k: res[k].cpu().numpy() for k in KEYS}
    if "attempt" in res:
        out["attempt"] = res["attempt"].cpu().numpy()
    return out


def _same_rows(a, b, sel_a=slice(None), sel_b=slice(None)):
    return all(np.array_equal(_bits(a[k][sel_a]), _bits(b[k][sel_b])) for k in KEYS)


def _quad(h, sel=slice(None)):
    return h["stop"][sel], h["pos_err"][sel], h["rot_err"][sel], h["clearance"][sel]


# ---- 1. select ---------------------------------------------------------------------------------------------
def _clearance_patterns(B):
    rng = np.random.RandomState(1000 + B)
    ok = lambda: (np.zeros(B, dtype=np.int32), np.full(B, 1e-3), np.full(B, 2e-3), np.full(B, 0.05))     # noqa: E731
    out = {}
    # the patterns of the plain restarts, with no obstacle in sight: the plain rule decides
    for name, (s, p, r) in _select_patterns(B).items():
        out["plain_" + name] = (s, p, r, np.full(B, np.inf))
    s, p, r, c = ok(); c[:] = np.inf; out["all_inf"] = (s, p, r, c)
    s, p, r, c = ok(); c[::3] = np.nan; out["every_third_nan"] = (s, p, r, c)
    s, p, r, c = ok(); c[:] = -CLEAR_TOL; out["at_the_tolerance"] = (s, p, r, c)
    s, p, r, c = ok(); c[:] = np.nextafter(-CLEAR_TOL, -1.0); out["one_ulp_below"] = (s, p, r, c)
    s, p, r, c = ok(); c[-1] = -0.036; out["last_only_colliding"] = (s, p, r, c)
    s, p, r = _select_patterns(B)["mixed"]
    c = rng.choice([np.inf, 0.05, 0.0, -CLEAR_TOL, np.nextafter(-CLEAR_TOL, -1.0), -0.036, np.nan, -np.inf], B)
    out["mixed"] = (s, p, r, c)
    return out


@pytest.mark.parametrize("B", SIZES)
def test_select_compacts_the_failed_goals(torch_cuda, B):
    torch = torch_cuda
    lib, _ffi = _lib()
    rs = _rs()
    expect = {"all_inf": 0, "every_third_nan": len(range(0, B, 3)), "at_the_tolerance": 0, "one_ulp_below": B,
              "last_only_colliding": 1, "plain_none": 0, "plain_all": B}
    for name, (stop, pos, rot, clr) in _clearance_patterns(B).items():
        want = np.flatnonzero(rs.anchored_retry_failed(stop, pos, rot, clr, **TOL))
        if name in expect:
            assert len(want) == expect[name], name
        if name.startswith("plain_"):
            assert np.array_equal(want, np.flatnonzero(plain_failed(stop, pos, rot))), name
        if name == "last_only_colliding":
            assert want.tolist() == [B - 1]
        stats = torch.from_numpy(_stats_buffer(torch, stop)).cuda()
        d_pos, d_rot, d_clr = (torch.from_numpy(a).cuda() for a in (pos, rot, clr))
        idx = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")        # a guard entry on either side
        cnt = torch.tensor([-7, 12345, -7], dtype=torch.int32, device="cuda")    # (the call zeroes the count itself)
        _ffi.check(lib.gik_anchored_retry_select(stats.data_ptr(), d_pos.data_ptr(), d_rot.data_ptr(), d_clr.data_ptr(), B,
                                                 POS_TOL, ROT_TOL, CLEAR_TOL, idx.data_ptr() + 4, cnt.data_ptr() + 4,
                                                 _stream(torch)))
        torch.cuda.synchronize()
        idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
        assert cnt.tolist() == [-7, len(want), -7], name
        assert np.array_equal(np.sort(idx[1:1 + len(want)]), want), name
        assert np.all(idx[1 + len(want):] == -7) and idx[0] == -7, name


# ---- 2. seeds ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", SIZES)
def test_seeds_copy_poses_and_draw_the_mirrors_angles(torch_cuda, B):
    torch = torch_cuda
    lib, _ffi = _lib()
    rs = _rs()
    robot, graph, ap = _problem()
    base = ap.base.template
    n, pose_w = robot.n, 16
    assert n == 6 and base.n_ee == 1
    rng = np.random.RandomState(200 + B)
    T = rng.standard_normal((B, pose_w))             # (the kernel copies rows: any bits will do)
    count = B if B < 64 else B - 3                   # a shuffled subset: slots and goals differ
    idx = rng.permutation(B)[:count].astype(np.int32)
    lo, hi = robot.limits_arrays()
    center = rng.uniform(lo, hi, size=(B, n))        # indexed by GOAL: a kernel that read row r would miss the mirror
    seed, attempt = 0xDEADBEEFCAFEF00D, 1 + B % 63
    d_T, d_idx, d_c = torch.from_numpy(T).cuda(), torch.from_numpy(idx).cuda(), torch.from_numpy(center).cuda()
    d_lo, d_hi = torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()

    def draw(spread, c_ptr):
        T_out = torch.full((count + 2, pose_w), -7.0, dtype=torch.float64, device="cuda")
        q_out = torch.full((count + 2, n), -7.0, dtype=torch.float64, device="cuda")
        _ffi.check(lib.gik_anchored_retry_seeds(base._h, d_T.data_ptr(), d_idx.data_ptr(), count, seed, attempt,
                                                d_lo.data_ptr(), d_hi.data_ptr(), c_ptr, spread,
                                                T_out.data_ptr() + 8 * pose_w, q_out.data_ptr() + 8 * n, _stream(torch)))
        torch.cuda.synchronize()
        T_out, q_out = T_out.cpu().numpy(), q_out.cpu().numpy()
        for buf in (T_out, q_out):
            assert np.all(buf[0] == -7.0) and np.all(buf[-1] == -7.0)
        assert np.array_equal(_bits(T_out[1:-1]), _bits(T[idx]))      # pose rows, copied exactly
        return q_out[1:-1]

    # spread = 0: the bits of gik_retry_seeds on the same inputs (and of the mirror), with or without a centre
    T_ref = torch.empty(count, pose_w, dtype=torch.float64, device="cuda")
    q_ref = torch.empty(count, n, dtype=torch.float64, device="cuda")
    _ffi.check(lib.gik_retry_seeds(base._h, d_T.data_ptr(), d_idx.data_ptr(), count, seed, attempt, d_lo.data_ptr(),
                                   d_hi.data_ptr(), T_ref.data_ptr(), q_ref.data_ptr(), _stream(torch)))
    torch.cuda.synchronize()
    for c_ptr in (None, d_c.data_ptr()):
        q0 = draw(0.0, c_ptr)
        assert np.array_equal(_bits(q0), _bits(q_ref.cpu().numpy()))
        assert np.array_equal(_bits(q0), _bits(rs.retry_seeds_host(seed, idx, attempt, lo, hi)))
    # local mode: the mirror's bits.  Centres inside the limits: 0.05 rad clips hardly any joint, 10 rad about two in three
    for spread in (0.05, 10.0):
        q = draw(spread, d_c.data_ptr())
        want = rs.retry_seeds_host(seed, idx, attempt, lo, hi, center=center[idx], spread=spread)
        assert np.array_equal(_bits(q), _bits(want)), spread
        assert np.all(q >= lo) and np.all(q <= hi)
        if count > 1 and spread < 1:
            assert not np.array_equal(q, rs.retry_seeds_host(seed, idx, attempt, lo, hi, center=center[:count], spread=spread))
    assert ((q == lo) | (q == hi)).any()
    # centres 20 rad beyond a limit: 10 rad clips every joint, to the limit on the centre's side
    above = rng.rand(B, n) < 0.5
    far = np.where(above, hi + 20.0, lo - 20.0)
    d_far = torch.from_numpy(far).cuda()
    q = draw(10.0, d_far.data_ptr())
    assert np.array_equal(_bits(q), _bits(np.where(above[idx], hi, lo)))
    assert np.array_equal(_bits(q), _bits(rs.retry_seeds_host(seed, idx, attempt, lo, hi, center=far[idx], spread=10.0)))
    # refusals of the call itself
    assert lib.gik_anchored_retry_seeds(base._h, d_T.data_ptr(), d_idx.data_ptr(), count, seed, attempt, d_lo.data_ptr(),
                                        d_hi.data_ptr(), None, 0.1, T_ref.data_ptr(), q_ref.data_ptr(), _stream(torch)) != 0
    assert "d_q_center" in lib.gik_last_error().decode()
    assert lib.gik_anchored_retry_seeds(base._h, d_T.data_ptr(), d_idx.data_ptr(), count, seed, attempt, d_lo.data_ptr(),
                                        d_hi.data_ptr(), d_c.data_ptr(), -0.1, T_ref.data_ptr(), q_ref.data_ptr(),
                                        _stream(torch)) != 0
    assert "spread" in lib.gik_last_error().decode()


# ---- 3. merge ----------------------------------------------------------------------------------------------
# (stop, pos_err, rot_err, clearance): three successes and three failures of rising score, two NaN answers
OK_LO, OK_MID, OK_HI = (0, 0.002, 0.001, 0.05), (0, 0.005, 0.005, np.inf), (0, 0.01, 0.002, -CLEAR_TOL)
F_STOP, F_POSE, F_CLEAR = (1, 0.002, 0.001, 0.05), (0, 0.05, 0.005, 0.05), (0, 0.001, 0.001, -0.036)
N_CLEAR, N_POSE = (0, 0.001, 0.001, np.nan), (0, np.nan, 0.001, 0.05)
F_CLEAR_SMALL = (0, 0.001, 0.001, -0.001)
VARIANTS = [OK_LO, OK_MID, OK_HI, F_STOP, F_POSE, F_CLEAR, N_CLEAR, N_POSE]


def _merge_table():
    """65 (incumbent, restart) cells: every pair of the eight variants -- (ok_old, ok_new) x (lower, equal, higher
    score), a NaN on either side and on both, failure by clearance alone on either side -- and one more pair of two
    failures by clearance alone."""
    cells = [(o, n) for o in VARIANTS for n in VARIANTS] + [(F_CLEAR, F_CLEAR_SMALL)]
    assert len(cells) == 65
    cols = lambda side: tuple(np.array([c[side][k] for c in cells], dtype=np.int32 if k == 0 else np.float64)      # noqa: E731
                              for k in range(4))
    return cells, cols(0), cols(1)


def _run_merge(torch, ap, old, new, B, idx, rng, attempt_no=5):
    """Incumbents `old` at goals idx of a batch of B (other goals: arbitrary), restarts `new` in slots 0 .. count-1, a
    guard row before and after every buffer.  Returns (host buffers before, restart buffers, device buffers after)."""
    lib, _ffi = _lib()
    tpl, base = ap.template, ap.base.template
    row, n, count = tpl.full_N * 3, base.n_joints, len(idx)
    inc_stop = rng.choice([0, 1], B).astype(np.int32)
    inc_pos, inc_rot, inc_clr = rng.uniform(0, 0.02, B), rng.uniform(0, 0.02, B), rng.uniform(-0.01, 0.1, B)
    inc_stop[idx], inc_pos[idx], inc_rot[idx], inc_clr[idx] = old

    def guarded(a):
        g = np.full((1,) + a.shape[1:], -7, dtype=a.dtype)
        return np.concatenate([g, a, g])

    host = {"Y": guarded(rng.standard_normal((B, row))), "stats": guarded(_stats_buffer(torch, inc_stop, rng)),
            "q": guarded(rng.standard_normal((B, n))), "pos": guarded(inc_pos), "rot": guarded(inc_rot),
            "clr": guarded(inc_clr), "attempt": guarded(rng.randint(0, 3, B).astype(np.int32))}
    retry = {"Y": rng.standard_normal((count, row)), "stats": _stats_buffer(torch, new[0], rng),
             "q": rng.standard_normal((count, n)), "pos": new[1].copy(), "rot": new[2].copy(), "clr": new[3].copy()}
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    dre = {k: torch.from_numpy(v).cuda() for k, v in retry.items()}
    d_idx = torch.from_numpy(np.asarray(idx, dtype=np.int32)).cuda()

    def ptr(k):      # past the guard row
        t = dev[k]
        return t.data_ptr() + t.element_size() * (t.numel() // t.shape[0])

    _ffi.check(lib.gik_anchored_retry_merge(tpl._h, base._h, d_idx.data_ptr(), count, attempt_no, POS_TOL, ROT_TOL, CLEAR_TOL,
                                            dre["Y"].data_ptr(), dre["stats"].data_ptr(), dre["q"].data_ptr(),
                                            dre["pos"].data_ptr(), dre["rot"].data_ptr(), dre["clr"].data_ptr(), ptr("Y"),
                                            ptr("stats"), ptr("q"), ptr("pos"), ptr("rot"), ptr("clr"), ptr("attempt"),
                                            _stream(torch)))
    torch.cuda.synchronize()
    return host, retry, {k: v.cpu().numpy() for k, v in dev.items()}


def _check_merge(host, retry, got, idx, take, attempt_no=5):
    idx = np.asarray(idx)
    for k in host:
        want = host[k].copy()
        if k == "attempt":
            want[1 + idx[take]] = attempt_no
        else:
            want[1 + idx[take]] = retry[k][take]
        bits = np.int64 if want.dtype == np.float64 else np.int32
        assert np.array_equal(got[k].view(bits), want.view(bits)), k      # every other goal's bytes and the guard rows included


def test_merge_keeps_the_better_answer(torch_cuda):
    torch = torch_cuda
    rs = _rs()
    robot, graph, ap = _problem()
    assert ap.template.full_N * 3 > 24                 # (a row is wider than the kernel's other copies)
    cells, old, new = _merge_table()
    take = rs.anchored_retry_better(new, old, **TOL)
    # the table by hand, cell by cell
    cell = lambda o, n: bool(take[cells.index((o, n))])      # noqa: E731
    oks, fails, nans = (OK_LO, OK_MID, OK_HI), (F_STOP, F_POSE, F_CLEAR), (N_CLEAR, N_POSE)
    assert all(cell(f, o) for f in fails + nans for o in oks)            # a success replaces any failure ...
    assert not any(cell(o, f) for f in fails + nans for o in oks)        # ... and is never replaced by one
    assert cell(OK_MID, OK_LO) and cell(OK_HI, OK_MID) and not cell(OK_LO, OK_MID) and not cell(OK_MID, OK_HI)
    assert cell(F_POSE, F_STOP) and cell(F_CLEAR, F_POSE) and not cell(F_STOP, F_POSE) and not cell(F_POSE, F_CLEAR)
    assert not any(cell(v, v) for v in VARIANTS)                         # a tie keeps the incumbent
    assert not any(cell(v, nn) for v in VARIANTS for nn in nans)         # a NaN never wins
    assert all(cell(nn, v) for nn in nans for v in oks + fails)          # ... and loses to anything finite
    assert cell(F_CLEAR, F_CLEAR_SMALL) and cell(F_CLEAR, OK_HI) and not cell(OK_HI, F_CLEAR)      # failure by clearance alone
    assert 0.2 < take.mean() < 0.8
    rng = np.random.RandomState(9)
    B = 200
    idx = rng.permutation(B)[:65].astype(np.int32)
    host, retry, got = _run_merge(torch, ap, old, new, B, idx, rng)
    _check_merge(host, retry, got, idx, take)
    # count = 1: one slot, one block; a replaced goal, a kept one, a NaN restart, failure by clearance alone both ways
    for o, n, want in ((F_CLEAR, OK_HI, True), (OK_LO, OK_MID, False), (F_POSE, N_CLEAR, False), (OK_HI, F_CLEAR, False),
                       (F_CLEAR, F_CLEAR_SMALL, True), (OK_MID, OK_MID, False)):
        k = cells.index((o, n))
        one = lambda cols: tuple(c[k:k + 1] for c in cols)      # noqa: E731
        assert bool(take[k]) == want
        for B1, g in ((1, 0), (67, 66), (67, 0)):
            host, retry, got = _run_merge(torch, ap, one(old), one(new), B1, np.array([g], dtype=np.int32), rng, attempt_no=63)
            _check_merge(host, retry, got, [g], take[k:k + 1], attempt_no=63)


# ---- 3b. one kernel set: with no clearance in sight the anchored entries are the plain ones ---------------------------
@pytest.mark.parametrize("B", SIZES)
def test_plain_and_anchored_entries_agree(torch_cuda, B):
    """gik_retry_select / _seeds / _merge and their gik_anchored_* twins on the same inputs, every clearance +inf, spread 0
    and no centre: the same failed goals, the same seeds and the same merged batch, bit for bit.  The base template is
    3-D, so its row N K is the anchored row full_N 3 and the same buffers serve both calls."""
    torch = torch_cuda
    lib, _ffi = _lib()
    robot, graph, ap = _problem()
    tpl, base = ap.template, ap.base.template
    row, n, pose_w = tpl.full_N * 3, base.n_joints, base.n_ee * 16
    assert base.N * base.k == row
    st = _stream(torch)
    rng = np.random.RandomState(300 + B)
    inf_B = torch.full((B,), np.inf, dtype=torch.float64, device="cuda")

    # select: equal counts and equal index sets (the order of the list is unspecified)
    for name, (stop, pos, rot) in _select_patterns(B).items():
        assert not np.any(pos < 0) and not np.any(rot < 0)
        stats = torch.from_numpy(_stats_buffer(torch, stop)).cuda()
        d_pos, d_rot = torch.from_numpy(pos).cuda(), torch.from_numpy(rot).cuda()
        idx = torch.full((2, B + 2), -7, dtype=torch.int32, device="cuda")        # a guard entry on either side
        cnt = torch.tensor([[-7, 12345, -7]] * 2, dtype=torch.int32, device="cuda")
        _ffi.check(lib.gik_retry_select(stats.data_ptr(), d_pos.data_ptr(), d_rot.data_ptr(), B, POS_TOL, ROT_TOL,
                                        idx[0].data_ptr() + 4, cnt[0].data_ptr() + 4, st))
        _ffi.check(lib.gik_anchored_retry_select(stats.data_ptr(), d_pos.data_ptr(), d_rot.data_ptr(), inf_B.data_ptr(), B,
                                                 POS_TOL, ROT_TOL, CLEAR_TOL, idx[1].data_ptr() + 4, cnt[1].data_ptr() + 4, st))
        torch.cuda.synchronize()
        idx, cnt = idx.cpu().numpy(), cnt.cpu().numpy()
        k = int(cnt[0, 1])
        assert cnt[0].tolist() == cnt[1].tolist() == [-7, k, -7] and 0 <= k <= B, name
        assert k == int(plain_failed(stop, pos, rot).sum()), name
        assert np.array_equal(np.sort(idx[0, 1:1 + k]), np.sort(idx[1, 1:1 + k])), name
        assert np.all(idx[:, 1 + k:] == -7) and np.all(idx[:, 0] == -7), name

    count = B if B < 64 else B - 3                   # a shuffled subset: slots and goals differ
    goals = rng.permutation(B)[:count].astype(np.int32)
    d_goals = torch.from_numpy(goals).cuda()

    # seeds: pose rows and angles bit-identical
    lo, hi = robot.limits_arrays()
    d_T = torch.from_numpy(rng.standard_normal((B, pose_w))).cuda()
    d_lo, d_hi = torch.from_numpy(lo).cuda(), torch.from_numpy(hi).cuda()
    T_out = torch.full((2, count + 2, pose_w), -7.0, dtype=torch.float64, device="cuda")
    q_out = torch.full((2, count + 2, n), -7.0, dtype=torch.float64, device="cuda")
    seed, attempt = 0xDEADBEEFCAFEF00D, 1 + B % 63
    _ffi.check(lib.gik_retry_seeds(base._h, d_T.data_ptr(), d_goals.data_ptr(), count, seed, attempt, d_lo.data_ptr(),
                                   d_hi.data_ptr(), T_out[0].data_ptr() + 8 * pose_w, q_out[0].data_ptr() + 8 * n, st))
    _ffi.check(lib.gik_anchored_retry_seeds(base._h, d_T.data_ptr(), d_goals.data_ptr(), count, seed, attempt, d_lo.data_ptr(),
                                            d_hi.data_ptr(), None, 0.0, T_out[1].data_ptr() + 8 * pose_w,
                                            q_out[1].data_ptr() + 8 * n, st))
    torch.cuda.synchronize()
    for buf in (T_out.cpu().numpy(), q_out.cpu().numpy()):
        assert np.array_equal(_bits(buf[0]), _bits(buf[1]))
        assert np.all(buf[:, 0] == -7.0) and np.all(buf[:, -1] == -7.0) and not np.any(buf[:, 1:-1] == -7.0)

    # merge: the drawn cells of the plain tests (NaN errors among them), no error negative
    old, new = _merge_cases(count, seed=B)
    assert all(not np.any(a < 0) for a in old[1:] + new[1:]) and (count == 1 or np.isnan(new[1]).any())
    inc_stop = rng.choice([0, 1], B).astype(np.int32)
    inc_pos, inc_rot = rng.uniform(0, 0.02, B), rng.uniform(0, 0.02, B)
    inc_stop[goals], inc_pos[goals], inc_rot[goals] = old

    def guarded(a):
        g = np.full((1,) + a.shape[1:], -7, dtype=a.dtype)
        return np.concatenate([g, a, g])

    host = {"Y": guarded(rng.standard_normal((B, row))), "stats": guarded(_stats_buffer(torch, inc_stop, rng)),
            "q": guarded(rng.standard_normal((B, n))), "pos": guarded(inc_pos), "rot": guarded(inc_rot),
            "attempt": guarded(rng.randint(0, 3, B).astype(np.int32)), "clr": guarded(np.full(B, np.inf))}
    retry = {"Y": rng.standard_normal((count, row)), "stats": _stats_buffer(torch, new[0], rng),
             "q": rng.standard_normal((count, n)), "pos": new[1].copy(), "rot": new[2].copy(), "clr": np.full(count, np.inf)}
    dre = {k: torch.from_numpy(v).cuda() for k, v in retry.items()}
    plain = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    anch = {k: torch.from_numpy(v).cuda() for k, v in host.items()}

    def ptr(t):      # past the guard row
        return t.data_ptr() + t.element_size() * (t.numel() // t.shape[0])

    ATTEMPT = 5
    _ffi.check(lib.gik_retry_merge(base._h, d_goals.data_ptr(), count, ATTEMPT, POS_TOL, ROT_TOL, dre["Y"].data_ptr(),
                                   dre["stats"].data_ptr(), dre["q"].data_ptr(), dre["pos"].data_ptr(), dre["rot"].data_ptr(),
                                   ptr(plain["Y"]), ptr(plain["stats"]), ptr(plain["q"]), ptr(plain["pos"]), ptr(plain["rot"]),
                                   ptr(plain["attempt"]), st))
    _ffi.check(lib.gik_anchored_retry_merge(tpl._h, base._h, d_goals.data_ptr(), count, ATTEMPT, POS_TOL, ROT_TOL, CLEAR_TOL,
                                            dre["Y"].data_ptr(), dre["stats"].data_ptr(), dre["q"].data_ptr(),
                                            dre["pos"].data_ptr(), dre["rot"].data_ptr(), dre["clr"].data_ptr(), ptr(anch["Y"]),
                                            ptr(anch["stats"]), ptr(anch["q"]), ptr(anch["pos"]), ptr(anch["rot"]),
                                            ptr(anch["clr"]), ptr(anch["attempt"]), st))
    torch.cuda.synchronize()
    take = plain_better(new, old)
    want_attempt = host["attempt"].copy()
    want_attempt[1 + goals[take]] = ATTEMPT
    for k in host:
        a = anch[k].cpu().numpy()
        bits = np.int64 if a.dtype == np.float64 else np.int32
        assert np.array_equal(a[[0, -1]].view(bits), host[k][[0, -1]].view(bits)), k      # the guard rows
        if k == "clr":
            assert np.array_equal(a, host[k])      # +inf everywhere still; the plain call has no such array
            continue
        p = plain[k].cpu().numpy()
        assert np.array_equal(p.view(bits), a.view(bits)), k
        if k == "attempt":
            assert np.array_equal(p, want_attempt)


# ---- 4-7. end to end -----------------------------------------------------------------------------------------
def _check_identities(ap, T, q_init, retries, seed, tol=TOL, spread=0.0):
    """The contract of a solve with restarts against the plain call P on the same goals.  Returns (P, R) on the host."""
    rs = _rs()
    lo, hi = ap.robot.limits_arrays()
    P = _host(ap.solve(T, q_init=q_init, clearance=True))
    R = _host(ap.solve(T, q_init=q_init, retries=retries, retry_seed=seed, retry_spread=spread, **tol))
    att = R["attempt"]
    assert att.dtype == np.int32 and att.shape == (len(T),)
    assert att.min() >= 0 and att.max() <= retries
    failed_P = rs.anchored_retry_failed(*_quad(P), **tol)
    assert not np.any(att[~failed_P]), "a goal that succeeded at once was retried"
    # no goal is worse than in P under `better`, and no success is lost
    assert not np.any(rs.anchored_retry_better(_quad(P), _quad(R), **tol))
    failed_R = rs.anchored_retry_failed(*_quad(R), **tol)
    assert not np.any(failed_R & ~failed_P)
    # rows that kept the first answer are the plain call's, bit for bit
    first = att == 0
    assert _same_rows(R, P, first, first)
    if not failed_P.any():                      # the early exit: nothing was queued after the first attempt
        assert not att.any() and _same_rows(R, P)
    # a replaced row is the one-goal seeded solve from the generator's angles, bit for bit: the anchored solve runs on
    # the wavefront kernel, whose bits do not depend on the batch
    for g in np.flatnonzero(att > 0):
        c = None if spread == 0 else np.asarray(q_init)[g:g + 1]
        q0 = rs.retry_seeds_host(seed, [g], int(att[g]), lo, hi, center=c, spread=spread)
        S = _host(ap.solve(T[g:g + 1], q_init=q0, clearance=True))
        assert _same_rows(R, S, slice(g, g + 1)), (g, att[g])
        # an answer that replaced another one is strictly better than what the plain call had
        assert rs.anchored_retry_better(_quad(R, slice(g, g + 1)), _quad(P, slice(g, g + 1)), **tol)[0]
    # the clearance that comes back is the answer's
    fin = np.isfinite(R["clearance"])
    if len(ap.obstacles):
        assert np.abs(R["clearance"] - ap.clearance(R["x"]))[fin].max(initial=0.0) < 1e-12
    return P, R


def test_end_to_end_every_goal_retried(torch_cuda):
    """collision_input() from its colliding seeds, maxiter = 5: the CPU twin fails attempt 0 on 64 of 64 and improves 42
    with two restarts (tests/test_anchored_retry_host.py), so "at least one failed, at least one improved" has room."""
    rs = _rs()
    robot, graph, ap = _problem(TWIN_MAXITER)
    seeds, goals = collision_input()
    T = robot.fk_batch(goals)
    P, R = _check_identities(ap, T, seeds, retries=2, seed=TWIN_SEED)
    failed_P = rs.anchored_retry_failed(*_quad(P), **TOL)
    att = R["attempt"]
    print("failed attempt 0:", int(failed_P.sum()), "attempt histogram", np.bincount(att, minlength=3).tolist(), "successes",
          int((~failed_P).sum()), "->", int((~rs.anchored_retry_failed(*_quad(R), **TOL)).sum()))
    assert failed_P.any(), "no goal failed the first attempt: the test would check nothing"
    assert (att > 0).any(), "no restart improved on any of 64 five-iteration answers"
    # the same seed: the same bits; another seed: other angles, so some retried row differs
    R2 = _host(ap.solve(T, q_init=seeds, retries=2, retry_seed=TWIN_SEED, **TOL))
    assert _same_rows(R2, R) and np.array_equal(R2["attempt"], att)
    R3 = _host(ap.solve(T, q_init=seeds, retries=2, retry_seed=TWIN_SEED + 1, **TOL))
    seeded = (att > 0) | (R3["attempt"] > 0)
    assert not _same_rows(R3, R, seeded, seeded)


def test_end_to_end_default_budget(torch_cuda):
    """64 cold goals, default maxiter, one restart: properties only, no rescue rate."""
    rs = _rs()
    robot, graph, ap = _problem()
    _, goals = collision_input()
    T = robot.fk_batch(goals)
    P, R = _check_identities(ap, T, None, retries=1, seed=3)
    # attempt 0 of a cold batch: gik_anchored_ik_batch, then gik_anchored_clearance of its answer
    cold = ap.solve(T)
    assert "clearance" not in cold and "attempt" not in cold
    assert np.array_equal(_bits(cold["x"].cpu().numpy()), _bits(P["x"]))
    assert np.array_equal(_bits(ap.template.anchored_clearance(cold["x"]).cpu().numpy()), _bits(P["clearance"]))
    failed_P = rs.anchored_retry_failed(*_quad(P), **TOL)
    print("cold: failed in P", int(failed_P.sum()), "rescued", int((failed_P & ~rs.anchored_retry_failed(*_quad(R), **TOL)).sum()),
          "improved", int((R["attempt"] > 0).sum()))


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


def test_clearance_decides(torch_cuda):
    """pos_tol = rot_tol = 1e9: only `stop` and the clearance can fail a goal; with clear_tol = 1e9 too, only `stop`.
    Cold goals at the default budget, and the colliding seeds at maxiter = 5 (where goals do fail)."""
    torch = torch_cuda
    seeds, goals = collision_input()
    for maxiter, q_init in ((None, None), (TWIN_MAXITER, seeds)):
        robot, graph, ap = _problem(maxiter)
        T = robot.fk_batch(goals)
        loose = dict(pos_tol=1e9, rot_tol=1e9, clear_tol=CLEAR_TOL)
        P, R = _check_identities(ap, T, q_init, retries=1, seed=5, tol=loose)
        may = (P["stop"] != 0) | (P["clearance"] < -CLEAR_TOL)
        assert np.array_equal(_selected(torch, P, loose), np.flatnonzero(may))
        assert not np.any(R["attempt"][~may])
        assert _same_rows(R, P, ~may, ~may)
        looser = dict(pos_tol=1e9, rot_tol=1e9, clear_tol=1e9)
        P2, R2 = _check_identities(ap, T, q_init, retries=1, seed=5, tol=looser)
        assert _same_rows(P2, P)
        stopped = P["stop"] != 0
        assert np.array_equal(_selected(torch, P, looser), np.flatnonzero(stopped))
        assert not np.any(R2["attempt"][~stopped]) and _same_rows(R2, P, ~stopped, ~stopped)
        print("maxiter", maxiter, ": stop != 0:", int(stopped.sum()), "stop or clearance:", int(may.sum()), "improved",
              int((R["attempt"] > 0).sum()), int((R2["attempt"] > 0).sum()))


def test_no_obstacles(torch_cuda):
    """A bare UR10 through AnchoredProblem: the clearance is +inf everywhere, so the rule is the plain restarts'."""
    torch = torch_cuda
    ap = _scene(0)
    robot = ap.robot
    _, goals = collision_input()
    T = robot.fk_batch(goals)
    for q_init in (None, collision_input()[0]):
        P, R = _check_identities(ap, T, q_init, retries=1, seed=11)
        assert np.all(np.isposinf(P["clearance"])) and np.all(np.isposinf(R["clearance"]))
        want = np.flatnonzero(plain_failed(P["stop"], P["pos_err"], P["rot_err"]))
        assert np.array_equal(_selected(torch, P, TOL), want)
        assert not np.any(R["attempt"][np.setdiff1d(np.arange(len(T)), want)])
        print("no obstacles: failed", len(want), "improved", int((R["attempt"] > 0).sum()))


# ---- 8. local mode -----------------------------------------------------------------------------------------------
def test_local_mode_centres_on_the_original_seed(torch_cuda):
    """tracking_input() waypoint 3 from waypoint 0's angles, maxiter = 5 (the tracked solves of NOTEBOOK 18 take a median
    of 45 outer iterations: most goals stop at maxiter and are retried), one local restart of 0.1 rad."""
    torch = torch_cuda
    rs = _rs()
    robot, graph, ap = _problem(TWIN_MAXITER)
    Q, T = tracking_input()
    Tg, q0 = T[:, 3], Q[:, 0]
    P, R = _check_identities(ap, Tg, q0, retries=1, seed=13, spread=0.1)
    failed_P = rs.anchored_retry_failed(*_quad(P), **TOL)
    print("local mode: failed", int(failed_P.sum()), "improved", int((R["attempt"] > 0).sum()))
    assert failed_P.any()
    # the seed tensor may be the answer's own buffer: the centre is the copy taken before attempt 0 overwrites it
    tpl, base = ap.template, ap.base.template
    out = tpl.alloc_anchored_buffers(base, len(Tg), clearance=True)
    out["q"].copy_(torch.from_numpy(q0.copy()))
    kw = dict(retries=1, retry_seed=13, retry_spread=0.1, q_limits=robot.limits_arrays(), **TOL)
    res = tpl.anchored_ik(base, Tg, q_init=out["q"], out=out, clearance=True, **kw)
    assert res["q"].data_ptr() == out["q"].data_ptr()
    A = _host(res)
    assert _same_rows(A, R) and np.array_equal(A["attempt"], R["attempt"])
    # ... and a uniform restart of the same goals draws other angles
    U = _host(ap.solve(Tg, q_init=q0, retries=1, retry_seed=13, **TOL))
    both = (U["attempt"] > 0) | (R["attempt"] > 0)
    assert not both.any() or not _same_rows(U, R, both, both)


# ---- 9. path tracking ------------------------------------------------------------------------------------------
def test_solve_trajectory_with_retries(torch_cuda):
    robot, graph, ap = _problem(TWIN_MAXITER)
    Q, T = tracking_input()
    Bp, L = 8, 3
    T = T[:Bp, :L]
    lb, ub = robot.limits_arrays()
    q_start = np.random.RandomState(31).uniform(lb, ub, size=(Bp, robot.n))       # far from the paths
    for spread in (0.0, 0.1):
        kw = dict(retries=1, retry_seed=13, retry_spread=spread, **TOL)
        q, Y, info = ap.solve_trajectory(T, q_start, return_Y=True, **kw)
        assert info["attempt"].shape == (Bp, L) and info["attempt"].dtype == np.int32
        assert info["attempt"].min() >= 0 and info["attempt"].max() <= 1
        prev = q_start
        for l in range(L):
            S = _host(ap.solve(T[:, l], q_init=prev, **kw))
            way = {"x": Y[:, l], "q": q[:, l], **{k: info[k][:, l] for k in ("stop", "iterations", "pos_err", "rot_err", "clearance")}}
            assert _same_rows(way, S), (spread, l)
            assert np.array_equal(info["attempt"][:, l], S["attempt"]), (spread, l)
            prev = q[:, l]                                       # rescued angles seed the next waypoint
        print("spread", spread, "trajectory attempts", info["attempt"].tolist())
    # retries = 0: today's call -- waypoint l is the plain seeded solve from waypoint l-1's angles -- and no "attempt"
    q0, Y0, info0 = ap.solve_trajectory(T, q_start, return_Y=True)
    q1, Y1, info1 = ap.solve_trajectory(T, q_start, return_Y=True, retries=0, retry_spread=0.0)
    assert "attempt" not in info0 and "attempt" not in info1
    assert np.array_equal(_bits(q0), _bits(q1)) and np.array_equal(_bits(Y0), _bits(Y1))
    prev = q_start
    for l in range(L):
        S = _host(ap.solve(T[:, l], q_init=prev))
        way = {"x": Y0[:, l], "q": q0[:, l], **{k: info0[k][:, l] for k in ("stop", "iterations", "pos_err", "rot_err", "clearance")}}
        assert _same_rows(way, S), l
        prev = q0[:, l]


# ---- 10-11. the driver itself --------------------------------------------------------------------------------------
def _driver_setup(torch, ap, B):
    lib, _ffi = _lib()
    tpl, base = ap.template, ap.base.template
    out = tpl.alloc_anchored_buffers(base, B, clearance=True)
    del out["ws"]
    out["attempt"] = torch.empty(B, dtype=torch.int32, device="cuda")
    nbytes = int(lib.gik_anchored_retry_ws_bytes(tpl._h, base._h, B))
    assert nbytes >= 8 * int(lib.gik_anchored_ws_doubles(tpl._h, base._h, B)) and nbytes % 8 == 0
    ws = torch.empty(nbytes // 8 + 1, dtype=torch.float64, device="cuda")
    return out, ws


def test_retries_0_is_todays_path(torch_cuda):
    torch = torch_cuda
    lib, _ffi = _lib()
    robot, graph, ap = _problem()
    tpl, base = ap.template, ap.base.template
    seeds, goals = collision_input()
    B = len(goals)
    Tg = robot.fk_batch(goals)
    T = torch.from_numpy(np.ascontiguousarray(Tg)).cuda()
    q0 = torch.from_numpy(seeds.copy()).cuda()
    out, ws = _driver_setup(torch, ap, B)
    for q_ptr, ref in ((None, ap.solve(Tg, clearance=True)), (q0.data_ptr(), ap.solve(Tg, q_init=seeds))):
        for v in out.values():
            v.view(torch.int32).fill_(-7)
        # (no limits, no tolerances: with retries = 0 nothing reads them)
        opts = _ffi.AnchoredRetryOpts(retries=0, seed=1)
        _ffi.check(lib.gik_anchored_ik_batch_retry(tpl._h, base._h, T.data_ptr(), q_ptr, B, C.byref(opts), ws.data_ptr(),
                                                   out["Y"].data_ptr(), out["stats"].data_ptr(), out["q"].data_ptr(),
                                                   out["pos_err"].data_ptr(), out["rot_err"].data_ptr(),
                                                   out["clearance"].data_ptr(), out["attempt"].data_ptr(), _stream(torch)))
        torch.cuda.synchronize()
        from graphik_amd.engine import _decode_stats
        got = {"x": out["Y"].reshape(B, -1, 3), "q": out["q"], "pos_err": out["pos_err"], "rot_err": out["rot_err"],
               "clearance": out["clearance"], **_decode_stats(out["stats"])}
        assert _same_rows(_host(got), _host(ref))
        for key in ("f", "gradnorm", "inner_total", "n_accept"):
            assert torch.equal(got[key], ref[key]), key
        assert not out["attempt"].any()
    # the Python layer with retries = 0 is the call it always was: the same keys, the same bits
    r = ap.solve(Tg)
    assert set(r) == {"x", "q", "pos_err", "rot_err", "_ws", "f", "gradnorm", "stepsize", "iterations", "inner_total",
                      "stop", "n_accept", "inner_executed", "flags"}
    r0 = ap.solve(Tg, retries=0, retry_spread=0.0, clear_tol=1e-4)
    assert set(r0) == set(r) and torch.equal(r0["x"], r["x"]) and torch.equal(r0["q"], r["q"])


def test_driver_refusals_leave_the_outputs_alone(torch_cuda):
    torch = torch_cuda
    lib, _ffi = _lib()
    robot, graph, ap = _problem()
    tpl, base = ap.template, ap.base.template
    B = 8
    seeds, goals = collision_input()
    T = torch.from_numpy(np.ascontiguousarray(robot.fk_batch(goals[:B]))).cuda()
    q0 = torch.from_numpy(seeds[:B].copy()).cuda()
    lo, hi = (torch.from_numpy(a).cuda() for a in robot.limits_arrays())
    out, ws = _driver_setup(torch, ap, B)
    for v in out.values():
        v.view(torch.int32).fill_(-7)
    before = {k: v.clone() for k, v in out.items()}
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    DEFAULT = object()

    def call(anch=tpl._h, bs=base._h, retries=1, q_lo=lo.data_ptr(), q_hi=hi.data_ptr(), clear_tol=CLEAR_TOL, spread=0.0,
             q_init=DEFAULT, clearance=DEFAULT, attempt=DEFAULT, d_ws=DEFAULT, n=B, pos_tol=POS_TOL):
        opts = _ffi.AnchoredRetryOpts(retries=retries, seed=1, pos_tol=pos_tol, rot_tol=ROT_TOL, d_q_lo=q_lo, d_q_hi=q_hi,
                                      clear_tol=clear_tol, spread=spread)
        pick = lambda v, d: d if v is DEFAULT else v      # noqa: E731
        rc = lib.gik_anchored_ik_batch_retry(anch, bs, T.data_ptr(), pick(q_init, q0.data_ptr()), n, C.byref(opts),
                                             pick(d_ws, ws.data_ptr()), out["Y"].data_ptr(), out["stats"].data_ptr(),
                                             out["q"].data_ptr(), out["pos_err"].data_ptr(), out["rot_err"].data_ptr(),
                                             pick(clearance, out["clearance"].data_ptr()),
                                             pick(attempt, out["attempt"].data_ptr()), C.c_void_p(s.cuda_stream))
        return rc, lib.gik_last_error().decode()

    def untouched():
        torch.cuda.synchronize()
        return all(torch.equal(out[k].view(torch.int32), before[k].view(torch.int32)) for k in out)

    for kw, word in ((dict(retries=64), "retries"), (dict(retries=-1), "retries"), (dict(q_lo=None), "limits"),
                     (dict(q_hi=None), "limits"), (dict(clear_tol=0.0), "clear_tol"), (dict(clear_tol=float("nan")), "clear_tol"),
                     (dict(spread=-0.1), "spread"), (dict(spread=float("nan")), "spread"),
                     (dict(spread=0.1, q_init=None), "d_q_init"), (dict(clearance=None), "d_clearance"),
                     (dict(attempt=None), "d_attempt"), (dict(d_ws=None), "workspace"), (dict(pos_tol=0.0), "positive"),
                     (dict(bs=tpl._h), "pipeline"), (dict(anch=base._h), "fixed-anchor"), (dict(n=-1), "bad argument")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg and "gik_anchored_ik_batch_retry" in msg, (kw, msg)
        assert untouched(), kw
    assert lib.gik_anchored_retry_ws_bytes(base._h, base._h, B) == 0 and lib.gik_anchored_retry_ws_bytes(tpl._h, tpl._h, B) == 0
    # a capturing stream: refused, with and without retries, and the capture stays empty
    hip = _hip_runtime()
    hip.hipStreamBeginCapture.argtypes = [C.c_void_p, C.c_int]
    hip.hipStreamEndCapture.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphDestroy.argtypes = [C.c_void_p]
    assert hip.hipStreamBeginCapture(C.c_void_p(s.cuda_stream), 2) == 0      # hipStreamCaptureModeRelaxed
    rc, msg = call()
    rc0, msg0 = call(retries=0)
    graph_h = C.c_void_p()
    assert hip.hipStreamEndCapture(C.c_void_p(s.cuda_stream), C.byref(graph_h)) == 0
    n_nodes = C.c_size_t(99)
    assert hip.hipGraphGetNodes(graph_h, None, C.byref(n_nodes)) == 0
    hip.hipGraphDestroy(graph_h)
    assert rc != 0 and "capturing" in msg and rc0 != 0 and "capturing" in msg0
    assert n_nodes.value == 0 and untouched()
    # B = 0 returns 0 and queues nothing
    rc, msg = call(n=0)
    assert rc == 0 and untouched()
    r0 = ap.solve(robot.fk_batch(goals[:B])[:0], q_init=seeds[:0], retries=1)
    assert r0["x"].shape == (0, ap.base.N, 3) and r0["attempt"].shape == (0,) and r0["clearance"].shape == (0,)
    # the same call on the same stream, not capturing, runs: the answer of the Python layer
    rc, msg = call(retries=2)
    assert rc == 0, msg
    s.synchronize()
    ref = ap.solve(robot.fk_batch(goals[:B]), q_init=seeds[:B], retries=2, retry_seed=1, **TOL)
    torch.cuda.synchronize()
    assert torch.equal(out["q"], ref["q"]) and torch.equal(out["Y"].reshape(ref["x"].shape), ref["x"])
    assert torch.equal(out["attempt"], ref["attempt"]) and torch.equal(out["clearance"], ref["clearance"])
