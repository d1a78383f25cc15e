"""Goal-aware seeds from a configuration atlas, host side (CPU only): the nearest mirror against a brute-force double loop
on hand-made tables; the atlas of the room of docs/NOTEBOOK.md 46 and its keys; the prepared inputs of that section's
table, pinned; the CPU twin from the nearest row against the blind seed on the first 24 goals; the Python layer's
refusals; and the ABI's new names."""
import functools
import os

import numpy as np
import pytest

from conftest import REPO, make_graph
from test_anchored_screen_host import CLEAR_TOL, FLOOR, RHO, _NoDevice, pi_limits

ATLAS_DRAWS, ATLAS_SEED, ATLAS_ROWS = 32768, 11, 12370      # rows kept of the draws: 37.75 %
GOAL_DRAWS, GOAL_SEED, GOAL_COUNT, GOAL_CLEAR = 4096, 12, 256, 0.01
BLIND_SEED, BLIND_ATTEMPT = 7, 1


def _rs():
    from graphik_amd.solvers import riemannian_solver as rs
    return rs


def brute_nearest(keys, goal_keys, K):
    """The K smallest (d, m) per goal by a double loop over Python floats: the same operations, one pair at a time."""
    G, M, W = len(goal_keys), len(keys), keys.shape[1]
    nbr, dist = np.full((G, K), -1, dtype=np.int32), np.full((G, K), np.inf)
    for g in range(G):
        pairs = []
        for m in range(M):
            d = None
            for c in range(W):
                t = float(goal_keys[g, c]) - float(keys[m, c])
                d = t * t if d is None else d + t * t
            if np.isfinite(d):
                pairs.append((d, m))
        pairs.sort()
        for k, (d, m) in enumerate(pairs[:K]):
            nbr[g, k], dist[g, k] = m, d
    return nbr, dist


def hand_made_table(W, M=40, seed=3):
    """M keys of width W with two identical rows (5 and 17), a NaN row (9), an infinite entry (11) and goals of which
    goal 0 IS row 23 and goal 1 lies at equal distance of the identical rows."""
    rng = np.random.RandomState(seed)
    keys = rng.uniform(-1.0, 1.0, (M, W))
    keys[17] = keys[5]
    keys[9, W - 1] = np.nan
    keys[11, 0] = np.inf
    goals = rng.uniform(-1.0, 1.0, (6, W))
    goals[0] = keys[23]
    goals[1] = keys[5] + 0.01
    return keys, goals


@pytest.mark.parametrize("W", [3, 6])
def test_nearest_mirror_against_a_double_loop(W):
    rs = _rs()
    keys, goals = hand_made_table(W)
    for K in (1, 5, 38, 64):      # (38 rows are finite: K = 64 pads)
        nbr, dist = rs.atlas_nearest_host(keys, goals, K)
        want_n, want_d = brute_nearest(keys, goals, K)
        assert nbr.dtype == np.int32 and np.array_equal(nbr, want_n), K
        assert np.array_equal(dist.view(np.int64), want_d.view(np.int64)), K
        assert 9 not in nbr and 11 not in nbr                                   # a NaN or infinite distance is never listed
    nbr, dist = rs.atlas_nearest_host(keys, goals, 64)
    assert nbr[0, 0] == 23 and dist[0, 0] == 0.0                                # a goal equal to a row: d = 0, first
    where5 = int(np.flatnonzero(nbr[1] == 5)[0])
    assert nbr[1, where5 + 1] == 17 and dist[1, where5] == dist[1, where5 + 1]  # identical rows: the lower index first
    assert np.all(nbr[:, 38:] == -1) and np.all(np.isposinf(dist[:, 38:]))      # K > finite rows: -1 / +inf
    assert np.all(nbr[:, :38] >= 0) and np.all(np.diff(dist[:, :38], axis=1) >= 0)
    # a chunk boundary inside the goals changes nothing
    a = rs.atlas_nearest_host(keys, goals, 5, chunk=4)
    b = rs.atlas_nearest_host(keys, goals, 5, chunk=64)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # M < K
    nbr, dist = rs.atlas_nearest_host(keys[:3], goals, 5)
    assert np.all(nbr[:, 3:] == -1) and sorted(nbr[0, :3].tolist()) == [0, 1, 2]
    with pytest.raises(ValueError, match="1 .. 64"):
        rs.atlas_nearest_host(keys, goals, 65)
    with pytest.raises(ValueError, match="share W"):
        rs.atlas_nearest_host(keys, goals[:, :2], 2)


# ---- the room of NOTEBOOK 46 -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def floor_problem():
    """A host-only UR10 with 3 cm capsules, every pair of links that share no end and a floor at z = -0.1."""
    robot, graph = make_graph("ur10")
    ap = _rs().AnchoredProblem(graph, host_only=True, link_radius=RHO, self_pairs="auto", halfspaces=[FLOOR])
    return robot, ap


@functools.lru_cache(maxsize=None)
def room_atlas():
    robot, ap = floor_problem()
    return ap.seed_atlas(ATLAS_DRAWS, seed=ATLAS_SEED, q_limits=pi_limits(), clearance_mode="links+self", clear_tol=CLEAR_TOL)


@functools.lru_cache(maxsize=None)
def room_goals():
    """(q [256, 6] the configurations the goals were made from, T [256, 4, 4], blind [256, 6] the blind seeds)."""
    rs = _rs()
    robot, ap = floor_problem()
    lo, hi = pi_limits()
    q = rs.retry_seeds_host(GOAL_SEED, np.arange(GOAL_DRAWS), 0, lo, hi)
    q = q[ap.candidate_clearance_host(q, "links+self") >= GOAL_CLEAR][:GOAL_COUNT]
    T = np.stack([np.asarray(robot.pose(robot.array_to_q(row), "p6").as_matrix()) for row in q])
    blind = rs.retry_seeds_host(BLIND_SEED, np.arange(GOAL_COUNT), BLIND_ATTEMPT, lo, hi)
    return q, T, blind


def test_room_atlas_rows_and_keys():
    rs = _rs()
    robot, ap = floor_problem()
    A = room_atlas()
    assert A.count == ATLAS_ROWS == len(A.q) and A.width == 6 and A.keys.shape == (ATLAS_ROWS, 6)
    assert A.d_q is None and A.d_keys is None                                  # host-only: nothing was uploaded
    assert np.all(A.clearance >= -CLEAR_TOL)
    lo, hi = pi_limits()
    draws = rs.retry_seeds_host(ATLAS_SEED, np.arange(ATLAS_DRAWS), 0, lo, hi)
    cl = ap.candidate_clearance_host(draws, "links+self")
    assert np.array_equal(A.q, draws[cl >= -CLEAR_TOL]) and np.array_equal(A.clearance, cl[cl >= -CLEAR_TOL])
    # the key of a row is where the goal of its own FK pose puts the goal nodes
    T = robot.fk_batch(A.q)
    err = np.abs(A.keys - ap.goal_anchors(T)).max()
    print("atlas rows", A.count, "of", ATLAS_DRAWS, "largest |key - goal_anchors(FK)|:", err)
    assert err < 1e-12
    assert np.array_equal(A.keys, ap.base.seed_points(A.q)[:, [14, 15]].reshape(-1, 6))      # UR10: rows 14 and 15
    # the caller's own rows: nothing is filtered unless asked for
    B = rs.SeedAtlas.from_configurations(ap, draws[:100], clearance_mode="links+self")
    assert B.count == 100 and np.array_equal(B.clearance, cl[:100])
    Bc = rs.SeedAtlas.from_configurations(ap, draws[:100], clearance_mode="links+self", keep_clear_only=True)
    assert Bc.count == int((cl[:100] >= -CLEAR_TOL).sum()) < 100


def test_prepared_inputs_of_the_table_are_pinned():
    robot, ap = floor_problem()
    q, T, blind = room_goals()
    assert len(q) == GOAL_COUNT == len(T) and T.shape == (GOAL_COUNT, 4, 4) and blind.shape == (GOAL_COUNT, 6)
    assert np.all(ap.candidate_clearance_host(q, "links+self") >= GOAL_CLEAR)      # a clear answer exists for every goal
    A = room_atlas()
    nbr, dist = _rs().atlas_nearest_host(A.keys, ap.goal_anchors(T), 2)
    assert np.all(nbr >= 0) and np.all(dist[:, 0] <= dist[:, 1])
    med = float(np.median(np.sqrt(dist[:, 0])))
    print("median key distance of the nearest row:", med)
    assert 0.15 < med < 0.30                                                      # (0.23 m in the section's table)


def test_atlas_seeds_mirror_is_the_pick_among_the_ranks():
    rs = _rs()
    robot, ap = floor_problem()
    q, T, blind = room_goals()
    A = room_atlas()
    T = T[:40]
    nbr, _ = rs.atlas_nearest_host(A.keys, ap.goal_anchors(T), 8)
    q1, pick1, cl1 = ap.atlas_seeds_host(T, A, 1, clearance_mode="links+self")
    assert not pick1.any() and np.array_equal(q1, A.q[nbr[:, 0]])                # candidates = 1, first = 0: the nearest row
    q4, pick4, cl4 = ap.atlas_seeds_host(T, A, 4, first=4, clearance_mode="links+self")
    rows, q_c, cl_c = ap.last_atlas
    assert np.array_equal(rows, nbr[:, 4:8].T) and np.array_equal(q_c, A.q[rows])
    assert np.array_equal(pick4, rs.retry_pick_host(cl_c, CLEAR_TOL)) and np.array_equal(q4, q_c[pick4, np.arange(40)])
    # a missing rank is a NaN row: never picked beside a real one, and picked (as 0) only where all are missing
    small = rs.SeedAtlas(A.q[:3], A.keys[:3], A.clearance[:3])
    qs, ps, cs = ap.atlas_seeds_host(T, small, 4, clearance_mode="links+self")
    assert np.all(ap.last_atlas[0][3] == -1) and np.all(ps < 3) and not np.isnan(qs).any()
    qn, pn, cn = ap.atlas_seeds_host(T, small, 2, first=3, clearance_mode="links+self")
    assert np.isnan(qn).all() and not pn.any() and np.isnan(cn).all()


def _full(ap, x, goal_anchor):
    Y = np.zeros((ap.base.N, 3))
    Y[ap.free] = x
    fixed = len(ap.anchors) - ap.n_goal_anchor
    Y[ap.anchors[:fixed]] = ap.anchor_pos[:fixed]
    Y[ap.anchors[fixed:]] = goal_anchor.reshape(-1, 3)
    return Y


def test_twin_from_the_nearest_row_against_the_blind_seed():
    """The first 24 goals of the section's table through the CPU twin (tests/anchored_twin.py, 600 outer iterations at
    the most): converged and clear from the nearest atlas row against the blind seed.  Measured here: 22 against 20 of
    24 (median outer iterations 125 against 267); on all 256 goals the section reports 232 against 192."""
    import anchored_twin as tw
    rs = _rs()
    robot, ap = floor_problem()
    q, T, blind = room_goals()
    A = room_atlas()
    n = 24
    nbr, _ = rs.atlas_nearest_host(A.keys, ap.goal_anchors(T[:n]), 1)

    def good(g, seed):
        ga = ap.goal_anchors(T[g:g + 1])[0]
        r = tw.rtr_numpy(tw.FastTerms(ap, ga), ap.seed_points(seed)[0], maxiter=600, trace_cap=0)
        return bool(r["f"] < 1e-9 and ap.halfspace_clearance(_full(ap, r["x"], ga), links=True)[0] >= -CLEAR_TOL)

    nearest = sum(good(g, A.q[nbr[g, 0]]) for g in range(n))
    blind_ok = sum(good(g, blind[g]) for g in range(n))
    print("converged and clear of", n, "-- nearest atlas row:", nearest, "blind seed:", blind_ok)
    assert nearest >= blind_ok


# ---- refusals, before any device call ----------------------------------------------------------------------------------
def test_atlas_arguments_are_refused_before_any_device_call():
    from graphik_amd.engine import Template, check_atlas_k
    rs = _rs()
    assert check_atlas_k(1, None) == 1 and check_atlas_k(64, 64) == 64 and check_atlas_k(np.int32(8), 100) == 8
    for bad in (0, 65, -1, 2.0, "4", None, True):
        with pytest.raises(ValueError, match="1 .. 64"):
            check_atlas_k(bad, None)
    with pytest.raises(ValueError, match="exceeds"):
        check_atlas_k(5, 4)
    robot, ap = floor_problem()                        # host_only: ap.template is None
    q, T, blind = room_goals()
    T, q0 = T[:2], blind[:2]
    A = room_atlas()
    tiny = rs.SeedAtlas(A.q[:5], A.keys[:5], A.clearance[:5])
    narrow = rs.SeedAtlas(A.q, A.keys[:, :3], A.clearance)      # the key width of a position goal
    cases = ((dict(atlas=A, q_init=q0, retries=1, retry_spread=0.2), "retry_spread"),
             (dict(atlas=A, retries=1, retry_candidates=2), "retry_candidates"),
             (dict(atlas=A, retries=4, atlas_candidates=16), "1 .. 64"),
             (dict(atlas=A, retries=4, atlas_candidates=13), "1 .. 64"),
             (dict(atlas=tiny, retries=2, atlas_candidates=2), "exceeds"),
             (dict(atlas=tiny, atlas_candidates=6), "exceeds"),
             (dict(atlas=A, atlas_candidates=0), "1 .. 16"),
             (dict(atlas=A, atlas_candidates=17), "1 .. 16"),
             (dict(atlas=narrow), "width"),
             (dict(atlas_candidates=2), "needs atlas"))
    for kw, word in cases:
        with pytest.raises(ValueError, match=word):
            ap.solve(T, **kw)
    with pytest.raises(TypeError, match="SeedAtlas"):
        ap.solve(T, atlas=(A.q, A.keys))
    with pytest.raises(ValueError, match="width"):
        ap.atlas_nearest(T, narrow, 2)
    with pytest.raises(ValueError, match="1 .. 64"):
        ap.atlas_nearest(T, A, 65)
    with pytest.raises(ValueError, match="1 .. 64"):
        ap.atlas_seeds_host(T, A, 16, first=49)
    with pytest.raises(ValueError, match="empty"):
        rs.SeedAtlas(A.q[:0], A.keys[:0], A.clearance[:0])
    with pytest.raises(ValueError, match="size"):
        ap.seed_atlas(0)
    # the engine's own checks, with a device stand-in that fails on any use
    tpl = Template.__new__(Template)
    tpl.anchored = True
    base = _NoDevice()
    base.__dict__["has_pipeline"] = True
    base.__dict__["atlas_key_width"] = lambda: 6
    try:
        for kw, word in ((dict(atlas=A, retries=1, retry_spread=0.2), "retry_spread"),
                         (dict(atlas=A, retries=1, retry_candidates=2, q_limits=robot.limits_arrays()), "retry_candidates"),
                         (dict(atlas=A, retries=4, atlas_candidates=16), "1 .. 64"),
                         (dict(atlas=tiny, retries=2, atlas_candidates=2), "exceeds"),
                         (dict(atlas=narrow), "width")):
            with pytest.raises(ValueError, match=word):
                Template.anchored_ik(tpl, base, T, **kw)
    finally:
        tpl.__dict__.clear()      # (nothing for __del__ to free)


def test_atlas_refusals_keep_their_texts_and_each_callers_order():
    """engine.check_atlas_args behind AnchoredProblem.solve and Template.anchored_ik: the whole text of each ValueError, and
    with two faults at once the one each caller has always raised first -- solve: the key width, retry_spread,
    retry_candidates, K; anchored_ik: retry_candidates, retry_spread, K, the key width."""
    import re
    from graphik_amd.engine import Template
    rs = _rs()
    robot, ap = floor_problem()
    T, q0 = room_goals()[1][:2], room_goals()[2][:2]
    A = room_atlas()
    tiny = rs.SeedAtlas(A.q[:5], A.keys[:5], A.clearance[:5])
    narrow_tiny = rs.SeedAtlas(A.q[:5], A.keys[:5, :3], A.clearance[:5])
    spread = "atlas= with retry_spread > 0 is not supported: the restarts take atlas rows, not draws around q_init"
    draws = "atlas= with retry_candidates > 1 is not supported: the restarts take atlas rows, not draws"
    rows = "(retries + 1) * atlas_candidates = 6 exceeds the atlas's 5 rows"
    both = dict(q_init=q0, retries=1, retry_spread=0.2, retry_candidates=2)
    many = dict(retries=2, atlas_candidates=2)
    tpl = Template.__new__(Template)
    tpl.anchored = True
    base = _NoDevice()
    base.__dict__.update(has_pipeline=True, atlas_key_width=lambda: 6)
    lim = dict(q_limits=robot.limits_arrays())
    try:
        for call, kw, text in (
                (ap.solve, dict(atlas=A, q_init=q0, retries=1, retry_spread=0.2), spread),
                (ap.solve, dict(atlas=A, retries=1, retry_candidates=2), draws),
                (ap.solve, dict(atlas=tiny, **many), rows),
                (ap.solve, dict(atlas=A, **both), spread),
                (ap.solve, dict(atlas=tiny, q_init=q0, retry_spread=0.2, **many), spread),
                (ap.solve, dict(atlas=tiny, retry_candidates=2, **many), draws),
                (ap.solve, dict(atlas=narrow_tiny, **many), "the atlas has keys of width 3, this problem's goals have 6"),
                (lambda T, **kw: Template.anchored_ik(tpl, base, T, **kw), dict(atlas=A, **both, **lim), draws),
                (lambda T, **kw: Template.anchored_ik(tpl, base, T, **kw), dict(atlas=tiny, q_init=q0, retry_spread=0.2, **many), spread),
                (lambda T, **kw: Template.anchored_ik(tpl, base, T, **kw), dict(atlas=tiny, retry_candidates=2, **many, **lim), draws),
                (lambda T, **kw: Template.anchored_ik(tpl, base, T, **kw), dict(atlas=narrow_tiny, **many), rows),
                (lambda T, **kw: Template.anchored_ik(tpl, base, T, **kw), dict(atlas=narrow_tiny),
                 "the atlas has keys of width 3, the base template's goals have 6")):
            with pytest.raises(ValueError, match="^" + re.escape(text) + "$"):
                call(T, **kw)
    finally:
        tpl.__dict__.clear()      # (nothing for __del__ to free)


def test_abi_carries_the_atlas_entry_points():
    from graphik_amd import _ffi, build
    for name in ("gik_atlas_nearest", "gik_anchored_atlas_seeds", "gik_anchored_atlas_seeds_ws_bytes",
                 "gik_anchored_ik_batch_atlas", "gik_anchored_ik_batch_atlas_ws_bytes", "gik_anchored_atlas_picks"):
        assert name in _ffi.SYMBOLS
    assert _ffi.ABI_VERSION == 12
    hdr = open(os.path.join(REPO, "include", "graphik_amd.h")).read()
    assert "#define GIK_ABI_VERSION 12" in hdr and "#define GIK_ATLAS_MAX_NEIGHBOURS 64" in hdr
    assert build.SOURCES.index("gik_k_atlas.hip") < build.SOURCES.index("gik_host_anch.hip")
    # the new kernel header stays clear of the prepare family: the goal key's three lines are restated in it
    text = open(os.path.join(REPO, "graphik_amd", "csrc", "gik_atlas.hip.h")).read()
    assert "gik_goal.hip.h" not in text and "gik_retry.hip.h" not in text
