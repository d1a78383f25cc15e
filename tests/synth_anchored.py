"""Seeded synthetic fixed-anchor problems at the compiled limits of the anchored wavefront kernels
(rtr_wave_kernel<3, 9 | 20, W_THETA1 | W_ANCH>, kat_wave_kernel<3, 9 | 20, W_ANCH>): 21 free nodes, 16 anchor rows, 8 pinned
terms at a node, 128 obstacles, 8 / 9 spheres on a near list, and the shapes gik_template_create_anchored refuses.

Plain module (numpy only at import), the anchored sibling of tests/synth_graphs.py: tests/test_anchored_limits_host.py
re-derives every count from what build() returns, tests/test_anchored_limits_gpu.py launches the same problems, and
synth_graphs.coverage() reads CASES for the kernels they reach.

A problem is B = 8 goals on one template.  A hidden point set P_b (0.5 randn) satisfies every term of goal b exactly:
equality targets are P's squared distances, lower thresholds those times U(0.4, 0.8), upper ones times U(1.25, 2.0)
(of the smallest / largest distance over the 8 goals, where a goal moves one end of the term).
  free-free   a chain through the free nodes and a hub with an exact term count (kinds EQ, LOWER, UPPER per pair)
  pinned      every node has three equality pins to distinct anchor rows; one node (pins_node) has exactly `pins`
              terms of all three kinds
  obstacles   spheres (c, r), every point of every P_b at least 4 mm outside; obs_node_mask leaves off_node out
  goals       the tip group (the last three chain nodes) is pinned to the two goal rows and to constant row 0, tied to
              each other by equalities and to the body by hinges only; goal b turns tip group and goal rows about
              anchor row 0 by at most 0.1 rad, which keeps every equality exact.  Where every anchor row is a goal row
              (a9_allgoal, a_min) the whole of P and all rows move by one rigid motion (<= 0.1 rad, shift <= 0.05).
"""
import functools
import types

import numpy as np

from synth_graphs import EQ, LOWER, UPPER, _Terms, _by_distance, _fill_hub

B = 8
NEAR_TAU = 0.05                 # WaveCtx::OBS_TAU: a sphere within 5 cm of a node goes on its near list
MIN_CLEAR = 0.004               # every hidden point is at least this far outside every sphere
NEAR_BAND = (0.006, 0.02)       # clearance of a sphere placed on a near list ...
FAR_CLEAR = 0.09                # ... and of every other sphere at the nodes whose lists are counted


def _solve9():
    return ["rtr_wave_kernel<3,9,W_THETA1|W_ANCH>", "kat_wave_kernel<3,9,W_ANCH>"]


def _solve20():
    return ["rtr_wave_kernel<3,20,W_THETA1|W_ANCH>", "kat_wave_kernel<3,20,W_ANCH>"]


# id -> shape.  N free nodes, `busiest` free-free terms at the hub, n_anchor rows of which the last n_goal are per-goal,
# `pins` pinned terms at pins_node, n_obs spheres; slots: the compiled slot count the template must report.
# seed: the graph's (default 0); sigma: spread of the start points around P (default 0.15).
CASES = {
    "a9_full": dict(N=21, busiest=9, n_anchor=16, n_goal=2, pins=8, n_obs=128, slots=9, reaches=_solve9()),
    "a9_allgoal": dict(N=21, busiest=9, n_anchor=16, n_goal=16, pins=8, n_obs=128, slots=9, reaches=_solve9()),
    "a9_noobs": dict(N=12, busiest=9, n_anchor=6, n_goal=2, pins=8, n_obs=0, slots=9, reaches=_solve9()),
    "a10": dict(N=21, busiest=10, n_anchor=16, n_goal=2, pins=8, n_obs=128, slots=20, reaches=_solve20()),
    "a20_full": dict(N=21, busiest=20, n_anchor=16, n_goal=2, pins=8, n_obs=128, slots=20, reaches=_solve20()),
    "a_min": dict(N=2, busiest=1, n_anchor=1, n_goal=1, pins=3, n_obs=1, slots=9, reaches=_solve9()),
    "near8": dict(N=12, busiest=9, n_anchor=6, n_goal=2, pins=3, n_obs=128, slots=9, reaches=_solve9(), near=8, sigma=0.01),
    "near9": dict(N=12, busiest=9, n_anchor=6, n_goal=2, pins=3, n_obs=128, slots=9, reaches=_solve9(), near=9, sigma=0.01),
    "crossing": dict(N=12, busiest=9, n_anchor=6, n_goal=2, pins=3, n_obs=16, slots=9, reaches=_solve9(), crossing=True),
}
SOLVE_CASES = sorted(CASES)                 # every case is solved
NEAR_LIST_CASES = ["near8", "near9", "crossing", "a20_full"]
# near lists: sphere indices placed next to near_node (ascending: list position = rank) and next to near_node2
NEAR_IDX = {8: [5, 20, 40, 60, 80, 100, 120, 127], 9: [5, 20, 40, 60, 80, 100, 120, 121, 127]}
NEAR2_IDX = [10, 50, 90, 127]               # 127 in list position 3 (byte 3 of idx[0]); at near_node in position 7


def _rot(rng, max_angle):
    """A rotation by U(0.5, 1) * max_angle about a random axis (Rodrigues)."""
    u = rng.randn(3)
    u /= np.linalg.norm(u)
    a = max_angle * rng.uniform(0.5, 1.0)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * (K @ K)


def clearance(points, obs):
    """[..., 3] points against spheres [n, 4] (c, r) -> [..., n] distances to the surfaces (negative: inside)."""
    points = np.asarray(points)
    return np.linalg.norm(points[..., None, :] - obs[:, :3], axis=-1) - obs[:, 3]


def _unit(rng):
    u = rng.randn(3)
    return u / np.linalg.norm(u)


def _place_obstacles(rng, c, P, tight):
    """n_obs spheres, every point of P [B, N, 3] at least MIN_CLEAR outside each.  tight: nodes whose near lists are
    counted -- every sphere that is not placed on their list stays FAR_CLEAR away from them."""
    n_obs = c["n_obs"]
    obs = np.zeros((n_obs, 4))
    special = {}
    flat = P.reshape(-1, 3)

    def ok(s, skip=()):
        if (np.linalg.norm(flat - s[:3], axis=1) - s[3]).min() <= MIN_CLEAR:
            return False
        pts = np.array([p for t in tight if t not in skip for p in P[:, t]]).reshape(-1, 3)
        return len(pts) == 0 or (np.linalg.norm(pts - s[:3], axis=1) - s[3]).min() > FAR_CLEAR

    def next_to(node, skip):
        for _ in range(10000):
            r = rng.uniform(0.05, 0.15)
            s = np.array([*(P[0, node] + _unit(rng) * (r + rng.uniform(*NEAR_BAND))), r])
            if ok(s, skip):
                return s
        raise AssertionError("no room for a near sphere")

    if c.get("near"):
        a, b2 = tight
        for k in NEAR_IDX[c["near"]][:-1]:
            special[k] = next_to(a, (a,))
        for k in NEAR2_IDX[:-1]:
            special[k] = next_to(b2, (b2,))
        # sphere 127 next to both: centre on the bisector plane of the two nodes
        mid, half = 0.5 * (P[0, a] + P[0, b2]), 0.5 * (P[0, a] - P[0, b2])
        for _ in range(100000):
            n = np.cross(half, rng.randn(3))
            n /= np.linalg.norm(n)
            t = rng.uniform(-0.6, 0.6)
            s = np.array([*(mid + t * n), np.sqrt(half @ half + t * t) - rng.uniform(*NEAR_BAND)])
            if ok(s, (a, b2)):
                special[127] = s
                break
        assert 127 in special, "no room for the shared sphere"
    if c.get("crossing"):
        # sphere n_obs - 1 lies on the way of cross_node: 1 cm behind its P row, radius 0.15 (start_points puts the
        # node's start row 0.5 along the same direction: 0.19 clear of the sphere, the midpoint inside it)
        node = tight[0]
        for _ in range(10000):
            u = _unit(rng)
            s = np.array([*(P[0, node] + u * (0.15 + 0.01)), 0.15])
            if (np.linalg.norm(flat - s[:3], axis=1) - s[3]).min() > MIN_CLEAR:
                special[n_obs - 1] = s
                special["dir"] = u
                break
        assert n_obs - 1 in special
    for k in range(n_obs):
        if k in special:
            obs[k] = special[k]
            continue
        for _ in range(10000):
            s = np.array([*(1.2 * rng.randn(3)), rng.uniform(0.05, 0.2)])
            if ok(s):
                obs[k] = s
                break
        else:
            raise AssertionError("no room for a sphere")
    return obs, special.get("dir")


@functools.lru_cache(maxsize=None)
def build(cid):
    """The problem of a case: a namespace with
      N, ti, tj, tk, target          free-free terms in engine.build_terms' order (row-major pairs; EQ, LOWER, UPPER)
      omega, psi_L, psi_U, D         the same as dense matrices (what oracle.c_oracle.rtr_solve_anchored takes)
      anchor_pos [A, 3], n_goal      constant rows (goal rows: zero), goal [B, 3 n_goal] the goal rows of every problem
      pins                           (node, row, kind, squared target), by node, row, kind
      obs [n_obs, 4] (c, r), mask    spheres and obs_node_mask
      P [B, N, 3]                    the hidden points
      hub, pins_node, off_node, tips, near_node, near_node2, cross_node, cross_sphere
    Arrays are shared between callers: do not write to them."""
    c = CASES[cid]
    N, A, ng = c["N"], c["n_anchor"], c["n_goal"]
    rng = np.random.RandomState(c.get("seed", 0) + 7919 * sorted(CASES).index(cid))
    P0 = 0.5 * rng.randn(N, 3)
    anchors = 0.7 * rng.randn(A, 3)
    all_goal = ng == A
    tips = [] if all_goal else list(range(N - 3, N))
    nc = A - ng                                     # constant rows
    tm = _Terms(N)
    for v in range(1, N):
        if tips and v == tips[0]:                   # body -- tip group: hinges only
            tm.add(v - 1, v, LOWER)
            tm.add(v - 1, v, UPPER)
        else:
            tm.add(v - 1, v, EQ)
    hub = N // 2
    assert hub not in tips
    _fill_hub(tm, hub, c["busiest"], [v for v in _by_distance(hub, N) if v not in tips], cap=c["busiest"])
    # the B hidden point sets and goal rows
    P = np.repeat(P0[None], B, axis=0)
    goal = np.zeros((B, ng, 3))
    for b in range(B):
        R = np.eye(3) if b == 0 else _rot(rng, 0.1)
        if all_goal:
            shift = np.zeros(3) if b == 0 else 0.05 * rng.uniform(0.5, 1.0) * _unit(rng)
            P[b] = P0 @ R.T + shift
            goal[b] = anchors @ R.T + shift
        else:
            pivot = anchors[0]
            P[b, tips] = (P0[tips] - pivot) @ R.T + pivot
            goal[b] = (anchors[nc:] - pivot) @ R.T + pivot
    # pinned terms
    pin_set = {}
    for i in range(N):
        if all_goal:
            rows = [0] if A == 1 else [(3 * i + j) % A for j in range(3)]
        elif i in tips:
            rows = [0, nc, nc + 1]
        else:
            rows = [(3 * i + j) % nc for j in range(3)]
        for r in rows:
            pin_set[(i, r, EQ)] = None
    pins_node = 1 if N > 2 else None
    pool = list(range(A)) if all_goal else list(range(nc))
    if A == 1:                                      # a_min: the three kinds to the one row, at each node
        for i in range(N):
            pin_set[(i, 0, LOWER)] = pin_set[(i, 0, UPPER)] = None
    else:
        eq_rows = [r for (i, r, k) in pin_set if i == pins_node]
        order = [r for r in pool if r not in eq_rows] + eq_rows
        cand = [(r, (LOWER, UPPER)[q % 2]) for q, r in enumerate(order)] + [(r, (UPPER, LOWER)[q % 2]) for q, r in enumerate(order)]
        for r, kind in cand[:c["pins"] - 3]:
            pin_set[(pins_node, r, kind)] = None
    # thresholds: below the smallest / above the largest squared distance over the B hidden point sets (a term between
    # two points that goal b does not move, or moves together, has one distance: that of P_0)
    rows = np.repeat(anchors[None], B, axis=0)
    rows[:, nc:] = goal

    def threshold(d, kind):
        if kind == EQ:
            assert d.max() - d.min() <= 1e-14 * d.max()
            return float(d[0])
        return float(d.min() * rng.uniform(0.4, 0.8) if kind == LOWER else d.max() * rng.uniform(1.25, 2.0))
    pins = [(i, r, kind, threshold(((P[:, i] - rows[:, r]) ** 2).sum(-1), kind)) for (i, r, kind) in sorted(pin_set)]
    # free-free terms: dense matrices and the list in build_terms' order
    Dp = ((P[:, :, None] - P[:, None]) ** 2).sum(-1)           # [B, N, N]
    om, pL, pU, D = (np.zeros((N, N)) for _ in range(4))
    ti, tj, tk, target = [], [], [], []
    for (i, j) in sorted(tm.kinds):
        for kind in sorted(tm.kinds[(i, j)]):
            t = threshold(Dp[:, i, j], kind)
            if kind == EQ:
                om[i, j] = om[j, i] = 1.0
                D[i, j] = D[j, i] = t
            elif kind == LOWER:
                pL[i, j] = pL[j, i] = t
            else:
                pU[i, j] = pU[j, i] = t
            ti.append(i); tj.append(j); tk.append(kind); target.append(t)
    # obstacles
    off_node = 3 if N > 3 else N - 1
    mask = np.ones(N, dtype=np.int32)
    mask[off_node] = 0
    near_node = near_node2 = cross_node = cross_sphere = cross_dir = None
    tight = []
    if c.get("near"):
        body = [v for v in range(N) if v not in tips and v != off_node]      # the closest pair of masked body nodes
        _, near_node, near_node2 = min((Dp[0, a, b2], a, b2) for a in body for b2 in body if a < b2)
        tight = [near_node, near_node2]
    if c.get("crossing"):
        cross_node, cross_sphere = 4, c["n_obs"] - 1
        tight = [cross_node]
    obs, cross_dir = _place_obstacles(rng, c, P, tight) if c["n_obs"] else (np.zeros((0, 4)), None)
    anchor_pos = anchors.copy()
    anchor_pos[nc:] = 0.0
    for a in (P, goal, anchor_pos, obs, mask, om, pL, pU, D):
        a.setflags(write=False)
    return types.SimpleNamespace(
        cid=cid, N=N, ti=np.array(ti, dtype=np.int32), tj=np.array(tj, dtype=np.int32), tk=np.array(tk, dtype=np.int32),
        target=np.array(target), omega=om, psi_L=pL, psi_U=pU, D=D, anchor_pos=anchor_pos, n_anchor=A, n_goal=ng,
        goal=goal.reshape(B, 3 * ng), pins=pins, obs=obs, mask=mask, P=P, hub=hub, pins_node=pins_node, off_node=off_node,
        tips=tips, near_node=near_node, near_node2=near_node2, cross_node=cross_node, cross_sphere=cross_sphere,
        cross_dir=cross_dir, sigma=c.get("sigma", 0.15))


def anchored_desc(p):
    """The `anchored=` dict of engine.Template for a problem of build() (obs as (x, y, z, r^2)); the full point matrix
    is the free rows followed by the anchor rows."""
    obs = p.obs.copy()
    obs[:, 3] = obs[:, 3] ** 2
    return dict(anchor_pos=p.anchor_pos, n_goal_anchor=p.n_goal, term_target=p.target,
                pin_node=[q[0] for q in p.pins], pin_anchor=[q[1] for q in p.pins], pin_kind=[q[2] for q in p.pins],
                pin_target=[q[3] for q in p.pins], obs=obs.reshape(-1, 4), obs_node_mask=p.mask, full_N=p.N + p.n_anchor,
                free_full_index=list(range(p.N)), anchor_full_index=list(range(p.N, p.N + p.n_anchor)), axis_length=1.0)


def free_terms(p):
    """(i, j, kind, target) of the free-free terms."""
    return p.ti, p.tj, p.tk, p.target


def row_positions(p, b):
    """[A, 3] anchor rows of problem b: the constant rows, then its goal rows."""
    pos = np.array(p.anchor_pos)
    pos[p.n_anchor - p.n_goal:] = p.goal[b].reshape(-1, 3)
    return pos


def anchor_terms(p, b):
    """Point-to-anchor terms (node, position, squared target, kind) of problem b: the pinned terms, then one lower
    hinge per (masked node, obstacle) -- the order of parity_util.anchored_terms."""
    pos_tab = row_positions(p, b)
    node = [q[0] for q in p.pins]
    pos = [pos_tab[q[1]] for q in p.pins]
    kind = [q[2] for q in p.pins]
    tgt = [q[3] for q in p.pins]
    for i in np.nonzero(p.mask)[0]:
        for o in p.obs:
            node.append(int(i)); pos.append(o[:3]); tgt.append(o[3] ** 2); kind.append(LOWER)
    return (np.array(node, dtype=np.int32), np.array(pos).reshape(-1, 3), np.array(tgt), np.array(kind, dtype=np.int32))


# start points and known-answer points.  The seeds are per problem: a start point that fails a condition of
# tests/test_anchored_limits_host.py is replaced there (Y0_SEEDS), never excused on the GPU.
# (cid, b) -> seed, where the start point of the default 1000 + b failed a condition (the first of 1000 + b + 8 t that
# meets them all; for most of these the twin did not reproduce its own first iterations under another summation order)
Y0_SEEDS = {("a9_full", 2): 1026, ("a9_full", 3): 1011, ("a9_full", 4): 1020, ("a9_full", 5): 1013, ("a9_full", 6): 1014,
            ("a9_full", 7): 1023, ("a_min", 0): 1064, ("a_min", 1): 1033, ("a_min", 2): 1058, ("a_min", 3): 1075,
            ("a_min", 4): 1044, ("a_min", 5): 1061, ("a_min", 6): 1230, ("a_min", 7): 1087, ("near8", 0): 1008,
            ("near8", 2): 1010, ("near9", 0): 1008, ("near9", 1): 1017, ("near9", 3): 1019, ("near9", 4): 1012,
            ("near9", 5): 1013}
# cid -> seed, where under the default 0 a class of terms had no active or no inactive member (test_known_answer_points_...)
KAT_SEEDS = {"a9_full": 1, "a9_noobs": 22, "a_min": 1560}


def start_points(cid):
    """Y0 [B, N, 3] = P_b + sigma randn (0.15; the near cases 0.01).  crossing: cross_node's row is put 0.5 from its P
    row, behind cross_sphere."""
    p = build(cid)
    Y0 = np.array(p.P)
    for b in range(B):
        rng = np.random.RandomState(Y0_SEEDS.get((cid, b), 1000 + b))
        Y0[b] += p.sigma * rng.randn(p.N, 3)
        if p.cross_node is not None:
            Y0[b, p.cross_node] = p.P[b, p.cross_node] + 0.5 * p.cross_dir
    return Y0


def known_answer_points(cid):
    """(Y, W) [B, N, 3]: Y = P_b + 0.07 randn, about half of the masked nodes moved onto a sphere's surface +- 2 cm
    (next to it or inside); W = randn."""
    p = build(cid)
    rng = np.random.RandomState(KAT_SEEDS.get(cid, 0) + 31)
    Y = p.P + 0.07 * rng.randn(B, p.N, 3)
    for b in range(B):
        for i in np.nonzero(p.mask)[0]:
            if len(p.obs) and rng.rand() < 0.5:
                o = p.obs[rng.randint(len(p.obs))]
                Y[b, i] = o[:3] + _unit(rng) * (o[3] + 0.02 * rng.randn())
    W = rng.randn(B, p.N, 3)
    return Y, W


# ---- refused shapes: (N, term_i, term_j, term_kind, anchored dict, a phrase of gik_host.hip's message) -------------
def _small(N=6, n_anchor=3, n_goal=1, n_obs=2, hub_terms=None):
    rng = np.random.RandomState(5)
    tm = _Terms(N)
    for v in range(1, N):
        tm.add(v - 1, v, EQ)
    if hub_terms:
        _fill_hub(tm, N // 2, hub_terms, _by_distance(N // 2, N), cap=hub_terms)
    ti, tj, tk = [], [], []
    for (i, j) in sorted(tm.kinds):
        for kind in sorted(tm.kinds[(i, j)]):
            ti.append(i); tj.append(j); tk.append(kind)
    obs = np.concatenate([3.0 + rng.rand(n_obs, 3), np.full((n_obs, 1), 0.01)], axis=1)
    pin_node = [i for i in range(N) for _ in range(min(3, n_anchor))]
    pin_anchor = [r for i in range(N) for r in range(min(3, n_anchor))]
    desc = dict(anchor_pos=rng.randn(n_anchor, 3), n_goal_anchor=n_goal, term_target=np.ones(len(ti)),
                pin_node=pin_node, pin_anchor=pin_anchor, pin_kind=[EQ] * len(pin_node), pin_target=[1.0] * len(pin_node),
                obs=obs, obs_node_mask=np.ones(N, dtype=np.int32), full_N=N + n_anchor, free_full_index=list(range(N)),
                anchor_full_index=list(range(N, N + n_anchor)), axis_length=1.0)
    return [N, np.array(ti, dtype=np.int32), np.array(tj, dtype=np.int32), np.array(tk, dtype=np.int32), desc]


def _with_pins(shape, extra):
    d = shape[4]
    for node, row, kind in extra:
        d["pin_node"] = d["pin_node"] + [node]
        d["pin_anchor"] = d["pin_anchor"] + [row]
        d["pin_kind"] = d["pin_kind"] + [kind]
        d["pin_target"] = d["pin_target"] + [1.0]
    return shape


REFUSED = {
    "r_n22": (lambda: _small(N=22), "N \\* k <= 64 free unknowns"),
    "r_busiest21": (lambda: _small(N=12, hub_terms=21), "at most 20 terms per node"),
    "r_anchors17": (lambda: _small(n_anchor=17), "1 <= n_anchor <= 16"),
    "r_goal_beyond_anchors": (lambda: _small(n_anchor=3, n_goal=4), "goal anchors are the last rows"),
    "r_obs129": (lambda: _small(n_obs=129), "at most 128 obstacles"),
    # node 0 has three pins already: six more make nine
    "r_pins9": (lambda: _with_pins(_small(n_anchor=3), [(0, r, k) for r in range(3) for k in (LOWER, UPPER)]),
                "more than 8 per node"),
    "r_pin_row": (lambda: _with_pins(_small(n_anchor=3), [(1, 3, EQ)]), "bad pinned term"),
}


def refused(rid):
    make, match = REFUSED[rid]
    return make(), match
