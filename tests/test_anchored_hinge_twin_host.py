"""The solve loop of the hinge builds, host side (CPU only): the numpy trust-region twin of tests/anchored_twin.py against
the C twin on problems without hinges (which makes it a reference), the case table of the six hinge builds with every
condition on its start points, and three planted faults that the pinned prefixes must see.
tests/test_anchored_hinge_twin_gpu.py compares the device with this twin on the same cases and excuses no seed."""
import functools

import numpy as np
import pytest

import anchored_twin as at
import synth_anchored as sa
from conftest import make_graph
from parity_util import CONTRACT_RTOL, anchored_terms, first_divergence, report
from test_anchored_halfspaces_gpu import _eight
from test_anchored_halfspaces_host import FLOOR, WALL, point_margins

B = 8
RHO = 0.03
TWIN_MAXITER = 6            # outer iterations the twin runs: the pinned prefix is at most 4
PREFIX = 4                  # outer iterations pinned on the device: min(PREFIX, n, stable_prefix)
STABLE_RTOL = 1e-9          # ten times below the 1e-8 at which the device is compared with the twin
STABLE_WANT = 3
N_RENDERINGS = 5            # renderings of the mirrors' own sum: start point + 1e-15 randn, the shares in alternating order
N_FAST = 48                 # ... and of anchored_twin.FastTerms, the same jitter: a decision that flips in one rendering
#                             of five (measured on three seeds: 5 to 7 of 24) is missed by five with probability 0.3 and
#                             by these with 2e-5
HINGE_SHARE = 0.1           # the hinge shares' part of f at the start point, at least


def _rs():
    from graphik_amd.solvers import riemannian_solver as rs
    return rs


# ---- the case table ----------------------------------------------------------------------------------------------------
# build: what the template must report as info["anchored"] (1 + 2 links + 4 self + 8 half-spaces).  stream: the
# RandomState seed of the joint angles uniform(-pi, pi, (n, 6)) the start points are drawn from -- 7: the stream of
# test_anchored_halfspaces_host.blind_spot_sample, 0: that of test_anchored_self_hinges_host.hinge_configurations -- and n
# its length (the rarer a case's candidates, the longer).  Every goal is its seed's own pose.
# sigma: the start point is the seed's own point matrix + sigma randn (RandomState(g) for row g).  From the configuration
# itself (sigma 0) f is the hinge shares alone, and where those are small -- a capsule of 3 cm is at most 3.6e-3 inside
# another in squared metres -- the full step is rejected three or four times before the radius is down to the millimetres
# the hinges act on: the four pinned iterations would hold no accepted point.  A millimetre of noise gives the first step
# something to win, and the hinge shares stay above the 10 % the conditions ask for.
# main: the families that must act at a row of sub-stream A (default: all the case carries).  UR10 cannot reach through
# the table's first row of spheres (z = 0.95) with a joint under the floor (z = -0.1), so half_links takes its floor rows
# from A and its link rows from B.
_INACTIVE6 = [[*p[:3], -5.0] for p in _eight()[:6]]      # _eight()'s normals, 5 m the other way: never active
CASES = {
    "half": dict(build=9, stream=7, n=2048, sigma=0.0, limit=(24, 160), kw=dict(halfspaces=[list(FLOOR)], halfspace_margin=0.0)),
    "half8": dict(build=9, stream=7, n=2048, sigma=0.0, limit=(24, 160),
                  kw=dict(halfspaces=[list(FLOOR), list(WALL)] + _INACTIVE6, halfspace_margin="points")),
    "half_links": dict(build=11, stream=7, n=1 << 18, sigma=0.001, limit=(24, 96), spheres=8, main=("half",),
                       kw=dict(halfspaces=[list(FLOOR)], link_radius=RHO, link_hinges=True)),
    "links": dict(build=3, stream=0, n=1 << 17, sigma=0.001, limit=(48, 48), spheres=8, kw=dict(link_radius=RHO, link_hinges=True)),
    "self": dict(build=5, stream=0, n=1 << 15, sigma=0.0005, limit=(64, 48), kw=dict(link_radius=RHO, self_pairs="auto", self_hinges=True)),
    "self_links": dict(build=7, stream=0, n=1 << 18, sigma=0.0005, limit=(80, 48), spheres=8,
                       kw=dict(link_radius=RHO, self_pairs="auto", self_hinges=True, link_hinges=True)),
}
FOOT_CASES = ("links", "self", "self_links")      # a foot parameter must be seen moving

# case -> the rows of its stream that are its eight start points, four of either sub-stream of candidates() (half_links:
# five and three): the first of A that meet every per-problem condition of start_point_faults, and the first of B that do
# and hold an accepted point with a changed active set inside their pinned prefix as well.  A row that fails a condition
# is replaced by the next one of its sub-stream here, never excused on the GPU (the rule of synth_anchored.Y0_SEEDS).
SEEDS = {
    "half": dict(A=(15, 19, 26, 46), B=(325, 602, 637, 660)),
    "half8": dict(A=(15, 26, 53, 56), B=(141, 214, 325, 378)),
    "half_links": dict(A=(15, 19, 21, 26, 46), B=(59147, 67359, 107060)),
    "links": dict(A=(651, 742, 1629, 1700), B=(42361, 66842, 74761, 89518)),
    "self": dict(A=(182, 262, 411, 542), B=(6075, 9977, 11637, 14364)),
    "self_links": dict(A=(40538, 103725, 158301, 163784), B=(6075, 9977, 11637, 14364)),
}
# what stable_prefix() gives for the rows of seeds(case) (renderings run four iterations, so 4 is "all of them"):
# test_start_points_meet_every_condition holds the table to the function, the GPU file reads the table and runs one twin
# solve per problem, not six
STABLE = {
    "half": (4, 4, 3, 4, 4, 4, 4, 4),
    "half8": (4, 3, 4, 4, 4, 4, 4, 4),
    "half_links": (4, 4, 4, 4, 4, 4, 3, 4),
    "links": (4, 4, 4, 4, 3, 4, 4, 3),
    "self": (4, 4, 3, 3, 4, 4, 4, 4),
    "self_links": (4, 4, 4, 4, 4, 4, 4, 4),
}


def seeds(case):
    """The eight rows of a case: A's, then B's."""
    return tuple(SEEDS[case]["A"]) + tuple(SEEDS[case]["B"])


@functools.lru_cache(maxsize=None)
def problem(case, host_only=True, maxiter=None):
    """(robot, graph, AnchoredProblem) of a case on UR10; maxiter: the device template's outer-iteration cap."""
    from graphik_amd.utils import table_environment
    c = CASES[case]
    robot, graph = make_graph("ur10")
    for idx, (centre, r) in enumerate(list(table_environment())[:c.get("spheres", 0)]):
        graph.add_spherical_obstacle(f"o{idx}", np.asarray(centre, dtype=float), float(r))
    kw = dict(c["kw"])
    if kw.get("halfspace_margin") == "points":
        kw["halfspace_margin"] = point_margins(_rs().AnchoredProblem(make_graph("ur10")[1], host_only=True)).tolist()
    ap = _rs().AnchoredProblem(graph, host_only=host_only, params=None if maxiter is None else {"maxiter": int(maxiter)}, **kw)
    return robot, graph, ap


@functools.lru_cache(maxsize=None)
def _angles(case):
    c = CASES[case]
    q = np.random.RandomState(c["stream"]).uniform(-np.pi, np.pi, (c["n"], 6))
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=None)
def start(case, g):
    """(Y0 [Nf, 3], goal anchors) of row g of the case's stream: the goal is the row's own pose, the start point its own
    point matrix + sigma randn."""
    robot, graph, ap = problem(case)
    q = _angles(case)[g:g + 1]
    Y0, ga = ap.seed_points(q)[0], ap.goal_anchors(robot.fk_batch(q))[0]
    if CASES[case]["sigma"]:
        Y0 = Y0 + CASES[case]["sigma"] * np.random.RandomState(g).randn(*Y0.shape)
    Y0.setflags(write=False)
    ga.setflags(write=False)
    return Y0, ga


def hinge_state(case, Y, ga):
    """The hinge state of a point (anchored_twin.HingeTerms.last_state)."""
    t = at.HingeTerms(problem(case)[2], ga)
    t(Y, np.zeros_like(Y))
    return t.last_state


CHUNK = 1 << 16


@functools.lru_cache(maxsize=None)
def candidates(case):
    """{"A": rows, "B": rows}: the first rows (CASES[case]["limit"] of either) of the two sub-streams of the case's stream,
    in stream order.  At every row no joint point p1 .. p5 is inside a sphere (a capsule passes through one between two of
    them), and with half-spaces the goal rows are more than 5 cm inside every plane's allowed side (blind_spot_sample's
    rule).
      A  every family of the case (its `main` families) has an active member at the configuration; for the half-spaces
         that is blind_spot_sample's: a masked node more than 1 cm beyond its margin to a plane.
      B  rows that are likely to change their active set with the first accepted step.  With start noise: a link or self
         hinge is active at the start point and the active set there differs from the configuration's own, which the
         first accepted step all but returns to.  Without: the rows of A (what B asks of them is start_point_faults')."""
    robot, graph, ap = problem(case)
    c = CASES[case]
    lim_a, lim_b = c["limit"]
    q_all = _angles(case)
    main = c.get("main", tuple(at.HingeTerms(ap, np.zeros(6)).families))
    A, near = [], []
    for lo in range(0, len(q_all), CHUNK):
        q = q_all[lo:lo + CHUNK]
        Y = ap.base.seed_points(q)
        ok = np.ones(len(q), dtype=bool)
        inf = np.full(len(q), np.inf)
        if len(ap.obstacles):
            ok &= ap.clearance(Y) > 0.0
        link = ap.link_clearance(Y) if ap.link_hinges else inf
        slf = ap.self_clearance(Y) if ap.self_hinges else inf
        fam = {"links": link < 0.0, "self": slf < 0.0}
        if ap.halfspaces is not None:
            masked = [ap.free[i] for i in np.flatnonzero(ap.obs_mask == 1)]
            res = ap.halfspace_margin[ap.obs_mask == 1][None, :, None] - ap._halfspace_s(Y[:, masked], ap.halfspaces)
            goal = ap._halfspace_s(Y[:, ap.anchors[len(ap.anchors) - ap.n_goal_anchor:]], ap.halfspaces)
            ok &= goal.min(axis=(1, 2)) > 0.05
            fam["half"] = res.max(axis=(1, 2)) > 0.01
        A += (lo + np.flatnonzero(ok & np.logical_and.reduce([fam[name] for name in main]))).tolist()
        near += (lo + np.flatnonzero(ok & ((link < 3 * c["sigma"]) | (slf < 3 * c["sigma"])))).tolist()
    if not c["sigma"]:
        return {"A": tuple(A[:lim_a]), "B": tuple(A[:lim_b])}
    B = []
    for g in near:
        Y0, ga = start(case, g)
        noisy, clean = hinge_state(case, Y0, ga), hinge_state(case, ap.seed_points(q_all[g:g + 1])[0], ga)
        if any(len(noisy[f]) for f in ("links", "self") if f in noisy) and at.state_changes(clean, noisy)[0]:
            B.append(g)
            if len(B) == lim_b:
                break
    return {"A": tuple(A[:lim_a]), "B": tuple(B)}


@functools.lru_cache(maxsize=None)
def twin(case, g, rendering=0, mutant=None):
    """The numpy twin on row g of the case's stream, TWIN_MAXITER outer iterations at the most.  rendering r > 0: the
    start point moved by 1e-15 randn and, for odd r, the shares added in the other order; r > N_RENDERINGS: through
    anchored_twin.FastTerms.  Renderings and mutants run PREFIX iterations: nothing beyond is asked of them."""
    robot, graph, ap = problem(case)
    y, ga = start(case, g)
    if rendering:
        y = y + 1e-15 * np.random.RandomState(1000 * rendering + g).randn(*y.shape)
    if rendering > N_RENDERINGS:
        terms = at.FastTerms(ap, ga, reverse=rendering % 2 == 1)
    else:
        terms = at.HingeTerms(ap, ga, reverse=rendering % 2 == 1, mutant=mutant)
    return at.rtr_numpy(terms, y, maxiter=PREFIX if rendering or mutant else TWIN_MAXITER, trace_cap=32)


@functools.lru_cache(maxsize=None)
def stable_prefix(case, g):
    """Number of leading outer iterations over which the twin reproduces itself (identical decisions, f and |grad| to
    STABLE_RTOL) in five renderings of the mirrors' sum and N_FAST of the vectorised one, which differ in rounding only.
    Beyond it the reference does not reproduce itself and nothing else can be asked to."""
    o = twin(case, g)
    k = o["iterations"]
    for r in list(range(N_RENDERINGS + 1, N_RENDERINGS + N_FAST + 1)) + list(range(1, N_RENDERINGS + 1)):      # (the cheap ones first)
        o2 = twin(case, g, r)
        k = min(k, first_divergence(o2["traj"], o["traj"], min(o["iterations"], o2["iterations"]), rtol=STABLE_RTOL))
        if k < STABLE_WANT:      # (the row is lost: what is returned is an upper bound)
            break
    return k


def pinned(case, g):
    """Outer iterations of row g that the device is held to."""
    return min(PREFIX, twin(case, g)["iterations"], stable_prefix(case, g))


def pinned_recorded(case, g):
    """pinned() from the recorded table STABLE."""
    return min(PREFIX, twin(case, g)["iterations"], STABLE[case][seeds(case).index(g)])


def hinge_share(case, g):
    """The hinge shares' part of f at the start point."""
    robot, graph, ap = problem(case)
    Y0, ga = start(case, g)
    t = at.HingeTerms(ap, ga)
    f = t(Y0, np.zeros_like(Y0))[0]
    return t.last_hinge_f / f if f > 0 else 0.0


def start_point_faults(case, g, kind="A"):
    """What is wrong with row g as a start point of sub-stream `kind`, or nothing: the per-problem conditions under which
    it is kept, the cheapest first (one twin solve decides most rows)."""
    if not hinge_share(case, g) >= HINGE_SHARE:
        return [f"the hinge shares are {hinge_share(case, g):.2e} of f at the start point"]
    tr = twin(case, g)["traj"]
    if not np.any(tr["accept"][:PREFIX] == 1):
        return ["the first four iterations hold no accepted point: nothing of what commit() leaves would be compared"]
    if kind == "B" and not any(tr["at"][k] < PREFIX and at.state_changes(tr["state"][k - 1], tr["state"][k])[0]
                               for k in range(1, len(tr["state"]))):
        return ["no accepted point of the first four iterations changes the active set"]
    if stable_prefix(case, g) < STABLE_WANT:
        return [f"the twin reproduces itself for {stable_prefix(case, g)} iterations, {STABLE_WANT} wanted"]
    if not np.any(tr["accept"][:pinned(case, g)] == 1):
        return ["the pinned prefix holds no accepted point"]
    if kind == "B" and not prefix_events(case, g)[1]:
        return ["no accepted point of the pinned prefix changes the active set"]
    return []


def prefix_events(case, g):
    """(a rejected step, an accepted point whose active set differs from the previous accepted point's, an active hinge
    whose foot parameter moved between two accepted points) inside the pinned prefix of row g."""
    tr = twin(case, g)["traj"]
    m = pinned(case, g)
    rejected = bool(np.any(tr["accept"][:m] == 0))
    changed = moved = False
    for k in range(1, len(tr["state"])):
        if tr["at"][k] < m:
            c, mv = at.state_changes(tr["state"][k - 1], tr["state"][k])
            changed, moved = changed or c, moved or mv
    return rejected, changed, moved


def mutant_leaves_at(case, g, mutant):
    """The outer iteration inside row g's pinned prefix at which a planted fault leaves the true twin at the device's bar
    (CONTRACT_RTOL), or None if it does not."""
    o, mu = twin(case, g), twin(case, g, 0, mutant)
    m = pinned(case, g)
    k = first_divergence(mu["traj"], o["traj"], min(m, mu["iterations"]), rtol=CONTRACT_RTOL)
    return k if k < m else None


# ---- (a) the twin against the C twin -------------------------------------------------------------------------------
def _dense(Nf, free_terms):
    om, pL, pU, D = (np.zeros((Nf, Nf)) for _ in range(4))
    for i, j, k_, t in zip(*free_terms):
        if k_ == 1:
            om[i, j] = om[j, i] = 1.0
            D[i, j] = D[j, i] = t
        elif k_ == 2:
            pL[i, j] = pL[j, i] = t
        else:
            pU[i, j] = pU[j, i] = t
    return D, om, pL, pU


def _assert_twin_is_the_c_twin(label, terms, Y0, dense, anchor_terms, stable=None):
    from oracle import c_oracle as co
    o = co.rtr_solve_anchored(Y0, *dense, *anchor_terms, traj_cap=32, maxiter=TWIN_MAXITER)
    t = at.rtr_numpy(terms, Y0, maxiter=TWIN_MAXITER, trace_cap=32)
    n = min(o["iterations"], t["iterations"])
    if stable is None:      # the C twin against itself: other summation order, start point 1e-15 away, the FMA build
        stable = n
        for r in range(1, N_RENDERINGS + 1):
            rng = np.random.RandomState(r)
            perm = rng.permutation(len(anchor_terms[0]))
            o2 = co.rtr_solve_anchored(Y0 + 1e-15 * rng.randn(*Y0.shape), *dense, *[a[perm] for a in anchor_terms], traj_cap=32,
                                       maxiter=TWIN_MAXITER, fast=r % 2 == 0)
            stable = min(stable, first_divergence(o2["traj"], o["traj"], min(n, o2["iterations"]), rtol=STABLE_RTOL))
    m = min(n, stable)
    leaves = first_divergence(t["traj"], o["traj"], n)
    print(f"{label}: {n} iterations, the C twin reproduces itself for {stable}, the numpy twin leaves it at {leaves}")
    assert n >= 4, (label, n)
    assert m >= 1 and leaves >= m, (label, leaves, m, {k: (t["traj"][k][:m], o["traj"][k][:m]) for k in ("numit", "stop", "accept", "f_before")})
    return leaves, m


@pytest.mark.parametrize("cid", sa.SOLVE_CASES)
def test_twin_is_the_c_twin_on_the_synthetic_problems(cid):
    """Problems 0 and 5 of every plain anchored case of tests/synth_anchored.py: decisions identical, f and |grad| to 1e-8
    over min(n, stable_prefix) outer iterations, at least 4 run."""
    from parity_util import anchored_numpy_terms
    from test_anchored_limits_host import stable_prefix as c_stable_prefix
    p = sa.build(cid)
    Y0 = sa.start_points(cid)
    for b in (0, 5):
        terms = lambda Y, W, b=b: anchored_numpy_terms(sa.free_terms(p), sa.anchor_terms(p, b), Y, W)      # noqa: E731
        _assert_twin_is_the_c_twin(f"{cid}/{b}", terms, Y0[b], (p.D, p.omega, p.psi_L, p.psi_U), sa.anchor_terms(p, b),
                                   stable=c_stable_prefix(cid, b))


def test_twin_is_the_c_twin_on_ur10():
    """Four UR10 problems without hinges (eight table spheres, node hinges only), goals and start points of
    test_anchored_trajectory_against_oracle's kind; the factory's own sum with no hinge family to add."""
    robot, graph = make_graph("ur10")
    from graphik_amd.utils import table_environment
    for idx, (centre, r) in enumerate(list(table_environment())[:8]):
        graph.add_spherical_obstacle(f"o{idx}", np.asarray(centre, dtype=float), float(r))
    ap = _rs().AnchoredProblem(graph, host_only=True)
    Nf = len(ap.free)
    rng = np.random.RandomState(9)
    lo, hi = robot.limits_arrays()
    ga = ap.goal_anchors(robot.fk_batch(lo + (hi - lo) * rng.rand(4, robot.n)))
    Y0 = 0.5 * rng.randn(4, Nf, 3) + np.array([0.0, 0.0, 0.6])
    dense = _dense(Nf, ap.free_terms)
    for b in range(4):
        terms = at.HingeTerms(ap, ga[b])
        assert terms.families == []
        _assert_twin_is_the_c_twin(f"ur10/{b}", terms, Y0[b], dense, anchored_terms(ap, ga[b]))


def test_a_doubled_gradient_leaves_the_c_twin_at_once():
    """The scale is settled: with G = grad f instead of 1/2 grad f the numpy loop leaves the C twin in iteration 0."""
    from oracle import c_oracle as co
    from parity_util import anchored_numpy_terms
    p = sa.build("a9_noobs")
    Y0 = sa.start_points("a9_noobs")[0]

    def doubled(Y, W):
        f, G, H = anchored_numpy_terms(sa.free_terms(p), sa.anchor_terms(p, 0), Y, W)
        return f, 2.0 * G, H
    o = co.rtr_solve_anchored(Y0, p.D, p.omega, p.psi_L, p.psi_U, *sa.anchor_terms(p, 0), traj_cap=32, maxiter=TWIN_MAXITER)
    t = at.rtr_numpy(doubled, Y0, maxiter=TWIN_MAXITER)
    assert first_divergence(t["traj"], o["traj"], min(o["iterations"], t["iterations"])) == 0


def test_the_fast_rendering_is_the_mirrors_sum():
    """anchored_twin.FastTerms against HingeTerms at every start point and a random direction: f, G and H W to 1e-12 of
    |f|, max |G|, max |H W| (measured: 7.4e-14 at the most).  It only ever serves as a rendering: were it wrong, no seed
    would have a stable prefix."""
    worst = 0.0
    for case in CASES:
        ap = problem(case)[2]
        for g in seeds(case):
            y, ga = start(case, g)
            W = np.random.RandomState(g).randn(*y.shape)
            a, b = at.HingeTerms(ap, ga)(y, W), at.FastTerms(ap, ga)(y, W)
            assert a[0] > 0
            worst = max(worst, abs(a[0] - b[0]) / abs(a[0]), np.abs(a[1] - b[1]).max() / np.abs(a[1]).max(),
                        np.abs(a[2] - b[2]).max() / np.abs(a[2]).max())
    print(f"FastTerms against HingeTerms: {worst:.2e}")
    assert worst <= 1e-12


# ---- (b), (c) the case table and its conditions ----------------------------------------------------------------------
def test_the_case_table_names_every_hinge_build():
    """One case per solve instantiation outside the plain anchored group: the flag words 3, 5, 7, 9, 11 (9 twice: one
    plane and eight), each the sum its keywords spell."""
    for case, c in CASES.items():
        kw = c["kw"]
        assert c["build"] == 1 + 2 * bool(kw.get("link_hinges")) + 4 * bool(kw.get("self_hinges")) + 8 * ("halfspaces" in kw), case
        robot, graph, ap = problem(case)
        assert len(ap.obstacles) == c.get("spheres", 0) and len(ap.free) == 10
        assert (0 if ap.halfspaces is None else len(ap.halfspaces)) == len(kw.get("halfspaces", []))
    assert sorted(c["build"] for c in CASES.values()) == [3, 5, 7, 9, 9, 11]
    assert len(CASES["half8"]["kw"]["halfspaces"]) == 8 and set(FOOT_CASES) == {c for c in CASES if CASES[c]["build"] & 6 and not CASES[c]["build"] & 8}


@pytest.mark.parametrize("case", sorted(CASES))
def test_start_points_meet_every_condition(case):
    """Per problem: the hinge shares are at least 10 % of f at the start point, the twin reproduces itself for at least 3
    outer iterations in five renderings, and the pinned prefix holds an accepted point; the rows of sub-stream B hold one
    whose active set differs from the previous accepted point's as well.  Per case, inside the pinned prefixes: at least
    three problems hold a rejected step, three an accepted point with a changed active set and -- links, self, self_links
    -- three an active hinge whose foot parameter moved between two accepted points.  The seeds are the first four of
    either sub-stream that meet its conditions: every candidate passed over fails one."""
    cand = candidates(case)
    chosen = set(seeds(case))
    assert len(chosen) == B
    for kind in ("A", "B"):
        rows = SEEDS[case][kind]
        assert len(rows) >= 3 and list(rows) == sorted(rows) and set(rows) <= set(cand[kind])
        for g in rows:
            assert not start_point_faults(case, g, kind), (case, kind, g, start_point_faults(case, g, kind))
        for g in cand[kind][:cand[kind].index(rows[-1])]:
            assert g in chosen or start_point_faults(case, g, kind), (case, kind, g, "meets every condition and was passed over")
    assert tuple(stable_prefix(case, g) for g in seeds(case)) == STABLE[case]
    assert all(pinned_recorded(case, g) == pinned(case, g) for g in seeds(case))
    ev = np.array([prefix_events(case, g) for g in seeds(case)])
    fams = at.HingeTerms(problem(case)[2], np.zeros(6)).families
    acts = {f: int(sum(bool(len(twin(case, g)["traj"]["state"][0][f])) for g in seeds(case))) for f in fams}
    report(f"hinge_twin/twin/{case}", {"seeds": list(seeds(case)), "iterations": [twin(case, g)["iterations"] for g in seeds(case)],
                                       "reproduces_itself_for": [stable_prefix(case, g) for g in seeds(case)],
                                       "pinned": [pinned(case, g) for g in seeds(case)],
                                       "accept": ["".join(map(str, twin(case, g)["traj"]["accept"].tolist())) for g in seeds(case)],
                                       "rejected_step": ev[:, 0].tolist(), "active_set_changed": ev[:, 1].tolist(),
                                       "foot_moved": ev[:, 2].tolist(), "stop": [twin(case, g)["stop"] for g in seeds(case)],
                                       "hinge_share": [round(float(hinge_share(case, g)), 3) for g in seeds(case)],
                                       "problems_with_an_active_member_at_the_start": acts,
                                       "f": [twin(case, g)["f"] for g in seeds(case)]})
    assert min(acts.values()) >= 3, (case, acts)      # every family of the case acts at three start points at least
    assert ev[:, 0].sum() >= 3, (case, "rejected steps", ev[:, 0])
    assert ev[:, 1].sum() >= 3, (case, "active-set changes", ev[:, 1])
    if case in FOOT_CASES:
        assert ev[:, 2].sum() >= 3, (case, "moved feet", ev[:, 2])


# ---- (d) the prefix sees planted faults ------------------------------------------------------------------------------
@pytest.mark.parametrize("mutant", at.MUTANTS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_the_pinned_prefix_sees_a_planted_fault(case, mutant):
    """A twin whose Hessian reads the last trial point's hinge state, one whose trial cost lacks the hinge shares, one
    whose hinge gradient is off by 1e-6: each leaves the true twin inside the pinned prefix of at least one problem at the
    device's own bar, so a kernel with that fault fails tests/test_anchored_hinge_twin_gpu.py."""
    leaves = [mutant_leaves_at(case, g, mutant) for g in seeds(case)]
    report(f"hinge_twin/mutant/{mutant}/{case}", {"leaves_the_twin_at": leaves})
    assert any(k is not None for k in leaves), (case, mutant, leaves)
