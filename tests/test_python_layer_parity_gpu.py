"""The Python layer after its plain and anchored call paths were folded (docs/NOTEBOOK.md 26): every public entry point
of graphik_amd/engine.py and graphik_amd/solvers/riemannian_solver.py returns what the parent commit's copy returned,
bit for bit.

A table of scenarios (SCENARIOS) runs solve_batch, solve_trajectory, AnchoredProblem.solve / solve_trajectory,
Template.ik and Template.anchored_ik over the paths the fold touched: cold, seeded ([n] and [B, n]), Y_init, restarts
(cold, seeded, local), the host paths of graphs off the device pipeline, planar poses, tracking with and without the
point matrices, the clearance modes (nodes, links, links+self), per-goal scenes (cold, seeded, with restarts, per
waypoint), the sweep, link and self hinges, reused `out` buffers, and the small Template methods (the costgrd twins,
prepare, recover, seed, the clearances, the sweep, Template.solve with scenes).  Every returned array is hashed
by key (sha256 over dtype, shape and bytes; not hashed: time, solve_time, inner_executed, flags and keys that begin
with "_") and compared with tests/golden/python_layer_parent.json, which tools/python_layer_digest.py recorded on the
MI355X from a checkout of the parent commit with this table.  The recording refuses a file in which a restart scenario
improved no goal (attempt all zero) or a clearance scenario has no finite clearance; the test checks the same of the
file it reads, so no scenario passes on a path that did nothing.  (planar_cold was recorded again when prep_quad_kernel's
K x K Jacobi schedule became a function of the goal alone, docs/NOTEBOOK.md 36: the floating-point arrays moved in their
last bits, every count stayed.  The file was recorded again from a checkout of c11b7a7 when the self clearance, the
scenes and the self hinges joined the table, docs/NOTEBOOK.md 40, and from a checkout of d57bfde when six scenarios
for the entries and branches the table had missed joined it, docs/NOTEBOOK.md 41: both times every hash that was there
before came out unchanged.  And from a checkout of bcb1840 when the screened restarts, the atlas, the floor problem and the
step entries joined it, docs/NOTEBOOK.md 47: 33 scenarios unchanged byte for byte, and the 29 hashes of the small-methods
scenario unchanged beside its 14 new keys.  An atlas scenario whose atlas_pick names no row is refused like the others.)

Shapes: B = 5 goals (a multiple of nothing), trajectories of L = 3 waypoints for B = 4 paths.  Inputs: conftest.make_graph
and the inputs of the anchored host tests (collision_input, tracking_input, TWIN_MAXITER, TWIN_SEED); fixed seeds."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, make_graph
from test_anchored_retry_host import TWIN_MAXITER, TWIN_SEED
from test_anchored_screen_host import FLOOR, RHO, pi_limits
from test_anchored_seeded_host import collision_input, tracking_input

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "python_layer_parent.json")
NOT_HASHED = ("time", "solve_time", "inner_executed", "flags")
B, PATHS, WAYPOINTS = 5, 4, 3
SHORT = {"maxiter": 5}      # a budget at which first attempts fail, so that restarts have something to improve


def _rs():
    from graphik_amd.solvers import riemannian_solver as rs
    return rs


def host(res):
    """A returned dict (device tensors or arrays; None entries dropped) -> numpy arrays by key."""
    out = {}
    for key, v in res.items():
        if v is None or key.startswith("_") or key in NOT_HASHED:
            continue
        out[key] = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    return out


def triple(ret):
    """(q, Y, info) of solve_batch / solve_trajectory -> one dict."""
    q, Y, info = ret
    return host({"q": q, "Y": Y, **info})


def sha(a):
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(repr((a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def digest(arrays):
    return {key: sha(arrays[key]) for key in sorted(arrays)}


# ---- inputs and problems, built once ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plain(name):
    """(robot, graph, goal poses [B, ...], seeds [B, n] unrelated to the goals) of a packaged graph."""
    robot, graph = make_graph(name)
    rng = np.random.RandomState(101)
    lb, ub = robot.limits_arrays()
    goals = rng.uniform(0.8 * lb, 0.8 * ub, size=(B, robot.n))
    seeds = rng.uniform(lb, ub, size=(B, robot.n))
    return robot, graph, robot.fk_batch(goals), seeds


@functools.lru_cache(maxsize=None)
def plain_paths():
    """LWA4D: (graph, T [PATHS, WAYPOINTS, 4, 4], the paths' own start angles, start angles unrelated to the paths)."""
    robot, graph = plain("lwa4d")[:2]
    rng = np.random.RandomState(102)
    lb, ub = robot.limits_arrays()
    q0 = rng.uniform(0.6 * lb, 0.6 * ub, size=(PATHS, robot.n))
    sign = rng.choice([-1.0, 1.0], size=(PATHS, robot.n))
    Q = q0[:, None] + 0.02 * sign[:, None] * np.arange(WAYPOINTS)[None, :, None]
    T = robot.fk_batch(Q.reshape(-1, robot.n)).reshape(PATHS, WAYPOINTS, 4, 4)
    return graph, T, Q[:, 0], rng.uniform(lb, ub, size=(PATHS, robot.n))


@functools.lru_cache(maxsize=None)
def anchored(maxiter=None, link_hinges=False, self_pairs=None, self_hinges=False):
    """One AnchoredProblem (UR10 + table, skeleton links) per iteration budget and hinge setting; with self pairs the
    links are capsules of 3 cm."""
    robot, graph = make_graph("ur10_table")
    params = None if maxiter is None else {"maxiter": maxiter}
    return robot, _rs().AnchoredProblem(graph, params=params, link_hinges=link_hinges, self_pairs=self_pairs,
                                        self_hinges=self_hinges, link_radius=0.0 if self_pairs is None else 0.03)


@functools.lru_cache(maxsize=None)
def room(maxiter=None):
    """The anchored problem of the screened and the atlas tests per iteration budget: UR10 + table, 3 cm capsules, every
    self pair, and a floor 10 cm under the base (halfspaces=[FLOOR]).  The table stays in the problem with the floor: the
    goals and seeds of this file (anchored_goals) are chosen against its spheres and _three_scenes is made of them, so one
    problem serves the screened, the atlas and the floor scenarios ("anch_floor_*": the floor on top of the table).  Its
    atlas keeps 94 of the 512 draws (183 with the floor alone); the largest K used is 6."""
    robot, graph = make_graph("ur10_table")
    params = None if maxiter is None else {"maxiter": maxiter}
    return robot, _rs().AnchoredProblem(graph, params=params, link_radius=RHO, self_pairs="auto", halfspaces=[list(FLOOR)])


@functools.lru_cache(maxsize=None)
def room_atlas():
    """512 draws, the rows that are clear of the room in "links+self"."""
    return room()[1].seed_atlas(size=512, seed=3, clearance_mode="links+self")


@functools.lru_cache(maxsize=None)
def anchored_goals():
    """(goal poses [B, 4, 4] of clear configurations, seeds [B, n] in collision)."""
    robot = anchored()[0]
    seeds, goals = collision_input()
    return robot.fk_batch(goals[:B]), seeds[:B]


@functools.lru_cache(maxsize=None)
def anchored_paths():
    """(T [PATHS, WAYPOINTS, 4, 4] collision-free paths, their own start angles, colliding start angles)."""
    Q, T = tracking_input()
    return T[:PATHS, :WAYPOINTS], Q[:PATHS, 0], collision_input()[0][:PATHS]


# ---- the scenarios -----------------------------------------------------------------------------------------------
def _batch(name, seeded=None, **kw):
    def run():
        robot, graph, T, seeds = plain(name)
        q_init = {None: None, "one": seeds[0], "each": seeds}[seeded]      # [n] for all goals, or [B, n]
        return triple(_rs().solve_batch(graph, T, q_init=q_init, **kw))
    return run


def _batch_Y_init():
    robot, graph, T, seeds = plain("lwa4d")
    Y_cold = _rs().solve_batch(graph, T)[1]
    Y_init = Y_cold + 1e-3 * np.random.RandomState(103).randn(*Y_cold.shape)
    return triple(_rs().solve_batch(graph, T, Y_init=Y_init))


def _off_pipeline(run):
    """run() with the cached LWA4D problem taken off the device pipeline: the host prepares and recovers."""
    def wrapped():
        rs = _rs()
        rs.clear_problem_cache()
        prob = rs._problem_for(plain("lwa4d")[1])
        prob.device_pipeline = False
        try:
            return run()
        finally:
            rs.clear_problem_cache()
    return wrapped


def _track(start, **kw):
    def run():
        graph, T, q_own, q_far = plain_paths()
        return triple(_rs().solve_trajectory(graph, T, q_own if start == "own" else q_far, **kw))
    return run


def _anch(maxiter=None, seeded=False, link_hinges=False, self_pairs=None, self_hinges=False, scenes=False, in_room=False,
          atlas=False, **kw):
    def run():
        T, seeds = anchored_goals()
        ap = room(maxiter)[1] if in_room else anchored(maxiter, link_hinges, self_pairs, self_hinges)[1]
        extra = {}
        if atlas:
            extra["atlas"] = room_atlas()
        if scenes:      # three scenes, goal b in scene b % 3
            extra.update(scenes=_three_scenes(ap), scene_id=(np.arange(B) % 3).astype(np.int32))
        return host(ap.solve(T, q_init=seeds if seeded else None, **kw, **extra))
    return run


def _three_scenes(ap):
    """The table, the table 0.2 m further in x, its first ten spheres."""
    return ap.scene_set([ap.obstacles, ap.obstacles + np.array([0.2, 0.0, 0.0, 0.0]), ap.obstacles[:10]])


def _anch_track(maxiter=None, start="own", self_pairs=None, scenes=False, in_room=False, **kw):
    def run():
        T, q_own, q_hit = anchored_paths()
        ap = room(maxiter)[1] if in_room else anchored(maxiter, False, self_pairs)[1]
        extra = {}
        if scenes:      # a scene per waypoint: waypoint l of path b in scene (b + l) % 3
            extra = dict(scenes=_three_scenes(ap),
                         scene_id=((np.arange(PATHS)[:, None] + np.arange(WAYPOINTS)[None, :]) % 3).astype(np.int32))
        return triple(ap.solve_trajectory(T, q_own if start == "own" else q_hit, **kw, **extra))
    return run


def _template_entries():
    """The small Template methods, each result under its own key: the costgrd twins, prepare, recover and seed on the
    LWA4D template; on the anchored one (UR10 + table, self pairs) the seed, the clearances against its own obstacles
    and against scenes, the sweep, and Template.solve with scenes."""
    rs = _rs()
    robot, graph, T, seeds = plain("lwa4d")
    tpl = rs.BatchProblem(graph).template
    out = {}
    targets, Y0 = tpl.prepare(T)
    W = np.random.RandomState(104).randn(*Y0.shape)
    out["prepare_targets"], out["prepare_Y"] = targets, Y0
    out["cost"], out["grad"] = tpl.cost(Y0, targets), tpl.grad(Y0, targets)
    out["cost_and_grad_f"], out["cost_and_grad_G"] = tpl.cost_and_grad(Y0, targets)
    out["hess"], out["proj"] = tpl.hess(Y0, W, targets), tpl.proj(Y0, W)
    out["recover_q"], out["recover_pos_err"], out["recover_rot_err"] = tpl.recover(Y0, T)
    out["seed_targets"], out["seed_Y"] = tpl.seed(T, seeds)
    Ta, seeds_a = anchored_goals()
    ap = anchored(None, False, "auto")[1]
    atpl, base = ap.template, ap.base.template
    Y_free, goal = atpl.anchored_seed(base, Ta, seeds_a)
    out["anchored_seed_Y"], out["anchored_seed_goal"] = Y_free, goal
    answer = ap.solve(Ta, q_init=seeds_a)
    sc = dict(scenes=_three_scenes(ap), scene_id=(np.arange(B) % 3).astype(np.int32))
    out["clearance"] = atpl.anchored_clearance(answer["x"])
    out["clearance_scenes"] = atpl.anchored_clearance(answer["x"], **sc)
    out["link_clearance"] = atpl.anchored_link_clearance(answer["x"])
    out["link_clearance_scenes"] = atpl.anchored_link_clearance(answer["x"], **sc)
    out["self_clearance"] = atpl.anchored_self_clearance(answer["x"])
    out["sweep_clearance"] = atpl.anchored_sweep_clearance(base, seeds_a, answer["q"], 3)
    out.update({"solve_scenes_" + key: v for key, v in host(atpl.solve(Y_free, goal, **sc)).items()})
    # the step entries of the screened and the atlas restarts, and the half-space clearance, in the room
    rp, A = room()[1], room_atlas()
    rtpl, rbase = rp.template, rp.base.template
    mode = dict(clearance_mode="links+self")
    step = rtpl.anchored_retry_seeds_screened(rbase, Ta, np.arange(B), TWIN_SEED, 1, 4, pi_limits(), **mode)
    out.update({"screened_seeds_" + key: v for key, v in host(step).items()})
    out["atlas_nearest_nbr"], out["atlas_nearest_dist"] = nbr, _ = rbase.atlas_nearest(A, Ta, 6)
    step = rtpl.anchored_atlas_seeds(rbase, A, Ta, nbr, 2, first=2, **mode)
    out.update({"atlas_seeds_" + key: v for key, v in host(step).items()})
    in_room = rp.solve(Ta, q_init=seeds_a, **mode)
    out["halfspace_clearance"] = rtpl.anchored_halfspace_clearance(in_room["x"])
    out["halfspace_link_clearance"] = rtpl.anchored_halfspace_clearance(in_room["x"], links=True)
    out["sweep_link_clearance"], out["sweep_self_clearance"] = rtpl.anchored_sweep_clearances(rbase, seeds_a, in_room["q"], 3)
    return host(out)


def _reuse(call, alloc):
    """One call twice into the same `out`: the same bits both times, and q, pos_err, rot_err are the caller's tensors."""
    out = alloc()
    first = call(out)
    first_host = host(first)
    again = call(out)
    assert digest(host(again)) == digest(first_host)
    for res in (first, again):
        for key in ("q", "pos_err", "rot_err"):
            assert res[key].data_ptr() == out[key].data_ptr(), key
    return first_host


def _reuse_ik():
    robot, graph, T, seeds = plain("lwa4d")
    tpl = _rs().BatchProblem(graph).template
    return _reuse(lambda out: tpl.ik(T, out=out), lambda: tpl.alloc_ik_buffers(B))


def _reuse_anchored_ik():
    T, seeds = anchored_goals()
    ap = anchored()[1]
    tpl, base = ap.template, ap.base.template
    return _reuse(lambda out: tpl.anchored_ik(base, T, q_init=seeds, out=out, clearance=True),
                  lambda: tpl.alloc_anchored_buffers(base, B, clearance=True))


SCENARIOS = {
    # plain, LWA4D
    "batch_cold": _batch("lwa4d"),
    "batch_seed_one": _batch("lwa4d", "one"),
    "batch_seed_each": _batch("lwa4d", "each"),
    "batch_Y_init": _batch_Y_init,
    "batch_retry_cold": _batch("lwa4d", retries=2, params=SHORT),
    "batch_retry_seeded": _batch("lwa4d", "each", retries=2, params=SHORT),
    # plain, the host paths of a graph off the device pipeline
    "host_batch_cold": _off_pipeline(_batch("lwa4d")),
    "host_batch_seeded": _off_pipeline(_batch("lwa4d", "each")),
    "host_track": _off_pipeline(_track("own", return_Y=True)),
    # plain, planar: k = 2 and its pose shapes
    "planar_cold": _batch("planar10_limits_halfpi"),
    # plain, tracking
    "track_Y": _track("own", return_Y=True),
    "track_retry": _track("far", retries=1, params=SHORT, return_Y=False),
    # anchored: UR10 + table, skeleton links
    "anch_cold": _anch(),
    "anch_cold_clearance_nodes": _anch(clearance=True),
    "anch_cold_clearance_links": _anch(clearance=True, clearance_mode="links"),
    "anch_seeded_clearance_nodes": _anch(seeded=True),
    "anch_seeded_clearance_links": _anch(seeded=True, clearance_mode="links"),
    "anch_retry_cold_clearance_nodes": _anch(TWIN_MAXITER, retries=2, retry_seed=TWIN_SEED),
    "anch_retry_seeded_clearance_links": _anch(TWIN_MAXITER, seeded=True, retries=2, retry_seed=TWIN_SEED, retry_spread=0.3,
                                               clearance_mode="links"),
    "anch_track_sweep_clearance": _anch_track(sweep=2, return_Y=True),
    "anch_track_retry_clearance_links": _anch_track(TWIN_MAXITER, "hit", retries=1, retry_seed=TWIN_SEED, retry_spread=0.3,
                                                    clearance_mode="links"),
    "anch_hinges_seeded_clearance_links": _anch(seeded=True, link_hinges=True, clearance_mode="links"),
    # anchored: self pairs ("auto", capsules of 3 cm) and per-goal scenes
    "anch_self_cold_clearance_links_self": _anch(self_pairs="auto", clearance=True, clearance_mode="links+self"),
    "anch_scenes_seeded_clearance_links": _anch(seeded=True, scenes=True, clearance_mode="links"),
    "anch_self_hinges_seeded_clearance_links_self": _anch(seeded=True, self_pairs="auto", self_hinges=True,
                                                          clearance_mode="links+self"),
    "anch_self_track_sweep_clearance_links_self": _anch_track(self_pairs="auto", sweep=2, clearance_mode="links+self"),
    # anchored: the entries and branches the table missed until docs/NOTEBOOK.md 41 -- restarts among scenes, scenes with
    # a null seed, restarts in "links+self", a scene per waypoint, tracking on the shared restart workspace
    "anch_scenes_retry_seeded_clearance_links": _anch(TWIN_MAXITER, seeded=True, scenes=True, retries=2, retry_seed=TWIN_SEED,
                                                      clearance_mode="links"),
    "anch_scenes_cold_clearance_nodes": _anch(scenes=True, clearance=True),
    "anch_self_retry_cold_clearance_links_self": _anch(TWIN_MAXITER, self_pairs="auto", retries=2, retry_seed=TWIN_SEED,
                                                       clearance_mode="links+self"),
    "anch_scenes_track_clearance_links": _anch_track(scenes=True, clearance_mode="links"),
    "anch_self_track_clearance_links_self": _anch_track(self_pairs="auto", clearance_mode="links+self"),
    # anchored, in the room (table, capsules, self pairs, floor): screened restarts, seeds from the atlas, and the floor without either
    "anch_screen_retry_cold_clearance_nodes": _anch(SHORT["maxiter"], in_room=True, retries=2, retry_candidates=4,
                                                    retry_seed=TWIN_SEED),
    "anch_screen_scenes_retry_seeded_clearance_links": _anch(SHORT["maxiter"], in_room=True, seeded=True, scenes=True, retries=2,
                                                             retry_candidates=4, retry_seed=TWIN_SEED, clearance_mode="links"),
    "anch_screen_track_retry_clearance_nodes": _anch_track(SHORT["maxiter"], "hit", in_room=True, retries=2, retry_candidates=4,
                                                           retry_seed=TWIN_SEED),
    "anch_atlas_cold_clearance_links": _anch(SHORT["maxiter"], in_room=True, atlas=True, atlas_candidates=4, clearance_mode="links"),
    "anch_atlas_retry_cold_clearance_links_self": _anch(SHORT["maxiter"], in_room=True, atlas=True, retries=2, atlas_candidates=2,
                                                        clearance_mode="links+self"),
    "anch_atlas_scenes_retry_seeded_clearance_links": _anch(SHORT["maxiter"], in_room=True, atlas=True, seeded=True, scenes=True,
                                                            retries=2, atlas_candidates=2, clearance_mode="links"),
    "anch_floor_cold_clearance_nodes": _anch(in_room=True, clearance=True),
    "anch_floor_cold_clearance_links_self": _anch(in_room=True, clearance=True, clearance_mode="links+self"),
    "anch_floor_seeded_clearance_nodes": _anch(in_room=True, seeded=True),
    "anch_floor_seeded_clearance_links_self": _anch(in_room=True, seeded=True, clearance_mode="links+self"),
    # the small Template methods
    "template_entries_clearance": _template_entries,
    # reused buffers
    "reuse_ik": _reuse_ik,
    "reuse_anchored_ik_clearance": _reuse_anchored_ik,
}


def conditions(name, arrays):
    """What keeps a scenario from passing on a path that did nothing: {"attempt_nonzero": count} for a restart scenario,
    {"clearance_finite": count} for one that returns a clearance.  A zero count is a scenario to change (seed, budget)."""
    cond = {}
    if "retry" in name:
        cond["attempt_nonzero"] = int(np.count_nonzero(arrays["attempt"]))
    if "clearance" in name:
        cond["clearance_finite"] = int(np.isfinite(arrays["clearance"]).sum())
    if "atlas" in name:
        cond["atlas_pick_named"] = int(np.count_nonzero(arrays["atlas_pick"] >= 0))
    return cond


# ---- the test ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parent():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def test_the_table_is_the_recorded_one(parent):
    assert sorted(parent["scenarios"]) == sorted(SCENARIOS)
    for name, rec in parent["scenarios"].items():
        assert all(count > 0 for count in rec["conditions"].values()), (name, rec["conditions"])
        assert ("retry" in name) == ("attempt_nonzero" in rec["conditions"]), name
        assert ("clearance" in name) == ("clearance_finite" in rec["conditions"]), name
        assert ("atlas" in name) == ("atlas_pick_named" in rec["conditions"]), name
        assert not any(key.startswith("_") or key in NOT_HASHED for key in rec["sha"]), name


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_returns_what_the_parent_returned(parent, name):
    arrays = SCENARIOS[name]()
    rec = parent["scenarios"][name]
    got = digest(arrays)
    differ = sorted(key for key in set(got) | set(rec["sha"]) if got.get(key) != rec["sha"].get(key))
    print(name, "keys", len(got), conditions(name, arrays), "differ", differ)
    assert sorted(got) == sorted(rec["sha"]), "the returned keys changed"
    assert not differ, differ
    assert conditions(name, arrays) == rec["conditions"]
