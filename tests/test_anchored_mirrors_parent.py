"""The numpy mirrors of the fixed-anchor pair geometry after they were folded onto one closest-points function, one foot
parameter and one NaN-propagating minimum (docs/NOTEBOOK.md 40): every mirror returns what the parent commit's copy
returned, bit for bit (CPU only).

A table (ENTRIES) runs link_clearance, self_clearance and clearance (own obstacles and a scene), link_foot_host and
self_feet_host on every pair of 16 configurations, link_hinge_terms_host and self_hinge_terms_host with and without
frozen parameters, and the two sweeps, on UR10 + table and on LWA4D (three zero-length links) at radius 0 and 3 cm, and
the two clearances on the hand-made degenerate cells of the host tests (clamp cells, parallel, crossing, zero-length,
NaN ends).  Every returned array is hashed by key (sha256 over dtype, shape and bytes) and compared with
tests/golden/anchored_mirrors_parent.json, which tools/anchored_mirror_digest.py recorded from a checkout of the parent
commit with this table.  The recording refuses a file in which a clearance entry holds no finite value or a hinge entry
no active hinge; the test checks the same of the file it reads."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, make_graph
from test_anchored_self_host import NINE

GOLDEN_FILE = os.path.join(GOLDEN, "anchored_mirrors_parent.json")
ROBOTS = ("ur10_table", "lwa4d")
RADII = {"r0": 0.0, "r3": 0.03}
CONFIGS = 16


def _rs():
    from graphik_amd.solvers import riemannian_solver as rs
    return rs


def sha(a):
    a = np.ascontiguousarray(a)
    h = hashlib.sha256(repr((a.dtype.str, a.shape)).encode())
    h.update(a.tobytes())
    return h.hexdigest()


def digest(arrays):
    return {key: sha(arrays[key]) for key in sorted(arrays)}


# ---- inputs, built once --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene():
    """Eight spheres around the base, [8, 4] (centre, radius): what LWA4D, which has no obstacles of its own, is measured
    against, and the scene of the obstacles= keyword."""
    rng = np.random.RandomState(12)
    s = np.concatenate([rng.uniform(-0.8, 0.8, (8, 3)), rng.uniform(0.05, 0.2, (8, 1))], axis=1)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def problem(robot, rad):
    """(robot, host-only AnchoredProblem with the skeleton at that radius and "auto" self pairs, q [16, n], q2 a step of up
    to 0.6 rad away, full point matrices, free rows, goal anchors, directions W).  The configurations: of 256 uniform
    ones the six whose links are deepest in the spheres (the problem's own, else the scene's), the four whose links are
    deepest in each other, and the first of the rest, so that hinges are active and most configurations are ordinary."""
    rob, graph = make_graph(robot)
    ap = _rs().AnchoredProblem(graph, host_only=True, link_radius=RADII[rad], self_pairs="auto")
    rng = np.random.RandomState(11)
    cand = rng.uniform(-np.pi, np.pi, (256, rob.n))
    Yc = ap.base.seed_points(cand)
    deep = list(np.argsort(ap.link_clearance(Yc, obstacles=None if len(ap.obstacles) else scene()), kind="stable")[:6])
    deep += [b for b in np.argsort(ap.self_clearance(Yc), kind="stable") if b not in deep][:4]
    q = cand[sorted(deep + [b for b in range(256) if b not in deep][:CONFIGS - len(deep)])]
    q2 = np.clip(q + rng.uniform(-0.6, 0.6, q.shape), -np.pi, np.pi)
    Y = ap.base.seed_points(q)
    Yf, ga = ap.seed_points(q), ap.goal_anchors(rob.fk_batch(q))
    W = np.random.RandomState(13).randn(*Yf.shape)
    for v in (q, q2, Y, Yf, ga, W):
        v.setflags(write=False)
    return rob, ap, q, q2, Y, Yf, ga, W


# ---- the entries -----------------------------------------------------------------------------------------------------
def _clearance(robot, rad):
    def run():
        rob, ap, q, q2, Y = problem(robot, rad)[:5]
        out = {"link_scene": ap.link_clearance(Y, obstacles=scene()), "self": ap.self_clearance(Y),
               "node_scene": ap.clearance(Y, obstacles=scene()),
               "node_scene_goal": ap.clearance(Y, include_goal=True, obstacles=scene())}
        if len(ap.obstacles):
            out.update(link=ap.link_clearance(Y), node=ap.clearance(Y), node_goal=ap.clearance(Y, include_goal=True))
        assert all(np.isfinite(v).all() for v in out.values())
        return out
    return run


def _feet(robot, rad):
    def run():
        rob, ap, q, q2, Y = problem(robot, rad)[:5]
        link = [[[np.concatenate([[t], m, [d]]) for t, m, d in [ap.link_foot_host(Y[b, ra], Y[b, rb], c[:3])]][0]
                 for c in scene()] for ra, rb in ap.link_rows for b in range(CONFIGS)]
        ends = lambda b, l, m: [Y[b, r] for r in (*ap.link_rows[l], *ap.link_rows[m])]      # noqa: E731
        feet = [[[np.concatenate([[s, t], v, [d]]) for s, t, v, d in [ap.self_feet_host(*ends(b, l, m))]][0]
                 for l, m in ap.self_pairs.tolist()] for b in range(CONFIGS)]
        return {"link_t_m_d": np.array(link), "self_s_t_v_d": np.array(feet)}
    return run


def _hinges(robot, rad, kind):
    """(f, G, H) of the link or self hinges at every configuration, then at a point 1e-3 W away with the parameters frozen
    at the first point's; "active": how many hinges were active over the configurations."""
    def run():
        rob, ap, q, q2, Y, Yf, ga, W = problem(robot, rad)
        terms = ap.link_hinge_terms_host if kind == "link" else ap.self_hinge_terms_host
        out = {k: [] for k in ("f", "G", "H", "frozen_f", "frozen_G", "frozen_H", "params")}
        active = 0
        for b in range(CONFIGS):
            f, G, H = terms(Yf[b], W[b], ga[b])
            held = dict(ap.last_link_t if kind == "link" else ap.last_self_st)
            active += len(held)
            f2, G2, H2 = terms(Yf[b] + 1e-3 * W[b], W[b], ga[b], held)
            for k, v in zip(out, (f, G, H, f2, G2, H2)):
                out[k].append(v)
            out["params"] += [np.ravel([*key] if kind == "link" else [key]).tolist() + np.ravel(val).tolist()
                              for key, val in sorted(held.items())]
        return {**{k: np.array(v, dtype=np.float64) for k, v in out.items()}, "active": np.array(active)}
    return run


def _sweeps(robot, rad):
    def run():
        rob, ap, q, q2 = problem(robot, rad)[:4]
        out = {"self": ap.sweep_self_clearance_host(q, q2, 3)}
        if len(ap.obstacles):
            out["link"] = ap.sweep_clearance_host(q, q2, 3)
        assert all(np.isfinite(v).all() for v in out.values())
        return out
    return run


class _Stub:
    """What link_clearance and self_clearance read of a problem: hand-made links, no robot behind them."""

    def __init__(self, links, pairs=(), spheres=(), rho=0.0):
        self.link_rows = np.asarray(links, dtype=np.int32).reshape(-1, 2)
        self.link_radius = np.broadcast_to(np.asarray(rho, dtype=float), (len(self.link_rows),))
        self.self_pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        self.obstacles = np.asarray(spheres, dtype=float).reshape(-1, 4)


def _cells():
    """The planted cells of test_anchored_self_host.py and test_anchored_links_host.py, one goal each: the nine clamp
    cells, parallel (overlapping, disjoint), crossing, zero-length (either link, both), and a NaN in each of the ends."""
    ap = _rs().AnchoredProblem
    X = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]
    second = [[(x0, y0, z0), (x0, y0 + 1.0, z0)] for x0, y0, z0 in NINE]
    second += [[(0.5, 0.25, 0), (1.5, 0.25, 0)], [(1.375, 0.5, 0), (2.375, 0.5, 0)], [(0.5, -0.5, 0), (0.5, 0.5, 0)],
               [(0.5, 0.25, 0), (0.5, 0.25, 0)]]
    Y = np.array([X + [list(a2), list(b2)] for a2, b2 in second], dtype=float)
    bad = np.array([X + [[0.5, -0.5, 0.25], [0.5, 0.5, 0.25]]] * 4, dtype=float)
    for k in range(4):
        bad[k, k, k % 3] = np.nan
    Y = np.concatenate([Y, bad])
    out = {}
    for name, rho in (("thin", 0.0), ("thick", [0.03, 0.02])):
        out["self_" + name] = ap.self_clearance(_Stub([(0, 1), (2, 3)], [(0, 1)], rho=rho), Y)
        out["self_swapped_" + name] = ap.self_clearance(_Stub([(2, 3), (0, 1)], [(0, 1)], rho=rho), Y)
        out["self_points_" + name] = ap.self_clearance(_Stub([(0, 0), (2, 2)], [(0, 1)], rho=rho), Y)
        # the second link's ends as sphere centres against the first link and a zero-length one
        spheres = [[*Y[k, 2], 0.1] for k in range(len(second))] + [[np.nan, 0.0, 0.0, 0.1]]
        for k, s in enumerate(spheres):
            out[f"link_{name}_{k}"] = ap.link_clearance(_Stub([(0, 1), (3, 3)], spheres=[s], rho=rho), Y)
    out["self_none"] = ap.self_clearance(_Stub([(0, 1), (2, 3)]), Y)
    out["link_none"] = ap.link_clearance(_Stub([(0, 1)]), Y)
    return out


ENTRIES = {"cells_clearance": _cells}
for _robot in ROBOTS:
    for _rad in RADII:
        ENTRIES[f"{_robot}_{_rad}_clearance"] = _clearance(_robot, _rad)
        ENTRIES[f"{_robot}_{_rad}_feet"] = _feet(_robot, _rad)
        ENTRIES[f"{_robot}_{_rad}_sweep_clearance"] = _sweeps(_robot, _rad)
    ENTRIES[f"{_robot}_r3_self_hinges"] = _hinges(_robot, "r3", "self")
for _rad in RADII:
    ENTRIES[f"ur10_table_{_rad}_link_hinges"] = _hinges("ur10_table", _rad, "link")


def conditions(name, arrays):
    """What keeps an entry from passing on inputs that exercise nothing: {"clearance_finite": count} for a clearance
    entry, {"hinges_active": count} for a hinge entry.  A zero count is an entry to change (its seed)."""
    cond = {}
    if "clearance" in name:
        cond["clearance_finite"] = int(sum(np.isfinite(v).sum() for v in arrays.values()))
    if "hinges" in name:
        cond["hinges_active"] = int(arrays["active"])
    return cond


# ---- the test ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parent():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


def test_the_table_is_the_recorded_one(parent):
    assert sorted(parent["entries"]) == sorted(ENTRIES)
    for name, rec in parent["entries"].items():
        assert all(count > 0 for count in rec["conditions"].values()), (name, rec["conditions"])
        assert ("clearance" in name) == ("clearance_finite" in rec["conditions"]), name
        assert ("hinges" in name) == ("hinges_active" in rec["conditions"]), name


@pytest.mark.parametrize("name", list(ENTRIES))
def test_returns_what_the_parent_returned(parent, name):
    arrays = ENTRIES[name]()
    rec = parent["entries"][name]
    got = digest(arrays)
    differ = sorted(key for key in set(got) | set(rec["sha"]) if got.get(key) != rec["sha"].get(key))
    print(name, "keys", len(got), conditions(name, arrays), "differ", differ)
    assert sorted(got) == sorted(rec["sha"]), "the returned keys changed"
    assert not differ, differ
    assert conditions(name, arrays) == rec["conditions"]
