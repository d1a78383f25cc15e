"""Per-goal obstacle scenes for the synthetic fixed-anchor problems of tests/synth_anchored.py: the graphs, goals and
start points of four of its cases, with spheres of this module's own -- three scenes per case, placed so that the scene a
goal is solved in shows in its very first cost.

The spheres synth_anchored places do not discriminate between scenes (every start point is clear of them in most goals).
Here, per case:
  scene A, scene B   for every goal b one masked node of the start point Y0[b] lies 1 to 3 cm INSIDE a sphere made for it
                     (`inside[s][b]` = (node, sphere)), every hidden point of every goal stays at least MIN_CLEAR outside
                     every sphere, and A and B share no sphere; the rest are fillers, placed as synth_anchored places its
  scene C            empty (count 0)
  near9              scene A has exactly 128 spheres, nine of them 6 to 20 mm from near_node's hidden point (within NEAR_TAU
                     of it in every goal: the near list overflows); its stride is therefore 128, the largest a scene set takes
  every other case   the stride is greater than every count
Padding rows -- from a scene's count up to the stride -- are NaN: a kernel that reads one returns a NaN cost.

Plain module (numpy only at import).  tests/test_anchored_scenes_host.py asserts every condition above and runs the CPU
twin under all three scenes; tests/test_anchored_scenes_gpu.py launches the same problems.  A placement that fails a
condition gets another seed HERE (SEEDS), never in synth_anchored."""
import functools
import types

import numpy as np

import synth_anchored as sa

B = sa.B
N_SCENE = 3
SCENE_ID = np.array([0, 1, 2, 0, 1, 2, 0, 1], dtype=np.int32)      # the scene of each of the 8 goals
INSIDE = (0.01, 0.03)           # how deep the chosen node of a start point lies inside its sphere
NEAR_COUNT = 9

# case -> (spheres of scene A, of scene B, stride)
CASES = {
    "a9_full": (96, 37, 100),
    "a20_full": (64, 50, 70),
    "near9": (128, 40, 128),
    "a9_noobs": (20, 9, 24),
}
SEEDS = {}                      # case -> seed, where the default 0 failed a condition of the host test


def _unit(rng):
    u = rng.randn(3)
    return u / np.linalg.norm(u)


def _outside(flat, s):
    """every hidden point at least MIN_CLEAR outside the sphere s = (c, r)"""
    return (np.linalg.norm(flat - s[:3], axis=1) - s[3]).min() > sa.MIN_CLEAR


def _biting_sphere(rng, flat, y0, nodes):
    """(node, sphere): a sphere with y0[node] INSIDE[0] .. INSIDE[1] deep in it and every hidden point outside, for the
    first of `nodes` (tried in random order, many times) that has room for one."""
    for _ in range(20000):
        i = int(nodes[rng.randint(len(nodes))])
        r = rng.uniform(0.03, 0.12)
        depth = rng.uniform(*INSIDE)
        s = np.array([*(y0[i] + _unit(rng) * (r - depth)), r])
        if _outside(flat, s):
            return i, s
    raise AssertionError("no room for a sphere around a start point")


def _scene(rng, p, Y0, count, near_node=None):
    """`count` spheres [count, 4] (c, r) and, per goal, the (node, sphere) pair that bites."""
    flat = p.P.reshape(-1, 3)
    masked = np.flatnonzero(p.mask)
    obs, inside = [], []
    for b in range(B):
        i, s = _biting_sphere(rng, flat, Y0[b], masked)
        inside.append((i, len(obs)))
        obs.append(s)
    if near_node is not None:
        for _ in range(NEAR_COUNT):
            for _ in range(20000):
                r = rng.uniform(0.05, 0.15)
                s = np.array([*(p.P[0, near_node] + _unit(rng) * (r + rng.uniform(*sa.NEAR_BAND))), r])
                if _outside(flat, s):
                    obs.append(s)
                    break
            else:
                raise AssertionError("no room for a near sphere")
    while len(obs) < count:
        s = np.array([*(1.2 * rng.randn(3)), rng.uniform(0.05, 0.2)])
        if _outside(flat, s):
            obs.append(s)
    obs = np.array(obs).reshape(-1, 4)
    # a walk visits the spheres in row order: shuffle, so that the spheres that bite are not the first rows
    perm = rng.permutation(len(obs))
    where = np.argsort(perm)
    return obs[perm], [(i, int(where[k])) for i, k in inside]


@functools.lru_cache(maxsize=None)
def build(cid):
    """The scenes of a case: a namespace with
      p                   synth_anchored.build(cid) (graph, goals, hidden points; its own spheres play no part)
      Y0 [B, N, 3]        synth_anchored.start_points(cid)
      scenes              [A, B, C]: arrays [m_s, 4] of (centre, radius)
      counts, stride      [3] int32; rows per scene of `obs`
      obs [3, stride, 4]  (centre, SQUARED radius) as gik_scene_set.d_obs takes it, padding rows NaN
      inside              [A, B]: per goal the (node, sphere) whose sphere the start point's node lies in
      near_node           near9: the node with NEAR_COUNT spheres of scene A next to it
    Arrays are shared between callers: do not write to them."""
    nA, nB, stride = CASES[cid]
    p = sa.build(cid)
    Y0 = sa.start_points(cid)
    rng = np.random.RandomState(SEEDS.get(cid, 0) + 104729 * sorted(CASES).index(cid) + 17)
    near_node = p.near_node if cid == "near9" else None
    A, inA = _scene(rng, p, Y0, nA, near_node)
    Bs, inB = _scene(rng, p, Y0, nB)
    scenes = [A, Bs, np.zeros((0, 4))]
    counts = np.array([len(s) for s in scenes], dtype=np.int32)
    obs = np.full((N_SCENE, stride, 4), np.nan)
    for s, sc in enumerate(scenes):
        obs[s, :len(sc), :3] = sc[:, :3]
        obs[s, :len(sc), 3] = sc[:, 3] ** 2
    for a in (*scenes, counts, obs, Y0):
        a.setflags(write=False)
    return types.SimpleNamespace(cid=cid, p=p, Y0=Y0, scenes=scenes, counts=counts, stride=stride, obs=obs, inside=[inA, inB],
                                 near_node=near_node)


def with_scene(p, spheres):
    """The problem p of synth_anchored.build with `spheres` [m, 4] (c, r) for obstacles: what sa.anchored_desc and
    sa.anchor_terms read."""
    q = types.SimpleNamespace(**vars(p))
    q.obs = np.asarray(spheres, dtype=np.float64).reshape(-1, 4)
    return q


def anchor_terms(cid, s, b):
    """synth_anchored.anchor_terms of goal b under scene s: the pinned terms, then a lower hinge per (masked node, sphere of
    the scene) in row order."""
    sc = build(cid)
    return sa.anchor_terms(with_scene(sc.p, sc.scenes[s]), b)
