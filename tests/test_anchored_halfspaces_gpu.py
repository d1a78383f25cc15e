"""Half-space obstacles (floors, walls) in the fixed-anchor solve on the MI355X (AnchoredProblem(halfspaces=...),
gik_anchored_attach_halfspaces): the known answers of the half-space builds against numpy, inactive half-spaces changing
nothing, the configurations under the floor that nothing else sees, whole links kept out by node margins, the clearance
kernel and its merge into every clearance, the pipeline on random goals, restarts, scenes and tracking on top, the refusals,
and which compiled kernels ran.  One wavefront per problem.
The points and the mirror's own tests: tests/test_anchored_halfspaces_host.py."""
import functools
import types

import numpy as np
import pytest

from conftest import make_graph
from parity_util import anchored_numpy, anchored_numpy_terms
from test_anchored_halfspaces_host import FLOOR, RHO, WALL, blind_spot_sample, halfspace_points, point_margins

pytestmark = pytest.mark.gpu

TOL = dict(pos_tol=0.01, rot_tol=0.01, clear_tol=1e-4)
KEYS = ("x", "q", "stop", "iterations", "pos_err", "rot_err", "clearance")
HALF_BOUND = -np.sqrt(1e-9)      # what f < 1e-9 leaves of a hinge: no residual mu - s exceeds sqrt(f)


def _eight():
    """Eight planes that every point within 3 m of the origin is 2 m and more beyond: unit normals, d0 = 5."""
    n = np.random.RandomState(8).randn(8, 3)
    n /= np.linalg.norm(n, axis=1)[:, None]
    return tuple((*row, 5.0) for row in n.tolist())


PLANES = {1: (FLOOR,), 2: (FLOOR, WALL), 8: _eight()}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _np(t):
    return t.detach().cpu().numpy()


def _rs():
    from graphik_amd.solvers import riemannian_solver as rs
    return rs


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64) if x.dtype == np.float64 else x


def _host(res, keys=KEYS):
    out = {k: _np(res[k]) for k in keys if k in res}
    if "attempt" in res:
        out["attempt"] = _np(res["attempt"])
    return out


def _same_rows(a, b, sel_a=slice(None), sel_b=slice(None), keys=KEYS):
    return all(np.array_equal(_bits(a[k][sel_a]), _bits(b[k][sel_b])) for k in keys)


def _table():
    from graphik_amd.utils import table_environment
    return tuple(tuple(float(v) for v in (*c, r)) for c, r in table_environment())


@functools.lru_cache(maxsize=None)
def _problem(planes=(FLOOR,), margin=None, rho=0.0, link_hinges=False, spheres=(), self_pairs=None, name="ur10"):
    """A device problem: the robot's skeleton as capsules of radius rho, spheres (x, y, z, r), planes (None: no half-spaces),
    margin None (from the radii), a scalar, "points" (point_margins) or a tuple."""
    robot, graph = make_graph(name)
    for idx, s in enumerate(spheres):
        graph.add_spherical_obstacle(f"o{idx}", np.asarray(s[:3], dtype=float), float(s[3]))
    kw = {}
    if planes is not None:
        if isinstance(margin, str):
            margin = tuple(point_margins(_rs().AnchoredProblem(make_graph(name)[1], host_only=True)).tolist())
        kw = dict(halfspaces=[list(p) for p in planes], halfspace_margin=list(margin) if isinstance(margin, tuple) else margin)
    ap = _rs().AnchoredProblem(graph, link_radius=rho, link_hinges=link_hinges, self_pairs=self_pairs, **kw)
    assert ap.template.info["anchored"] == 1 + (2 if link_hinges else 0) + (8 if planes is not None else 0)
    return robot, graph, ap


# ---- 1. known answers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_half", [1, 8])
@pytest.mark.parametrize("link_hinges", [False, True])
@pytest.mark.parametrize("scene", ["none", "table"])
def test_halfspace_known_answers(torch_cuda, n_half, link_hinges, scene):
    """cost / grad / hess / cost_and_grad of the half-space builds against anchored_numpy (+ link_hinge_terms_host) +
    halfspace_terms_host: 1e-12 relative, the project's kernel tolerance, at the six points of the host test (deep inside,
    on the boundary, an unmasked node below the floor, margins 0 and 0.03), on both builds (anchored = 9 and 11), with the
    floor alone and with eight planes that every masked node is beyond at every point, without spheres and with the table."""
    robot, graph, ap = _problem(PLANES[n_half], "points", RHO, link_hinges, _table() if scene == "table" else ())
    T = ap.template
    assert T.n_half == n_half and T.info["anchored"] == (11 if link_hinges else 9)
    Nf = len(ap.free)
    Y, ga, W = (np.array(a) for a in halfspace_points())
    f = _np(T.cost(Y, ga))
    G = _np(T.grad(Y, ga))
    H = _np(T.hess(Y, W, ga))
    f2, G2 = T.cost_and_grad(Y, ga)
    assert np.array_equal(_np(f2), f) and np.array_equal(_np(G2), G)
    n_act, worst = 0, [0.0, 0.0, 0.0]
    n_masked = int((ap.obs_mask == 1).sum())
    for b in range(len(Y)):
        fr, Gr, Hr = anchored_numpy(ap, Nf, Y[b], W[b], ga[b])
        fh, Gh, Hh = ap.halfspace_terms_host(Y[b], W[b])
        if n_half == 8:
            assert len(ap.last_half_active) == 8 * n_masked
        fr, Gr, Hr = fr + fh, Gr + Gh, Hr + Hh
        if link_hinges:
            fl, Gl, Hl = ap.link_hinge_terms_host(Y[b], W[b], ga[b])
            fr, Gr, Hr = fr + fl, Gr + Gl, Hr + Hl
        n_act += fh > 0
        err = [abs(f[b] - fr) / abs(fr), np.abs(G[b] - Gr).max() / np.abs(Gr).max(), np.abs(H[b] - Hr).max() / np.abs(Hr).max()]
        worst = [max(w, e) for w, e in zip(worst, err)]
        assert max(err) <= 1e-12, (b, err, fh / fr)
        if fh > 0:      # the half-space share is there: without it the cost is off by far more than the bar
            assert f[b] - (fr - fh) > 0.5 * fh
    print(f"n_half {n_half} link_hinges {link_hinges} {scene}: {n_act} of 6 points with a half-space share, worst errors "
          f"f {worst[0]:.2e} G {worst[1]:.2e} H {worst[2]:.2e}")
    assert n_act >= (6 if n_half == 8 else 3)
    assert np.array_equal(_np(T.proj(Y, W)), W)


def test_known_answers_on_the_largest_template(torch_cuda):
    """A hand-made chain of 21 free nodes, every one masked: 63 live lanes and one idle, the largest template the 9-slot
    context takes; the margin row is read at rows 0 .. 20 and, by the idle lane, at the dump row.  Floor, wall and a slanted
    plane, margins 0 .. 0.05."""
    from graphik_amd.engine import Template
    N = 21
    ti, tj = np.arange(N - 1, dtype=np.int32), np.arange(1, N, dtype=np.int32)
    rng = np.random.RandomState(21)
    P = np.cumsum(0.2 * rng.randn(N, 3), axis=0)
    target = ((P[ti] - P[tj]) ** 2).sum(-1)
    anchor = np.array([P[0] + (0.1, 0.0, 0.0), (0.0, 0.0, 0.0)])
    goal = P[-1] + (0.0, 0.1, 0.0)
    pins = [(0, 0, 1, 0.01), (N - 1, 1, 1, 0.01)]
    desc = dict(anchor_pos=anchor, n_goal_anchor=1, term_target=target, pin_node=[p[0] for p in pins],
                pin_anchor=[p[1] for p in pins], pin_kind=[p[2] for p in pins], pin_target=[p[3] for p in pins],
                obs=np.zeros((0, 4)), obs_node_mask=np.ones(N, dtype=np.int32), full_N=N + 2,
                free_full_index=list(range(N)), anchor_full_index=[N, N + 1], axis_length=1.0)
    T = Template(N, 3, ti, tj, np.ones(N - 1, dtype=np.int32), None, anchored=desc)
    assert T.info["max_terms_per_node"] == 9 and T.info["anchored"] == 1
    s = np.sqrt(0.5)
    planes = np.array([FLOOR, WALL, (s, 0.0, s, -0.2)])
    mu = np.linspace(0.0, 0.05, N)
    T.attach_halfspaces(planes, mu)
    assert T.info["anchored"] == 9
    B = 3
    Y = P[None] + 0.05 * rng.randn(B, N, 3)
    W = rng.randn(B, N, 3)
    ga = np.repeat(goal[None], B, axis=0)
    mirror = types.SimpleNamespace(free=list(range(N)), obs_mask=np.ones(N, dtype=np.int32), halfspaces=planes, halfspace_margin=mu)
    f, G, H = _np(T.cost(Y, ga)), _np(T.grad(Y, ga)), _np(T.hess(Y, W, ga))
    for b in range(B):
        rows = np.array([anchor[0], goal])
        fr, Gr, Hr = anchored_numpy_terms((ti, tj, np.ones(N - 1, dtype=np.int32), target),
                                          (np.array([0, N - 1]), rows, np.array([0.01, 0.01]), np.array([1, 1])), Y[b], W[b])
        fh, Gh, Hh = _rs().AnchoredProblem.halfspace_terms_host(mirror, Y[b], W[b])
        assert fh > 0 and len(mirror.last_half_active) >= 8
        fr, Gr, Hr = fr + fh, Gr + Gh, Hr + Hh
        err = [abs(f[b] - fr) / abs(fr), np.abs(G[b] - Gr).max() / np.abs(Gr).max(), np.abs(H[b] - Hr).max() / np.abs(Hr).max()]
        assert max(err) <= 1e-12, (b, err)
    # the clearance kernel on the same handle: 21 nodes x 3 planes = 63 pairs, one lane idle
    full = np.concatenate([Y, np.repeat(anchor[None, :1], B, axis=0), ga[:, None]], axis=1)
    mirror.link_rows, mirror.link_radius = np.zeros((0, 2), dtype=np.int32), np.zeros(0)
    mirror._halfspace_s = _rs().AnchoredProblem._halfspace_s
    want = _rs().AnchoredProblem.halfspace_clearance(mirror, full)
    assert np.array_equal(_bits(_np(T.anchored_halfspace_clearance(full))), _bits(want))


# ---- 2. inactive half-spaces change nothing ------------------------------------------------------------------------------
def test_inactive_halfspaces_change_nothing(torch_cuda):
    """A floor at z = -10: no node ever reaches it.  12 goals from the same Y0 without and with it: x, f, iterations,
    inner_total, stop, n_accept, gradnorm and all 32 trace rows are equal as numbers."""
    out = []
    for planes in (None, ((0.0, 0.0, 1.0, -10.0),)):
        robot, graph, ap = _problem(planes)
        assert ap.template.info["anchored"] == (1 if planes is None else 9)
        rng = np.random.RandomState(12)
        Tg = robot.fk_batch(rng.uniform(-np.pi, np.pi, (12, robot.n)))
        Y0 = ap.seed_points(rng.uniform(-np.pi, np.pi, (12, robot.n)))
        out.append(ap.template.solve(Y0, ap.goal_anchors(Tg), trace_cap=32))
    a, b = out
    for k in ("x", "f", "iterations", "inner_total", "stop", "n_accept", "gradnorm"):
        assert np.array_equal(_np(a[k]), _np(b[k])), k
    for k in a["trace"]:
        assert np.array_equal(_np(a["trace"][k]), _np(b["trace"][k]), equal_nan=True), k
    assert int(_np(a["iterations"]).max()) > 1


# ---- 3. the blind spot closes; 4. whole links through node margins ---------------------------------------------------------
def _under_the_floor16():
    sel, q, Y = blind_spot_sample()
    assert len(sel) == 16
    return q[sel]


def _joint_z(ap, x):
    return x[:, [ap.base.graph.index(f"p{i}") for i in range(1, 6)], 2]


def test_the_blind_spot_closes(torch_cuda):
    """UR10 without spheres, floor (0, 0, 1, -0.1), margin 0: the first 16 of RandomState(7)'s configurations whose end
    effector is more than 5 cm above the floor and that have a joint point more than 1 cm below it, each asked for its own
    pose and seeded with itself.  Without half-spaces the solve stops at once, still under.  With them every seed costs at
    least (1 cm)^2, every answer costs less than its seed after at least one iteration, an answer with f < 1e-9 has no node
    more than sqrt(1e-9) beyond the plane, and the clearance returned is the device half-space clearance of x bit for bit."""
    robot, graph, off = _problem(None)
    _, _, on = _problem((FLOOR,), 0.0)
    q = _under_the_floor16()
    T = robot.fk_batch(q)
    P = _host(off.solve(T, q_init=q))
    assert int(P["iterations"].max()) <= 1 and np.all(_joint_z(off, P["x"]).min(axis=1) < -0.1 - 0.01)
    assert np.all(np.isposinf(P["clearance"]))      # (no sphere, no half-space: nothing is measured)
    Y0, ga = on.seed_points(q), on.goal_anchors(T)
    f_seed = _np(on.template.cost(Y0, ga))
    assert np.all(f_seed >= 0.01 ** 2)
    A = on.solve(T, q_init=q)
    f, it, cl = _np(A["f"]), _np(A["iterations"]), _np(A["clearance"])
    conv = f < 1e-9
    print(f"floor on: {int(conv.sum())} of 16 converge, clearance {cl.min():.2e} .. {cl.max():.2e}, iterations {it.min()} .. "
          f"{it.max()}, pos_err of the converged {_np(A['pos_err'])[conv].max() if conv.any() else None}")
    assert np.all(f < f_seed) and np.all(it >= 1)
    half = _np(on.template.anchored_halfspace_clearance(A["x"]))
    assert np.all(half[conv] >= HALF_BOUND)
    assert np.array_equal(_bits(cl), _bits(half))
    assert np.array_equal(_bits(half), _bits(on.halfspace_clearance(_np(A["x"]))))


def test_whole_links_through_node_margins(torch_cuda):
    """The same 16 with capsules of 3 cm and the default margin (the radius at every masked node), clearance_mode="links":
    converged answers have their link clearance at or above -sqrt(1e-9).  The goal end is 5 cm - 3 cm above the floor by
    construction and p0 10 cm - 3 cm, so the constant ends cannot push it lower."""
    robot, graph, on = _problem((FLOOR,), None, RHO)
    assert np.array_equal(on.halfspace_margin, np.where(on.obs_mask == 1, RHO, 0.0))
    q = _under_the_floor16()
    T = robot.fk_batch(q)
    A = on.solve(T, q_init=q, clearance_mode="links")
    f, cl = _np(A["f"]), _np(A["clearance"])
    conv = f < 1e-9
    print(f"capsules of 3 cm: {int(conv.sum())} of 16 converge, link clearance {cl.min():.2e} .. {cl.max():.2e}")
    assert np.all(cl[conv] >= HALF_BOUND)
    assert np.array_equal(_bits(cl), _bits(_np(on.template.anchored_halfspace_clearance(A["x"], links=True))))
    assert np.all(_np(A["iterations"]) >= 1)


# ---- 5. the clearance kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5])
def test_clearance_kernel_against_the_mirror(torch_cuda, B):
    """Nodes and links, bit for bit the numpy mirror; a NaN row poisons its goal alone; what anchored_clearance and
    anchored_link_clearance report on the table is min(spheres, half-spaces) of the same points."""
    robot, graph, on = _problem((FLOOR, WALL), None, RHO, False, _table())
    _, _, off = _problem(None, None, RHO, False, _table())
    q = np.random.RandomState(50 + B).uniform(-np.pi, np.pi, (B, robot.n))
    Y = on.base.seed_points(q)
    T = on.template
    for links in (False, True):
        got = _np(T.anchored_halfspace_clearance(Y, links=links))
        assert got.shape == (B,) and np.array_equal(_bits(got), _bits(on.halfspace_clearance(Y, links=links)))
        spheres = _np((off.template.anchored_link_clearance if links else off.template.anchored_clearance)(Y))
        folded = _np((T.anchored_link_clearance if links else T.anchored_clearance)(Y))
        assert np.array_equal(_bits(folded), _bits(np.minimum(spheres, got)))
    assert np.any(_np(T.anchored_halfspace_clearance(Y)) < 0) or B == 1
    if B > 1:
        Yn = Y.copy()
        Yn[B // 2, on.free[list(on.free_names).index("p3")], 1] = np.nan
        for links in (False, True):
            got = _np(T.anchored_halfspace_clearance(Yn, links=links))
            ref = _np(T.anchored_halfspace_clearance(Y, links=links))
            assert np.isnan(got[B // 2]) and np.array_equal(_bits(np.delete(got, B // 2)), _bits(np.delete(ref, B // 2)))
            folded = _np((T.anchored_link_clearance if links else T.anchored_clearance)(Yn))
            assert np.isnan(folded[B // 2]) and not np.isnan(np.delete(folded, B // 2)).any()


def test_folded_clearance_of_links_and_self_and_the_sweep(torch_cuda):
    """clearance_mode="links+self": the clearance a solve returns is min(link spheres, self, half-spaces over the links)
    of its x.  sweep_clearance with samples = 2 against _sweep_min_host of the folded mirror, to the 1e-11 the sphere sweep
    is held to (tests/test_anchored_links_gpu.py: the device realization is within 1e-12 per coordinate of the host's)."""
    robot, graph, on = _problem((FLOOR, WALL), None, RHO, False, _table(), "auto")
    _, _, off = _problem(None, None, RHO, False, _table(), "auto")
    rng = np.random.RandomState(5)
    q = rng.uniform(-np.pi, np.pi, (5, robot.n))
    A = on.solve(robot.fk_batch(q + 0.05), q_init=q, clearance_mode="links+self")
    x = A["x"]
    want = np.minimum(np.minimum(_np(off.template.anchored_link_clearance(x)), _np(off.template.anchored_self_clearance(x))),
                      _np(on.template.anchored_halfspace_clearance(x, links=True)))
    assert np.array_equal(_bits(_np(A["clearance"])), _bits(want))
    qa, qb = q, q + 0.2 * rng.randn(*q.shape)
    got = _np(on.sweep_clearance(qa, qb, 2))
    folded = lambda Y: np.minimum(on.link_clearance(Y), on.halfspace_clearance(Y, links=True))      # noqa: E731
    assert np.abs(got - on._sweep_min_host(qa, qb, 2, folded)).max() < 1e-11
    spheres_only = _np(off.sweep_clearance(qa, qb, 2))
    assert np.all(got <= spheres_only) and np.any(got < spheres_only)


# ---- 6. the pipeline on random goals ----------------------------------------------------------------------------------
def test_pipeline_property_on_random_goals(torch_cuda):
    """256 random cold goals, table and floor, link hinges on: every problem stops by a legal rule, at least one converges,
    every converged answer (f < 1e-9) has no masked node more than sqrt(1e-9) beyond the floor's margin and meets the link
    bound of the spheres (_clear_bound of tests/test_anchored_link_hinges_gpu.py), and the anchors of x are the constants
    they were given."""
    robot, graph, on = _problem((FLOOR,), None, RHO, True, _table())
    _, _, off = _problem(None, None, RHO, True, _table())
    rng = np.random.RandomState(256)
    T = robot.fk_batch(rng.uniform(-np.pi, np.pi, (256, robot.n)))
    A = on.solve(T, clearance=True, clearance_mode="links")
    stop, f, x = _np(A["stop"]), _np(A["f"]), _np(A["x"])
    assert np.all((stop == 0) | (stop == 1))
    conv = f < 1e-9
    assert conv.any()
    half = _np(on.template.anchored_halfspace_clearance(A["x"]))
    spheres = _np(off.template.anchored_link_clearance(A["x"]))
    print(f"{int(conv.sum())} of 256 converge; of the converged: half-space clearance {half[conv].min():.2e} .. {half[conv].max():.2e}, "
          f"link clearance {spheres[conv].min():.2e}; of all: {int((half < -1e-4).sum())} with a node beyond the floor")
    assert np.all(half[conv] >= HALF_BOUND)
    R = float(on.obstacles[:, 3].min() + on.link_radius.min())
    assert np.all(spheres[conv] >= np.sqrt(R * R - np.sqrt(1e-9)) - R)
    assert np.array_equal(_bits(_np(A["clearance"])),
                          _bits(np.minimum(spheres, _np(on.template.anchored_halfspace_clearance(A["x"], links=True)))))
    n_const = len(on.anchors) - on.n_goal_anchor
    assert np.abs(x[:, on.anchors[:n_const]] - on.anchor_pos[None, :n_const]).max() < 1e-12
    assert np.abs(x[:, on.anchors[n_const:]] - on.goal_anchors(T).reshape(256, -1, 3)).max() < 1e-12


# ---- 7. restarts, scenes and tracking -----------------------------------------------------------------------------------
def test_restarts_run_on_the_halfspace_problem(torch_cuda):
    """solve(retries=2) on the 16 configurations under the floor: rows that did not fail keep attempt 0's bits, every
    replaced row equals the one-goal seeded solve from retry_seeds_host's angles on the same problem."""
    rs = _rs()
    robot, graph, on = _problem((FLOOR,), 0.0)
    q = _under_the_floor16()
    T = robot.fk_batch(q)
    lo, hi = robot.limits_arrays()
    seed = 43
    P = _host(on.solve(T, q_init=q))
    R = _host(on.solve(T, q_init=q, retries=2, retry_seed=seed, **TOL))
    att = R["attempt"]
    assert att.min() >= 0 and att.max() <= 2
    print("attempt histogram", np.bincount(att, minlength=3).tolist(), "clear after", int((R["clearance"] >= -1e-4).sum()), "of 16")
    first = att == 0
    failed = rs.anchored_retry_failed(P["stop"], P["pos_err"], P["rot_err"], P["clearance"], **TOL)
    assert not np.any(att[~failed]) and _same_rows(R, P, first, first)
    for g in np.flatnonzero(att > 0):
        q0 = rs.retry_seeds_host(seed, [g], int(att[g]), lo, hi)
        S = _host(on.solve(T[g:g + 1], q_init=q0))
        assert _same_rows(R, S, slice(g, g + 1)), (g, att[g])


@pytest.mark.parametrize("link_hinges", [False, True])
def test_scenes_are_bit_identical_to_their_own_templates(torch_cuda, link_hinges):
    """Two scenes, 5 goals, either scene build: each goal equals, bit for bit, the goal solved on a problem created with its
    scene's spheres and the same half-spaces -- the room stays, the spheres vary."""
    table = _table()
    scenes = (table[:40], table[60:])
    robot, graph, ap = _problem((FLOOR, WALL), None, RHO, link_hinges, table)
    q = np.random.RandomState(9).uniform(-np.pi, np.pi, (5, robot.n))
    T = robot.fk_batch(q + 0.05)
    ids = np.array([0, 1, 1, 0, 1])
    S = ap.scene_set([np.array(s) for s in scenes])
    keys = KEYS + ("f", "inner_total")
    got = _host(ap.solve(T, q_init=q, clearance=True, clearance_mode="links", scenes=S, scene_id=ids), keys)
    assert int(got["iterations"].max()) > 1
    for s in (0, 1):
        _, _, own = _problem((FLOOR, WALL), None, RHO, link_hinges, scenes[s])
        sel = np.flatnonzero(ids == s)
        ref = _host(own.solve(T[sel], q_init=q[sel], clearance=True, clearance_mode="links"), keys)
        assert _same_rows(got, ref, sel, slice(None), keys), s


def test_tracking_runs_on_the_halfspace_problem(torch_cuda):
    """solve_trajectory(sweep=2) on 8 paths x 4 waypoints returns finite clearances and sweep clearances; with the room
    folded in the sweep sees the floor and the wall (some value is below every sphere's)."""
    robot, graph, on = _problem((FLOOR, WALL), None, RHO, False, _table())
    qs = np.random.RandomState(84).uniform(-np.pi, np.pi, (8, robot.n))
    path = np.stack([robot.fk_batch(qs + 0.05 * (l + 1)) for l in range(4)], axis=1)      # [8, 4, 4, 4]
    qt, _, info = on.solve_trajectory(path, qs, clearance_mode="links", sweep=2)
    assert qt.shape == (8, 4, robot.n) and info["sweep_clearance"].shape == (8, 4)
    assert np.all(np.isfinite(info["sweep_clearance"])) and np.all(np.isfinite(info["clearance"]))


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------
def _star20():
    """The 20-slot variant: a free node with 11 terms (the hand-made template of the link- and self-hinge tests)."""
    from graphik_amd.engine import Template
    N, terms = 12, [(0, k) for k in range(1, 12)]
    ti, tj = np.array([t[0] for t in terms]), np.array([t[1] for t in terms])
    return Template(N, 3, ti, tj, np.ones(len(terms), dtype=np.int32), None,
                    anchored=dict(anchor_pos=np.zeros((1, 3)), n_goal_anchor=0, term_target=np.ones(len(terms)),
                                  pin_node=[], pin_anchor=[], pin_kind=[], pin_target=[], obs=np.zeros((0, 4)),
                                  obs_node_mask=np.ones(N, dtype=np.int32), full_N=13, free_full_index=list(range(1, 13)),
                                  anchor_full_index=[0], axis_length=1.0))


def test_refusals(torch_cuda):
    """Each refusal of the two C entries, and of the two attach calls that may no longer follow, has its own message and
    leaves the handle as it was: flags, kernels' form, LDS bytes, occupancy."""
    import ctypes as C
    from graphik_amd import _ffi
    rs = _rs()
    robot, graph = make_graph("ur10")
    dbl = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))      # noqa: E731

    def refused(tpl, match, n_half=1, planes=(FLOOR,), mu=0.0, null=False):
        before = dict(tpl.info)
        h = np.ascontiguousarray(planes, dtype=np.float64).reshape(-1, 4)
        m = np.full(tpl.N, mu) if np.isscalar(mu) else np.asarray(mu, dtype=np.float64)
        with pytest.raises(_ffi.GikError, match=match):
            tpl._call("gik_anchored_attach_halfspaces", tpl._h, n_half, None if null else dbl(h), None if null else dbl(m))
        tpl._read_info()
        assert tpl.info == before

    ap = rs.AnchoredProblem(graph, link_radius=RHO, self_pairs="auto")
    tpl = ap.template
    refused(ap.base.template, "must be a fixed-anchor template")
    refused(tpl, "n_half must be within 1 .. 8", n_half=0)
    refused(tpl, "n_half must be within 1 .. 8", n_half=9, planes=[FLOOR] * 9)
    refused(tpl, "null array", null=True)
    refused(tpl, "not finite", planes=[(0.0, 0.0, 1.0, np.inf)])
    refused(tpl, "not finite", planes=[(np.nan, 0.0, 1.0, 0.0)])
    refused(tpl, "unit length", planes=[(0.0, 0.0, 1.0 + 1e-9, -0.1)])
    refused(tpl, "unit length", planes=[(0.0, 0.0, 0.0, -0.1)])
    masked = int(np.flatnonzero(ap.obs_mask == 1)[0])
    for bad in (-1e-3, np.nan, np.inf):
        mu = np.zeros(tpl.N)
        mu[masked] = bad
        refused(tpl, rf"node_margin\[{masked}\] must be finite and at least 0", mu=mu)
    refused(_star20(), "20-slot variant, which has none")
    hinged = rs.AnchoredProblem(graph, link_radius=RHO, self_pairs="auto", self_hinges=True).template
    refused(hinged, "self hinges are attached")
    assert hinged.info["anchored"] == 5
    # a margin at an unmasked node is not read
    mu = np.zeros(tpl.N)
    mu[int(np.flatnonzero(ap.obs_mask == 0)[0])] = np.nan
    assert not (tpl.info["anchored"] & 8)
    tpl.attach_halfspaces([FLOOR], mu)
    assert tpl.n_half == 1 and tpl.info["anchored"] == 9
    refused(tpl, "half-spaces already attached")
    before = dict(tpl.info)
    with pytest.raises(_ffi.GikError, match="half-spaces are attached"):
        tpl.attach_self_hinges()
    tpl._read_info()
    assert tpl.info == before
    bare = rs.AnchoredProblem(graph, links=[], halfspaces=[FLOOR])
    before = dict(bare.template.info)
    with pytest.raises(_ffi.GikError, match="half-spaces are attached; link hinges come before"):
        bare.template.attach_links([bare.free[0]], [bare.free[1]], [RHO], hinges=True)
    bare.template._read_info()
    assert bare.template.info == before and bare.template.info["anchored"] == 9
    # gik_anchored_halfspace_clearance
    Y = torch_cuda.zeros(2, tpl.full_N * 3, dtype=torch_cuda.float64, device=tpl.device)
    out = torch_cuda.full((2,), 7.0, dtype=torch_cuda.float64, device=tpl.device)

    def clearance_refused(t, match, links=0, y=Y, o=out):
        with pytest.raises(_ffi.GikError, match=match):
            t._call("gik_anchored_halfspace_clearance", t._h, None if y is None else y.data_ptr(), 2, links,
                    None if o is None else o.data_ptr(), None)
        torch_cuda.cuda.synchronize()
        assert np.all(_np(out) == 7.0)
    clearance_refused(ap.base.template, "must be a fixed-anchor template")
    clearance_refused(rs.AnchoredProblem(graph).template, "no half-spaces attached")
    clearance_refused(tpl, "links must be 0", links=2)
    clearance_refused(bare.template, "no links attached", links=1)
    clearance_refused(tpl, "null buffer", y=None)
    clearance_refused(tpl, "null buffer", o=None)
    tpl._call("gik_anchored_halfspace_clearance", tpl._h, Y.data_ptr(), 0, 0, out.data_ptr(), None)      # B == 0: nothing
    torch_cuda.cuda.synchronize()
    assert np.all(_np(out) == 7.0)


# ---- 9. which kernels ran ----------------------------------------------------------------------------------------------
def test_the_new_kernel_group_is_what_the_halfspace_templates_run(torch_cuda):
    """Each of the six instantiations of GIK_KERNELS_ANCH_HALF (named by tests/test_anchored_halfspaces_host.py) is what a
    template of the tests above launches: the solve, known-answer and scene kernels of the form gik_template_get_info
    reports -- 3-D, 9 slots, anchored = 9 and 11 -- at no more than 40 KB of LDS and four waves per CU."""
    ran = set()
    for link_hinges in (False, True):
        robot, graph, on = _problem((FLOOR,), None, RHO, link_hinges, _table())
        _, _, off = _problem(None, None, RHO, link_hinges, _table())
        info, base = on.template.info, off.template.info
        assert not info["is_block"] and info["anchored"] == (11 if link_hinges else 9) and info["max_terms_per_node"] == 9
        flags = "W_ANCH|W_LINKS|W_HALF" if link_hinges else "W_ANCH|W_HALF"
        # 8 planes of 4 doubles and a margin row of 34 doubles (the 33 tile rows, even) on top of the form's context
        assert info["lds_bytes"] - base["lds_bytes"] == 8 * 4 * 8 + 34 * 8
        print(f"anchored = {info['anchored']}: lds_bytes {info['lds_bytes']}, waves_per_cu {info['waves_per_cu']}")
        assert info["lds_bytes"] <= 40 * 1024 and info["waves_per_cu"] >= 4
        q = _under_the_floor16()[:2]
        T = robot.fk_batch(q)
        Y0, ga = on.seed_points(q), on.goal_anchors(T)
        assert np.all(_np(on.template.cost(Y0, ga)) > _np(off.template.cost(Y0, ga)))
        ran.add(f"kat_wave_kernel<3,9,{flags}>")
        A = on.solve(T, q_init=q)
        assert np.all(_np(A["iterations"]) >= 1)
        ran.add(f"rtr_wave_kernel<3,9,W_THETA1|{flags}>")
        S = on.scene_set([on.obstacles])
        Bs = on.solve(T, q_init=q, scenes=S)
        assert np.array_equal(_bits(_np(Bs["x"])), _bits(_np(A["x"])))
        ran.add(f"rtr_wave_scene_kernel<3,9,W_THETA1|{flags}>")
    assert len(ran) == 6
