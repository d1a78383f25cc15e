"""Self hinges in the fixed-anchor solve on the MI355X (AnchoredProblem(self_hinges=True), gik_anchored_attach_self_hinges): the
known answers of the six self builds against numpy, inactive hinges changing nothing, the self-colliding configurations
that no other term can move, the pipeline on random goals, scenes, restarts and tracking on top, the refusals, and which
compiled kernels ran.  One wavefront per problem; batches of 1, 5 and 65.
The points and the mirror's own tests: tests/test_anchored_self_hinges_host.py."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import REPO, make_graph
from parity_util import anchored_numpy
from test_anchored_self_hinges_host import RHO, hinge_configurations

pytestmark = pytest.mark.gpu

TOL = dict(pos_tol=0.01, rot_tol=0.01, clear_tol=1e-4)
KEYS = ("x", "q", "stop", "iterations", "pos_err", "rot_err", "clearance")
R_SELF = 2 * RHO


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


def _graph(name, spheres=None):
    """make_graph; "<robot>_table": with the table's spheres; spheres: [m, 4] (centre, radius) to add instead."""
    from graphik_amd.utils import table_environment
    robot, graph = make_graph(name.replace("_table", ""))
    if spheres is None:
        spheres = [(*c, r) for c, r in table_environment()] if name.endswith("_table") else []
    for idx, s in enumerate(spheres):
        graph.add_spherical_obstacle(f"o{idx}", np.asarray(s[:3], dtype=float), float(s[3]))
    return robot, graph


@functools.lru_cache(maxsize=None)
def _problem(name, self_hinges=True, link_hinges=False, rho=RHO, pairs="auto", extra_links=(), spheres=None):
    """A device problem: the robot's skeleton (and extra_links) as capsules of radius rho (scalar or one per link), self
    pairs "auto" or a tuple of (l, m); spheres: a tuple of (x, y, z, r) instead of the scene the name gives."""
    robot, graph = _graph(name, spheres)
    links = None
    if extra_links:
        links = [(f"p{i}", f"p{i + 1}") for i in range(robot.n)] + [tuple(l) for l in extra_links]
    ap = _rs().AnchoredProblem(graph, links=links, link_radius=rho if np.isscalar(rho) else list(rho),
                               self_pairs=pairs if isinstance(pairs, str) else [tuple(p) for p in pairs],
                               link_hinges=link_hinges, self_hinges=self_hinges)
    assert ap.template.info["anchored"] == 1 + (2 if link_hinges else 0) + (4 if self_hinges else 0)
    return robot, graph, ap


def _self_bound(R=R_SELF):
    """What f < 1e-9 leaves of a hinge (tests/test_anchored_link_hinges_gpu.py, _clear_bound): no residual R^2 - d exceeds
    sqrt(f), so the clearance sqrt(d) - R is at least sqrt(R^2 - sqrt(1e-9)) - R."""
    return np.sqrt(R * R - np.sqrt(1e-9)) - R


def _folded(ap, robot, seed, count, n_sample=512):
    """The first `count` of RandomState(seed).uniform(-pi, pi, (n_sample, n)) with an active self hinge, by the mirror."""
    q = np.random.RandomState(seed).uniform(-np.pi, np.pi, (n_sample, robot.n))
    Y, ga = ap.seed_points(q), ap.goal_anchors(robot.fk_batch(q))
    hit = [b for b in range(n_sample) if ap.self_hinge_terms_host(Y[b], np.zeros_like(Y[b]), ga[b])[0] > 0][:count]
    assert len(hit) == count
    return q[hit]


# ---- 5. known answers ----------------------------------------------------------------------------------------------
SIXTEEN = tuple((l, m) for l in range(7) for m in range(l + 2, 7)) + ((0, 7),)      # KUKA's 15 "auto" pairs and one more
CASES = {
    "ur10-table-10": dict(name="ur10_table", points="chosen"),
    "ur10-table-10-links-mixed": dict(name="ur10_table", link_hinges=True, rho=(0.03, 0.05, 0.02, 0.04, 0.03, 0.03), points=5),
    "lwa4d-15": dict(name="lwa4d", points="chosen"),
    "kuka-16-on-8-links": dict(name="kuka", pairs=SIXTEEN, extra_links=(("q2", "q4"),), points=5),
    "ur10-1-pair-links": dict(name="ur10", pairs=((1, 4),), link_hinges=True, points=1),
    "ur10-table-10-links-65": dict(name="ur10_table", link_hinges=True, points=65),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_self_hinge_known_answers(torch_cuda, case):
    """cost / grad / hess / cost_and_grad of the self builds against anchored_numpy + self_hinge_terms_host
    (+ link_hinge_terms_host): 1e-12 relative, the bar of test_link_hinge_known_answers.  UR10 with its 10 pairs at the
    configurations of the host test (seven clamp classes, parallel pairs), LWA4D with 15 (the other two, zero-length
    links), 16 explicit pairs on 8 links, one pair; radii 0.03 and mixed; the table and no obstacle; link hinges off and
    on; batches of 1, 5 and 65 (the 65: random configurations, most of them with nothing active)."""
    kw = dict(CASES[case])
    points = kw.pop("points")
    robot, graph, ap = _problem(**kw)
    T = ap.template
    assert T.self_hinges and len(ap.self_pairs) == (1 if "1-pair" in case else {"ur10": 10, "lwa4d": 15, "kuka": 16}[kw["name"].split("_")[0]])
    Nf = len(ap.free)
    if points == "chosen":
        c = hinge_configurations(kw["name"].replace("_table", ""))
        Y, ga = c["Y"].copy(), c["ga"].copy()
    else:
        q = _folded(ap, robot, 11, points) if points < 65 else np.random.RandomState(65).uniform(-np.pi, np.pi, (65, robot.n))
        Y, ga = ap.seed_points(q), ap.goal_anchors(robot.fk_batch(q))
    rng = np.random.RandomState(2)
    if points != "chosen":      # (off the constraint set: every free-free and anchor term has a residual; the chosen
        Y = Y + 0.004 * rng.randn(*Y.shape)      # points stay where their parallel and zero-length links are exactly that)
    W = rng.randn(*Y.shape)
    f = _np(T.cost(Y, ga))
    G = _np(T.grad(Y, ga))
    H = _np(T.hess(Y, W, ga))
    f2, G2 = T.cost_and_grad(Y, ga)
    assert np.array_equal(_np(f2), f) and np.array_equal(_np(G2), G)
    n_self, worst = 0, [0.0, 0.0, 0.0]
    for b in range(len(Y)):
        fr, Gr, Hr = anchored_numpy(ap, Nf, Y[b], W[b], ga[b])
        fs, Gs, Hs = ap.self_hinge_terms_host(Y[b], W[b], ga[b])
        fr, Gr, Hr = fr + fs, Gr + Gs, Hr + Hs
        if ap.link_hinges:
            fl, Gl, Hl = ap.link_hinge_terms_host(Y[b], W[b], ga[b])
            fr, Gr, Hr = fr + fl, Gr + Gl, Hr + Hl
        n_self += fs > 0
        err = [abs(f[b] - fr) / abs(fr), np.abs(G[b] - Gr).max() / np.abs(Gr).max(), np.abs(H[b] - Hr).max() / np.abs(Hr).max()]
        worst = [max(w, e) for w, e in zip(worst, err)]
        assert max(err) <= 1e-12, (b, err, fs / fr)
        # the self share of f is positive where the mirror says so: without it the cost is off by far more than the bar
        if fs > 0:
            assert f[b] - (fr - fs) > 0.5 * fs
    print(f"{case}: {len(Y)} points, {n_self} with a self share, worst errors f {worst[0]:.2e} G {worst[1]:.2e} H {worst[2]:.2e}")
    assert n_self >= 1 and (n_self == len(Y) or points != "chosen")
    assert np.array_equal(_np(T.proj(Y, W)), W)


# ---- 6. inactive hinges change nothing -----------------------------------------------------------------------------
def test_inactive_hinges_change_nothing(torch_cuda):
    """link_radius = 0 makes R = 0: no pair is ever active.  12 goals from the same Y0 with self hinges off and on: x, f,
    iterations, inner_total, stop, n_accept, gradnorm and all 32 trace rows are equal as numbers."""
    out = []
    for hinges in (False, True):
        robot, graph, ap = _problem("ur10", self_hinges=hinges, rho=0.0)
        assert ap.template.info["anchored"] == (5 if hinges else 1)
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


# ---- 7. the blind spot closes --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _self_colliding16():
    """The first 16 configurations of RandomState(0).uniform(-pi, pi, (2048, 7)) on KUKA (3 cm, "auto") whose mirror self
    clearance is below -1 cm."""
    robot, graph = make_graph("kuka")
    ap = _rs().AnchoredProblem(graph, host_only=True, link_radius=RHO, self_pairs="auto")
    q = np.random.RandomState(0).uniform(-np.pi, np.pi, (2048, 7))
    idx = np.flatnonzero(ap.self_clearance(ap.base.seed_points(q)) < -0.01)
    print(f"KUKA: {len(idx)} of 2048 uniform configurations are more than 1 cm inside themselves")
    assert len(idx) >= 16
    return q[idx[:16]]


def test_the_blind_spot_closes(torch_cuda):
    """16 KUKA configurations more than 1 cm inside themselves, each asked for its own pose and seeded with itself.
    Without self hinges the solve stops at once, still inside.  With them every seed costs at least (2 R delta - delta^2)^2
    (R = 0.06, delta = 0.01), every answer costs less than its seed after at least one iteration, an answer with f < 1e-9
    has its self clearance at or above what that f leaves, at least one of the 16 converges, and the clearance reported
    is the device self clearance of x bit for bit.  (Measured: NOTEBOOK 39.)"""
    robot, graph, off = _problem("kuka", self_hinges=False)
    _, _, on = _problem("kuka")
    q = _self_colliding16()
    T = robot.fk_batch(q)
    P = _host(off.solve(T, q_init=q, clearance_mode="links+self"))
    assert int(P["iterations"].max()) <= 1 and np.all(P["clearance"] < -0.01)
    Y0, ga = on.seed_points(q), on.goal_anchors(T)
    f_seed = _np(on.template.cost(Y0, ga))
    R, delta = R_SELF, 0.01
    assert np.all(f_seed >= (2 * R * delta - delta * delta) ** 2)
    A = on.solve(T, q_init=q, clearance_mode="links+self")
    f, it, cl = _np(A["f"]), _np(A["iterations"]), _np(A["clearance"])
    conv = f < 1e-9
    print(f"self hinges on: {int(conv.sum())} of 16 converge, self clearance {cl.min():.2e} .. {cl.max():.2e}, "
          f"iterations {it.min()} .. {it.max()}, pos_err of the converged {_np(A['pos_err'])[conv].max() if conv.any() else None}")
    assert np.all(f < f_seed) and np.all(it >= 1)
    assert np.all(cl[conv] >= _self_bound())
    assert conv.sum() >= 1
    assert np.array_equal(_bits(cl), _bits(_np(on.template.anchored_self_clearance(A["x"]))))


# ---- 8. the pipeline on random goals -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kuka", "kuka_table"])
def test_pipeline_property_on_random_goals(torch_cuda, name):
    """256 random cold KUKA goals with self hinges on: every problem stops by a legal rule, at least one converges, every
    converged answer (f < 1e-9) meets the self-clearance bound -- with the table attached the node bound as well -- and
    the anchors of x are the constants they were given."""
    robot, graph, on = _problem(name)
    rng = np.random.RandomState(256)
    T = robot.fk_batch(rng.uniform(-np.pi, np.pi, (256, robot.n)))
    A = on.solve(T, clearance=True, clearance_mode="links+self")
    stop, f, x = _np(A["stop"]), _np(A["f"]), _np(A["x"])
    assert np.all((stop == 0) | (stop == 1))
    conv = f < 1e-9
    assert conv.any()
    self_cl = _np(on.template.anchored_self_clearance(A["x"]))
    print(f"{name}: {int(conv.sum())} of 256 converge, self clearance of the converged {self_cl[conv].min():.2e} .. {self_cl[conv].max():.2e}; "
          f"of all: {int((self_cl < -1e-4).sum())} below -1e-4")
    assert np.all(self_cl[conv] >= _self_bound())
    assert np.all(np.minimum(self_cl, _np(on.template.anchored_link_clearance(A["x"]))) == _np(A["clearance"]))
    if len(on.obstacles):
        r = float(on.obstacles[:, 3].min())
        assert np.all(_np(on.template.anchored_clearance(A["x"]))[conv] >= np.sqrt(r * r - np.sqrt(1e-9)) - r)
    n_const = len(on.anchors) - on.n_goal_anchor
    assert np.abs(x[:, on.anchors[:n_const]] - on.anchor_pos[None, :n_const]).max() < 1e-12
    assert np.abs(x[:, on.anchors[n_const:]] - on.goal_anchors(T).reshape(256, -1, 3)).max() < 1e-12


# ---- 9. scenes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("link_hinges", [False, True])
def test_scenes_are_bit_identical_to_their_own_templates(torch_cuda, link_hinges):
    """Two scenes, 5 goals, either scene build (without and with link hinges): each goal equals, bit for bit, the goal
    solved on a problem created with its scene's spheres."""
    from graphik_amd.utils import table_environment
    table = [(*c, r) for c, r in table_environment()]
    scenes = (tuple(tuple(float(v) for v in s) for s in table[:40]), tuple(tuple(float(v) for v in s) for s in table[60:]))
    robot, graph, ap = _problem("ur10_table", link_hinges=link_hinges)
    q = _folded(ap, robot, 9, 5)
    T = robot.fk_batch(q + 0.05)
    ids = np.array([0, 1, 1, 0, 1])
    S = ap.scene_set([np.array(s) for s in scenes])
    keys = KEYS + ("f", "inner_total")
    got = _host(ap.solve(T, q_init=q, clearance=True, clearance_mode="links+self", scenes=S, scene_id=ids), keys)
    assert int(got["iterations"].max()) > 1
    for s in (0, 1):
        _, _, own = _problem("ur10", link_hinges=link_hinges, spheres=scenes[s])
        sel = np.flatnonzero(ids == s)
        ref = _host(own.solve(T[sel], q_init=q[sel], clearance=True, clearance_mode="links+self"), keys)
        assert _same_rows(got, ref, sel, slice(None), keys), s


# ---- 10. restarts and tracking ---------------------------------------------------------------------------------------
def test_restarts_and_tracking_run_on_the_self_hinge_problem(torch_cuda):
    """solve(retries=1, clearance_mode="links+self") on the 16 configurations: rows that did not fail keep attempt 0's
    bits, a replaced row equals the one-goal seeded solve from retry_seeds_host's angles on the same problem.
    solve_trajectory(sweep=2) on 4 paths x 3 waypoints returns finite sweep_self_clearance."""
    rs = _rs()
    robot, graph, on = _problem("kuka")
    q = _self_colliding16()
    T = robot.fk_batch(q)
    lo, hi = robot.limits_arrays()
    seed = 41
    P = _host(on.solve(T, q_init=q, clearance_mode="links+self"))
    R = _host(on.solve(T, q_init=q, retries=1, retry_seed=seed, clearance_mode="links+self", **TOL))
    att = R["attempt"]
    assert att.min() >= 0 and att.max() <= 1
    print("attempt histogram", np.bincount(att, minlength=2).tolist(), "clear after", int((R["clearance"] >= -1e-4).sum()), "of 16")
    first = att == 0
    failed = rs.anchored_retry_failed(P["stop"], P["pos_err"], P["rot_err"], P["clearance"], **TOL)
    assert not np.any(att[~failed]) and _same_rows(R, P, first, first)
    for g in np.flatnonzero(att > 0):
        q0 = rs.retry_seeds_host(seed, [g], int(att[g]), lo, hi)
        S = _host(on.solve(T[g:g + 1], q_init=q0, clearance_mode="links+self"))
        assert _same_rows(R, S, slice(g, g + 1)), (g, att[g])
    qs = q[:4]
    path = np.stack([robot.fk_batch(qs + 0.05 * (l + 1)) for l in range(3)], axis=1)      # [4, 3, 4, 4]
    qt, _, info = on.solve_trajectory(path, qs, clearance_mode="links+self", sweep=2)
    assert qt.shape == (4, 3, robot.n) and info["sweep_self_clearance"].shape == (4, 3)
    assert np.all(np.isfinite(info["sweep_self_clearance"])) and np.all(np.isfinite(info["clearance"]))


# ---- 11. refusals; the kernel group ----------------------------------------------------------------------------------
def _hand_made(N, terms, full_N, free_full, anchor_full):
    """An anchored template by hand: N free nodes, constant anchors at the origin, no goal anchor, no obstacle."""
    from graphik_amd.engine import Template
    ti, tj = np.array([t[0] for t in terms]), np.array([t[1] for t in terms])
    return Template(N, 3, ti, tj, np.ones(len(terms), dtype=np.int32), None,
                    anchored=dict(anchor_pos=np.zeros((len(anchor_full), 3)), n_goal_anchor=0, term_target=np.ones(len(terms)),
                                  pin_node=[], pin_anchor=[], pin_kind=[], pin_target=[], obs=np.zeros((0, 4)),
                                  obs_node_mask=np.zeros(N, dtype=np.int32), full_N=full_N, free_full_index=free_full,
                                  anchor_full_index=anchor_full, axis_length=1.0))


def test_refusals_of_attach_self_hinges(torch_cuda):
    """Each refusal has its own message and leaves the template as it was: flag, kernels' form, LDS bytes, occupancy."""
    from graphik_amd import _ffi
    rs = _rs()

    def refused(tpl, match):
        before = dict(tpl.info)
        with pytest.raises(_ffi.GikError, match=match):
            tpl.attach_self_hinges()
        tpl._read_info()
        assert not tpl.self_hinges and tpl.info == before and not (tpl.info["anchored"] & 4)

    robot, graph = make_graph("ur10")
    refused(rs.AnchoredProblem(graph, links=[]).template, "no links attached")
    refused(rs.AnchoredProblem(graph, link_radius=RHO).template, "no self pairs attached")
    skeleton = [(f"p{i}", f"p{i + 1}") for i in range(6)]
    many = rs.AnchoredProblem(graph, links=skeleton + [("q1", "q2"), ("q3", "q4")], link_radius=RHO, self_pairs="auto")
    assert len(many.self_pairs) == 23
    refused(many.template, "23 self pairs attached; the solve carries hinges for at most 16")
    # the 20-slot variant: a free node with 11 terms
    star = _hand_made(12, [(0, k) for k in range(1, 12)], 13, list(range(1, 13)), [0])
    assert star.info["max_terms_per_node"] == 20
    star.attach_links([1, 3], [2, 4], [RHO, RHO])
    star.attach_self_pairs([0], [1])
    refused(star, "20-slot variant, which has none")
    # a link that ends at a row which is neither a free node nor an anchor row
    chain = _hand_made(4, [(0, 1), (1, 2), (2, 3)], 6, [1, 2, 3, 4], [0])
    chain.attach_links([1, 3], [5, 4], [RHO, RHO])
    chain.attach_self_pairs([0], [1])
    refused(chain, "link 0 of pair 0 ends at row 5, which is neither a free node nor an anchor row")
    # accepted: a pair with an anchor-ended link; then the second call is refused and changes nothing
    good = _hand_made(4, [(0, 1), (1, 2), (2, 3)], 6, [1, 2, 3, 4], [0])
    good.attach_links([0, 3], [1, 4], [RHO, RHO])
    good.attach_self_pairs([0], [1])
    good.attach_self_hinges()
    assert good.self_hinges and good.info["anchored"] == 5
    before = dict(good.info)
    with pytest.raises(_ffi.GikError, match="self hinges already attached"):
        good.attach_self_hinges()
    good._read_info()
    assert good.info == before


def test_the_new_kernel_group_is_what_the_self_hinge_templates_run(torch_cuda):
    """GIK_KERNELS_ANCH_SELF (gik_instances.h) holds six instantiations and is a group of GIK_ALL_KERNELS, which the host
    unit expands once; each of the six is what a template of the tests above launches: the solve, known-answer and scene
    kernels of the form gik_template_get_info reports -- 3-D, 9 slots, anchored = 5 (self hinges) and 7 (with link
    hinges) -- at the LDS bytes of the self context and four waves per CU."""
    import synth_graphs as sg
    group = set(sg.group_members("GIK_KERNELS_ANCH_SELF"))
    assert len(group) == 6
    assert "GIK_KERNELS_ANCH_SELF(X)" in sg.macro_body("GIK_ALL_KERNELS")
    umbrella = open(os.path.join(REPO, "graphik_amd", "csrc", "gik_kernels.hip.h")).read()
    host = open(os.path.join(REPO, "graphik_amd", "csrc", "gik_host.hip")).read()
    unit = open(os.path.join(REPO, "graphik_amd", "csrc", "gik_k_anch_self.hip")).read()
    assert "GIK_KERNELS_ANCH_SELF(GIK_EXTERN_TEMPLATE)" not in umbrella and "GIK_KERNELS_ANCH_SELF(GIK_INSTANTIATE)" in unit
    assert re.findall(r"GIK_\w+\(GIK_EXTERN_TEMPLATE\)", host) == ["GIK_ALL_KERNELS(GIK_EXTERN_TEMPLATE)"]
    ran = set()
    for link_hinges in (False, True):
        robot, graph, on = _problem("ur10_table", link_hinges=link_hinges)
        _, _, off = _problem("ur10_table", self_hinges=False, link_hinges=link_hinges)
        info, base = on.template.info, off.template.info
        assert not info["is_block"] and info["anchored"] == (7 if link_hinges else 5) and info["max_terms_per_node"] == 9
        flags = "W_ANCH|W_LINKS|W_SELF" if link_hinges else "W_ANCH|W_SELF"
        # 16 descriptors of 16 bytes and 16 states of 48 on top of the form's context
        assert info["lds_bytes"] - base["lds_bytes"] == 16 * (16 + 48)
        print(f"anchored = {info['anchored']}: lds_bytes {info['lds_bytes']}, waves_per_cu {info['waves_per_cu']}")
        assert info["lds_bytes"] <= 40 * 1024 and info["waves_per_cu"] >= 4
        # ... and the three kernels run: a known answer, a solve, a scene solve, all with the hinges at work
        q = _folded(on, robot, 9, 2)
        T = robot.fk_batch(q)
        Y0, ga = on.seed_points(q), on.goal_anchors(T)
        assert np.all(_np(on.template.cost(Y0, ga)) > _np(off.template.cost(Y0, ga)))
        ran.add(f"kat_wave_kernel<3,9,{flags}>")
        A = on.solve(T, q_init=q)
        assert np.all(_np(A["iterations"]) >= 1)
        ran.add(f"rtr_wave_kernel<3,9,W_THETA1|{flags}>")
        S = on.scene_set([on.obstacles])
        B = on.solve(T, q_init=q, scenes=S)
        assert np.array_equal(_bits(_np(B["x"])), _bits(_np(A["x"])))
        ran.add(f"rtr_wave_scene_kernel<3,9,W_THETA1|{flags}>")
    assert ran == group
