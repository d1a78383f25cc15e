"""Link hinges in the fixed-anchor solve on the MI355X (AnchoredProblem(link_hinges=True), gik_anchored_attach_links with
hinges = 1): the known answers of the link builds of the solve and known-answer kernels against numpy, inactive hinges
changing nothing, culling bit-neutral, the node-clear / link-colliding configurations the node hinges cannot move, the
pipeline on random goals, restarts and tracking on top, the refusals, and which compiled kernels ran.
UR10 + table_environment() unless said.  The points and the mirror's own tests: tests/test_anchored_link_hinges_host.py."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import REPO, make_graph
from parity_util import anchored_numpy
from test_anchored_link_hinges_host import hinge_points, hinge_problem, table_spheres

pytestmark = pytest.mark.gpu

TOL = dict(pos_tol=0.01, rot_tol=0.01, clear_tol=1e-4)
KEYS = ("x", "q", "stop", "iterations", "pos_err", "rot_err", "clearance")
STATS = ("f", "gradnorm", "iterations", "inner_total", "stop", "n_accept")


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


@functools.lru_cache(maxsize=None)
def _table(hinges=True, dbg=0):
    """UR10 + table on the device, skeleton links of radius 0, with or without link hinges (dbg: debug_flags)."""
    robot, graph = make_graph("ur10_table")
    return robot, graph, _rs().AnchoredProblem(graph, link_hinges=hinges, params={"debug_flags": dbg} if dbg else None)


def _clear_bound(ap):
    """What f < 1e-9 leaves of a hinge: no residual R^2 - d exceeds sqrt(f), so the clearance |m| - R is at least
    sqrt(R^2 - sqrt(1e-9)) - R, most negative at the scene's smallest R = r + rho."""
    R = float(ap.obstacles[:, 3].min() + ap.link_radius.min())
    return np.sqrt(R * R - np.sqrt(1e-9)) - R


@functools.lru_cache(maxsize=None)
def _colliding16():
    """The first 16 configurations of RandomState(7).uniform(-pi, pi, (2048, 6)) whose joint points are more than 1 cm
    outside the spheres while a link is more than 1 cm inside one (numpy, on the host problem)."""
    robot, graph, ap = hinge_problem()
    qa = np.random.RandomState(7).uniform(-np.pi, np.pi, (2048, 6))
    Ya = ap.base.seed_points(qa)
    idx = np.flatnonzero((ap.clearance(Ya) > 0.01) & (ap.link_clearance(Ya) < -0.01))[:16]
    assert len(idx) == 16
    return qa[idx]


# ---- 1. known answers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rho,n_obs", [(0.0, None), (0.03, None), (0.0, 0), (0.0, 1), (0.0, 128)])
def test_link_hinge_known_answers(torch_cuda, rho, n_obs):
    """cost / grad / hess / cost_and_grad of the hinge template at the points of the host test (every clamp case active,
    both anchor-ended links) against anchored_numpy + link_hinge_terms_host: 1e-12 relative, the project's kernel
    tolerance.  Thin and 3 cm links; the table, no sphere, one, and the 128-sphere limit.  proj is the identity."""
    robot, graph, ap = hinge_problem(rho=rho, n_obs=n_obs, host_only=False)
    T = ap.template
    assert T.link_hinges and T.info["anchored"] == 3
    Nf = len(ap.free)
    Tg, ga, Y, W = hinge_points(robot, ap, ap.obstacles if len(ap.obstacles) else table_spheres())
    f = _np(T.cost(Y, ga))
    G = _np(T.grad(Y, ga))
    H = _np(T.hess(Y, W, ga))
    f2, G2 = T.cost_and_grad(Y, ga)
    assert np.array_equal(_np(f2), f) and np.array_equal(_np(G2), G)
    link_f = 0.0
    for b in range(len(Y)):
        fr, Gr, Hr = anchored_numpy(ap, Nf, Y[b], W[b], ga[b])
        fl, Gl, Hl = ap.link_hinge_terms_host(Y[b], W[b], ga[b])
        link_f += fl
        fr, Gr, Hr = fr + fl, Gr + Gl, Hr + Hl
        print(f"goal {b}: link share of f {fl / fr:.3f}, errors {abs(f[b] - fr) / abs(fr):.2e} "
              f"{np.abs(G[b] - Gr).max() / np.abs(Gr).max():.2e} {np.abs(H[b] - Hr).max() / np.abs(Hr).max():.2e}")
        assert abs(f[b] - fr) <= 1e-12 * abs(fr)
        assert np.abs(G[b] - Gr).max() <= 1e-12 * np.abs(Gr).max()
        assert np.abs(H[b] - Hr).max() <= 1e-12 * np.abs(Hr).max()
    assert (link_f > 0) == (len(ap.obstacles) > 0)      # the hinges are exercised wherever there is a sphere
    assert np.array_equal(_np(T.proj(Y, W)), W)


# ---- 2. inactive hinges change nothing -----------------------------------------------------------------------------
def test_inactive_hinges_change_nothing(torch_cuda):
    """UR10 with one sphere 10 m away, 12 goals from the same Y0, link hinges off and on: Y, f, iterations, inner_total
    and every trace row are equal as numbers."""
    rs = _rs()
    out = []
    for hinges in (False, True):
        robot, graph = make_graph("ur10")
        graph.add_spherical_obstacle("far", np.array([10.0, 0.0, 0.0]), 0.1)
        ap = rs.AnchoredProblem(graph, link_hinges=hinges)
        assert ap.template.info["anchored"] == (3 if hinges else 1)
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


# ---- 3. culling is bit-neutral -------------------------------------------------------------------------------------
def test_culling_is_bit_neutral(torch_cuda):
    """debug_flags 128 (every walk visits every obstacle, nodes and links) against the default: 65 cold goals and one
    seeded batch of 63, x, q, statistics and errors bit for bit."""
    robot, graph, ap = _table(True)
    _, _, full = _table(True, 128)
    rng = np.random.RandomState(65)
    q = rng.uniform(-np.pi, np.pi, (65, robot.n))
    T = robot.fk_batch(q)
    keys = ("x", "q", "pos_err", "rot_err") + STATS
    a, b = _host(ap.solve(T), keys), _host(full.solve(T), keys)
    assert _same_rows(a, b, keys=keys)
    q0 = q[:63] + rng.uniform(-0.3, 0.3, (63, robot.n))
    a, b = _host(ap.solve(T[:63], q_init=q0), keys + ("clearance",)), _host(full.solve(T[:63], q_init=q0), keys + ("clearance",))
    assert _same_rows(a, b, keys=keys + ("clearance",))
    assert int(a["iterations"].max()) > 1


# ---- 4. the blind spot closes --------------------------------------------------------------------------------------
def test_the_blind_spot_closes(torch_cuda):
    """16 configurations whose joint points are clear and whose links are more than 1 cm inside a sphere, each asked for
    its own pose and seeded with itself.  Without link hinges the solve stops at once, the link still inside.  With them
    the seed costs at least (2 R delta - delta^2)^2 (R = 0.1, delta = 0.01), the answer costs less and took iterations, and
    an answer with f < 1e-9 has its links out of the spheres up to what that f leaves."""
    robot, graph, off = _table(False)
    _, _, on = _table(True)
    q = _colliding16()
    T = robot.fk_batch(q)
    P = _host(off.solve(T, q_init=q, clearance_mode="links"))
    assert int(P["iterations"].max()) <= 1 and np.all(P["clearance"] < -0.01)
    Y0, ga = on.seed_points(q), on.goal_anchors(T)
    f_seed = _np(on.template.cost(Y0, ga))
    R, delta = 0.1, 0.01
    assert np.all(f_seed >= (2 * R * delta - delta * delta) ** 2)
    A = on.solve(T, q_init=q, clearance_mode="links")
    f, it, cl = _np(A["f"]), _np(A["iterations"]), _np(A["clearance"])
    assert np.all(f < f_seed) and np.all(it >= 1)
    conv = f < 1e-9
    print(f"hinges on: {int(conv.sum())} of 16 converge, link clearance {cl.min():.2e} .. {cl.max():.2e}, iterations {it.min()} .. {it.max()}")
    assert np.all(cl[conv] >= _clear_bound(on))
    assert np.array_equal(_bits(cl), _bits(_np(on.template.anchored_link_clearance(A["x"]))))


# ---- 5. the pipeline on random goals -------------------------------------------------------------------------------
def test_pipeline_property_on_random_goals(torch_cuda):
    """256 random goals, cold, link hinges on, clearance_mode="links": every problem stops by a legal rule, every
    converged answer (f < 1e-9) has link and node clearance at or above the bound of f, at least one converges, and the
    anchors of x are the constants they were given."""
    robot, graph, on = _table(True)
    _, _, off = _table(False)
    rng = np.random.RandomState(256)
    T = robot.fk_batch(rng.uniform(-np.pi, np.pi, (256, robot.n)))
    A = on.solve(T, clearance=True, clearance_mode="links")
    stop, f, cl, x = _np(A["stop"]), _np(A["f"]), _np(A["clearance"]), _np(A["x"])
    assert np.all((stop == 0) | (stop == 1))
    conv = f < 1e-9
    assert conv.any()
    bound = _clear_bound(on)
    assert np.all(cl[conv] >= bound)
    assert np.all(_np(on.template.anchored_clearance(A["x"]))[conv] >= bound)
    n_const = len(on.anchors) - on.n_goal_anchor
    assert np.abs(x[:, on.anchors[:n_const]] - on.anchor_pos[None, :n_const]).max() < 1e-12
    assert np.abs(x[:, on.anchors[n_const:]] - on.goal_anchors(T).reshape(256, -1, 3)).max() < 1e-12
    B = off.solve(T, clearance=True, clearance_mode="links")
    twin = _np(B["clearance"])
    print(f"hinges on: {int(conv.sum())} of 256 converge; {int((twin[conv] < -1e-2).sum())} of them had a hinges-off twin with link "
          f"clearance < -1e-2 (hinges off: {int((_np(B['f']) < 1e-9).sum())} converge, {int((twin < -1e-2).sum())} below -1e-2)")


# ---- 6. restarts and tracking run on it ----------------------------------------------------------------------------
def test_restarts_and_tracking_run_on_the_hinge_problem(torch_cuda):
    """solve(retries=2, clearance_mode="links") on the 16 configurations: each kept row is, bit for bit, attempt 0's or the
    one-goal seeded solve from retry_seeds_host's angles on the same hinge problem.  solve_trajectory with sweep=2 on
    8 paths x 4 waypoints returns finite sweep clearances."""
    rs = _rs()
    robot, graph, on = _table(True)
    q = _colliding16()
    T = robot.fk_batch(q)
    lo, hi = robot.limits_arrays()
    seed = 41
    P = _host(on.solve(T, q_init=q, clearance_mode="links"))
    R = _host(on.solve(T, q_init=q, retries=2, retry_seed=seed, clearance_mode="links", **TOL))
    att = R["attempt"]
    assert att.min() >= 0 and att.max() <= 2
    print("attempt histogram", np.bincount(att, minlength=3).tolist(), "clear after", int((R["clearance"] >= -1e-4).sum()), "of 16")
    first = att == 0
    assert _same_rows(R, P, first, first)
    for g in np.flatnonzero(att > 0):
        q0 = rs.retry_seeds_host(seed, [g], int(att[g]), lo, hi)
        S = _host(on.solve(T[g:g + 1], q_init=q0, clearance_mode="links"))
        assert _same_rows(R, S, slice(g, g + 1)), (g, att[g])
    qs = q[:8]
    path = np.stack([robot.fk_batch(qs + 0.05 * (l + 1)) for l in range(4)], axis=1)      # [8, 4, 4, 4]
    qt, _, info = on.solve_trajectory(path, qs, clearance_mode="links", sweep=2)
    assert qt.shape == (8, 4, robot.n) and info["sweep_clearance"].shape == (8, 4)
    assert np.all(np.isfinite(info["sweep_clearance"])) and np.all(np.isfinite(info["clearance"]))


# ---- 7. refusals ---------------------------------------------------------------------------------------------------
def _hand_made(N, terms, full_N, free_full, anchor_full):
    """An anchored template by hand: N free nodes, one constant anchor at the origin, no goal anchor, no obstacle."""
    from graphik_amd.engine import Template
    ti, tj = np.array([t[0] for t in terms]), np.array([t[1] for t in terms])
    return Template(N, 3, ti, tj, np.ones(len(terms), dtype=np.int32), None,
                    anchored=dict(anchor_pos=np.zeros((len(anchor_full), 3)), n_goal_anchor=0, term_target=np.ones(len(terms)),
                                  pin_node=[], pin_anchor=[], pin_kind=[], pin_target=[], obs=np.zeros((0, 4)),
                                  obs_node_mask=np.zeros(N, dtype=np.int32), full_N=full_N, free_full_index=free_full,
                                  anchor_full_index=anchor_full, axis_length=1.0))


def test_refusals_of_attach_with_hinges(torch_cuda):
    from graphik_amd import _ffi
    robot, graph = make_graph("ur10_table")
    ap = _rs().AnchoredProblem(graph, links=[])
    T, g = ap.template, ap.base.graph
    row = lambda name: g.index(name)      # noqa: E731

    def refused(tpl, links, match, hinges=True, rho=0.0):
        with pytest.raises(_ffi.GikError, match=match):
            tpl.attach_links([l[0] for l in links], [l[1] for l in links], [rho] * len(links), hinges=hinges)
        assert tpl.n_link is None and not tpl.link_hinges

    import ctypes as C
    a = np.array([row("p1")], dtype=np.int32)
    r = np.zeros(1)
    d = _ffi.LinkDesc(n_link=1, hinges=2, link_a=a.ctypes.data_as(C.POINTER(C.c_int32)),
                      link_b=a.ctypes.data_as(C.POINTER(C.c_int32)), link_radius=r.ctypes.data_as(C.POINTER(C.c_double)))
    assert T.lib.gik_anchored_attach_links(T._h, C.byref(d)) != 0
    assert "hinges must be 0 (measure only) or 1" in T.lib.gik_last_error().decode()
    with pytest.raises(TypeError, match="hinges must be a bool"):
        T.attach_links([row("p1")], [row("p2")], [0.0], hinges=2)
    # more than two hinge links at one free node
    refused(T, [(row("p1"), row("p2")), (row("p0"), row("p1")), (row("p1"), row("q1"))], "more than 2 hinge links at free node")
    # two free ends without a common term
    ti, tj, _, _ = ap.free_terms
    tied = {(int(i), int(j)) for i, j in zip(ti, tj)} | {(int(j), int(i)) for i, j in zip(ti, tj)}
    i, j = next((i, j) for i in range(len(ap.free)) for j in range(i + 1, len(ap.free)) if (i, j) not in tied)
    refused(T, [(ap.free[i], ap.free[j])], "share no term")
    # the 20-slot variant: a free node with 11 terms
    star = _hand_made(12, [(0, k) for k in range(1, 12)], 13, list(range(1, 13)), [0])
    assert star.info["max_terms_per_node"] == 20
    refused(star, [(1, 2)], "20-slot variant, which has no link hinges")
    # a row that is neither a free node nor an anchor row
    chain = _hand_made(4, [(0, 1), (1, 2), (2, 3)], 6, [1, 2, 3, 4], [0])
    assert chain.info["max_terms_per_node"] == 9
    refused(chain, [(1, 5)], "neither a free node nor an anchor row")
    refused(chain, [(1, 2)], "link_radius", rho=-1.0)
    # accepted: a link with two constant ends next to a real one; then the second attach is refused
    chain.attach_links([0, 1], [0, 2], [0.0, 0.0], hinges=True)
    assert chain.link_hinges and chain.n_link == 2 and chain.info["anchored"] == 3
    with pytest.raises(_ffi.GikError, match="links already attached"):
        chain.attach_links([1], [2], [0.0], hinges=True)
    # the problem above is still without links, and takes them now
    T.attach_links([row("p1")], [row("p2")], [0.0], hinges=True)
    assert T.link_hinges and T.info["anchored"] == 3


# ---- 8. the compiled kernels of the new group are the ones that ran ------------------------------------------------
def test_the_new_kernel_group_is_what_the_hinge_template_runs(torch_cuda):
    """GIK_KERNELS_ANCH_LINK (gik_instances.h, a group of GIK_ALL_KERNELS) holds two instantiations, the solve and the
    known-answer kernel, both in the coverage table of tests/synth_graphs.py; the hinge
    template of the tests above reports them through gik_template_get_info: 3-D, 9 slots, anchored with link hinges
    (anchored = 3), at the LDS bytes of the link context and four waves per CU."""
    import synth_graphs as sg
    group = set(sg.group_members("GIK_KERNELS_ANCH_LINK"))
    # in the table of tests/synth_graphs.py, and covered there by a test that exists
    assert "GIK_KERNELS_ANCH_LINK(X)" in sg.macro_body("GIK_ALL_KERNELS")
    cov, compiled = sg.coverage(), sg.compiled_instances()
    assert group <= set(compiled) and all(cov.get(inst) for inst in group)
    robot, graph, on = _table(True)
    _, _, off = _table(False)
    info, base = on.template.info, off.template.info
    assert not info["is_block"] and info["anchored"] == 3 and base["anchored"] == 1
    slots = info["max_terms_per_node"]
    ran = {f"rtr_wave_kernel<3,{slots},W_THETA1|W_ANCH|W_LINKS>", f"kat_wave_kernel<3,{slots},W_ANCH|W_LINKS>"}
    assert ran == group
    # radii [128] + per-node link records and near lists [2][22] x (16 + 72) bytes on top of the anchored context
    assert info["lds_bytes"] - base["lds_bytes"] == 128 * 8 + 2 * 22 * (16 + 72)
    assert info["lds_bytes"] <= 40 * 1024 and info["waves_per_cu"] >= 4
    # ... and both kernels run: a known answer and a solve
    q = _colliding16()[:2]
    T = robot.fk_batch(q)
    assert np.all(_np(on.template.cost(on.seed_points(q), on.goal_anchors(T))) > 0)
    assert np.all(_np(on.solve(T, q_init=q)["iterations"]) >= 1)
