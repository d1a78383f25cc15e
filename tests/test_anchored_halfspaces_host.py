"""Half-space obstacles (floors, walls) in the fixed-anchor solve, host side (CPU only): the numpy mirror of the hinge
(AnchoredProblem.halfspace_terms_host) against finite differences on a point set that holds every case -- deep inside, on
the boundary, two planes at once, an unmasked node below the floor, margins 0 and 0.03 --, whole links kept out by node
margins alone, the Python layer's argument checks, and the header and bindings.
tests/test_anchored_halfspaces_gpu.py takes its points from here."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import REPO, make_graph

FLOOR = (0.0, 0.0, 1.0, -0.1)       # z >= -0.1: a floor 10 cm under the base
WALL = (1.0, 0.0, 0.0, -0.3)        # x >= -0.3: a wall 30 cm behind it
RHO = 0.03


def _rs():
    from graphik_amd.solvers import riemannian_solver as rs
    return rs


def point_margins(ap_or_names):
    """The per-node margins of the point set: 0 on p1, p3, p5 (and the q nodes, which are unmasked), 0.03 on p2, p4."""
    names = ap_or_names if isinstance(ap_or_names, (list, tuple)) else ap_or_names.free_names
    return np.array([RHO if n in ("p2", "p4") else 0.0 for n in names])


@functools.lru_cache(maxsize=None)
def halfspace_problem(planes=(FLOOR, WALL), margin="points", rho=0.0, name="ur10"):
    """A host-only UR10 with half-spaces; margin "points": point_margins, else what AnchoredProblem takes."""
    robot, graph = make_graph(name)
    if margin == "points":
        bare = _rs().AnchoredProblem(graph, host_only=True)
        margin = tuple(point_margins(bare).tolist())
    ap = _rs().AnchoredProblem(graph, host_only=True, link_radius=rho, halfspaces=[list(p) for p in planes],
                               halfspace_margin=list(margin) if isinstance(margin, tuple) else margin)
    return robot, graph, ap


@functools.lru_cache(maxsize=None)
def halfspace_points():
    """Six points (Y_free [6, Nf, 3], goal anchors, W) on UR10 from RandomState(3), rows moved so that the set holds:
    0: p1 deep inside (z = 1); 1: p1 exactly on the floor's boundary (z = -0.1, margin 0: res == 0 in every summation
    order, since the normal is an axis); 2: p2 (margin 0.03) below the floor and behind the wall at once; 3: the unmasked
    q3 half a metre below the floor, every masked node above it; 4, 5: the random configurations themselves, moved off the
    constraint set by 4 mm of noise."""
    robot, graph, ap = halfspace_problem()
    rng = np.random.RandomState(3)
    q = rng.uniform(-np.pi, np.pi, (6, robot.n))
    Y, ga = ap.seed_points(q).copy(), ap.goal_anchors(robot.fk_batch(q)).copy()
    Y += 0.004 * rng.randn(*Y.shape)
    row = {n: i for i, n in enumerate(ap.free_names)}
    assert ap.obs_mask[row["p1"]] == 1 and ap.obs_mask[row["p2"]] == 1 and ap.obs_mask[row["q3"]] == 0
    Y[0, row["p1"]] = (0.2, 0.1, 1.0)
    Y[1, row["p1"]] = (0.2, 0.1, -0.1)
    Y[2, row["p2"]] = (-0.5, 0.2, -0.3)
    for i, n in enumerate(ap.free_names):      # point 3: nothing masked is below the floor or behind the wall ...
        if ap.obs_mask[i] == 1:
            Y[3, i, 2] = abs(Y[3, i, 2]) + 0.05
            Y[3, i, 0] = abs(Y[3, i, 0])
    Y[3, row["q3"]] = (0.1, 0.0, -0.6)         # ... and an unmasked node is
    W = rng.randn(*Y.shape)
    for a in (Y, ga, W):
        a.setflags(write=False)
    return Y, ga, W


# ---- 1. the mirror against finite differences ----------------------------------------------------------------------------
def test_point_set_holds_every_case():
    robot, graph, ap = halfspace_problem()
    Y, ga, W = halfspace_points()
    row = {n: i for i, n in enumerate(ap.free_names)}
    mu = ap.halfspace_margin
    assert sorted(set(mu.tolist())) == [0.0, RHO] and mu[row["p1"]] == 0.0 and mu[row["p2"]] == RHO
    act = []
    for b in range(6):
        ap.halfspace_terms_host(Y[b], W[b])
        act.append(set(ap.last_half_active))
    p1, p2, q3 = row["p1"], row["p2"], row["q3"]
    assert not any(i == p1 for i, h in act[0])                               # deep inside
    s = ap._halfspace_s(Y[1, p1], ap.halfspaces)
    assert s[0] == 0.0 and (p1, 0) not in act[1]                             # exactly on the boundary: inactive
    assert {(p2, 0), (p2, 1)} <= act[2]                                      # two at once
    f3, G3, H3 = ap.halfspace_terms_host(Y[3], W[3])
    assert Y[3, q3, 2] < -0.1 and f3 == 0.0 and not G3.any() and not H3.any() and not act[3]   # unmasked: nothing
    assert act[4] or act[5]


def test_mirror_gradient_and_hessian_against_finite_differences():
    """G against central differences of f, H against central differences of G along W: step 1e-6, within 1e-5 of the
    largest entry (the bars of test_mirror_gradient_and_frozen_t_hessian_against_finite_differences).  f is C^1, so its
    central difference is off by at most h / 2 per boundary it touches (point 1 sits on one): 5e-7 against entries of
    0.2 and more.  G has a kink there, so the difference of G is taken with the active set frozen at the point's own
    (frozen_active) -- H claims exactness only where the active set does not change -- and, at the points where no masked
    node is within 1e-4 of a boundary, with the active set free as well."""
    robot, graph, ap = halfspace_problem()
    Y, ga, W = halfspace_points()
    h = 1e-6
    checked = 0
    for b in range(6):
        f, G, H = ap.halfspace_terms_host(Y[b], W[b])
        active = set(ap.last_half_active)
        if not active:
            assert f == 0.0 and not G.any() and not H.any()
            continue
        Gfd = np.zeros_like(G)
        for i in range(Y.shape[1]):
            for c in range(3):
                E = np.zeros_like(Y[b])
                E[i, c] = h
                Gfd[i, c] = 0.5 * (ap.halfspace_terms_host(Y[b] + E, W[b])[0] - ap.halfspace_terms_host(Y[b] - E, W[b])[0]) / (2 * h)
        assert np.abs(Gfd - G).max() <= 1e-5 * np.abs(G).max(), (b, np.abs(Gfd - G).max(), np.abs(G).max())
        Hfd = (ap.halfspace_terms_host(Y[b] + h * W[b], W[b], frozen_active=active)[1] -
               ap.halfspace_terms_host(Y[b] - h * W[b], W[b], frozen_active=active)[1]) / (2 * h)
        assert np.abs(Hfd - H).max() <= 1e-5 * np.abs(H).max(), (b, np.abs(Hfd - H).max(), np.abs(H).max())
        res = ap.halfspace_margin[ap.obs_mask == 1][:, None] - ap._halfspace_s(Y[b][ap.obs_mask == 1], ap.halfspaces)
        if np.abs(res).min() > 1e-4:
            Hfree = (ap.halfspace_terms_host(Y[b] + h * W[b], W[b])[1] - ap.halfspace_terms_host(Y[b] - h * W[b], W[b])[1]) / (2 * h)
            assert np.abs(Hfree - H).max() <= 1e-5 * np.abs(H).max(), b
        checked += 1
    assert checked >= 4


def test_terms_are_the_formulas_of_the_header():
    """One node, by hand: p2 (margin 0.03) at (-0.5, 0.2, -0.3) against floor and wall -- residuals 0.03 + 0.2 each."""
    robot, graph, ap = halfspace_problem()
    Y, ga, W = halfspace_points()
    row = {n: i for i, n in enumerate(ap.free_names)}
    Yb = np.array(Y[3])
    Yb[row["p2"]] = (-0.5, 0.2, -0.3)
    Wb = np.zeros_like(Yb)
    Wb[row["p2"]] = (2.0, 3.0, 5.0)
    f, G, H = ap.halfspace_terms_host(Yb, Wb)
    r = 0.03 + 0.2
    assert abs(f - 2 * r * r) < 1e-15
    assert np.allclose(G[row["p2"]], (-r, 0.0, -r), atol=1e-15) and np.abs(np.delete(G, row["p2"], axis=0)).max() == 0.0
    assert np.allclose(H[row["p2"]], (2.0, 0.0, 5.0), atol=1e-15)
    # the clearance mirror: the same residuals, negated, and the minimum over them
    full = np.zeros((1, ap.base.N, 3))
    full[0, :, 2] = 1.0
    full[0, :, 0] = 1.0
    full[0, ap.free] = Yb
    full[0, ap.free, 2] = np.where(ap.obs_mask == 1, np.maximum(Yb[:, 2], 0.5), Yb[:, 2])
    full[0, ap.free[row["p2"]]] = Yb[row["p2"]]
    assert ap.halfspace_clearance(full)[0] == min(-0.5 + 0.3, -0.3 + 0.1) - 0.03
    bad = full.copy()
    bad[0, ap.free[row["p4"]], 1] = np.nan
    assert np.isnan(ap.halfspace_clearance(bad)[0])
    bad = full.copy()
    bad[0, ap.free[row["q3"]], 1] = np.nan                   # (an unmasked node is not measured)
    assert ap.halfspace_clearance(bad)[0] == ap.halfspace_clearance(full)[0]


# ---- 2. whole links through node margins -----------------------------------------------------------------------------
def test_link_clearance_without_link_code():
    """Capsules of 3 cm, halfspace_margin=None: every masked free node gets the largest radius of the links that end at
    it.  s_h is linear, so on a link its minimum is at an end: at a FREE end P of link l, s_h(P) - rho_l >= s_h(P) - mu_P
    = -res_P >= -t with t the largest node residual of the configuration.  Checked per configuration on 256 random ones;
    the mirror's value halfspace_clearance(Y, links=True) is, bit for bit, the minimum of that over the free ends and the
    same over the constant ends (p0, p6), so with t the largest residual of all 256 it is >= -t wherever the constant
    ends are."""
    robot, graph, ap = halfspace_problem(planes=(FLOOR, WALL), margin=None, rho=RHO)
    assert np.array_equal(ap.halfspace_margin, np.where(ap.obs_mask == 1, RHO, 0.0))
    q = np.random.RandomState(256).uniform(-np.pi, np.pi, (256, robot.n))
    Y = ap.base.seed_points(q)
    masked = [ap.free[i] for i in range(len(ap.free)) if ap.obs_mask[i] == 1]
    res = RHO - ap._halfspace_s(Y[:, masked], ap.halfspaces)                  # [256, nodes, H]
    t = res.max(axis=(1, 2))
    rows = np.asarray(ap.link_rows)
    assert all(a in ap.free or b in ap.free for a, b in rows.tolist())         # every skeleton link has a free end
    val = ap._halfspace_s(Y[:, rows], ap.halfspaces) - RHO                     # [256, links, 2, H]
    free_end = np.isin(rows, ap.free)                                          # [links, 2]
    at_free = np.where(free_end[None, :, :, None], val, np.inf).min(axis=(1, 2, 3))
    at_const = np.where(free_end[None, :, :, None], np.inf, val).min(axis=(1, 2, 3))
    assert np.all(at_free >= -t)
    # every masked node is the end of a link of radius mu: the bound is attained
    assert np.array_equal(at_free, -t)
    mirror = ap.halfspace_clearance(Y, links=True)
    assert np.array_equal(mirror, np.minimum(at_free, at_const))
    assert np.array_equal(ap.halfspace_clearance(Y), -t)
    ok = at_const >= -t.max()
    assert ok.sum() >= 200 and np.all(mirror[ok] >= -t.max())
    print(f"256 configurations: largest node residual {t.max():.3f}, {int((t > 0).sum())} with a node beyond a plane, "
          f"{int((~ok).sum())} whose goal end is deeper than every joint point of the sample")


# ---- 3. validation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw, match", [
    (dict(halfspaces=[0.0, 0.0, 1.0, -0.1]), r"shape \[H, 4\]"),
    (dict(halfspaces=[[0.0, 0.0, 1.0]]), r"shape \[H, 4\]"),
    (dict(halfspaces=np.zeros((0, 4))), "1 .. 8 rows"),
    (dict(halfspaces=[list(FLOOR)] * 9), "1 .. 8 rows"),
    (dict(halfspaces=[[0.0, 0.0, 0.0, -0.1]]), "zero"),
    (dict(halfspaces=[[0.0, np.nan, 1.0, -0.1]]), "non-finite"),
    (dict(halfspaces=[[0.0, 0.0, 1.0, np.inf]]), "non-finite"),
    (dict(halfspaces=[list(FLOOR)], halfspace_margin=-0.01), "finite and at least 0"),
    (dict(halfspaces=[list(FLOOR)], halfspace_margin=np.nan), "finite and at least 0"),
    (dict(halfspaces=[list(FLOOR)], halfspace_margin=[0.0, 0.01]), "one entry per free node"),
    (dict(halfspace_margin=0.01), "needs halfspaces"),
    (dict(halfspaces=[list(FLOOR)], link_radius=RHO, self_pairs="auto", self_hinges=True), "self_hinges"),
])
def test_bad_arguments_raise_before_any_device_object(kw, match):
    robot, graph = make_graph("ur10")
    with pytest.raises(ValueError, match=match):
        _rs().AnchoredProblem(graph, host_only=True, **kw)


def test_rows_are_normalised_and_none_changes_nothing():
    robot, graph = make_graph("ur10")
    ap = _rs().AnchoredProblem(graph, host_only=True, halfspaces=[[0.0, 0.0, 2.0, -0.2], [3.0, 4.0, 0.0, 5.0]])
    assert np.array_equal(ap.halfspaces[0], (0.0, 0.0, 1.0, -0.1))
    assert np.allclose(ap.halfspaces[1], (0.6, 0.8, 0.0, 1.0), rtol=0, atol=1e-16)
    n2 = (ap.halfspaces[:, :3] ** 2).sum(axis=1)
    assert np.abs(n2 - 1.0).max() <= 1e-12
    assert ap.template is None and np.array_equal(ap.halfspace_margin, np.zeros(len(ap.free)))   # (no links: margin 0)
    off = _rs().AnchoredProblem(graph, host_only=True)
    assert off.halfspaces is None and off.halfspace_margin is None
    Y = off.base.seed_points(np.zeros((2, robot.n)))
    assert np.all(np.isposinf(off.halfspace_clearance(Y))) and np.all(np.isposinf(off.halfspace_clearance(Y, links=True)))
    assert off.halfspace_terms_host(Y[0, off.free], Y[0, off.free])[0] == 0.0


# ---- 4. header and bindings ----------------------------------------------------------------------------------------------
def test_header_bindings_and_kernel_group():
    from graphik_amd import _ffi
    header = open(os.path.join(REPO, "include", "graphik_amd.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    flat = re.sub(r"\s+", " ", code)
    assert ("int gik_anchored_attach_halfspaces(gik_template *anch, int n_half, const double *halfspaces , "
            "const double *node_margin );") in flat
    assert ("int gik_anchored_halfspace_clearance(const gik_template *anch, const double *d_Y_full, int B, int links , "
            "double *d_clearance, void *stream);") in flat
    for name in ("gik_anchored_attach_halfspaces", "gik_anchored_halfspace_clearance"):
        assert name in _ffi.SYMBOLS and re.fullmatch(r"gik_[a-z_]+", name)
    assert re.search(r"#define\s+GIK_ABI_VERSION\s+12\b", header)
    args = open(os.path.join(REPO, "graphik_amd", "csrc", "gik_args.h")).read()
    assert re.search(r"constexpr int ANCH_HALF_MAX = 8;", args) and _ffi.HALF_MAX == 8
    import synth_graphs as sg
    group = sg.group_members("GIK_KERNELS_ANCH_HALF")
    assert len(group) == 6 and set(group) == {f"{k}<3,9,{flags}>" for k, flags in (
        ("rtr_wave_kernel", "W_THETA1|W_ANCH|W_HALF"), ("rtr_wave_kernel", "W_THETA1|W_ANCH|W_LINKS|W_HALF"),
        ("kat_wave_kernel", "W_ANCH|W_HALF"), ("kat_wave_kernel", "W_ANCH|W_LINKS|W_HALF"),
        ("rtr_wave_scene_kernel", "W_THETA1|W_ANCH|W_HALF"), ("rtr_wave_scene_kernel", "W_THETA1|W_ANCH|W_LINKS|W_HALF"))}
    assert "GIK_KERNELS_ANCH_HALF(X)" in sg.macro_body("GIK_ALL_KERNELS")
    umbrella = open(os.path.join(REPO, "graphik_amd", "csrc", "gik_kernels.hip.h")).read()
    host = open(os.path.join(REPO, "graphik_amd", "csrc", "gik_host.hip")).read()
    unit = open(os.path.join(REPO, "graphik_amd", "csrc", "gik_k_anch_half.hip")).read()
    assert "GIK_KERNELS_ANCH_HALF(GIK_EXTERN_TEMPLATE)" not in umbrella and "GIK_KERNELS_ANCH_HALF(GIK_INSTANTIATE)" in unit
    assert re.findall(r"GIK_\w+\(GIK_EXTERN_TEMPLATE\)", host) == ["GIK_ALL_KERNELS(GIK_EXTERN_TEMPLATE)"]
    assert re.findall(r'#include "([^"]+)"', unit) == ["gik_wave_kernels.hip.h", "gik_instances.h"]
    from graphik_amd import build
    assert build.SOURCES.index("gik_k_anch_half.hip") < build.SOURCES.index("gik_host_anch.hip")
    assert re.search(r"W_HALF = 64,", open(os.path.join(REPO, "graphik_amd", "csrc", "gik_wave_kernels.hip.h")).read())


def test_blind_spot_figures_of_the_readme_workload():
    """The figures the feature was asked for with: among RandomState(7).uniform(-pi, pi, (2048, 6)) on UR10, 59 % have a
    joint point p1 .. p5 below a floor 10 cm under the base; 242 have one more than 1 cm below it and the end effector
    more than 5 cm above it at the same time, and the first 16 of those sit within the first 96 draws."""
    robot, graph, ap = halfspace_problem(planes=(FLOOR,), margin=0.0)
    sel, q, Y = blind_spot_sample()
    z = Y[:, [ap.base.graph.index(f"p{i}") for i in range(1, 6)], 2]
    below = (z < -0.1).any(axis=1)
    ee = Y[:, ap.base.graph.index("p6"), 2]
    assert round(100 * below.mean()) == 59 and int(((z.min(axis=1) < -0.11) & (ee > -0.05)).sum()) == 242
    assert len(sel) == 16 and sel.max() < 96


@functools.lru_cache(maxsize=None)
def blind_spot_sample():
    """(indices of the first 16 configurations of RandomState(7).uniform(-pi, pi, (2048, 6)) whose end effector is more
    than 5 cm above the floor and that have a joint point p1 .. p5 more than 1 cm below it, all 2048 angles, their full
    point matrices)."""
    robot, graph, ap = halfspace_problem(planes=(FLOOR,), margin=0.0)
    q = np.random.RandomState(7).uniform(-np.pi, np.pi, (2048, 6))
    Y = ap.base.seed_points(q)
    z = Y[:, [ap.base.graph.index(f"p{i}") for i in range(1, 6)], 2]
    ee = Y[:, ap.base.graph.index("p6"), 2]
    sel = np.flatnonzero((ee > -0.1 + 0.05) & (z.min(axis=1) < -0.1 - 0.01))[:16]
    return sel, q, Y
