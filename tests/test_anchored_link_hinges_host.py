"""Link hinges in the fixed-anchor solve, host side (CPU only): the numpy mirror of the hinge terms
(AnchoredProblem.link_hinge_terms_host) against finite differences on points with every clamp case active, the cases that
contribute exactly zero, the Python layer's argument checks and the ABI, and the device pair function (anch_link_foot)
walked by a stand-alone program under the address and undefined-behaviour sanitizers.
tests/test_anchored_link_hinges_gpu.py takes its points from here."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, make_graph

# anch_link_foot of a = (.1, -.2, .3), b = (.7, .4, -.1), c = (.35, .2, .25): tests/host/anch_link_hinge_walk.cpp prints it
PINNED_A, PINNED_B, PINNED_C = (0.1, -0.2, 0.3), (0.7, 0.4, -0.1), (0.35, 0.2, 0.25)
# the "digest" line of tests/host/anch_link_hinge_walk.cpp (walk_digest.h: FNV-1a over the bits of (t, m, d) of its
# random cells), as that program prints it when compiled against the headers of c11b7a7, where anch_link_foot stood
# next to a second copy of its foot parameter
PARENT_DIGEST = "9bbfbba67255d075"


def _rs():
    from graphik_amd.solvers import riemannian_solver as rs
    return rs


@functools.lru_cache(maxsize=None)
def hinge_problem(rho=0.0, n_obs=None, host_only=True, link_hinges=True):
    """UR10 + table with the skeleton's links of radius rho; n_obs: UR10 with the first n_obs spheres of the table instead
    (128: the table + 28 more, the limit)."""
    if n_obs is None:
        robot, graph = make_graph("ur10_table")
    else:
        from graphik_amd.utils import table_environment
        robot, graph = make_graph("ur10")
        spheres = [(np.asarray(c, dtype=float), float(r)) for c, r in table_environment()]
        rng = np.random.RandomState(31)
        while len(spheres) < n_obs:
            spheres.append((rng.uniform(-1.0, 1.0, size=3), 0.05 + 0.1 * rng.rand()))
        for idx, (c, r) in enumerate(spheres[:n_obs]):
            graph.add_spherical_obstacle(f"o{idx}", c, r)
    ap = _rs().AnchoredProblem(graph, host_only=host_only, link_radius=rho, link_hinges=link_hinges)
    assert len(ap.obstacles) == (100 if n_obs is None else n_obs) and len(ap.link_rows) == 6
    return robot, graph, ap


def hinge_points(robot, ap, spheres, B=6):
    """Points built like test_anchored_kernel_known_answers (RandomState(4): goals, free rows around the table top, p-nodes
    next to spheres), then link mid-sections moved into spheres: per goal two free-free links get their middle next to a
    centre, one more is laid radially with one end inside a sphere (the foot clamps to that end: t = 0 for even goals,
    t = 1 for odd ones), and the two anchor-ended links p0 -> p1 and p5 -> p6 are pointed through a sphere.
    spheres [n, 4] (x, y, z, r): where the mid-sections go (the scene's own, or the table's for a scene without)."""
    rng = np.random.RandomState(4)
    Nf = len(ap.free)
    Tg = robot.fk_batch(-np.pi + 2 * np.pi * rng.rand(B, robot.n))
    ga = ap.goal_anchors(Tg)
    Y = 0.6 * rng.randn(B, Nf, 3) + np.array([0.0, 0.0, 0.9])
    S = np.asarray(spheres, dtype=float)
    for b in range(B):
        for i in np.nonzero(ap.obs_mask)[0]:
            Y[b, i] = S[rng.randint(len(S)), :3] + 0.07 * rng.randn(3)
    W = rng.randn(B, Nf, 3)
    f = {name: i for i, name in enumerate(ap.free_names)}
    p0 = np.asarray(ap.anchor_pos[ap.anchors.index(ap.base.graph.index("p0"))], dtype=float)
    unit = lambda v: v / np.linalg.norm(v)      # noqa: E731
    for b in range(B):
        first = 1 + b % 2
        for k in (first, first + 2):            # p1-p2, p3-p4 / p2-p3, p4-p5: the middle next to a centre
            C, u = S[rng.randint(len(S)), :3], unit(rng.randn(3))
            off = 0.03 * rng.randn(3)
            Y[b, f[f"p{k}"]] = C + off - rng.uniform(0.15, 0.3) * u
            Y[b, f[f"p{k + 1}"]] = C + off + rng.uniform(0.15, 0.3) * u
        # one end inside a sphere, the link pointing away from the centre: the foot is that end
        k = 3 - first                           # p2-p3 (even goals) / p1-p2 (odd ones) -- re-lays a link the loop above left alone
        C, u = S[rng.randint(len(S)), :3], unit(rng.randn(3))
        inside, outside = C + 0.04 * u, C + 0.45 * u
        Y[b, f[f"p{k}"]], Y[b, f[f"p{k + 1}"]] = (inside, outside) if b % 2 == 0 else (outside, inside)
    # the anchor-ended links through a sphere (goals 0 and 1: p0 -> p1; goals 2 and 3: p5 -> p6, p6 is the goal's)
    for b in (0, 1):
        C = S[rng.randint(len(S)), :3]
        Y[b, f["p1"]] = p0 + 1.7 * (C - p0) + 0.02 * rng.randn(3)
    for b in (2, 3):
        C, p6 = S[rng.randint(len(S)), :3], ga[b].reshape(-1, 3)[0]
        Y[b, f["p5"]] = p6 + 1.7 * (C - p6) + 0.02 * rng.randn(3)
    return Tg, ga, Y, W


def table_spheres():
    return hinge_problem()[2].obstacles


def active_pairs(ap, Y, W, ga):
    """[(goal, link, obstacle, t)] of the active pairs of a point set."""
    out = []
    for b in range(len(Y)):
        ap.link_hinge_terms_host(Y[b], W[b], ga[b])
        out += [(b, l, o, t) for (l, o), t in ap.last_link_t.items()]
    return out


# ---- 1. the mirror against finite differences ----------------------------------------------------------------
def test_mirror_gradient_and_frozen_t_hessian_against_finite_differences():
    """G of the mirror = central differences of its f (step 1e-6), H = central differences of the FROZEN-t gradient along W,
    both within 1e-5 of the largest entry: f is C^1 and its second derivative jumps where t reaches 0 or 1 (and where a
    hinge switches on), so the difference error is O(h) there, h^2 elsewhere.  The point set holds every clamp case."""
    robot, graph, ap = hinge_problem()
    Tg, ga, Y, W = hinge_points(robot, ap, ap.obstacles)
    pairs = active_pairs(ap, Y, W, ga)
    n_in = sum(0.0 < t < 1.0 for _, _, _, t in pairs)
    n_0 = sum(t == 0.0 for _, _, _, t in pairs)
    n_1 = sum(t == 1.0 for _, _, _, t in pairs)
    names = [ap.link_names[l] for _, l, _, _ in pairs]
    print(f"active pairs: {n_in} interior, {n_0} at t = 0, {n_1} at t = 1")
    assert n_in >= 20 and n_0 >= 3 and n_1 >= 3
    assert ("p0", "p1") in names and ("p5", "p6") in names
    h = 1e-6
    for b in range(len(Y)):
        f0, G, H = ap.link_hinge_terms_host(Y[b], W[b], ga[b])
        t0 = dict(ap.last_link_t)
        assert f0 > 0
        Gd = np.zeros_like(G)
        for i in range(Y.shape[1]):
            for c in range(3):
                Yp, Ym = Y[b].copy(), Y[b].copy()
                Yp[i, c] += h
                Ym[i, c] -= h
                Gd[i, c] = (ap.link_hinge_terms_host(Yp, W[b], ga[b])[0] - ap.link_hinge_terms_host(Ym, W[b], ga[b])[0]) / (2 * h)
        # G is 1/2 grad f (the kernels' convention)
        assert np.abs(0.5 * Gd - G).max() <= 1e-5 * np.abs(G).max(), (b, np.abs(0.5 * Gd - G).max(), np.abs(G).max())
        Gp = ap.link_hinge_terms_host(Y[b] + h * W[b], W[b], ga[b], frozen_t=t0)[1]
        Gm = ap.link_hinge_terms_host(Y[b] - h * W[b], W[b], ga[b], frozen_t=t0)[1]
        Hd = (Gp - Gm) / (2 * h)
        assert np.abs(Hd - H).max() <= 1e-5 * np.abs(H).max(), (b, np.abs(Hd - H).max(), np.abs(H).max())


# ---- 2. what contributes exactly zero ----------------------------------------------------------------------------
class _Cell:
    """AnchoredProblem.link_hinge_terms_host on a hand-made scene: two free rows, two constant rows, no robot."""

    def __init__(self, links, spheres, rho=0.0):
        self.link_rows = np.asarray(links, dtype=np.int32).reshape(-1, 2)
        self.obstacles = np.asarray(spheres, dtype=float).reshape(-1, 4)
        self.link_radius = np.broadcast_to(np.asarray(rho, dtype=float), (len(self.link_rows),))
        self.free, self.anchors = [0, 1], [2, 3]
        self.anchor_pos, self.n_goal_anchor = np.array([[0.0, 0.0, 0.0], [9.0, 9.0, 9.0]]), 1
        rs = _rs().AnchoredProblem
        self.link_foot_host, self.link_ends_host = rs.link_foot_host, lambda *a: rs.link_ends_host(self, *a)

    def __call__(self, Y, W, goal):
        return _rs().AnchoredProblem.link_hinge_terms_host(self, np.asarray(Y, float), np.asarray(W, float), np.asarray(goal, float))


@pytest.mark.parametrize("rho", [0.0, 0.03])
def test_what_contributes_exactly_zero(rho):
    Y, W, goal = [[0.3, 0.0, 0.0], [0.3, 0.0, 0.0]], [[1.0, 2.0, 3.0], [-1.0, 0.5, 2.0]], [1.0, 0.0, 0.0]
    zero = lambda r: r[0] == 0.0 and not r[1].any() and not r[2].any()      # noqa: E731
    # a zero-length link away from the sphere; the same one inside it is its point: a node hinge on both ends
    assert zero(_Cell([(0, 1)], [[0.3, 0.5, 0.0, 0.1]], rho)(Y, W, goal))
    f, G, H = _Cell([(0, 1)], [[0.3, 0.05, 0.0, 0.1]], rho)(Y, W, goal)
    R = np.sqrt(0.1 * 0.1) + rho
    res = R * R - 0.05 * 0.05
    assert f == res * res and not G[1].any() and G[0, 1] == 2.0 * -res * -0.05      # (t = 0: all of it at end a)
    # a link with two constant ends through the sphere's centre
    assert zero(_Cell([(2, 3)], [[0.5, 0.0, 0.0, 0.1]], rho)(Y, W, goal))
    # a sphere 10 m away
    Y2 = [[0.0, 0.1, 0.0], [0.6, 0.1, 0.0]]
    assert zero(_Cell([(0, 1), (2, 0), (1, 3)], [[10.0, 0.0, 0.0, 0.1]], rho)(Y2, W, goal))
    # ... and the same cell with the sphere on the link is not zero, at both ends
    f, G, H = _Cell([(0, 1)], [[0.3, 0.15, 0.0, 0.1]], rho)(Y2, W, goal)
    assert f > 0 and G[0].any() and G[1].any() and H[0].any() and H[1].any()
    # a constant end: its share is dropped, the free end keeps its own
    f, G, H = _Cell([(2, 0)], [[0.3, 0.05, 0.0, 0.1]], rho)([[0.6, 0.0, 0.0], [5.0, 5.0, 5.0]], W, goal)
    assert f > 0 and G[0].any() and not G[1].any() and not H[1].any()


# ---- 3. argument checks, before any device call; the ABI ---------------------------------------------------------
def test_link_hinges_argument_checks_need_no_device(monkeypatch):
    from graphik_amd import engine
    rs = _rs()
    robot, graph = make_graph("ur10_table")

    def no_device(*a, **k):
        raise AssertionError("a device handle was created before the arguments were checked")
    monkeypatch.setattr(engine.Template, "__init__", no_device)
    monkeypatch.setattr(rs.BatchProblem, "__init__", no_device)
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="link_hinges must be a bool"):
            rs.AnchoredProblem(graph, link_hinges=bad)
    with pytest.raises(ValueError, match="link_hinges=True needs a link set"):
        rs.AnchoredProblem(graph, links=[], link_hinges=True)


def test_host_only_problem_keeps_the_flag():
    robot, graph, ap = hinge_problem()
    assert ap.link_hinges is True and ap.template is None
    assert _rs().AnchoredProblem(graph, host_only=True).link_hinges is False


def test_abi_carries_the_hinges_field():
    import ctypes as C
    from graphik_amd import _ffi
    hdr = open(os.path.join(REPO, "include", "graphik_amd.h")).read()
    assert int(re.search(r"#define GIK_ABI_VERSION (\d+)", hdr).group(1)) == 12 and _ffi.ABI_VERSION == 12
    nocomment = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = [n.strip().lstrip("*") for n in re.findall(
        r"\b(?:const\s+)?(?:double|int32_t|uint64_t)\s+([^;]+);",
        re.search(r"typedef struct \{([^}]*)\} gik_link_desc;", nocomment).group(1))]
    assert names == [n for n, _ in _ffi.LinkDesc._fields_] and names[1] == "hinges"
    assert C.sizeof(_ffi.LinkDesc) == 32 and _ffi.LinkDesc.hinges.offset == 4 and _ffi.LinkDesc.link_a.offset == 8
    assert _ffi.LinkDesc(n_link=1).hinges == 0
    doc = re.search(r"gik_anchored_attach_links:.*?gik_anchored_link_clearance:", hdr, flags=re.S).group(0)
    assert "frozen-t" in doc and "envelope" in doc and "counted once more" in doc


# ---- 4. the device pair function, walked on the host under sanitizers ----------------------------------------
def test_pair_function_walked_by_a_sanitized_host_program(tmp_path):
    """tests/host/anch_link_hinge_walk.cpp: host-only compile of gik_anch_pairs.h (no device code, nothing loaded into
    this interpreter), -fsanitize=address,undefined, run as a program.  It walks anch_link_foot over 400 point matrices x
    66 pairs against a long-double restatement and prints one pinned pair, which must be the mirror's, bit for bit."""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "the HIP toolchain builds this project; it is needed here too"
    exe = str(tmp_path / "anch_link_hinge_walk")
    cmd = [hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           "-static-libsan",      # (the sanitizer runtime inside the program: it runs in whatever environment it is given)
           "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "graphik_amd", "csrc"),
           os.path.join(REPO, "tests", "host", "anch_link_hinge_walk.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith("ok cells 400 pairs 26400 ") and "FAILED" not in r.stdout
    t, m, d = _rs().AnchoredProblem.link_foot_host(PINNED_A, PINNED_B, PINNED_C)
    assert 0.0 < t < 1.0
    tok = lines[1].split()
    assert [tok[0], tok[1], tok[3], tok[7]] == ["pinned", "t", "m", "d"] and len(tok) == 9
    assert [float.fromhex(tok[i]) for i in (2, 4, 5, 6, 8)] == [t, *m, d]
    assert lines[2].split() == ["digest", PARENT_DIGEST]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
