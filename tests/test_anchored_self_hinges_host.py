"""Self hinges in the fixed-anchor solve, host side (CPU only): the device pair function (anch_self_feet) walked by a
stand-alone program under the address and undefined-behaviour sanitizers, the numpy mirror of the hinge terms
(AnchoredProblem.self_hinge_terms_host) against finite differences on configurations that hold every clamp class, the cases
that contribute exactly zero, the Python layer's argument checks and the ABI.
tests/test_anchored_self_hinges_gpu.py takes its points from here."""
import copy
import ctypes as C
import functools
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, make_graph

RHO = 0.03
# anch_self_feet of the pinned pair of tests/host/anch_self_walk.cpp: tests/host/anch_self_hinge_walk.cpp prints it
PINNED = ((0.1, -0.2, 0.3), (0.7, 0.4, -0.1), (0.35, 0.2, 0.25), (-0.15, 0.6, 0.45))
PINNED_PAIR = "0x1.131b36db275a9p-3"      # anch_self_pair of the same ends with radii 0.03 and 0.02 (test_anchored_self_host.py)
# the "digest" line of tests/host/anch_self_hinge_walk.cpp (walk_digest.h: FNV-1a over the bits of (s, t, v, d) of its
# random cells), as that program prints it when compiled against the headers of c11b7a7, where anch_self_feet stood
# next to a second copy of its branches
PARENT_DIGEST = "fe2f9f30117cc5f9"


def _rs():
    from graphik_amd.solvers import riemannian_solver as rs
    return rs


@functools.lru_cache(maxsize=None)
def self_hinge_problem(name="ur10", rho=RHO, pairs="auto", host_only=True, link_hinges=False, self_hinges=True):
    """A robot with its skeleton as capsules of radius rho (a scalar or a tuple, one entry per link) and self pairs."""
    robot, graph = make_graph(name)
    ap = _rs().AnchoredProblem(graph, host_only=host_only, link_radius=rho if np.isscalar(rho) else list(rho), self_pairs=pairs,
                               link_hinges=link_hinges, self_hinges=self_hinges)
    return robot, graph, ap


def clamp_class(s, t):
    """3 i + j: s (i) and t (j) at 0, inside, at 1."""
    c = lambda x: 0 if x == 0.0 else (2 if x == 1.0 else 1)      # noqa: E731
    return 3 * c(s) + c(t)


def active_pairs(ap, Y, ga):
    """Per point: {pair: (s, t)} of the active self hinges, by the mirror."""
    out = []
    for b in range(len(Y)):
        ap.self_hinge_terms_host(Y[b], np.zeros_like(Y[b]), ga[b])
        out.append(dict(ap.last_self_st))
    return out


@functools.lru_cache(maxsize=None)
def hinge_configurations(name):
    """Configurations chosen with the mirror from RandomState(0).uniform(-pi, pi, (4096 | 512, n)) at 3 cm, "auto" pairs:
    per clamp class the first three that hold an active pair of it (and a gradient of at least 1e-5: the differences of
    test 2 need one to compare with), and the one with the most active pairs.  Returns
    (q, Y_free, goal anchors, W, active pairs per point, classes seen in the whole sample)."""
    robot, graph, ap = self_hinge_problem(name)
    q = np.random.RandomState(0).uniform(-np.pi, np.pi, (4096 if name == "ur10" else 512, robot.n))
    Y, ga = ap.seed_points(q), ap.goal_anchors(robot.fk_batch(q))
    act = active_pairs(ap, Y, ga)
    per_class = {k: [] for k in range(9)}
    for b, st in enumerate(act):
        # (a configuration whose only active pairs touch, v = 0, has no gradient to compare a difference with)
        if not st or np.abs(ap.self_hinge_terms_host(Y[b], np.zeros_like(Y[b]), ga[b])[1]).max() < 1e-5:
            continue
        for k in {clamp_class(s, t) for s, t in st.values()}:
            if len(per_class[k]) < 3:
                per_class[k].append(b)
    n_act = np.array([len(st) for st in act])
    pick = sorted({b for v in per_class.values() for b in v} | {int(n_act.argmax())})
    W = np.random.RandomState(1).randn(len(pick), Y.shape[1], 3)
    out = dict(q=q[pick], Y=Y[pick], ga=ga[pick], W=W, act=[act[b] for b in pick],
               seen=sorted(k for k, v in per_class.items() if v), n_active=int((n_act > 0).sum()), most=int(n_act.max()))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---- 1. the device pair function, walked on the host under sanitizers ----------------------------------------
def test_pair_function_walked_by_a_sanitized_host_program(tmp_path):
    """tests/host/anch_self_hinge_walk.cpp: host-only compile of gik_anch_pairs.h (no device code, nothing loaded into
    this interpreter), -fsanitize=address,undefined, run as a program.  It walks anch_self_feet over the planted cells of
    anch_self_walk.cpp and 400 point matrices x 66 pairs: sqrt(d) - rho - rho' is anch_self_pair's value in all 64 bits,
    and distance, vector and square agree with a long-double restatement to the project's 1e-12 (measured worst: distance
    4.9e-16, vector 2.7e-16, square 5.8e-16).  The pinned pair it prints must be the mirror's, bit for bit."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "the HIP toolchain builds this project; it is needed here too"
    exe = str(tmp_path / "anch_self_hinge_walk")
    cmd = [hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           "-static-libsan",      # (the sanitizer runtime inside the program: it runs in whatever environment it is given)
           "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "graphik_amd", "csrc"),
           os.path.join(REPO, "tests", "host", "anch_self_hinge_walk.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith("ok cells 400 pairs 26400 ") and "FAILED" not in r.stdout
    tok = lines[0].split()
    worst = [float(tok[tok.index(w) + 1]) for w in ("distance", "vector", "square")]
    assert max(worst) < 1e-12
    s, t, v, d = _rs().AnchoredProblem.self_feet_host(*PINNED)
    tok = lines[1].split()
    assert [tok[i] for i in (0, 1, 3, 5, 9, 11)] == ["pinned", "s", "t", "v", "d", "value"] and len(tok) == 13
    assert [float.fromhex(tok[i]) for i in (2, 4, 6, 7, 8, 10)] == [s, t, *v, d]
    assert 0.0 < s < 1.0 and t == 0.0      # (the far link's start is the nearest point)
    assert float(np.sqrt(d) - 0.03 - 0.02).hex() == tok[12] == PINNED_PAIR
    assert lines[2].split() == ["digest", PARENT_DIGEST]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


def test_feet_agree_with_the_clearance_mirror_bit_for_bit():
    """sqrt(d) - rho_l - rho_m of self_feet_host is self_clearance's value of the pair, on every pair of 64 UR10 and 64
    LWA4D configurations (zero-length links included)."""
    for name in ("ur10", "lwa4d"):
        robot, graph, ap = self_hinge_problem(name)
        Yf = ap.base.seed_points(np.random.RandomState(5).uniform(-np.pi, np.pi, (64, robot.n)))
        one = _rs().AnchoredProblem(graph, host_only=True, link_radius=RHO, self_pairs="auto")
        for p, (l, m) in enumerate(ap.self_pairs.tolist()):
            one.self_pairs = ap.self_pairs[p:p + 1]
            want = one.self_clearance(Yf)
            for b in range(len(Yf)):
                ends = [Yf[b, r] for r in (*ap.link_rows[l], *ap.link_rows[m])]
                d = ap.self_feet_host(*ends)[3]
                assert float(np.sqrt(d) - RHO - RHO).hex() == float(want[b]).hex(), (name, p, b)


# ---- 2. the mirror against finite differences ----------------------------------------------------------------
def test_mirror_gradient_and_frozen_st_hessian_against_finite_differences():
    """G of the mirror = differences of its f (step 1e-6), H = central differences of the FROZEN-(s, t) gradient along W,
    both within 1e-5 of the largest entry -- the step and the bar of the link hinges' test.  UR10 at 3 cm holds seven of the
    nine clamp classes among its active pairs, (s, t) = (0, 0) and (1, 0) do not occur; LWA4D "auto" (15 pairs, three
    zero-length links: arithmetic, not a robot to solve with) holds the rest.  All nine are covered.

    f is C^1 wherever the closest pair of points is unique in (s, t), with a second derivative that jumps where s or t
    reaches 0 or 1, and C^0 only where it is not: at the ends of a ZERO-LENGTH link (moved towards the other link that end
    becomes the nearest point, moved away the other end stays nearest) and of an exactly PARALLEL pair (the nearest points
    are an interval; a rotation of either link moves the minimum to one end of it or the other).  Neither is rare on these
    skeletons: LWA4D has three zero-length links, whose neighbours touch in every configuration, and UR10's links p0 -> p1
    and p3 -> p4 lie along parallel joint axes in every configuration.  The pair function picks one foot pair, at an end of
    the interval, so there the term's gradient is one of the two one-sided derivatives.  The test therefore takes the
    three-point one-sided differences on either side of every coordinate (O(h^2) like the central one, and blind to a
    jump at the point itself) and asks G to be one of them; where f is C^1 the two agree and it is the central check.
    Pair by pair, each pair's share of f against its share of G (the shares add up to G): two pairs that meet in a kinked
    coordinate may each have picked another side of it.  The bar is that of the whole gradient."""
    h, covered, kinks, coords = 1e-6, set(), 0, 0
    for name in ("ur10", "lwa4d"):
        robot, graph, ap = self_hinge_problem(name)
        c = hinge_configurations(name)
        print(f"{name}: {c['n_active']} configurations with an active pair, up to {c['most']} at once, classes in the sample "
              f"{c['seen']}; {len(c['Y'])} chosen")
        here = set()
        for b in range(len(c["Y"])):
            Y, W, ga = c["Y"][b], c["W"][b], c["ga"][b]
            f0, G, H = ap.self_hinge_terms_host(Y, W, ga)
            st0 = dict(ap.last_self_st)
            assert f0 > 0 and st0 == c["act"][b] and np.abs(G).max() >= 1e-5
            here |= {clamp_class(s, t) for s, t in st0.values()}
            bar = 1e-5 * np.abs(G).max()
            G_sum = np.zeros_like(G)
            for p in st0:      # pair by pair: two pairs that share a kinked coordinate may each sit on another side of it
                one = copy.copy(ap)
                one.self_pairs = ap.self_pairs[p:p + 1]
                f1, G1, _ = one.self_hinge_terms_host(Y, W, ga)
                G_sum += G1
                for i in np.flatnonzero([r is not None and r in ap.free for r in
                                         (*ap.link_rows[ap.self_pairs[p][0]], *ap.link_rows[ap.self_pairs[p][1]])]):
                    i = ap.free.index(int((*ap.link_rows[ap.self_pairs[p][0]], *ap.link_rows[ap.self_pairs[p][1]])[i]))
                    for q in range(3):
                        fs = []
                        for k in (-2, -1, 1, 2):
                            Yk = Y.copy()
                            Yk[i, q] += k * h
                            fs.append(one.self_hinge_terms_host(Yk, W, ga)[0])
                        fmm, fm, fp, fpp = fs
                        right, left = (-3 * f1 + 4 * fp - fpp) / (2 * h), (3 * f1 - 4 * fm + fmm) / (2 * h)
                        err = min(abs(0.5 * right - G1[i, q]), abs(0.5 * left - G1[i, q]))      # (G is 1/2 grad f)
                        assert err <= bar, (name, b, p, i, q, err, bar)
                        coords += 1
                        kinks += abs(0.5 * (fp - fm) / (2 * h) - G1[i, q]) > bar
            assert np.abs(G_sum - G).max() <= 1e-15 * np.abs(G).max()
            Gp = ap.self_hinge_terms_host(Y + h * W, W, ga, frozen_st=st0)[1]
            Gm = ap.self_hinge_terms_host(Y - h * W, W, ga, frozen_st=st0)[1]
            Hd = (Gp - Gm) / (2 * h)
            assert np.abs(Hd - H).max() <= 1e-5 * np.abs(H).max(), (name, b, np.abs(Hd - H).max(), np.abs(H).max())
        print(f"{name}: clamp classes of the chosen configurations' active pairs {sorted(here)}")
        if name == "ur10":
            assert here == {1, 2, 3, 4, 5, 7, 8} and c["most"] >= 6 and c["n_active"] >= 300
        covered |= here
    print(f"{kinks} of {coords} coordinates sit on a kink or a curvature jump that the central difference does not resolve")
    assert covered == set(range(9))


# ---- 3. what contributes exactly zero ----------------------------------------------------------------------------
class _Cell:
    """AnchoredProblem.self_hinge_terms_host on a hand-made scene: four free rows, four constant rows, no robot."""

    def __init__(self, links, pairs, rho=0.0):
        self.link_rows = np.asarray(links, dtype=np.int32).reshape(-1, 2)
        self.link_radius = np.broadcast_to(np.asarray(rho, dtype=float), (len(self.link_rows),))
        self.self_pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        self.free, self.anchors = [0, 1, 2, 3], [4, 5, 6, 7]
        self.anchor_pos = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [9.0, 9.0, 9.0], [9.0, 9.0, 9.0]])
        self.n_goal_anchor = 2
        rs = _rs().AnchoredProblem
        self.self_feet_host, self.link_ends_host = rs.self_feet_host, lambda *a: rs.link_ends_host(self, *a)

    def __call__(self, Y, W, goal):
        return _rs().AnchoredProblem.self_hinge_terms_host(self, np.asarray(Y, float), np.asarray(W, float), np.asarray(goal, float))


def test_what_contributes_exactly_zero():
    # rows 0-1: a link along x; rows 2-3: a link along y that crosses it 1 cm above; anchors 4-5: along x, 6-7 (goal): along y
    Y = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, -0.5, 0.01], [0.5, 0.5, 0.01]]
    W = np.random.RandomState(3).randn(4, 3)
    goal = [0.5, -0.5, 0.01, 0.5, 0.5, 0.01]
    zero = lambda r: r[0] == 0.0 and not r[1].any() and not r[2].any()      # noqa: E731
    links = [(0, 1), (2, 3), (4, 5), (6, 7)]
    # R = 0: never active, whatever the distance -- crossing links included
    assert zero(_Cell(links, [(0, 1), (0, 3), (2, 1), (2, 3)], 0.0)(Y, W, goal))
    Yx = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.5, -0.5, 0.0], [0.5, 0.5, 0.0]]
    assert zero(_Cell(links, [(0, 1)], 0.0)(Yx, W, goal))
    # thick links 1 cm apart are active, at all four ends: v = (0, 0, -0.01), w = (1/2, 1/2, -1/2, -1/2)
    f, G, H = _Cell(links, [(0, 1)], RHO)(Y, W, goal)
    R = RHO + RHO
    res = R * R - 0.01 * 0.01
    assert f == res * res and np.all(G[:, 2] != 0) and not G[:, :2].any() and H.any(axis=1).all()
    assert np.allclose(G[:, 2], [0.5 * 2 * -res * -0.01] * 2 + [-0.5 * 2 * -res * -0.01] * 2, rtol=1e-15)
    # a pair far apart; mixed radii: R is the sum of the two
    assert zero(_Cell(links, [(0, 1)], RHO)([[0, 0, 0], [1, 0, 0], [0.5, -0.5, 0.07], [0.5, 0.5, 0.07]], W, goal))
    f2 = _Cell(links, [(0, 1)], [0.05, 0.01, 0.0, 0.0])(Y, W, goal)[0]
    assert abs(f2 - f) <= 1e-14 * f      # (0.05 + 0.01 and 0.03 + 0.03 differ in the last bit)
    # a pair whose four ends are constants contributes to f only
    f, G, H = _Cell(links, [(2, 3)], RHO)(Y, W, goal)
    assert f == res * res and not G.any() and not H.any()
    # a constant link against a free one: the free ends keep their share, and om holds only their W
    f, G, H = _Cell(links, [(0, 3)], RHO)(Y, W, goal)
    assert f == res * res and G[0].any() and G[1].any() and not G[2:].any() and not H[2:].any()
    f, G, H0 = _Cell(links, [(0, 3)], RHO)(Y, np.zeros((4, 3)), goal)
    assert not H0.any()


# ---- 4. argument checks, before any device call; the ABI ---------------------------------------------------------
def test_self_hinges_argument_checks_need_no_device(monkeypatch):
    from graphik_amd import engine
    rs = _rs()
    robot, graph = make_graph("ur10")

    def no_device(*a, **k):
        raise AssertionError("a device handle was created before the arguments were checked")
    monkeypatch.setattr(engine.Template, "__init__", no_device)
    monkeypatch.setattr(rs.BatchProblem, "__init__", no_device)
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="self_hinges must be a bool"):
            rs.AnchoredProblem(graph, self_pairs="auto", self_hinges=bad)
    with pytest.raises(ValueError, match="self_hinges=True needs self pairs"):
        rs.AnchoredProblem(graph, self_hinges=True)
    with pytest.raises(ValueError, match="link set"):
        rs.AnchoredProblem(graph, links=[], self_pairs="auto", self_hinges=True)
    # more than 16 pairs: the skeleton's six links and two more that share no row with them have 10 + 13
    skeleton = [(f"p{i}", f"p{i + 1}") for i in range(6)]
    with pytest.raises(ValueError, match="at most 16 self pairs, got 23"):
        rs.AnchoredProblem(graph, links=skeleton + [("q1", "q2"), ("q3", "q4")], self_pairs="auto", self_hinges=True)


def test_host_only_problem_keeps_the_flag():
    robot, graph, ap = self_hinge_problem()
    assert ap.self_hinges is True and ap.template is None and len(ap.self_pairs) == 10
    plain = _rs().AnchoredProblem(graph, host_only=True, self_pairs="auto")
    assert plain.self_hinges is False
    # the seven links of a 7-DOF skeleton have 15 pairs: inside the limit
    assert len(self_hinge_problem("kuka")[2].self_pairs) == 15 and len(self_hinge_problem("lwa4d")[2].self_pairs) == 15


def test_abi_carries_the_self_hinge_entry_point():
    from graphik_amd import _ffi
    assert "gik_anchored_attach_self_hinges" in _ffi.SYMBOLS
    hdr = open(os.path.join(REPO, "include", "graphik_amd.h")).read()
    assert int(re.search(r"#define GIK_ABI_VERSION (\d+)", hdr).group(1)) == _ffi.ABI_VERSION == 12
    assert re.search(r"int gik_anchored_attach_self_hinges\(gik_template \*anch\);", hdr)
    # no struct changed: the sizes of test_abi_carries_the_self_entry_points
    sizes = {"TemplateDesc": 152, "TemplateInfo": 68, "Stats": 48, "Trace": 56, "PipelineDesc": 208, "AnchoredDesc": 120,
             "RetryOpts": 48, "AnchoredRetryOpts": 64, "LinkDesc": 32, "SceneSet": 32, "PrepareDiag": 24}
    assert {name: C.sizeof(getattr(_ffi, name)) for name in sizes} == sizes
    assert _ffi.SELF_HINGE_MAX_PAIRS == 16 and _ffi.SELF_MAX_PAIRS == 2016
    doc = re.search(r"gik_anchored_attach_self_hinges: SELF HINGES.*?\*/", hdr, flags=re.S).group(0)
    assert "bit for bit" in doc and "frozen" in doc and "more than 16 pairs" in doc
    from graphik_amd import build
    assert "gik_k_anch_self.hip" in build.SOURCES
