"""Self-collision clearance (link against link) in the fixed-anchor solve, host side (CPU only): the numpy mirror of
gik_anchored_self_clearance on hand-made cells, its symmetry, the scene figures that say how often the robot meets itself
where every other measure calls it clear (UR10 + table_environment(), reproduced from their seeds), the Python layer's
argument checks, the ABI's new entry points, and the pair function walked by a stand-alone program under the address and
undefined-behaviour sanitizers.  tests/test_anchored_self_gpu.py takes its inputs from here."""
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

PINNED_PAIR = "0x1.131b36db275a9p-3"      # the pinned line of tests/host/anch_self_walk.cpp: its four ends, radii 0.03 and 0.02
# the "digest" line of tests/host/anch_self_walk.cpp (walk_digest.h: FNV-1a over the bits of every pair value of its
# random cells), as that program prints it when compiled against the headers of c11b7a7, where anch_self_pair was a
# copy of anch_self_feet's branches
PARENT_DIGEST = "a918a60f3b204b35"
RHO = 0.03


def _rs():
    from graphik_amd.solvers import riemannian_solver as rs
    return rs


class _Cell:
    """AnchoredProblem.self_clearance on hand-made links: rows of Y are the points, no robot behind them."""

    def __init__(self, links, pairs, rho=0.0):
        self.link_rows = np.asarray(links, dtype=np.int32).reshape(-1, 2)
        self.link_radius = np.broadcast_to(np.asarray(rho, dtype=float), (len(self.link_rows),))
        self.self_pairs = np.asarray(pairs, dtype=np.int32).reshape(-1, 2)

    def __call__(self, Y):
        return _rs().AnchoredProblem.self_clearance(self, np.asarray(Y, dtype=float))


def clamp_cells(cell, Y):
    """[B, P] ints 3 i + j: where the closest points of every pair lie -- s (i) and t (j) at 0, inside, at 1 -- by the steps
    of the mirror."""
    Y = np.asarray(Y, dtype=float)
    rows, pairs = np.asarray(cell.link_rows), np.asarray(cell.self_pairs)
    a1, b1 = Y[:, rows[pairs[:, 0], 0]], Y[:, rows[pairs[:, 0], 1]]
    a2, b2 = Y[:, rows[pairs[:, 1], 0]], Y[:, rows[pairs[:, 1], 1]]
    dot = lambda x, y: (x * y).sum(-1)      # noqa: E731
    clamp = lambda x: np.clip(x, 0.0, 1.0)      # noqa: E731
    with np.errstate(invalid="ignore", divide="ignore"):
        d1, d2, r = b1 - a1, b2 - a2, a1 - a2
        a, e, f, c, b = dot(d1, d1), dot(d2, d2), dot(d2, r), dot(d1, r), dot(d1, d2)
        den = a * e - b * b
        s = np.where((a > 0) & (den > 0), clamp((b * f - c * e) / den), 0.0)
        t = np.where(e > 0, (b * s + f) / e, -1.0)
        s = np.where(t < 0, np.where(a > 0, clamp(-c / a), 0.0), np.where(t > 1, np.where(a > 0, clamp((b - c) / a), 0.0), s))
        t = clamp(t)
    cls = lambda x: np.where(x == 0.0, 0, np.where(x == 1.0, 2, 1))      # noqa: E731
    return 3 * cls(s) + cls(t)


# ---- 1. the mirror on hand-made cells ------------------------------------------------------------------------
# link 1 along x from 0 to 1; link 2 of length 1 along y from (x0, y0, z0), in eighths (exact): s = clamp(x0),
# t = clamp(-y0), and every clamped cell is a 3-4-5 triangle of hypotenuse 0.625
NINE = [(-0.375, 0.5, 0), (-0.375, -0.5, 0.5), (-0.375, -1.5, 0),       # s = 0: t = 0, interior, 1
        (0.25, 0.5, 0.375), (0.5, -0.5, 0.25), (0.25, -1.5, 0.375),     # s interior (the fifth: two skew links, both interior)
        (1.375, 0.5, 0), (1.375, -0.5, 0.5), (1.375, -1.5, 0)]          # s = 1


def test_mirror_on_hand_made_cells():
    X = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]
    two = _Cell([(0, 1), (2, 3)], [(0, 1)])
    one = lambda a2, b2, cell=two: float(cell([X + [list(a2), list(b2)]])[0])      # noqa: E731
    for k, (x0, y0, z0) in enumerate(NINE):
        Y = [X + [[x0, y0, z0], [x0, y0 + 1.0, z0]]]
        assert clamp_cells(two, Y)[0, 0] == k
        assert two(Y)[0] == (0.25 if k == 4 else 0.625), k
    assert one((0.5, 0.25, 0), (1.5, 0.25, 0)) == 0.25                      # parallel, overlapping
    assert one((1.375, 0.5, 0), (2.375, 0.5, 0)) == 0.625                   # parallel, disjoint: end against end
    thick = _Cell([(0, 1), (2, 3)], [(0, 1)], [0.03, 0.02])
    assert one((0.5, -0.5, 0), (0.5, 0.5, 0), thick) == -0.03 - 0.02        # crossing: exactly -rho1 - rho2
    pt = (0.5, 0.25, 0)
    assert one(pt, pt) == 0.25                                              # one zero-length link, second ...
    assert float(_Cell([(2, 3), (0, 1)], [(0, 1)])([X + [list(pt), list(pt)]])[0]) == 0.25      # ... and first of its pair
    assert float(_Cell([(0, 0), (2, 2)], [(0, 1)])([X + [[-0.375, 0.5, 0]] * 2])[0]) == 0.625   # two: point against point
    assert one((0.5, 0.25, 0), (1.5, 0.25, 0), _Cell([(0, 1), (2, 3)], [(0, 1)], [0.125, 0.0625])) == 0.0625   # radii subtract exactly
    # a NaN in each of the four ends: NaN for that goal alone
    good = X + [[0.5, -0.5, 0.25], [0.5, 0.5, 0.25]]
    Yb = np.array([good] * 6, dtype=float)
    for k in range(4):
        Yb[k + 1, k, k % 3] = np.nan
    got = two(Yb)
    assert np.all(np.isnan(got[1:5])) and got[0] == got[5] == 0.25
    # several pairs: the minimum; a NaN in a link no pair names is not read; no pairs: +inf
    many = _Cell([(0, 1), (2, 3), (4, 5), (6, 7)], [(0, 1), (0, 2), (1, 2)])
    Y = X + [[0.5, -0.5, 0.25], [0.5, 0.5, 0.25], [1.375, 0.5, 0], [1.375, 1.5, 0], [np.nan, 0, 0], [0, 0, 0]]
    assert many([Y])[0] == 0.25
    assert np.isposinf(_Cell([(0, 1), (2, 3)], [])([good])[0])
    none = _Cell([(0, 1)], [])
    none.self_pairs = None
    assert np.isposinf(none([good])[0])
    # the pinned vector of tests/host/anch_self_walk.cpp, bit for bit
    v = thick([[[0.1, -0.2, 0.3], [0.7, 0.4, -0.1], [0.35, 0.2, 0.25], [-0.15, 0.6, 0.45]]])[0]
    assert float(v).hex() == PINNED_PAIR


# ---- 2. the scene ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def self_problem():
    """UR10 + table, host only: the skeleton as capsules of 3 cm, the ten pairs that share no end row."""
    robot, graph = make_graph("ur10_table")
    ap = _rs().AnchoredProblem(graph, host_only=True, link_radius=RHO, self_pairs="auto")
    return robot, graph, ap


@functools.lru_cache(maxsize=None)
def uniform_configurations():
    """RandomState(7).uniform(-pi, pi, (2048, 6)) on UR10 + table with its realizations and the three clearances."""
    robot, graph, ap = self_problem()
    q = np.random.RandomState(7).uniform(-np.pi, np.pi, (2048, 6))
    Y = ap.base.seed_points(q)
    out = dict(q=q, Y=Y, node=ap.clearance(Y), link=ap.link_clearance(Y), self=ap.self_clearance(Y))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def world_clear_self_colliding():
    """Indices into uniform_configurations()["q"]: every joint point and every link (3 cm) more than 1 cm clear of the
    table, two of the robot's own capsules more than 1 cm inside each other."""
    u = uniform_configurations()
    return np.flatnonzero((u["node"] > 0.01) & (u["link"] > 0.01) & (u["self"] < -0.01))


def test_auto_pairs_and_symmetry():
    robot, graph, ap = self_problem()
    assert ap.self_pairs.dtype == np.int32
    assert ap.self_pairs.tolist() == [[0, 2], [0, 3], [0, 4], [0, 5], [1, 3], [1, 4], [1, 5], [2, 4], [2, 5], [3, 5]]
    u = uniform_configurations()
    swapped = _Cell(ap.link_rows, ap.self_pairs[:, ::-1], ap.link_radius)
    diff = np.abs(swapped(u["Y"]) - u["self"]).max()
    print("swapping the links of every pair moves the value by at most", diff)
    assert diff <= 1e-15
    assert np.array_equal(ap.self_clearance(u["Y"][:7]), u["self"][:7])      # a goal's value does not depend on the batch
    # thicker capsules are nearer by exactly twice the difference, pair by pair: the minimum moves by it up to a rounding
    _, graph2 = make_graph("ur10_table")
    thin = _rs().AnchoredProblem(graph2, host_only=True, self_pairs="auto")
    assert np.abs(thin.self_clearance(u["Y"]) - (u["self"] + 2 * RHO)).max() < 1e-15
    # the short wrist: links 2 and 4 are joined by link 3, 11.5 cm long -- capsules of 6 cm always overlap
    L3 = np.linalg.norm(u["Y"][:, ap.link_rows[3, 1]] - u["Y"][:, ap.link_rows[3, 0]], axis=-1)
    assert np.abs(L3 - 0.1149).max() < 1e-4
    assert np.all(_Cell(ap.link_rows, [(2, 4)], 0.06)(u["Y"]) < 0)


def test_scene_figures_from_their_seeds():
    """What every existing measure calls clear.  Counts with room below what this checkout measures (104 of 2048 world-clear
    and self-colliding by more than 1 cm, of 150 self-colliding; 9.3 % of RandomState(0)'s 4096)."""
    robot, graph, ap = self_problem()
    u = uniform_configurations()
    hit = world_clear_self_colliding()
    depth = -u["self"][hit]
    print("self-colliding:", int((u["self"] < 0).sum()), "of 2048; world-clear by > 1 cm and self-colliding by > 1 cm:", len(hit),
          "; median depth", np.median(depth), "deepest", depth.max())
    assert len(hit) >= 64
    # all nine clamp combinations occur among the pairs of these configurations (with l < m as "auto" orders a pair, the
    # rarest -- s = 0, t = 1 -- 31 times; among the 150 self-colliding ones alone it happens not to), and among the
    # self-colliding configurations of RandomState(0): none of the branches is exotic
    cells = np.bincount(clamp_cells(ap, u["Y"]).ravel(), minlength=9)
    print("clamp combinations, all pairs of the 2048 configurations:", cells.tolist(), "; of the self-colliding ones:",
          np.bincount(clamp_cells(ap, u["Y"][u["self"] < 0]).ravel(), minlength=9).tolist())
    assert np.all(cells >= 16)
    q = np.random.RandomState(0).uniform(-np.pi, np.pi, (4096, 6))
    Y0 = ap.base.seed_points(q)
    hit0 = ap.self_clearance(Y0) < 0
    print("self-colliding share of RandomState(0): %.1f %%" % (100 * hit0.mean()))
    assert 0.05 <= hit0.mean() <= 0.15
    cells0 = np.bincount(clamp_cells(ap, Y0[hit0]).ravel(), minlength=9)
    print("clamp combinations among the self-colliding configurations of RandomState(0):", cells0.tolist())
    assert np.all(cells0 > 0)


def test_sweep_mirror():
    robot, graph, ap = self_problem()
    u = uniform_configurations()
    qa, qb = u["q"][:33], u["q"][33:66]
    one = ap.sweep_self_clearance_host(qa, qb, 1)
    assert np.array_equal(one, np.minimum(u["self"][:33], u["self"][33:66]))
    eight = ap.sweep_self_clearance_host(qa, qb, 8)
    assert np.all(eight <= one) and np.all(ap.sweep_self_clearance_host(qa, qb, 4) >= eight)      # nested samples


# ---- 3. argument checks ------------------------------------------------------------------------------------------
def test_python_layer_refuses_before_any_device_call():
    from graphik_amd.engine import check_clearance_mode
    assert check_clearance_mode("links+self") == 2 and check_clearance_mode("links", True, False) == 1
    assert check_clearance_mode("nodes", has_links=False, has_self=False) == 0
    with pytest.raises(ValueError, match="self pairs"):
        check_clearance_mode("links+self", has_links=True, has_self=False)
    with pytest.raises(ValueError, match="link set"):
        check_clearance_mode("links+self", has_links=False, has_self=False)
    AP = _rs().AnchoredProblem
    _, graph = make_graph("ur10_table")
    for kw, word in ((dict(links=[], self_pairs="auto"), "link set"), (dict(links=[], self_pairs=[]), "link set"),
                     (dict(self_pairs=[(0, 6)]), "outside"), (dict(self_pairs=[(-1, 2)]), "outside"),
                     (dict(self_pairs=[(2, 2)]), "l == m"), (dict(self_pairs=[(0, 2), (1, 2)]), "share"),
                     (dict(self_pairs="all"), "'auto'"), (dict(self_pairs=[(0, 2, 4)]), "two link indices"),
                     (dict(self_pairs=[(0, 2.5)]), "two link indices")):
        with pytest.raises(ValueError, match=word):
            AP(graph, host_only=True, **kw)
    explicit = AP(graph, host_only=True, self_pairs=[(4, 0), (1, 5)])
    assert explicit.self_pairs.tolist() == [[4, 0], [1, 5]] and explicit.template is None
    assert AP(graph, host_only=True, self_pairs=[]).self_pairs.shape == (0, 2)
    plain = AP(graph, host_only=True)
    assert plain.self_pairs is None and np.all(np.isposinf(plain.self_clearance(np.zeros((3, plain.base.N, 3)))))
    # a host-only problem has no template: any device call would raise AttributeError, not ValueError
    robot = graph.robot
    T = robot.fk_batch(np.zeros((2, robot.n)))
    q0 = np.zeros((2, robot.n))
    for kw in (dict(), dict(retries=1)):
        with pytest.raises(ValueError, match="self pairs"):
            plain.solve(T, q_init=q0, clearance_mode="links+self", **kw)
        with pytest.raises(ValueError, match="self pairs"):
            plain.solve_trajectory(T[:, None], q0, clearance_mode="links+self", **kw)
    with pytest.raises(ValueError, match="self pairs"):
        plain.sweep_self_clearance(q0, q0, 2)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="samples"):
            explicit.sweep_self_clearance(q0, q0, bad)
        with pytest.raises(ValueError, match="samples"):
            explicit.sweep_self_clearance_host(q0, q0, bad)


def test_abi_carries_the_self_entry_points():
    from graphik_amd import _ffi
    for name in ("gik_anchored_attach_self_pairs", "gik_anchored_self_clearance", "gik_anchored_sweep_clearances"):
        assert name in _ffi.SYMBOLS
    hdr = open(os.path.join(REPO, "include", "graphik_amd.h")).read()
    assert int(re.search(r"#define GIK_ABI_VERSION (\d+)", hdr).group(1)) == _ffi.ABI_VERSION == 12
    assert re.search(r"#define GIK_CLEARANCE_LINKS_SELF (\d+)", hdr).group(1) == str(_ffi.CLEARANCE_LINKS_SELF) == "2"
    assert _ffi.CLEARANCE_MODES == {"nodes": 0, "links": 1, "links+self": 2}
    # no struct changed: the sizes of the parent commit
    sizes = {"TemplateDesc": 152, "TemplateInfo": 68, "Stats": 48, "Trace": 56, "PipelineDesc": 208, "AnchoredDesc": 120,
             "RetryOpts": 48, "AnchoredRetryOpts": 64, "LinkDesc": 32, "SceneSet": 32, "PrepareDiag": 24}
    assert {name: C.sizeof(getattr(_ffi, name)) for name in sizes} == sizes
    doc = re.search(r"gik_anchored_sweep_clearances:.*?\*/", hdr, flags=re.S).group(0)
    assert "NOT\n *   CONSERVATIVE" in doc or "NOT CONSERVATIVE" in " ".join(doc.replace(" *", " ").split())
    assert "SHARE AN END ROW" in hdr
    assert "NOT CONSERVATIVE" in " ".join(_rs().AnchoredProblem.sweep_self_clearance.__doc__.split())


# ---- 4. the pair function in a program of its own, under the sanitizers ------------------------------------------
def test_pair_function_walked_by_a_sanitized_host_program(tmp_path):
    """tests/host/anch_self_walk.cpp: host-only compile of gik_anch_pairs.h (no device code, nothing loaded into this
    interpreter), -fsanitize=address,undefined, run as a program.  It walks anch_self_pair over hand-made cells and 400
    point matrices x 66 pairs against a long-double restatement (measured worst difference: 4.9e-16; the bar is the
    1e-12 the project holds device against mirror to), and prints one pinned value, which must be the mirror's."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "the HIP toolchain builds this project; it is needed here too"
    exe = str(tmp_path / "anch_self_walk")
    cmd = [hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           "-static-libsan",      # (the sanitizer runtime inside the program: it runs in whatever environment it is given)
           "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "graphik_amd", "csrc"),
           os.path.join(REPO, "tests", "host", "anch_self_walk.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith("ok cells 400 pairs 26400 ") and "FAILED" not in r.stdout
    assert float(lines[0].split()[-1]) < 1e-12
    assert lines[1].split() == ["pinned", "pair", PINNED_PAIR]
    assert lines[2].split() == ["digest", PARENT_DIGEST]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
