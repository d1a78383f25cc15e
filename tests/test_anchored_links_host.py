"""Clearance of whole links in the fixed-anchor solve, host side (CPU only): the numpy mirror of
gik_anchored_link_clearance on hand-made cells, its order against the node clearance, the two scene figures that say why
the node clearance is not enough (UR10 + table_environment(), reproduced from their seeds), the Python layer's argument
checks, the ABI's new entry points, and the header's __host__ __device__ helpers walked by a stand-alone program under
the address and undefined-behaviour sanitizers.  tests/test_anchored_links_gpu.py takes its inputs from here."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, make_graph
from test_anchored_seeded_host import host_problem

PINNED_PAIR = "0x1.bd10b276dadacp-5"          # a = (.1, -.2, .3), b = (.7, .4, -.1), c = (.35, .2, .25), r^2 = .01, rho = .03
PINNED_INTERP = "-0x1.1d41d41d41d42p-1"       # (1 - 3/7) 0.3 + (3/7) (-1.7)
# the "digest" line of tests/host/anch_link_walk.cpp (walk_digest.h: FNV-1a over the bits of every pair value of its
# random cells), as that program prints it when compiled against the headers of c11b7a7, where anch_link_pair had its
# foot parameter written out
PARENT_DIGEST = "675263e7176170bd"


def _rs():
    from graphik_amd.solvers import riemannian_solver as rs
    return rs


class _Cell:
    """AnchoredProblem.link_clearance on a hand-made scene: rows of Y are the points, no robot behind them."""

    def __init__(self, links, spheres, rho=0.0):
        self.link_rows = np.asarray(links, dtype=np.int32).reshape(-1, 2)
        self.obstacles = np.asarray(spheres, dtype=float).reshape(-1, 4)
        self.link_radius = np.broadcast_to(np.asarray(rho, dtype=float), (len(self.link_rows),))

    def __call__(self, Y):
        return _rs().AnchoredProblem.link_clearance(self, np.asarray(Y, dtype=float))


# ---- 1. the mirror on hand-made cells ------------------------------------------------------------------------
def test_mirror_on_hand_made_cells():
    """A link along x from 0 to 1 and one sphere of radius 0.1: the three clamp cases, the degenerate ones, by hand."""
    r = 0.1
    rr = np.sqrt(r * r)                        # (what the device holds is r^2)
    Y = [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]
    one = lambda c, rho=0.0, links=((0, 1),), Y=Y: float(_Cell(links, [[*c, r]], rho)([Y])[0])      # noqa: E731
    assert one((0.5, 0.3, 0.0)) == 0.3 - rr                         # nearest point in the interior
    assert one((-0.3, 0.4, 0.0)) == 0.5 - rr                        # at end a (3-4-5)
    assert one((1.3, 0.0, 0.4)) == np.sqrt((1.3 - 1.0) ** 2 + 0.4 ** 2) - rr      # at end b
    assert one((0.25, 0.0, 0.0)) == -rr                             # the centre on the segment: -r
    assert one((-0.3, 0.4, 0.0), links=((0, 0),)) == 0.5 - rr       # a zero-length link is its point
    assert one((0.5, 0.3, 0.0), rho=0.03) == 0.3 - rr - 0.03        # rho subtracts exactly
    assert one((0.5, 0.05, 0.0)) == 0.05 - rr < 0                   # both ends outside the sphere, the link inside it
    # a NaN end, either one, gives NaN -- for that goal alone
    cell = _Cell([(0, 1)], [[-0.3, 0.4, 0.0, r]])
    Yb = np.array([Y, Y, Y, Y], dtype=float)
    Yb[1, 1, 2] = np.nan                      # in b alone: L2 is NaN, t would be 0 and v = u finite
    Yb[2, 0, 0] = np.nan
    got = cell(Yb)
    assert np.isnan(got[1]) and np.isnan(got[2]) and got[0] == got[3] == 0.5 - rr
    # two links, two spheres: the minimum over the four pairs; no link or no sphere: +inf
    two = _Cell([(0, 1), (1, 2)], [[0.5, 0.3, 0.0, r], [1.0, 2.0, 0.0, 0.25]])
    assert two([[[0, 0, 0], [1, 0, 0], [1, 1, 0]]])[0] == min(0.3 - rr, 1.0 - 0.25)
    assert np.isposinf(_Cell([], [[0, 0, 0, r]])([Y])[0]) and np.isposinf(_Cell([(0, 1)], [])([Y])[0])
    # the pinned vector of tests/host/anch_link_walk.cpp
    # (the program holds r^2 = 0.01, here r = 0.1 and r^2 rounds to 0.010000000000000002: one ulp of 0.1 at the most)
    v = _Cell([(0, 1)], [[0.35, 0.2, 0.25, 0.1]], rho=0.03)([[[0.1, -0.2, 0.3], [0.7, 0.4, -0.1]]])[0]
    assert abs(v - float.fromhex(PINNED_PAIR)) <= 2.0 ** -56


# ---- 2. the scene ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def uniform_pairs():
    """The issue's waypoint pairs on UR10 + table: qa = RandomState(7).uniform(-pi, pi, (2048, 6)), qb = qa + U(-0.6, 0.6)
    clipped to [-pi, pi], with the realizations and clearances both tests below (and the GPU tests) read."""
    robot, graph, ap = host_problem()
    rng = np.random.RandomState(7)
    qa = rng.uniform(-np.pi, np.pi, (2048, 6))
    qb = np.clip(qa + rng.uniform(-0.6, 0.6, (2048, 6)), -np.pi, np.pi)
    Ya, Yb = ap.base.seed_points(qa), ap.base.seed_points(qb)
    out = dict(qa=qa, qb=qb, Ya=Ya, node_a=ap.clearance(Ya), link_a=ap.link_clearance(Ya), link_b=ap.link_clearance(Yb))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def node_clear_link_colliding():
    """Indices into uniform_pairs()["qa"]: every joint point more than 1 cm outside the spheres, a link more than 1 cm inside."""
    u = uniform_pairs()
    return np.flatnonzero((u["node_a"] > 0.01) & (u["link_a"] < -0.01))


@functools.lru_cache(maxsize=None)
def sweep_colliding_pairs(S=8):
    """Indices of the pairs whose two ends are link-clear by more than 1 cm and whose S-sample sweep goes more than 1 cm in."""
    robot, graph, ap = host_problem()
    u = uniform_pairs()
    ends = (u["link_a"] > 0.01) & (u["link_b"] > 0.01)
    sw = ap.sweep_clearance_host(u["qa"], u["qb"], S)
    return np.flatnonzero(ends & (sw < -0.01)), int(ends.sum())


def test_default_links_are_the_chain_skeleton():
    robot, graph, ap = host_problem()
    g = ap.base.graph
    assert ap.link_names == [(f"p{i}", f"p{i + 1}") for i in range(6)]
    assert ap.link_rows.tolist() == [[g.index(f"p{i}"), g.index(f"p{i + 1}")] for i in range(6)]
    assert ap.link_radius.tolist() == [0.0] * 6
    AP = _rs().AnchoredProblem
    _, graph2 = make_graph("ur10_table")
    a2 = AP(graph2, host_only=True, links=[("p2", "p3"), ("p1", "q1")], link_radius=[0.03, 0.0])
    assert a2.link_rows.tolist() == [[g.index("p2"), g.index("p3")], [g.index("p1"), g.index("q1")]]
    assert a2.link_radius.tolist() == [0.03, 0.0]
    assert AP(graph2, host_only=True, links=[]).link_rows.shape == (0, 2)
    assert AP(graph2, host_only=True, link_radius=0.05).link_radius.tolist() == [0.05] * 6
    for kw, word in ((dict(links=[("p2", "nowhere")]), "node names"), (dict(link_radius=[0.1, 0.2]), "one entry per link"),
                     (dict(link_radius=-0.01), "at least 0"), (dict(link_radius=np.nan), "at least 0")):
        with pytest.raises(ValueError, match=word):
            AP(graph2, host_only=True, **kw)


def test_skeleton_link_clearance_is_below_the_node_clearance():
    """A segment holds its ends, so with rho = 0 the skeleton's value is the node clearance's (end effector included) or
    less.  In floating point the end-b case computes |(c - a) - 1 (b - a)| where the node formula computes |b - c|: three
    more roundings per coordinate of points within 2.5 m of the origin, each at most 2^-52 -- 1e-15 covers them."""
    robot, graph, ap = host_problem()
    q = np.random.RandomState(5).uniform(-np.pi, np.pi, (256, 6))
    Y = ap.base.seed_points(q)
    link, node = ap.link_clearance(Y), ap.clearance(Y, include_goal=True)
    assert link.shape == (256,) and np.all(np.isfinite(link))
    assert np.all(link <= node + 1e-15)
    assert (link < node - 1e-3).sum() >= 64                      # ... and it is often smaller: a link is nearer than its ends
    assert np.all(ap.link_clearance(Y[:7]) == link[:7])          # a goal's value does not depend on the batch
    # a thicker link is nearer by exactly its radius, pair by pair, so the minimum moves by it up to one rounding
    _, graph2 = make_graph("ur10_table")
    thick = _rs().AnchoredProblem(graph2, host_only=True, link_radius=0.03)
    assert np.abs(thick.link_clearance(Y) - (link - 0.03)).max() < 1e-15


def test_scene_figures_from_their_seeds():
    """UR10 + table_environment(), uniform configurations: what the joint points miss.  Counts with room below what this
    checkout measures (135 of 2048; 20 of 1415)."""
    robot, graph, ap = host_problem()
    u = uniform_pairs()
    hit = node_clear_link_colliding()
    print("node-clear by > 1 cm and link-colliding by > 1 cm:", len(hit), "of 2048")
    assert len(hit) >= 100
    pairs, ends = sweep_colliding_pairs()
    print("pairs with both ends link-clear by > 1 cm:", ends, "; of them sweep-colliding by > 1 cm at S = 8:", len(pairs))
    assert len(pairs) >= 10
    # the 4096 configurations of RandomState(0): share that is node-clear, share that is link-clear
    q = np.random.RandomState(0).uniform(-np.pi, np.pi, (4096, 6))
    Y = ap.base.seed_points(q)
    node, link = ap.clearance(Y) >= 0, ap.link_clearance(Y) >= 0
    print("node-clear %.1f %%, link-clear %.1f %%" % (100 * node.mean(), 100 * link.mean()))
    assert node.mean() - link.mean() > 0.05 and not np.any(link & ~node)


def test_sweep_mirror():
    robot, graph, ap = host_problem()
    u = uniform_pairs()
    qa, qb = u["qa"][:33], u["qb"][:33]
    for S in (1, 7, 8):
        qs = ap.sweep_points(qa, qb, S)
        assert qs.shape == (S + 1, 33, 6)
        assert np.array_equal(qs[0].view(np.int64), qa.view(np.int64)) and np.array_equal(qs[S].view(np.int64), qb.view(np.int64))
        w = 3 / S if S > 3 else 1 / S
        assert np.array_equal(qs[3 if S > 3 else 1], (1.0 - w) * qa + w * qb)
    assert ap.sweep_points([[0.3]], [[-1.7]], 7)[3, 0, 0] == float.fromhex(PINNED_INTERP)
    one = ap.sweep_clearance_host(qa, qb, 1)
    assert np.array_equal(one, np.minimum(u["link_a"][:33], u["link_b"][:33]))
    eight = ap.sweep_clearance_host(qa, qb, 8)
    assert np.all(eight <= one) and np.all(ap.sweep_clearance_host(qa, qb, 4) >= eight)      # nested samples


# ---- 3. argument checks ------------------------------------------------------------------------------------------
def test_python_layer_refuses_before_any_device_call():
    from graphik_amd.engine import check_clearance_mode
    assert check_clearance_mode("nodes") == 0 and check_clearance_mode("links") == 1
    assert check_clearance_mode("nodes", has_links=False) == 0
    robot, graph, ap = host_problem()             # host_only: ap.template is None, any device call would raise AttributeError
    T = robot.fk_batch(np.zeros((2, robot.n)))
    q0 = np.zeros((2, robot.n))
    for bad in ("link", "Nodes", 1, None):
        with pytest.raises(ValueError, match="clearance_mode"):
            ap.solve(T, q_init=q0, clearance_mode=bad)
        with pytest.raises(ValueError, match="clearance_mode"):
            ap.solve_trajectory(T[:, None], q0, clearance_mode=bad)
    _, graph2 = make_graph("ur10_table")
    bare = _rs().AnchoredProblem(graph2, host_only=True, links=[])
    for kw in (dict(), dict(retries=1)):
        with pytest.raises(ValueError, match="link set"):
            bare.solve(T, q_init=q0, clearance_mode="links", **kw)
        with pytest.raises(ValueError, match="link set"):
            bare.solve_trajectory(T[:, None], q0, clearance_mode="links", **kw)
    with pytest.raises(ValueError, match="link set"):
        bare.solve_trajectory(T[:, None], q0, sweep=2)
    with pytest.raises(ValueError, match="link set"):
        bare.sweep_clearance(q0, q0, 2)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="sweep"):
            ap.solve_trajectory(T[:, None], q0, sweep=bad)
        with pytest.raises(ValueError, match="samples"):
            ap.sweep_clearance(q0, q0, bad)
        with pytest.raises(ValueError, match="samples"):
            ap.sweep_clearance_host(q0, q0, bad)


def test_abi_carries_the_link_entry_points():
    import ctypes as C
    from graphik_amd import _ffi
    for name in ("gik_anchored_attach_links", "gik_anchored_link_clearance", "gik_anchored_sweep_ws_bytes",
                 "gik_anchored_sweep_clearance"):
        assert name in _ffi.SYMBOLS
    hdr = open(os.path.join(REPO, "include", "graphik_amd.h")).read()
    assert int(re.search(r"#define GIK_ABI_VERSION (\d+)", hdr).group(1)) == _ffi.ABI_VERSION >= 10
    assert re.search(r"#define GIK_CLEARANCE_NODES (\d+)", hdr).group(1) == str(_ffi.CLEARANCE_NODES) == "0"
    assert re.search(r"#define GIK_CLEARANCE_LINKS (\d+)", hdr).group(1) == str(_ffi.CLEARANCE_LINKS) == "1"
    nocomment = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    fields = lambda cname: [n.strip().lstrip("*") for n in re.findall(      # noqa: E731
        r"\b(?:const\s+)?(?:double|int32_t|uint64_t)\s+([^;]+);",
        re.search(r"typedef struct \{([^}]*)\} %s;" % cname, nocomment).group(1))]
    # the renamed field: the second of gik_anchored_retry_opts, where reserved0 was -- the layout is the old one
    names = fields("gik_anchored_retry_opts")
    assert names == [n for n, _ in _ffi.AnchoredRetryOpts._fields_]
    assert names[1] == "clearance_mode" and "reserved0" not in names
    assert _ffi.AnchoredRetryOpts.clearance_mode.offset == 4 and _ffi.AnchoredRetryOpts.seed.offset == 8
    assert C.sizeof(_ffi.AnchoredRetryOpts) == 64 and _ffi.AnchoredRetryOpts(retries=1).clearance_mode == 0
    assert fields("gik_link_desc") == [n for n, _ in _ffi.LinkDesc._fields_]
    assert C.sizeof(_ffi.LinkDesc) == 32 and _ffi.LinkDesc.link_a.offset == 8
    # the header says what the sweep is not
    doc = re.search(r"gik_anchored_sweep_clearance:.*?\*/", hdr, flags=re.S).group(0)
    assert "NOT CONSERVATIVE" in doc and "joint step" in doc
    assert "NOT CONSERVATIVE" in " ".join(_rs().AnchoredProblem.sweep_clearance.__doc__.split())


# ---- 4. the header's helpers in a program of their own, under the sanitizers -------------------------------------
def test_header_helpers_walked_by_a_sanitized_host_program(tmp_path):
    """tests/host/anch_link_walk.cpp: host-only compile of gik_anch_pairs.h (no device code, nothing loaded into this
    interpreter), -fsanitize=address,undefined, run as a program.  It walks anch_link_pair over 400 point matrices x 66
    pairs against a long-double restatement, anch_sweep_interp and anch_sweep_min, and prints two pinned values, which
    must be the mirror's."""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "the HIP toolchain builds this project; it is needed here too"
    exe = str(tmp_path / "anch_link_walk")
    cmd = [hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           "-static-libsan",      # (the sanitizer runtime inside the program: it runs in whatever environment it is given)
           "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "graphik_amd", "csrc"),
           os.path.join(REPO, "tests", "host", "anch_link_walk.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith("ok cells 400 pairs 26400 ") and "FAILED" not in r.stdout
    assert lines[1].split() == ["pinned", "pair", PINNED_PAIR, "interp", PINNED_INTERP]
    assert lines[2].split() == ["digest", PARENT_DIGEST]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
