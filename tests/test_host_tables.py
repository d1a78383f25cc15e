"""The host tables of a template (graphik_amd/csrc/gik_tables.hip.h: slot lists and slot tables, the rigid clique, the
workgroup and node-per-lane tables, the FK recipe of the seed kernel, the link records of the fixed-anchor solve) built on
the CPU by tests/host/tables_walk.cpp -- a program of its own, host-only compile under the address and
undefined-behaviour sanitizers, nothing loaded into this interpreter.  The program asserts on every case what makes a
table safe to hand to a kernel; its output (lengths, 64-bit FNV-1a of the bytes, scalars, reasons of refusals) is compared
for equality with tests/golden/host_tables.json, recorded from the lines of gik_host.hip these functions were before they
moved (docs/NOTEBOOK.md 28).  No GPU."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import synth_graphs as sg
from conftest import GOLDEN, REPO, make_graph, planar_tree

EQ, LOWER, UPPER = sg.EQ, sg.LOWER, sg.UPPER
CLIQUE_AUTO, CLIQUE_OFF, CLIQUE_DENSE = 0, 1, 2      # (asserted against graphik_amd._ffi below)


# ---- the case files --------------------------------------------------------------------------------------------
def _ints(a):
    return " ".join(str(int(x)) for x in np.asarray(a).ravel())


def _hex(a):
    return " ".join(float(x).hex() for x in np.asarray(a, dtype=float).ravel())


def _wave_slots(k):
    """The compiled slot counts of the one-unknown-per-lane kernels of dimension k (gik_instances.h)."""
    found = {tuple(map(int, m.groups())) for s in sg.compiled_instances()
             for m in [re.match(r"rtr_wave_kernel<(\d),(\d+),", s)] if m}
    return sorted(D for K, D in found if K == k)


def _tables(name, N, k, terms, ccf=CLIQUE_AUTO, dbg=0):
    ti, tj, tk = terms[:3]
    big = N > 128
    two_waves = big or not dbg & 2048      # create_impl's layout arguments of npt_tables
    NW = 4 if big else (2 if two_waves else 1)
    slots = _wave_slots(k)
    return (f"tables {name} {N} {k} {len(ti)} {ccf} {dbg} {int(two_waves)} {NW} {256 if big else 128} "
            f"{len(slots)} {_ints(slots)}\n{_ints(ti)}\n{_ints(tj)}\n{_ints(tk)}\n")


def _synth_terms(k, N, graph):
    from graphik_amd.engine import build_terms
    om, pL, pU, _, _ = sg.build_graph(k, N, **graph)
    return build_terms(om, pL, pU, True)


def _packaged():
    """name -> (robot, graph, use_limits): the graphs the package ships, and the two obstacle scenes."""
    from graphik_amd.utils import table_environment
    from graphik_amd.utils.roboturdf import load_panda, load_schunk_lwa4p, load_ur10
    out = {n: (*make_graph(n), True) for n in ("ur10", "kuka", "lwa4d", "ur10_table")}
    out["panda"] = (*load_panda(), True)
    out["lwa4p"] = (*load_schunk_lwa4p(), True)
    out["planar10_limits"] = (*make_graph("planar10_limits_pi"), True)
    out["planar10_nolimits"] = (*make_graph("planar10_nolimits"), False)
    robot, graph = load_ur10()
    for idx, obs in enumerate(table_environment(n_width=12, n_height=14)):
        graph.add_spherical_obstacle(f"o{idx}", obs[0], obs[1])
    out["ur10_200_spheres"] = (robot, graph, True)
    return out


def _problems():
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    return {n: BatchProblem(g, use_limits=lim, host_only=True) for n, (_, g, lim) in _packaged().items()}


def _seed(name, bp, path=None, anchor_index=None):
    """The arguments of seed_recipe as BatchProblem._attach_device_pipeline hands them to gik_pipeline_attach."""
    g, robot, n = bp.graph, bp.robot, bp.robot.n
    K = bp.dim
    p_idx = [g.index(f"p{i}") for i in range(n + 1)]
    q_idx = [g.index(f"q{i}") for i in range(n + 1)] if K == 3 else p_idx
    n_ee = len(bp.end_effectors)
    if path is None:
        path = np.full((n_ee, n + 1), -1, dtype=np.int32)
        for e, ee in enumerate(bp.end_effectors):      # (a chain: 0 .. n, what end_effector_paths writes itself)
            joints = [int(j[1:]) for j in robot.kinematic_map["p0"][ee]]
            path[e, :len(joints)] = joints
    path = np.asarray(path).reshape(-1, n + 1)
    anchors = bp.anchor_nodes if anchor_index is None else anchor_index
    return (f"seed {name} {bp.N} {K} {n} {len(anchors)} {len(path)} {float(g.axis_length).hex()}\n{_hex(robot.T0_array())}\n"
            f"{_ints(p_idx)}\n{_ints(q_idx)}\n{_ints(anchors)}\n{_ints(path)}\n")


def _links(name, terms, free, anchors, la, lb, rho):
    ti, tj, tk = terms[:3]
    deg = int(np.bincount(np.concatenate([ti, tj]), minlength=len(free)).max())
    slots = min(s for s in (9, 20) if s >= deg)      # the fixed-anchor builds
    return (f"links {name} {len(free)} {len(ti)} {slots}\n{_ints(ti)}\n{_ints(tj)}\n{_ints(tk)}\n{_ints(free)}\n"
            f"{len(anchors)} {_ints(anchors)}\n{len(la)} {_ints(la)}\n{_ints(lb)}\n{_hex(rho)}\n")


def build_cases():
    """group -> the text of its case file."""
    from graphik_amd import _ffi
    assert (_ffi.CLIQUE_AUTO, _ffi.CLIQUE_OFF, _ffi.CLIQUE_DENSE) == (CLIQUE_AUTO, CLIQUE_OFF, CLIQUE_DENSE)
    probs = _problems()
    tables = []
    # every dispatch boundary of synth_graphs, accepted and refused
    for cid, c in sorted({**sg.CASES, **sg.REFUSED}.items()):
        tables.append(_tables(cid, c["N"], c["k"], _synth_terms(c["k"], c["N"], c["graph"]),
                              dbg=int(c["params"].get("debug_flags", 0))))
    for name, bp in probs.items():
        tables.append(_tables(name, bp.N, bp.dim, bp.terms))
    # the switches of clique_rows and the one-wavefront layout, on a graph with a clique and on one without; a clique of 8 is
    # kept only under debug_flags 64 (clique_min 4 instead of 16)
    variants = [("dbg64", CLIQUE_AUTO, 64), ("dbg128", CLIQUE_AUTO, 128), ("dbg2048", CLIQUE_AUTO, 2048),
                ("off", CLIQUE_OFF, 0), ("dense", CLIQUE_DENSE, 0)]
    for gname, (k, N, graph) in {"clq40": (3, 100, dict(clique=40, outside=64)), "noclq": (3, 22, dict()),
                                 "clq8": (3, 40, dict(clique=8))}.items():
        terms = _synth_terms(k, N, graph)
        for tag, ccf, dbg in [("plain", CLIQUE_AUTO, 0)] + variants:
            tables.append(_tables(f"{gname}_{tag}", N, k, terms, ccf, dbg))
    # refusals of slot_lists
    ti, tj, tk = (np.array(a) for a in ([0, 1, 2], [1, 2, 3], [EQ, LOWER, UPPER]))
    for tag, (i, j, kd) in {"bad_index_high": ([0, 1, 2], [1, 2, 4], tk), "bad_index_negative": ([0, -1, 2], tj, tk),
                            "bad_index_self": ([0, 2, 2], [1, 2, 3], tk), "bad_kind_0": (ti, tj, [EQ, 0, UPPER]),
                            "bad_kind_4": (ti, tj, [EQ, LOWER, 4]),
                            "bad_kind_before_bad_index": ([0, 1, 2], [1, 2, 9], [EQ, 7, UPPER])}.items():
        tables.append(_tables(tag, 4, 3, (i, j, kd)))

    # the FK recipe: every packaged chain, a planar tree, a 3-D tree with two end effectors, a joint with two parents, a
    # node that nothing places
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    from test_host_layer import tree_robot
    seeds = [_seed("seed_" + name, bp) for name, bp in probs.items()]
    tree2 = BatchProblem(planar_tree("y5")[1], host_only=True)
    tree3 = BatchProblem(tree_robot()[1], host_only=True)
    assert len(tree2.end_effectors) == 2 and len(tree3.end_effectors) == 2 and tree3.dim == 3 and tree2.dim == 2
    seeds += [_seed("planar_tree_y5", tree2), _seed("tree5", tree3)]
    n = tree3.robot.n
    two_parents = [[0, 1, 2, 4] + [-1] * (n - 3), [0, 1, 3, 4] + [-1] * (n - 3)]
    seeds.append(_seed("two_parents", tree3, path=two_parents))
    ur10 = probs["ur10"]
    x = ur10.graph.index("x")      # (no joint frame places the node "x": without its anchor nothing does)
    assert x in ur10.anchor_nodes
    seeds.append(_seed("unplaced_node", ur10, anchor_index=[a for a in ur10.anchor_nodes if a != x]))
    seeds.append(_seed("short_path", tree3, path=[[0, 1, 2] + [-1] * (n - 2), [0, 1, 3] + [-1] * (n - 2)]))

    # the link records: UR10 + table with the skeleton's links, constant ends, and the four refusals
    from test_anchored_link_hinges_host import hinge_problem
    ap = hinge_problem()[2]
    terms, free, anchors = ap.free_terms, list(ap.free), list(ap.anchors)
    la, lb, rho = ap.link_rows[:, 0], ap.link_rows[:, 1], 0.03 + 0.01 * np.arange(len(ap.link_rows))
    ti, tj, tk = (np.asarray(a) for a in terms[:3])
    Nf = len(free)
    tied = {(int(a), int(b)) for a, b in zip(ti, tj)} | {(int(b), int(a)) for a, b in zip(ti, tj)}
    apart = next((a, b) for a in range(Nf) for b in range(a + 1, Nf) if (a, b) not in tied)
    hub = next(a for a in range(Nf) if sum(1 for b in range(Nf) if (a, b) in tied) >= 3)
    spokes = [b for b in range(Nf) if (hub, b) in tied][:3]
    # node 0 made busier than the 9- and 10-slot builds hold: hinges it does not carry yet, until it has 11 terms
    have = {(int(a), int(b), int(kd)) for a, b, kd in zip(ti, tj, tk)}
    extra = [(b, kd) for b in range(1, Nf) for kd in (LOWER, UPPER) if (0, b, kd) not in have]
    extra = extra[:11 - int(np.bincount(np.concatenate([ti, tj]))[0])]
    busy = (np.concatenate([ti, np.zeros(len(extra), int)]), np.concatenate([tj, [b for b, _ in extra]]),
            np.concatenate([tk, [kd for _, kd in extra]]))
    assert np.bincount(np.concatenate(busy[:2])).max() == 11 and la[0] in anchors
    links = [
        _links("ur10_table_skeleton", terms, free, anchors, la, lb, rho),
        _links("two_anchor_rows", terms, free, anchors, [anchors[0]], [anchors[-1]], [0.05]),
        _links("one_constant_end", terms, free, anchors, [anchors[0], free[2]], [free[1], anchors[-1]], [0.0, 0.25]),
        _links("no_links", terms, free, anchors, [], [], []),
        _links("refused_20_slots", busy, free, anchors, la, lb, rho),
        _links("refused_unknown_row", terms, free, [a for a in anchors if a != la[0]], la, lb, rho),
        _links("refused_no_shared_term", terms, free, anchors, [free[apart[0]]], [free[apart[1]]], [0.0]),
        _links("refused_same_node", terms, free, anchors, [free[1]], [free[1]], [0.0]),
        _links("refused_three_at_a_node", terms, free, anchors, [free[hub]] * 3, [free[b] for b in spokes], [0.0] * 3),
    ]
    return {"tables": "".join(tables), "seed": "".join(seeds), "links": "".join(links)}


def walk(tmp, case_text, header_dir=None):
    """Compile tests/host/tables_walk.cpp and run it over the case files: (its JSON, its stderr, its stdout).  header_dir: where
    to look for gik_tables.hip.h first (docs/NOTEBOOK.md 28: how the golden file was recorded)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "the HIP toolchain builds this project; it is needed here too"
    exe = os.path.join(str(tmp), "tables_walk")
    cmd = [hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           "-static-libsan",      # (the sanitizer runtime inside the program: it runs in whatever environment it is given)
           "-I" + os.path.join(REPO, "include")] + (["-I" + header_dir] if header_dir else []) + \
          ["-I" + os.path.join(REPO, "graphik_amd", "csrc"), os.path.join(REPO, "tests", "host", "tables_walk.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    files = []
    for group, text in case_text.items():
        files.append(os.path.join(str(tmp), group + ".txt"))
        with open(files[-1], "w") as f:
            f.write(text)
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert r.returncode in (0, 1), (r.returncode, r.stderr[-3000:])      # (1: an invariant broke; the test below says which)
    return json.loads(r.stdout), r.stderr, r.stdout


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    return walk(tmp_path_factory.mktemp("host_tables"), build_cases())


def test_every_table_is_safe_to_hand_to_a_kernel(walked):
    """What tables_walk.cpp asserts on every case: packed rows, terms, slots and pair ids inside their tables, every kept
    term in exactly two slot lists and once as owner, loop bounds in order, the node-per-lane rows a bijection, gather
    entries the pad value or a term slot, a root-first FK order, link records that name a real term of their node."""
    out, err = walked[:2]
    assert out["broken"] == 0, err[-3000:]


def test_tables_equal_the_recorded_ones(walked):
    got = walked[0]["cases"]
    with open(os.path.join(GOLDEN, "host_tables.json")) as f:
        want = json.load(f)["cases"]
    assert [c["case"] for c in got] == [c["case"] for c in want]
    differ = [g["case"] for g, w in zip(got, want) if g != w]
    for g, w in zip(got, want):
        assert g == w, (g["case"], f"{len(differ)} of {len(want)} cases differ")


def test_case_list_reaches_every_branch(walked):
    with open(os.path.join(GOLDEN, "host_tables.json")) as f:
        cases = {c["case"]: c for c in json.load(f)["cases"]}
    by = lambda group: [c for c in cases.values() if c["group"] == group]      # noqa: E731
    tabs, seeds, links = by("tables"), by("seed"), by("links")
    assert len(tabs) >= len(sg.CASES) + len(sg.REFUSED) + 9 + 18 and len(seeds) >= 13 and len(links) >= 9
    # synth_graphs' refused graphs: no table (N = 256), or tables the node-per-lane kernel cannot take
    assert cases["r_n256"]["refused"] == "N"
    for rid in ("r_n200_out257", "r_n129_noclq", "r_force2_out257", "r_force2_per_node17", "r_force2_rows128"):
        assert cases[rid]["npt_ok"] == 0, rid
    assert {c["slot_lists"] for c in tabs if "slot_lists" in c} == {"", "bad term indices", "bad term kind"}
    assert cases["bad_kind_before_bad_index"]["slot_lists"] == "bad term kind"      # (the first bad term decides)
    # every compiled slot count of the wavefront kernels
    assert {key for c in tabs for key in c if re.fullmatch(r"wave\d+", key)} == {f"wave{s}" for k in (2, 3) for s in _wave_slots(k)}
    npt = [c for c in tabs if c.get("npt_ok")]
    fields = ("n_clq", "n_pairs", "DEG0", "DEG1", "n_wrows", "TL", "clq_euclid", "cbase", "n_rows", "n_terms", "term_sync", "n_helped")
    counts = [dict(zip(fields, c["npt_counts"]), NW=c["npt_NW"]) for c in npt]
    assert {c["NW"] for c in counts} == {1, 2, 4}                       # both layouts, and four wavefronts
    assert {c["TL"] for c in counts} == {1, 4}
    assert any(c["n_helped"] > 0 for c in counts) and any(c["n_helped"] == 0 for c in counts)
    assert {c["term_sync"] for c in counts} == {0, 1}
    assert any(c["DEG0"] + c["DEG1"] == 16 for c in counts) and any(c["n_wrows"] == 127 for c in counts)
    assert any(c["n_terms"] == 64 for c in counts) and any(c["n_terms"] == 65 for c in counts) and any(c["n_terms"] == 256 for c in counts)
    block = [c for c in tabs if "SL" in c]
    assert any(c["merged_waves"] > 0 for c in block) and any(c["split_waves"] > 0 for c in block)
    # a clique kept, and one refused by clique_min; the switches that turn it off
    assert cases["clq8_plain"]["n_clq"] == 0 and cases["clq8_dbg64"]["n_clq"] == 8
    assert cases["clq40_plain"]["n_clq"] == 40 and cases["clq40_dbg128"]["n_clq"] == 0 and cases["clq40_off"]["n_clq"] == 0
    assert cases["clq40_dense"]["n_clq"] == 40 and cases["noclq_dbg64"]["n_clq"] == 0
    assert cases["ur10_table"]["n_clq"] == 106 and cases["ur10_200_spheres"]["n_clq"] == 206 and cases["ur10_200_spheres"]["N"] == 216
    # seed recipe: accepted chains and trees of both dimensions, both refusals
    assert {(c["K"], c["seed_ok"]) for c in seeds} == {(2, 1), (3, 1), (3, 0)}
    assert cases["two_parents"]["seed_why"] == "joint 4 has two parents on the end-effector paths"
    assert cases["unplaced_node"]["seed_why"].endswith("is placed by neither a joint frame nor an anchor")
    assert cases["short_path"]["seed_why"].endswith("is placed by neither a joint frame nor an anchor")
    # link records: of the skeleton's 6 links 4 tie two free nodes (two records each), the first and the last end at a constant
    assert cases["ur10_table_skeleton"]["n_rec"] == 2 * 4 + 2 and cases["two_anchor_rows"]["n_rec"] == 0
    assert cases["one_constant_end"]["n_rec"] == 2 and cases["no_links"]["n_rec"] == 0
    why = {c["case"]: c["links_why"] for c in links}
    assert why["refused_20_slots"] == ("hinges = 1 needs the 9-slot fixed-anchor kernel; this template runs the 20-slot variant, "
                                       "which has no link hinges")
    assert re.fullmatch(r"hinges = 1: link 0 ends at row \d+, which is neither a free node nor an anchor row", why["refused_unknown_row"])
    assert why["refused_no_shared_term"] == why["refused_same_node"] == "hinges = 1: the two free ends of link 0 share no term"
    assert re.fullmatch(r"hinges = 1: more than 2 hinge links at free node \d+", why["refused_three_at_a_node"])
