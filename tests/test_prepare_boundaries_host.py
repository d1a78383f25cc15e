"""The boundary cases of the device prepare (tests/synth_prepare.py) proved on the CPU: every case reaches the prepare
kernel it claims (plan_prepare through tests/host/prep_plan_cases.cpp, the LDS rule from the kernel's own __shared__
arrays), sits on the in-kernel path it claims (the host Gram rank against PREP_COMPRESS_MIN_N and PREP_RMAX), the host
reference stays within the census cap the GPU test uses, and a table that loses a case fails.  No GPU needed;
tests/test_prepare_boundaries_gpu.py runs the same rows on the device."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import synth_prepare as sp
from conftest import REPO

CSRC = os.path.join(REPO, "graphik_amd", "csrc")
PLAIN = sorted(cid for cid, c in sp.CASES.items() if not c["env"])      # (a switch changes the kernel, not the graph)


def _constants():
    """The integer constants of gik_args.h and gik_prep.hip.h, by name."""
    text = "".join(open(os.path.join(CSRC, f)).read() for f in ("gik_args.h", "gik_prep.hip.h"))
    known = {}
    for name, expr in re.findall(r"constexpr int (\w+) = ([^;]+);", text):
        try:
            known[name] = int(eval(expr.replace("/", "//"), {"__builtins__": {}}, dict(known)))
        except Exception:
            pass      # (an expression over something that is no plain integer constant)
    return known, text


def block_kernel_static_lds(maxn_name="PREP_MAXN"):
    """Bytes of the __shared__ arrays prep_block_kernel declares (the extern one is the dynamic segment), MAXN as given."""
    known, text = _constants()
    body = text[text.index("void __launch_bounds__(PREP_NT) prep_block_kernel("):]
    known = dict(known, MAXN=known[maxn_name])
    total, arrays = 0, 0
    for extern, ctype, decls in re.findall(r"(extern\s+)?__shared__\s+(?:__attribute__\(\(aligned\(16\)\)\)\s+)?(double|int)\s+([^;]+);", body):
        if extern:
            continue
        for _, dim in re.findall(r"(\w+)\[([^\]]+)\]", decls):
            total += (8 if ctype == "double" else 4) * int(eval(dim.replace("/", "//"), {"__builtins__": {}}, known))
            arrays += 1
    assert arrays == 9, arrays      # gd, cs, ev, sg, red, pq, rk, cinv, dl
    return total


def test_table_constants_are_the_kernels():
    known, _ = _constants()
    assert (known["PREPQ_MAXN"] if "PREPQ_MAXN" in known else known["QUAD_NODES"]) == sp.PREPQ_MAXN
    assert (known["PREP_COMPRESS_MIN_N"], known["PREP_RMAX"], known["PREP_MAXN"], known["PREP_BIGN"]) == (
        sp.PREP_COMPRESS_MIN_N, sp.PREP_RMAX, sp.PREP_MAXN, sp.PREP_BIGN)
    # the work matrix in LDS: 8 N^2 bytes next to the static arrays within 160 KB, up to N = 123
    static = block_kernel_static_lds()
    assert 40 * 1024 < static < 42 * 1024
    assert 8 * sp.LDS_MAXN ** 2 + static <= 160 * 1024 < 8 * (sp.LDS_MAXN + 1) ** 2 + static


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler (c++, g++, clang++) on this machine")
    exe = str(tmp_path_factory.mktemp("prep_plan_cases") / "prep_plan_cases")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + CSRC, os.path.join(REPO, "tests", "host", "prep_plan_cases.cpp"), "-o", exe],
                   check=True)
    args = [str(block_kernel_static_lds())]
    for cid, c in sp.CASES.items():
        args += [cid, str(c["N"]), str(c["dim"]), str(c["n_anchor"])] + [str(int(k in c["env"])) for k in sp.ENV_FACT]
    rows = json.loads(subprocess.run([exe] + args, check=True, capture_output=True, text=True, timeout=60).stdout)
    return {r["id"]: r for r in rows}


def test_every_case_reaches_its_variant(plans):
    assert set(plans) == set(sp.CASES)
    for cid, c in sp.CASES.items():
        p = plans[cid]
        assert p["variant"] == c["variant"], (cid, p)
        assert p["slab_matrices"] == {"block_lds": 5, "block": 5, "block_big": 6}.get(c["variant"], 0), (cid, p)
        if c["is_block"]:      # the work matrix in the dynamic LDS segment, or none at all
            assert p["lds"] == (8 * c["N"] ** 2 if c["variant"] == "block_lds" else 0), (cid, p)
        else:
            assert p["lds"] > 0, (cid, p)
        assert p["no_compress"] == int("GIK_PREP_NO_COMPRESS" in c["env"])
        assert p["grid_b8"] == (2 if c["variant"].startswith("quad") else 8)      # eight goals: a wavefront / workgroup each
    assert {p["variant"] for p in plans.values()} == set(sp.VARIANTS)      # every variant of enum class Prep
    with open(os.path.join(CSRC, "gik_plan.h")) as f:
        enum = re.search(r"enum class Prep \{([^}]*)\}", f.read()).group(1)
    assert [v.strip().lower() for v in enum.split(",")] == sp.VARIANTS


def test_the_table_is_complete_and_a_dropped_case_fails():
    assert sp.gaps() == []
    # ... and the check notices: a table without one case misses the boundary (variant, path, multi-goal case) it stood for
    for cid, missing in (("planar_n65", ["boundary N = 65", "path compressed r=64 at N = 65"]),
                         ("planar_n66", ["boundary N = 66", "path fallback at N = 66"]),
                         ("planar_n13", ["variant quad13", "multi-goal quad13"]),
                         ("ur10_n255", ["boundary N = 255", "multi-goal block_big"]),
                         ("planar_n47", ["boundary N = 47", "path plain at N = 47"])):
        assert sp.gaps({k: v for k, v in sp.CASES.items() if k != cid}) == missing, cid
    for N in sp.BOUNDARIES:      # every listed boundary is held by at least one row that would be missed
        pool = sp.REFUSED if N == 256 else sp.CASES
        assert [cid for cid, c in pool.items() if c["N"] == N], N
    assert set(sp.RECOVER_SEED) <= set(sp.CASES)
    # the sizes on both sides of every rule
    sizes = {c["N"] for c in sp.CASES.values()}
    assert {sp.PREPQ_MAXN, sp.PREPQ_MAXN + 1, sp.WAVE_MAXN, sp.WAVE_MAXN + 1, sp.PREP_COMPRESS_MIN_N - 1, sp.PREP_COMPRESS_MIN_N,
            sp.PREP_RMAX + 1, sp.PREP_RMAX + 2, sp.LDS_MAXN, sp.LDS_MAXN + 1, sp.PREP_MAXN, sp.PREP_MAXN + 1, 255} <= sizes
    # ... and of the 64 lanes that write the N K entries of prep_wave_kernel's Y_init
    wave3 = {3 * c["N"] for c in sp.CASES.values() if c["variant"] == "wave" and c["dim"] == 3}
    assert {63, 66, 96} <= wave3
    # the one graph beyond 128 nodes whose rank exceeds PREP_RMAX: the slow full decomposition of the 256-row build
    assert [cid for cid, c in sp.CASES.items() if c["variant"] == "block_big" and c["path"] == "fallback"] == ["chain40_n129"]


def test_synth_graphs_names_these_cases():
    """The coverage table of the compiled instantiations (tests/synth_graphs.py) points the prepare kernels at this table."""
    import synth_graphs as sg
    templated = {i for i in sg.compiled_instances() if i.startswith("prep_")}      # (prep_wave_kernel is no template)
    assert templated | {"prep_wave_kernel"} == set(sp.coverage()) and len(templated) == 5
    for inst in templated:
        assert sp.coverage()[inst]
        assert any(ref.startswith("tests/test_prepare_boundaries_gpu.py::") for ref in sg.EXISTING[inst]), inst


@pytest.mark.parametrize("cid", PLAIN)
def test_case_sits_on_its_path(cid):
    """The host Gram rank at 1e-13 |B|_F decides the path: planar chains N - 1 (so N = 65 is the compression at its cap,
    N = 66 the fallback), sphere scenes at most PREP_RMAX; the smallest counted eigenvalue at least 1e3 above the
    threshold, so no goal sits near range_basis_blk's stop.  Planar: the host's near-threshold goals number at most 1 of 8
    (the census cap of the GPU test).  Scenes: MDS column counts and anchors within what the kernels stage."""
    c = sp.CASES[cid]
    ref = sp.host_reference(cid)
    N = c["N"]
    assert ref["n_anchor"] == c["n_anchor"] <= 256 and ref["lb"].shape == (len(ref["Tg"]), N, N)
    rank, gap = sp.gram_rank(ref)
    K = ref["info"]["K"]
    assert np.all(K >= c["dim"]) and np.all(K <= N)
    if c["family"] == "chain40":
        # The fallback is taken as soon as range_basis_blk has found PREP_RMAX directions and a residual column is left:
        # what has to stand clear of its stop is the 65th largest eigenvalue (here by 4e9), not the smallest counted one
        # (rank 113 and 120 of 128: the small end of this spectrum is a continuum, 2e2 above the threshold).
        assert len(ref["Tg"]) == 2 and rank.min() > sp.PREP_RMAX and sp.leading_gap(ref, sp.PREP_RMAX + 1).min() >= 1e3, (rank, gap)
        assert K.max() <= sp.PREP_MAXN and not sp.near_threshold(ref).any()
    else:
        assert len(ref["Tg"]) == 8 and gap.min() >= 1e3, (cid, gap)
    if c["family"] == "planar":
        assert np.all(rank == N - 1), (cid, rank)
        assert int(sp.near_threshold(ref).sum()) <= 1, cid
    elif c["family"] == "ur10":
        assert np.all(rank <= sp.PREP_RMAX) and np.all(rank == min(N - 1, 23)), (cid, rank)
        assert K.max() <= sp.PREP_MAXN
    for same in (k for k, o in sp.CASES.items() if (o["family"], o["size"]) == (c["family"], c["size"])):
        path = sp.CASES[same]["path"]
        if path.startswith("compressed"):
            assert np.all(rank == int(path.split("=")[1])) and rank.max() <= sp.PREP_RMAX, (same, rank)
        elif path == "fallback":
            assert rank.min() > sp.PREP_RMAX, (same, rank)
    if cid == "planar_n65":
        assert c["path"] == "compressed r=64" and sp.CASES["planar_n65_prep_no_compress"]["path"] == "plain"
    if cid == "planar_n66":
        assert c["path"] == "fallback"


@pytest.mark.parametrize("rid", sorted(sp.REFUSED))
def test_refused_graph_has_the_size_it_claims(rid):
    r = sp.REFUSED[rid]
    robot, graph, Tg, _ = sp.build(r)
    assert graph.number_of_nodes() == r["N"] and graph.dim == r["dim"] and r["unreachable"]
