"""The prepare plan of a template (graphik_amd/csrc/gik_plan.h: which of the six prepare kernels, its LDS bytes, waves per
CU, slab, the grids, the occupancy queries it makes) and the layout of the anchored scratch, against the table of the
arithmetic gik_pipeline_attach, gik_prepare_batch_debug and the anchored calls carried before it was split out of them
(tests/golden/prep_plan.json, docs/NOTEBOOK.md 27): every field of every row, for equality.
tests/host/prep_plan_table.cpp lists the facts, the stand-in occupancy answers and the batch sizes."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, REPO


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler (c++, g++, clang++) on this machine")
    exe = str(tmp_path_factory.mktemp("prep_plan") / "prep_plan_table")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(REPO, "graphik_amd", "csrc"),
                    os.path.join(REPO, "tests", "host", "prep_plan_table.cpp"), "-o", exe], check=True)
    got = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout)
    with open(os.path.join(GOLDEN, "prep_plan.json")) as f:
        return got, json.load(f)


def test_prepare_plan_equals_the_recorded_one(tables):
    got, want = tables
    pf, rf = want["plan_fields"], want["row_fields"]
    assert got["plan_fields"] == pf and got["row_fields"] == rf
    assert [c["case"] for c in got["cases"]] == [c["case"] for c in want["cases"]]
    rows = 0
    for g, w in zip(got["cases"], want["cases"]):
        assert g["queries"] == w["queries"], g["case"]
        assert dict(zip(pf, g["plan"])) == dict(zip(pf, w["plan"])), g["case"]
        assert [r[0] for r in g["rows"]] == [r[0] for r in w["rows"]], g["case"]
        for rg, rw in zip(g["rows"], w["rows"]):
            assert dict(zip(rf, rg)) == dict(zip(rf, rw)), f"{g['case']}, B = {rw[0]}"
            rows += 1
    assert rows == sum(len(c["rows"]) for c in want["cases"]) >= 3000

    # what the table has to reach
    cases = want["cases"]
    plan = [dict(zip(pf, c["plan"])) for c in cases]
    asked = [[q[0] for q in c["queries"]] for c in cases]
    assert {p["variant"] for p in plan} == {"quad13", "quad", "wave", "block_lds", "block", "block_big"}
    # the LDS variant kept, and given up for the global slab after its query; the quad variant likewise for the wave kernel
    assert any(p["variant"] == "block_lds" for p in plan)
    assert any(p["variant"] == "block" and a == ["block_lds", "block"] for p, a in zip(plan, asked))
    assert any(p["variant"] == "block" and a == ["block"] for p, a in zip(plan, asked))      # (GIK_PREP_A_GLOBAL)
    assert any(p["variant"] == "wave" and a[-1] in ("quad", "quad13") for p, a in zip(plan, asked))
    # the 40 KB cap of the quad kernel's LDS: at it the kernel runs, one step above it is not even queried
    assert any(p["variant"] == "quad" and p["lds"] == 40 * 1024 for p in plan)
    assert any("N16 " in c["case"] and "gg9 " in c["case"] and a == ["wave"] for c, a in zip(cases, asked))
    # every clamp at both ends: workgroups per CU 1 .. 2 (an override: 1 and up), waves per CU 1 .. 32
    for kind, ends in (("block_lds", {1, 2}), ("block", {1, 2, 40}), ("block_big", {1, 2, 40}), ("wave", {1, 32}),
                       ("quad", {1, 32}), ("quad13", {1, 32})):
        assert ends <= {p["wpc"] for p in plan if p["variant"] == kind}, kind
    # the diagnostics of a quad template run on the wave kernel with its own parameters
    assert any(p["variant"] == "quad" and p["diag_variant"] == "wave" and p["diag_wpc"] != p["wpc"] for p in plan)
    assert all(p["diag_variant"] == p["variant"] for p in plan if not p["variant"].startswith("quad"))
    # grids: a batch below, at and above the resident grid; the quad kernel's with B no multiple of four
    for c, p in zip(cases, plan):
        grids = {r[1] for r in c["rows"]}
        assert max(grids) == int(c["case"].split(" cu")[1].split()[0]) * p["wpc"] and 1 in grids, c["case"]
    assert any(p["variant"] == "quad" and any(r[0] % 4 and r[1] == (r[0] + 3) // 4 for r in c["rows"]) for c, p in zip(cases, plan))


def test_anchored_scratch_layout_equals_the_recorded_one(tables):
    got, want = tables
    fields = want["anch_ws_fields"]
    assert got["anch_ws_fields"] == fields and len(got["anch_ws"]) == len(want["anch_ws"]) >= 20
    for g, w in zip(got["anch_ws"], want["anch_ws"]):
        assert dict(zip(fields, g)) == dict(zip(fields, w))
    # targets | Y_full0 | Y_free | goal, nothing between them, B = 0 and B = 1 among the rows
    for r in map(lambda w: dict(zip(fields, w)), want["anch_ws"]):
        B = r["B"]
        assert (r["targets"], r["Y_full0"], r["Y_free"], r["goal"], r["doubles"]) == (
            0, B * r["base_T"], B * (r["base_T"] + 3 * r["base_N"]), B * (r["base_T"] + 3 * r["base_N"] + 3 * r["free_N"]),
            B * (r["base_T"] + 3 * r["base_N"] + 3 * r["free_N"] + 3 * r["n_goal"]))
    assert {0, 1} <= {w[4] for w in want["anch_ws"]}
