"""The launch plan of a batch call (graphik_amd/csrc/gik_plan.h: kernel, grid, waves per CU, slice, tail spreading,
queue capacities, workspace layout) against the table of the arithmetic gik_solve_batch carried before the plan was
split out of it (tests/golden/solve_plan.json, docs/NOTEBOOK.md 17): every field of every row, for equality.
tests/host/solve_plan_table.cpp lists the facts and the batch sizes: B = 1 and every threshold, one below, at, one above."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, REPO


def test_plan_table_equals_the_recorded_one(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler (c++, g++, clang++) on this machine")
    exe = str(tmp_path / "solve_plan_table")
    subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(REPO, "graphik_amd", "csrc"),
                    os.path.join(REPO, "tests", "host", "solve_plan_table.cpp"), "-o", exe], check=True)
    got = json.loads(subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout)
    with open(os.path.join(GOLDEN, "solve_plan.json")) as f:
        want = json.load(f)
    fields = want["fields"]
    assert got["fields"] == fields
    assert [c["case"] for c in got["cases"]] == [c["case"] for c in want["cases"]]
    rows = 0
    for g, w in zip(got["cases"], want["cases"]):
        assert [r[0] for r in g["rows"]] == [r[0] for r in w["rows"]], g["case"]
        for rg, rw in zip(g["rows"], w["rows"]):
            assert dict(zip(fields, rg)) == dict(zip(fields, rw)), f"{g['case']}, B = {rw[0]}"
            rows += 1
    # what the table has to reach: every launch, both bounds of the yield queue, a clique-target region
    col = {name: [r[i] for c in want["cases"] for r in c["rows"]] for i, name in enumerate(fields)}
    assert rows == len(col["B"]) >= 300
    assert set(col["launch"]) == {"quad", "npt", "block", "wave", "wave_spread"}
    assert set(col["wpc"]) >= {2, 4, 8, 12} and any(col["ctg_bytes"]) and any(b % 4 for b, k in zip(col["B"], col["launch"]) if k == "quad")
    tight = [y - 2 * g - 256 == 16 * b + 8192 for y, g, b in zip(col["ycap"], col["grid"], col["B"]) if y]
    assert any(tight) and not all(tight)
