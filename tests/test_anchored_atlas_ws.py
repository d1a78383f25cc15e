"""The layout of the workspace of gik_anchored_ik_batch_atlas (graphik_amd/csrc/gik_plan.h: anch_atlas_ws) without a
device: tests/host/atlas_ws_table.cpp, a stand-alone program built with -fsanitize=address,undefined, prints the byte
offset of every array over a null base, and every one of them is compared with the closed form of the layout comment,
written out here -- arrays in the comment's order, each padded to 8 bytes; nothing is recorded from the code under test."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def pad8(x):
    return (x + 7) // 8 * 8


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx is not None, "a C++ compiler builds this project's host programs; it is needed here too"
    exe = str(tmp_path_factory.mktemp("atlas_ws") / "atlas_ws_table")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(REPO, "graphik_amd", "csrc"), os.path.join(REPO, "tests", "host", "atlas_ws_table.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr[-2000:]
    table = json.loads(run.stdout)
    return [dict(zip(table["fields"], r)) for r in table["rows"]]


def test_grid(rows):
    # 2 robots x 7 batch sizes x (C, retries) with (retries + 1) C <= 64 x scenes or none
    pairs = [(C, R) for C in (1, 2, 3, 4, 16) for R in (0, 1, 3, 63) if (R + 1) * C <= 64]
    assert len(pairs) == 16 and len(rows) == 2 * 7 * len(pairs) * 2
    assert {r["n"] for r in rows} == {6, 7} and {r["B"] for r in rows} == {0, 1, 2, 3, 5, 64, 4096}


def test_every_offset_against_the_closed_form(rows):
    for r in rows:
        B, C, R, n, pw, T, fN = r["B"], r["C"], r["retries"], r["n"], r["pose_w"], r["base_T"], r["full_N"]
        K, M = (R + 1) * C, B * C
        # the head is the existing restart workspace with the scene entry's ids: every array in front keeps its place
        scratch = B * (r["base_T"] + 3 * r["base_N"] + 3 * r["free_N"] + 3 * r["n_goal"])
        assert r["retry_bytes"] == 8 * scratch + 8 + pad8(4 * B) + 8 * B * (pw + 2 * n + 3 * fN) + 48 * B + 8 * B * (n + 3)
        assert r["retry_ids"] == r["retry_bytes"]
        need = r["retry_bytes"] + (pad8(4 * B) if r["scenes"] else 0)      # what the call without an atlas uses of it
        assert r["head"] == r["retry_bytes"] + pad8(4 * B) >= need and r["head"] % 8 == 0
        arrays = [("nbr", 4 * B * K), ("q0", 8 * B * n), ("rows", 4 * B * (R + 1)),
                  ("q", 8 * M * n), ("poses", 8 * M * pw), ("targets", 8 * M * T), ("Y", 8 * M * 3 * fN), ("clearance", 8 * M),
                  ("ids", 4 * M), ("pick", 4 * B)]
        off = r["head"]
        for name, nbytes in arrays:      # disjoint, in order, 8-byte aligned
            assert r[name] == off and off % 8 == 0, (name, r)
            if name == "q":
                assert r["screen_head"] == off
            off += pad8(nbytes)
        assert r["bytes"] == off
        # the screened entry's workspace of the same batch is this one without the three arrays in front
        assert r["bytes"] - r["screened_bytes"] == r["screen_head"] - r["head"] == pad8(4 * B * K) + 8 * B * n + pad8(4 * B * (R + 1))


def test_monotone_in_batch_and_candidates(rows):
    size = {(r["n"], r["retries"], r["B"], r["C"]): r["bytes"] for r in rows}
    for (n, R, B, C), v in size.items():
        for (n2, R2, B2, C2), v2 in size.items():
            if (n2, R2) == (n, R) and B2 >= B and C2 >= C:
                assert v2 >= v and (v2 > v or (B2, C2) == (B, C) or B2 == B == 0), ((n, R, B, C), (B2, C2))
    # and the layout does not depend on whether the call has scenes
    for a, b in zip(rows[0::2], rows[1::2]):
        assert a["scenes"] == 0 and b["scenes"] == 1
        assert {k: v for k, v in a.items() if k != "scenes"} == {k: v for k, v in b.items() if k != "scenes"}
