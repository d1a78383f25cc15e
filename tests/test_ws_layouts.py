"""The layouts of the caller-owned workspaces of the two restart loops and the sweep (graphik_amd/csrc/gik_plan.h: RetryWs,
AnchSweepWs, AnchRetryWs) without a device: tests/host/ws_layout_table.cpp prints the byte offset of every array over a
null base, and every one of them is compared with the closed form of the layout comment, written out here -- arrays in
the comment's order, each padded to 8 bytes, pad8(x) = (x + 7) // 8 * 8; nothing is recorded from the code under test.
The program runs once more under AddressSanitizer and UBSan (docs/NOTEBOOK.md 30)."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import REPO

STATS = 48          # sizeof(gik_stats), include/graphik_amd.h


def pad8(x):
    return (x + 7) // 8 * 8


def _build_and_run(tmp, name, extra=()):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler (c++, g++, clang++) on this machine")
    exe = str(tmp / name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-I" + os.path.join(REPO, "graphik_amd", "csrc"), *extra,
                        os.path.join(REPO, "tests", "host", "ws_layout_table.cpp"), "-o", exe], capture_output=True, text=True)
    if r.returncode != 0 and extra:      # (the plain build of the same text has passed by then: the `table` fixture)
        pytest.skip("the sanitizers' runtime does not link here: " + r.stderr[-300:])
    assert r.returncode == 0, r.stderr[-3000:]
    return subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return json.loads(_build_and_run(tmp_path_factory.mktemp("ws_layouts"), "ws_layout_table"))


def _rows(table, name):
    fields = table[name + "_fields"]
    return [dict(zip(fields, r)) for r in table[name]]


def _check(r, arrays, total):
    """arrays: (field, bytes it holds) in layout order; every offset is the padded sum of what stands before it, a
    multiple of 8, and no array reaches into the next; the end of the last one is `total` bytes."""
    off = 0
    for k, (name, nbytes) in enumerate(arrays):
        assert r[name] == off, (name, r)
        assert r[name] % 8 == 0, (name, r)
        end = r[arrays[k + 1][0]] if k + 1 < len(arrays) else total
        assert r[name] + nbytes <= end, (name, r)
        off += pad8(nbytes)
    assert off == total, r


BATCHES = [0, 1, 2, 3, 5, 64]


def test_retry_ws(table):
    rows = _rows(table, "retry")
    assert sorted({r["B"] for r in rows}) == BATCHES and {2, 3} <= {r["K"] for r in rows} and len(rows) >= 18
    for r in rows:
        B, n, pw, T, NK = r["B"], r["n"], r["pose_w"], r["T"], r["N"] * r["K"]
        assert r["bytes"] == 8 + pad8(4 * B) + 8 * B * (pw + n + T + NK) + STATS * B + 8 * B * (n + 2), r
        _check(r, [("count", 8), ("idx", 4 * B), ("poses", 8 * B * pw), ("q_seed", 8 * B * n), ("targets", 8 * B * T),
                   ("Y", 8 * B * NK), ("stats", STATS * B), ("q", 8 * B * n), ("pos_err", 8 * B), ("rot_err", 8 * B)], r["bytes"])


def test_anchored_sweep_ws(table):
    rows = _rows(table, "sweep")
    assert sorted({r["B"] for r in rows}) == BATCHES and {r["S"] for r in rows} == {1, 4} and len(rows) >= 36
    for r in rows:
        M, n, pw, T, fN = r["B"] * (r["S"] + 1), r["n"], r["pose_w"], r["base_T"], r["full_N"]
        assert r["doubles"] == M * (n + pw + T + 3 * fN + 1), r
        _check(r, [("q", 8 * M * n), ("poses", 8 * M * pw), ("targets", 8 * M * T), ("Y", 8 * M * 3 * fN), ("clearance", 8 * M)],
               8 * r["doubles"])


def test_anchored_retry_ws(table):
    rows = _rows(table, "anch_retry")
    assert sorted({r["B"] for r in rows}) == BATCHES and len(rows) >= 18
    for r in rows:
        B, n, pw, fN = r["B"], r["n"], r["pose_w"], r["full_N"]
        scratch = B * (r["base_T"] + 3 * r["base_N"] + 3 * r["free_N"] + 3 * r["n_goal"])      # (AnchWs, in doubles)
        assert r["bytes"] == 8 * scratch + 8 + pad8(4 * B) + 8 * B * (pw + 2 * n + 3 * fN) + STATS * B + 8 * B * (n + 3), r
        _check(r, [("scratch", 8 * scratch), ("count", 8), ("idx", 4 * B), ("poses", 8 * B * pw), ("q_seed", 8 * B * n),
                   ("q_center", 8 * B * n), ("Y", 8 * B * 3 * fN), ("stats", STATS * B), ("q", 8 * B * n), ("pos_err", 8 * B),
                   ("rot_err", 8 * B), ("clearance", 8 * B)], r["bytes"])
        # the scene entry's ids: behind what gik_anchored_retry_ws_bytes reports, [B] int32 and 8-byte aligned
        assert r["ids"] == r["bytes"] and r["ids"] % 8 == 0, r


def test_the_table_program_is_clean_under_sanitizers(tmp_path, table):
    out = _build_and_run(tmp_path, "ws_layout_table_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    assert json.loads(out) == table
