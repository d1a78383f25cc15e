"""The slot hand-out that makes concurrent batch calls on one handle safe (graphik_amd/csrc/gik_slots.h: counter ring
and workspace pool), run without a device by tests/host/slot_ring.cpp -- a stand-alone program, built plain and with
the thread sanitizer: more host threads than slots, so the in_use / yield branch runs, which no GPU test reaches."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def _build(tmp_path, name, extra):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no C++ compiler (c++, g++, clang++) on this machine")
    exe = str(tmp_path / name)
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread", "-I" + os.path.join(REPO, "graphik_amd", "csrc")] + extra +
                       [os.path.join(REPO, "tests", "host", "slot_ring.cpp"), "-o", exe], capture_output=True, text=True)
    return exe, r


def test_slot_protocol(tmp_path):
    exe, r = _build(tmp_path, "slot_ring", [])
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr[-3000:]
    assert " 0 failures" in run.stdout


def test_slot_protocol_under_the_thread_sanitizer(tmp_path):
    exe, r = _build(tmp_path, "slot_ring_tsan", ["-fsanitize=thread"])
    if r.returncode != 0:
        pytest.skip("the thread sanitizer's runtime does not link here: " + r.stderr[-300:])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and "ThreadSanitizer" not in run.stderr, run.stdout + run.stderr[-3000:]
    assert " 0 failures" in run.stdout
