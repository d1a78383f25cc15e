"""Restarts with a clearance rule in the fixed-anchor solve, host side (CPU only): the numpy mirror of local-mode
seeds, the failure / score / better rule on hand-made cells, the Python layer's argument checks, the header's
__host__ __device__ helpers walked by a stand-alone program under the address and undefined-behaviour sanitizers, and
the CPU twin's evidence for the bars of tests/test_anchored_retry_gpu.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from test_anchored_seeded_host import collision_input, host_problem, twin_solve

TWIN_SEED, TWIN_MAXITER = 77, 5          # the generator seed and budget of the GPU end-to-end test
TOL = dict(pos_tol=0.01, rot_tol=0.01, clear_tol=1e-4)


def _rs():
    from graphik_amd.solvers import riemannian_solver as rs
    return rs


# ---- 1. the mirror ---------------------------------------------------------------------------------------------
def test_uniform_mode_is_todays_output():
    """spread = 0 and no centre: the pinned vector of tests/test_retry_host.py, and the formula's bits on a batch."""
    rs = _rs()
    assert rs.retry_seeds_host(1, [0], 1, [-1.0], [2.0])[0, 0] == float.fromhex("-0x1.221b88e62f024p-2")
    assert rs.retry_seeds_host(1, [0], 1, [-1.0], [2.0], center=None, spread=0.0)[0, 0] == float.fromhex("-0x1.221b88e62f024p-2")
    lo, hi = np.array([-3.0, -1.5, 0.25, -170.0]), np.array([3.0, 1.5, 0.25, 170.0])
    goals = np.arange(500)
    u = rs.retry_uniform_host(9, goals, 2, 4)
    a = rs.retry_seeds_host(9, goals, 2, lo, hi)
    assert np.array_equal(a.view(np.int64), (lo[None] + u * (hi - lo)[None]).view(np.int64))
    # a centre without a spread is not read
    assert np.array_equal(rs.retry_seeds_host(9, goals, 2, lo, hi, center=np.full((500, 4), np.nan)), a)


def test_local_mode_stays_in_the_box_and_inside_the_limits():
    rs = _rs()
    rng = np.random.RandomState(3)
    lo, hi = np.array([-3.0, -1.5, 0.25, -2.0, -1e-3, -6.0]), np.array([3.0, 1.5, 0.25, 2.0, 1e-3, 6.0])
    goals = rng.permutation(5000)[:2000]
    c = rng.uniform(lo, hi, size=(2000, 6))
    u = rs.retry_uniform_host(5, goals, 7, 6)
    t = 2.0 * u - 1.0
    # 2u - 1 is exact: u = k 2^-53, so t 2^52 is the integer 2k' - 2^52 ... and back
    assert np.array_equal((t + 1.0) / 2.0, u) and np.all(t * 2.0 ** 52 == np.round(t * 2.0 ** 52))
    assert t.min() >= -1.0 and t.max() < 1.0
    for spread in (0.05, 0.3):
        q = rs.retry_seeds_host(5, goals, 7, lo, hi, center=c, spread=spread)
        assert q.shape == (2000, 6) and q.dtype == np.float64
        assert np.all(q >= lo) and np.all(q <= hi)
        inside = (q >= c - spread) & (q <= c + spread)
        assert np.all(inside | (q == lo) | (q == hi))
        assert np.array_equal(q, np.minimum(np.maximum(c + spread * t, lo), hi))
        # a goal's row depends on (seed, goal, attempt) and its own centre alone
        assert np.array_equal(rs.retry_seeds_host(5, goals[::-1], 7, lo, hi, center=c[::-1], spread=spread), q[::-1])
    # a centre at a limit clips to the limit: every draw with t < 0 at lo, every draw with t > 0 at hi
    q = rs.retry_seeds_host(5, goals, 7, lo, hi, center=np.broadcast_to(lo, (2000, 6)), spread=0.1)
    assert np.all(q[t < 0] == np.broadcast_to(lo, (2000, 6))[t < 0]) and np.all(q >= lo)
    q = rs.retry_seeds_host(5, goals, 7, lo, hi, center=np.broadcast_to(hi, (2000, 6)), spread=0.1)
    assert np.all(q[t > 0] == np.broadcast_to(hi, (2000, 6))[t > 0]) and np.all(q <= hi)
    # a spread wider than the limits clips every joint to one of them
    q = rs.retry_seeds_host(5, goals, 7, lo, hi, center=c, spread=1e12)
    assert np.all((q == lo) | (q == hi))
    # a NaN centre gives a NaN seed, for that joint alone
    c2 = c.copy()
    c2[7, 3] = np.nan
    q2 = rs.retry_seeds_host(5, goals, 7, lo, hi, center=c2, spread=0.3)
    assert np.isnan(q2[7, 3]) and np.isnan(q2).sum() == 1
    with pytest.raises(ValueError, match="centre"):
        rs.retry_seeds_host(5, goals, 7, lo, hi, spread=0.3)
    with pytest.raises(ValueError, match="shape"):
        rs.retry_seeds_host(5, goals, 7, lo, hi, center=c[:5], spread=0.3)
    with pytest.raises(ValueError, match="spread"):
        rs.retry_seeds_host(5, goals, 7, lo, hi, center=c, spread=-0.1)


PINNED_U = "0x1.e942fa1135fe8p-3"            # (seed 1, goal 0, attempt 1, joint 0): tests/test_retry_host.py
PINNED_LOCAL = "0x1.ca86b29b52331p-2"        # 0.5 + 0.1 (2u - 1) on [-1, 2]
PINNED_CLIPPED = "-0x1p+0"                   # -1 + 0.1 (2u - 1) < -1: the lower limit


def test_pinned_local_vector():
    """u = 0x1.e942fa1135fe8p-3 = 0.2388972794058184, t = 2u - 1 = -0.5222054411883632 (exact), 0.1 t rounded once,
    0.5 + that rounded once = 0.44777945588116368."""
    rs = _rs()
    u = float.fromhex(PINNED_U)
    t = 2.0 * u - 1.0
    assert t == float.fromhex("-0x1.0b5e82f76500cp-1")
    want = 0.5 + 0.1 * t
    assert want == float.fromhex(PINNED_LOCAL) and abs(want - 0.44777945588116368) < 1e-16
    assert rs.retry_seeds_host(1, [0], 1, [-1.0], [2.0], center=[[0.5]], spread=0.1)[0, 0] == want
    assert rs.retry_seeds_host(1, [0], 1, [-1.0], [2.0], center=[[-1.0]], spread=0.1)[0, 0] == float.fromhex(PINNED_CLIPPED)


# ---- 2. the rule -------------------------------------------------------------------------------------------------
def _cell(stop, pos, rot, clear):
    return (np.array([stop], dtype=np.int32), np.array([pos]), np.array([rot]), np.array([clear]))


def test_the_rule_on_hand_made_cells():
    rs = _rs()
    failed = lambda *c: bool(rs.anchored_retry_failed(*_cell(*c), **TOL)[0])                       # noqa: E731
    score = lambda p, r, c: float(rs.anchored_retry_score([p], [r], [c], **TOL)[0])               # noqa: E731
    better = lambda new, old: bool(rs.anchored_retry_better(_cell(*new), _cell(*old), **TOL)[0])  # noqa: E731
    ct = TOL["clear_tol"]
    assert not failed(0, 1e-3, 1e-3, -ct)
    assert failed(0, 1e-3, 1e-3, np.nextafter(-ct, -1.0))
    assert failed(0, 1e-3, 1e-3, np.nan)
    assert not failed(0, 1e-3, 1e-3, np.inf)
    assert failed(0, 1e-6, 1e-6, -0.036)                  # converged, on the goal, 36 mm inside a sphere
    assert not failed(0, 0.01, 0.01, 0.0) and failed(1, 0.0, 0.0, 1.0) and failed(0, np.nan, 0.0, 1.0)
    assert score(1e-3, 2e-3, np.inf) == 2e-3 / 0.01 and score(1e-3, 2e-3, 0.5) == 2e-3 / 0.01
    assert score(1e-3, 2e-3, -0.036) == 0.036 / ct and score(1e-3, 2e-3, np.nan) == np.inf
    assert score(np.nan, 2e-3, 0.5) == np.inf and score(0.0, 0.0, -np.inf) == np.inf
    # a success beats a failure, whatever the scores; never the other way
    assert better((0, 9e-3, 9e-3, 0.0), (0, 1e-6, 1e-6, -0.036))
    assert not better((0, 1e-6, 1e-6, -0.036), (0, 9e-3, 9e-3, 0.0))
    # between two failures the smaller score wins, and a tie keeps the incumbent
    assert better((1, 0.02, 0.0, 0.1), (1, 0.03, 0.0, 0.1)) and not better((1, 0.03, 0.0, 0.1), (1, 0.02, 0.0, 0.1))
    assert better((0, 0.0, 0.0, -0.01), (0, 0.0, 0.0, -0.036)) and not better((0, 0.0, 0.0, -0.036), (0, 0.0, 0.0, -0.01))
    assert not better((1, 0.02, 0.0, 0.1), (1, 0.02, 0.0, 0.1))
    assert not better((0, 1e-3, 1e-3, 0.1), (0, 1e-3, 1e-3, 0.2))      # two successes, same pose score: clearance above 0 is not ranked
    # a NaN never wins, on either field, even against the worst finite failure; and it loses to anything finite
    assert not better((0, 0.0, 0.0, np.nan), (2, 9.0, 9.0, -9.0)) and not better((0, np.nan, 0.0, 1.0), (2, 9.0, 9.0, -9.0))
    assert better((2, 9.0, 9.0, -9.0), (0, 0.0, 0.0, np.nan)) and not better((0, 0.0, 0.0, np.nan), (0, 0.0, 0.0, np.nan))


# ---- 3. argument checks --------------------------------------------------------------------------------------------
def test_python_layer_refuses_before_any_device_call():
    from graphik_amd.engine import check_retry_args
    lo, hi = np.zeros(3), np.ones(3)
    assert check_retry_args(2, 0.01, 0.01, (lo, hi), 3)[0] == 2                       # the defaults: today's call
    assert check_retry_args(2, 0.01, 0.01, (lo, hi), 3, clear_tol=1e-4, retry_spread=0.1)[0] == 2
    for bad in (0.0, -1e-4, np.nan):
        with pytest.raises(ValueError, match="clear_tol"):
            check_retry_args(1, 0.01, 0.01, (lo, hi), 3, clear_tol=bad)
    for bad in (-0.1, np.nan):
        with pytest.raises(ValueError, match="retry_spread"):
            check_retry_args(1, 0.01, 0.01, (lo, hi), 3, clear_tol=1e-4, retry_spread=bad)
    with pytest.raises(ValueError, match="q_init"):
        check_retry_args(1, 0.01, 0.01, (lo, hi), 3, clear_tol=1e-4, retry_spread=0.1, has_center=False)


class _NoDevice:
    """Stands in for the device templates: any use fails the test, the checks must come first."""
    n_joints = 6

    def __getattr__(self, name):
        raise AssertionError("the device was touched before the arguments were checked: " + name)


def test_anchored_problem_refuses_before_any_device_call():
    robot, graph, ap = host_problem()             # host_only: ap.template is None
    T = robot.fk_batch(np.zeros((2, robot.n)))
    q0 = np.zeros((2, robot.n))
    for kw, word in ((dict(retries=1, clear_tol=0.0), "clear_tol"), (dict(retries=1, retry_spread=-0.1), "retry_spread"),
                     (dict(retries=64), "retries"), (dict(retries=1, pos_tol=0.0), "positive")):
        with pytest.raises(ValueError, match=word):
            ap.solve(T, q_init=q0, **kw)
        with pytest.raises(ValueError, match=word):
            ap.solve_trajectory(T[:, None], q0, **kw)
    with pytest.raises(ValueError, match="q_init"):
        ap.solve(T, retries=1, retry_spread=0.1)
    from graphik_amd.engine import Template
    tpl = Template.__new__(Template)
    tpl.anchored = True
    base = _NoDevice()
    base.__dict__["has_pipeline"] = True
    lim = robot.limits_arrays()
    try:
        for kw, word in ((dict(retries=1, clear_tol=-1.0, q_limits=lim), "clear_tol"),
                         (dict(retries=1, retry_spread=-1.0, q_limits=lim), "retry_spread"),
                         (dict(retries=1, retry_spread=0.1, q_limits=lim), "q_init"), (dict(retries=1), "q_limits")):
            with pytest.raises(ValueError, match=word):
                Template.anchored_ik(tpl, base, T, **kw)
    finally:
        tpl.__dict__.clear()      # (nothing for __del__ to free)


def test_abi_carries_the_anchored_retry_entry_points():
    import ctypes as C
    import re
    from graphik_amd import _ffi
    for name in ("gik_anchored_retry_select", "gik_anchored_retry_seeds", "gik_anchored_retry_merge",
                 "gik_anchored_retry_ws_bytes", "gik_anchored_ik_batch_retry"):
        assert name in _ffi.SYMBOLS
    hdr = open(os.path.join(REPO, "include", "graphik_amd.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} gik_anchored_retry_opts;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    names = [n.strip().lstrip("*") for n in re.findall(r"\b(?:const\s+)?(?:double|int32_t|uint64_t)\s+([^;]+);", body)]
    assert names == [n for n, _ in _ffi.AnchoredRetryOpts._fields_]
    assert names[:7] == [n for n, _ in _ffi.RetryOpts._fields_]
    assert C.sizeof(_ffi.AnchoredRetryOpts) == 64 and _ffi.AnchoredRetryOpts.clear_tol.offset == 48
    assert _ffi.AnchoredRetryOpts.spread.offset == 56


# ---- 4. the header's helpers in a program of their own, under the sanitizers -----------------------------------
def test_header_helpers_walked_by_a_sanitized_host_program(tmp_path):
    """tests/host/anch_retry_walk.cpp: host-only compile of gik_retry.hip.h (no device code, nothing loaded into
    this interpreter), -fsanitize=address,undefined, run as a program.  It walks select / seed / merge over 389 random
    slots on exactly sized heap arrays and prints the pinned local-mode value, which must be the mirror's; then it holds
    the helpers at clearance = +inf to the plain rule on every (stop, pos_err, rot_err) cell, restart answer x incumbent:
    (5 * 6 * 6)^2 cells."""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "the HIP toolchain builds this project; it is needed here too"
    exe = str(tmp_path / "anch_retry_walk")
    cmd = [hipcc, "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off",
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           "-static-libsan",      # (the sanitizer runtime inside the program: it runs in whatever environment it is given)
           "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "graphik_amd", "csrc"),
           os.path.join(REPO, "tests", "host", "anch_retry_walk.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    sys.stdout.write(r.stdout)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-2000:])
    lines = r.stdout.strip().splitlines()
    assert lines[0].startswith("ok slots 389 ") and "FAILED" not in r.stdout
    assert lines[1].split() == ["pinned", "u", PINNED_U, "local", PINNED_LOCAL, "clipped", PINNED_CLIPPED]
    assert lines[2] == "plain cells %d" % (5 * 6 * 6) ** 2
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr


# ---- 5. CPU-twin evidence for the GPU bars -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def twin_attempts(seed=TWIN_SEED, maxiter=TWIN_MAXITER, retries=2):
    """The CPU twin of ap.solve(T, q_init=seeds, params={"maxiter": 5}, retries=2, retry_seed=77) on collision_input():
    attempt 0 from the colliding seeds, restart a from retry_seeds_host(seed, all goals, a, lo, hi) -- EVERY goal is
    solved at every attempt, so the counts do not depend on which goals the rule sends back.  Returns a list of
    (stop, pos_err, rot_err, clearance) per attempt."""
    rs = _rs()
    robot, graph, ap = host_problem()
    seeds, goals = collision_input()
    T = robot.fk_batch(goals)
    lo, hi = robot.limits_arrays()
    out = []
    for a in range(retries + 1):
        q0 = seeds if a == 0 else rs.retry_seeds_host(seed, np.arange(len(T)), a, lo, hi)
        res, Y, q = twin_solve(ap, T, q0, maxiter=maxiter)
        pos, rot = ap.base.pose_errors(q, T)
        out.append((np.array([r["stop"] for r in res], dtype=np.int32), np.asarray(pos), np.asarray(rot), ap.clearance(Y)))
    return out


def test_cpu_twin_has_room_for_the_gpu_bars():
    """What tests/test_anchored_retry_gpu.py asserts on the same input, budget and generator seed -- at least one goal
    fails attempt 0 and at least one is improved by a restart -- holds on the CPU twin with room to spare: every goal
    fails attempt 0 (five iterations from a seed inside a sphere) and a restart improves at least 8 of 64."""
    rs = _rs()
    att = twin_attempts()
    failed0 = rs.anchored_retry_failed(*att[0], **TOL)
    best, improved = att[0], np.zeros(64, dtype=bool)
    for a in (1, 2):
        take = failed0 & rs.anchored_retry_failed(*best, **TOL) & rs.anchored_retry_better(att[a], best, **TOL)
        best = tuple(np.where(take, n, o) for n, o in zip(att[a], best))
        improved |= take
    by_clearance = ~(att[0][0] != 0) & (att[0][1] <= 0.01) & (att[0][2] <= 0.01) & failed0
    print("twin, maxiter", TWIN_MAXITER, "seed", TWIN_SEED, ": failed attempt 0:", int(failed0.sum()), "of 64 (by clearance alone:",
          int(by_clearance.sum()), "); improved by restarts 1-2:", int(improved.sum()), "; successes after:",
          int((~rs.anchored_retry_failed(*best, **TOL)).sum()))
    assert failed0.sum() >= 8
    assert improved.sum() >= 8
    assert not np.any(rs.anchored_retry_better(att[0], best, **TOL))      # nothing got worse
