"""Restarts from random joint seeds, host side (CPU only): the numpy mirror of the device generator
(retry_seeds_host) and solve_batch's argument checks, which come before any device call."""
import numpy as np
import pytest

from conftest import make_graph


def _mirror():
    from graphik_amd.solvers.riemannian_solver import retry_seeds_host, retry_uniform_host
    return retry_seeds_host, retry_uniform_host


def test_generator_is_deterministic_and_inside_the_limits():
    seeds, _ = _mirror()
    lo = np.array([-3.0, -1.5, 0.25, 2.0, -1e-3, 0.0, -170.0])
    hi = np.array([3.0, 1.5, 0.25, 2.0, 1e-3, 0.0, 170.0])       # lo == hi: degenerate joints
    goals = np.arange(5000)
    a = seeds(12345, goals, 3, lo, hi)
    b = seeds(12345, goals, 3, lo, hi)
    assert a.dtype == np.float64 and a.shape == (5000, 7)
    assert np.array_equal(a, b)
    assert np.all(a >= lo) and np.all(a <= hi)
    assert np.array_equal(a[:, 2], np.full(5000, 0.25)) and np.array_equal(a[:, 5], np.zeros(5000))
    # a goal's row depends on (seed, goal, attempt) alone: not on its position in `goals`, not on the others
    perm = np.random.RandomState(0).permutation(5000)
    assert np.array_equal(seeds(12345, goals[perm], 3, lo, hi), a[perm])
    assert np.array_equal(seeds(12345, [4711], 3, lo, hi)[0], a[4711])
    assert not np.array_equal(seeds(12346, goals, 3, lo, hi), a)


def test_distinct_goal_attempt_pairs_give_distinct_rows():
    seeds, _ = _mirror()
    lo, hi = -np.ones(6), np.ones(6)
    rows = np.concatenate([seeds(7, np.arange(300), a, lo, hi) for a in range(64)])       # 19200 (goal, attempt) pairs
    assert len({r.tobytes() for r in rows}) == len(rows)
    # ... and so are the numbers of one row
    assert all(len(set(r)) == 6 for r in rows[:100])
    # goals beyond 2^31 / 8192 keep distinct counters (the counter is 64 bits wide)
    big = seeds(7, [2 ** 31 - 1, 2 ** 31 - 2, 2 ** 18, 2 ** 18 + 1], 63, lo, hi)
    assert len({r.tobytes() for r in big}) == 4


def test_uniform_mean_and_range():
    _, uniform = _mirror()
    u = uniform(2024, np.arange(100000 // 8), 1, 8).reshape(-1)
    assert len(u) == 100000
    assert np.all(u >= 0.0) and np.all(u < 1.0)
    assert abs(u.mean() - 0.5) < 0.01
    assert np.all(u * 2.0 ** 53 == np.floor(u * 2.0 ** 53))      # 53-bit fractions


def test_pinned_vector():
    """(seed 1, goal 0, attempt 1, joint 0), by hand with unbounded integers: c = (0 * 64 + 1) * 128 + 0 + 1 = 129,
    z = 1 + 0x9E3779B97F4A7C15 * 129 mod 2^64 -> finaliser -> 0x3d285f4226bfd385, z >> 11 = 2151795397023738,
    u = 2151795397023738 * 2^-53, and on [-1, 2]: q = -1 + u * 3."""
    seeds, uniform = _mirror()
    M = 2 ** 64
    z = (1 + 0x9E3779B97F4A7C15 * 129) % M
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 % M
    z ^= z >> 27
    z = z * 0x94D049BB133111EB % M
    z ^= z >> 31
    assert z == 0x3D285F4226BFD385 and z >> 11 == 2151795397023738
    u = uniform(1, [0], 1, 1)[0, 0]
    assert u == float.fromhex("0x1.e942fa1135fe8p-3") == 2151795397023738 * 2.0 ** -53
    assert repr(float(u)) == "0.2388972794058184"
    q = seeds(1, [0], 1, [-1.0], [2.0])[0, 0]
    assert q == float.fromhex("-0x1.221b88e62f024p-2")


def test_generator_refuses_what_the_counter_cannot_hold():
    seeds, _ = _mirror()
    with pytest.raises(ValueError):
        seeds(0, [0], 64, np.zeros(3), np.ones(3))
    with pytest.raises(ValueError):
        seeds(0, [0], 1, np.zeros(126), np.ones(126))
    with pytest.raises(ValueError):
        seeds(0, [-1], 1, np.zeros(3), np.ones(3))


def _no_device(monkeypatch):
    """Any attempt to build a device problem fails the test: the checks below must come first."""
    from graphik_amd.solvers import riemannian_solver as rs

    def boom(*a, **k):
        raise AssertionError("solve_batch touched the device before checking its arguments")

    monkeypatch.setattr(rs, "_problem_for", boom)
    monkeypatch.setattr(rs, "BatchProblem", boom)
    return rs


def test_solve_batch_refuses_Y_init_with_retries(monkeypatch):
    rs = _no_device(monkeypatch)
    robot, graph = make_graph("lwa4d")
    T = robot.fk_batch(np.zeros((2, robot.n)))
    with pytest.raises(ValueError, match="Y_init"):
        rs.solve_batch(graph, T, Y_init=np.zeros((2, graph.number_of_nodes(), 3)), retries=1)


def test_solve_batch_refuses_64_retries(monkeypatch):
    rs = _no_device(monkeypatch)
    robot, graph = make_graph("lwa4d")
    T = robot.fk_batch(np.zeros((2, robot.n)))
    with pytest.raises(ValueError, match="retries"):
        rs.solve_batch(graph, T, retries=64)
    with pytest.raises(ValueError, match="retries"):
        rs.solve_batch(graph, T, retries=-1)
    with pytest.raises(ValueError, match="retries"):
        rs.solve_trajectory(graph, T[:, None], np.zeros(robot.n), retries=64)


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_solve_batch_refuses_non_finite_limits(monkeypatch, bad):
    rs = _no_device(monkeypatch)
    robot, graph = make_graph("lwa4d")
    T = robot.fk_batch(np.zeros((2, robot.n)))
    lb, ub = robot.limits_arrays()
    ub = ub.copy()
    ub[3] = bad
    monkeypatch.setattr(robot, "limits_arrays", lambda: (lb, ub))
    assert graph.robot is robot
    with pytest.raises(ValueError, match="non-finite"):
        rs.solve_batch(graph, T, retries=2)


def test_limits_must_be_ordered_and_tolerances_positive():
    from graphik_amd.engine import check_retry_args
    lo, hi = np.zeros(3), np.ones(3)
    assert check_retry_args(63, 0.01, 0.01, (lo, hi), 3)[0] == 63
    with pytest.raises(ValueError, match="exceeds"):
        check_retry_args(1, 0.01, 0.01, (hi, lo), 3)
    with pytest.raises(ValueError, match="positive"):
        check_retry_args(1, 0.0, 0.01, (lo, hi), 3)
    with pytest.raises(ValueError, match="shape"):
        check_retry_args(1, 0.01, 0.01, (lo, np.ones(4)), 3)
    with pytest.raises(ValueError, match="q_limits"):
        check_retry_args(1, 0.01, 0.01, None, 3)


def test_abi_carries_the_retry_entry_points():
    import re
    import os
    from conftest import REPO
    from graphik_amd import _ffi
    for name in ("gik_retry_select", "gik_retry_seeds", "gik_retry_merge", "gik_retry_ws_bytes", "gik_ik_batch_retry"):
        assert name in _ffi.SYMBOLS
    hdr = open(os.path.join(REPO, "include", "graphik_amd.h")).read()
    assert int(re.search(r"#define GIK_ABI_VERSION (\d+)", hdr).group(1)) == _ffi.ABI_VERSION
    # gik_retry_opts and its ctypes mirror: same fields, same order, same size
    body = re.search(r"typedef struct \{([^}]*)\} gik_retry_opts;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)).group(1)
    names = [n.strip().lstrip("*") for n in re.findall(r"\b(?:const\s+)?(?:double|int32_t|uint64_t)\s+([^;]+);", body)]
    assert names == [n for n, _ in _ffi.RetryOpts._fields_]
    import ctypes as C
    assert C.sizeof(_ffi.RetryOpts) == 48 and _ffi.RetryOpts.seed.offset == 8 and _ffi.RetryOpts.d_q_lo.offset == 32
