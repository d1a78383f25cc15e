"""Claim order of the wavefront solve kernels (SolveArgs::claim_order, gik_k_order.hip; docs/NOTEBOOK.md 21).

Part one: a batch solved with its claims ordered by the reach key against the same batch in index order.  Problems are
independent, so every output has to be equal bit for bit: x, every field of gik_stats, the trace arrays.  Batches of
one problem, fewer problems than waves, one more than the resident waves (waves_per_cu = 1: 256 CUs x 1), enough for a
second claim per wave at the default grid, the static block -> problem map (debug_flags 1), and KUKA through the
tail-spreading build (two waves per SIMD, more problems than waves).

Part two: the key and rank kernels on their own: a permutation, keys ascending, ties in index order, NaN last."""
import numpy as np
import pytest

from conftest import make_graph

pytestmark = pytest.mark.gpu

MAXITER = 40      # keeps a batch to milliseconds; the claim path does not depend on it


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_problems = {}


def _problem(robot, mode, extra):
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    key = (robot, mode, tuple(sorted(extra.items())))
    if key not in _problems:
        _, graph = make_graph(robot)
        _problems[key] = BatchProblem(graph, use_limits=True, device="cuda:0",
                                      params=dict(extra, maxiter=MAXITER, claim_order=mode))
    return _problems[key]


def _goals(robot_name, B, seed):
    robot, _ = make_graph(robot_name)
    lb, ub = robot.limits_arrays()
    return robot.fk_batch(lb + (ub - lb) * np.random.RandomState(seed).rand(B, robot.n))


# (robot, goals, template parameters, ordered claims expected, fields whose value depends on timing)
CASES = {
    "lwa4d-1": ("lwa4d", 1, {}, False, ()),
    "lwa4d-63": ("lwa4d", 63, {}, False, ()),
    "lwa4d-257": ("lwa4d", 257, {}, False, ()),
    "lwa4d-257-one-wave-per-cu": ("lwa4d", 257, {"waves_per_cu": 1}, True, ()),
    "lwa4d-300-static-map": ("lwa4d", 300, {"waves_per_cu": 1, "debug_flags": 1}, True, ()),
    "lwa4d-1100": ("lwa4d", 1100, {}, True, ()),
    "kuka-257-one-wave-per-cu": ("kuka", 257, {"waves_per_cu": 1}, True, ()),
    # the tail-spreading build: a problem may be paused and resumed by another wave, which include/graphik_amd.h
    # documents as timing-dependent in flags and inner_executed -- between two runs of the SAME order as well
    "kuka-2100-spread": ("kuka", 2100, {"waves_per_cu": 8}, True, ("flags", "inner_executed")),
}


@pytest.mark.parametrize("cid", sorted(CASES))
def test_ordered_claims_change_no_output(torch_cuda, cid):
    robot, B, extra, ordered, timing = CASES[cid]
    on, off = _problem(robot, "on", extra), _problem(robot, "off", extra)
    assert on.template.info["claim_key_terms"] == 1 and off.template.info["claim_key_terms"] == 0
    n_cu, wpc = on.template.info["n_cu"], extra.get("waves_per_cu", 4)
    assert (B > n_cu * wpc) == ordered, "the case no longer reaches the path it is named for"
    T_goal = _goals(robot, B, seed=7)
    out = []
    for prob in (on, off):
        targets, Y0 = prob.template.prepare(T_goal)
        r = prob.template.solve(Y0, targets, trace_cap=8)
        torch_cuda.cuda.synchronize()
        out.append((targets, r))
    (tg_a, a), (tg_b, b) = out
    assert np.array_equal(tg_a.cpu().numpy(), tg_b.cpu().numpy())
    for name in ("x", "f", "gradnorm", "stepsize", "iterations", "inner_total", "stop", "n_accept", "inner_executed", "flags"):
        if name in timing:
            continue
        assert a[name].cpu().numpy().tobytes() == b[name].cpu().numpy().tobytes(), name
    for name in a["trace"]:
        assert a["trace"][name].cpu().numpy().tobytes() == b["trace"][name].cpu().numpy().tobytes(), name
    assert int(a["iterations"].min()) >= 1


def test_default_is_the_robot_datas_key(torch_cuda):
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    for robot, want in (("lwa4d", 1), ("kuka", 0), ("ur10", 0)):
        _, graph = make_graph(robot)
        assert BatchProblem(graph, use_limits=True, device="cuda:0").template.info["claim_key_terms"] == want, robot


def test_keys_are_the_squared_reach(torch_cuda):
    prob = _problem("lwa4d", "on", {})
    T_goal = _goals("lwa4d", 130, seed=3)
    targets, _ = prob.template.prepare(T_goal)
    keys = prob.template.claim_keys(targets).cpu().numpy()
    t = prob.claim_key_terms()[0]
    assert np.array_equal(keys, targets.cpu().numpy()[:, t].astype(np.float32))
    reach2 = (T_goal[:, :3, 3] ** 2).sum(1)
    assert np.allclose(keys, reach2, rtol=1e-6)
    # several terms: weights that are powers of two, so every product is exact and the sum has one rounding order
    from graphik_amd.engine import Template
    tpl = prob.template
    T2 = Template(tpl.N, tpl.k, tpl.term_i, tpl.term_j, tpl.term_kind, tpl.targets_static, device="cuda:0")
    terms, w = [t, 0, tpl.T - 1], np.array([0.5, -2.0, 4.0])
    T2.set_claim_key(terms, w)
    assert T2.info["claim_key_terms"] == 3
    tg = targets.cpu().numpy()
    want = ((w[0] * tg[:, terms[0]] + w[1] * tg[:, terms[1]]) + w[2] * tg[:, terms[2]]).astype(np.float32)
    assert np.array_equal(T2.claim_keys(targets).cpu().numpy(), want)
    T2.set_claim_key([], [])
    assert T2.info["claim_key_terms"] == 0


def test_refused_keys(torch_cuda):
    from graphik_amd import _ffi
    from graphik_amd.engine import Template
    tpl = _problem("lwa4d", "on", {}).template
    T2 = Template(tpl.N, tpl.k, tpl.term_i, tpl.term_j, tpl.term_kind, tpl.targets_static, device="cuda:0")
    for terms in ([tpl.T], [-1], [0, 1, tpl.T + 5], list(range(9))):
        with pytest.raises(_ffi.GikError, match="claim key"):
            T2.set_claim_key(terms, np.ones(len(terms)))
        assert T2.info["claim_key_terms"] == 0
    T2.set_claim_key(list(range(8)), np.ones(8))
    assert T2.info["claim_key_terms"] == 8
    # templates on other kernels (planar; the workgroup path) take a valid key and stay on index order
    d = np.load(__import__("os").path.join(__import__("conftest").GOLDEN, "planar10_limits_halfpi.npz"))
    P = Template.from_matrices(d["omega"], d["psi_L"], d["psi_U"], k=2, use_limits=True, device="cuda:0")
    P.set_claim_key([0], [1.0])
    assert P.info["claim_key_terms"] == 0
    with pytest.raises(_ffi.GikError, match="claim key"):
        P.set_claim_key([P.T], [1.0])
    Bk = Template(tpl.N, tpl.k, tpl.term_i, tpl.term_j, tpl.term_kind, tpl.targets_static, device="cuda:0",
                  params={"force_block_path": 1})
    Bk.set_claim_key([0], [1.0])
    assert Bk.info["is_block"] and Bk.info["claim_key_terms"] == 0
    with pytest.raises(_ffi.GikError, match="claim order"):
        tpl.claim_order_of(np.zeros(tpl.lib.gik_claim_order_max_batch() + 1, dtype=np.float32))


def _key_sets(B, rng):
    sets = {"constant": np.full(B, 0.25, dtype=np.float32),
            "reversed": np.arange(B, 0, -1).astype(np.float32) - B / 2,
            "many ties": rng.randint(0, 7, size=B).astype(np.float32),
            "random": rng.randn(B).astype(np.float32)}
    special = rng.randn(B).astype(np.float32)
    pick = rng.rand(B)
    special[pick < 0.10] = np.nan
    special[(pick >= 0.10) & (pick < 0.15)] = np.inf
    special[(pick >= 0.15) & (pick < 0.20)] = -np.inf
    special[(pick >= 0.20) & (pick < 0.25)] = 0.0
    special[(pick >= 0.25) & (pick < 0.30)] = -0.0
    special[(pick >= 0.30) & (pick < 0.32)] = np.float32(1e-45)      # a denormal
    sets["nan, inf, signed zeros"] = special
    sets["all nan"] = np.full(B, np.nan, dtype=np.float32)
    return sets


def test_rank_kernel_sorts_stably_with_nan_last(torch_cuda):
    tpl = _problem("lwa4d", "on", {}).template
    largest = int(tpl.lib.gik_claim_order_max_batch())
    assert largest >= 8192
    rng = np.random.RandomState(11)
    for B in (0, 1, 64, 4097, largest):
        for name, keys in _key_sets(B, rng).items():
            order = tpl.claim_order_of(keys).cpu().numpy()
            assert order.shape == (B,)
            assert np.array_equal(np.sort(order), np.arange(B)), (B, name, "not a permutation")
            k = keys[order]
            nan = np.isnan(k)
            assert not nan[:B - int(nan.sum())].any(), (B, name, "NaN before a number")
            body = k[~nan]
            assert np.all(body[1:] >= body[:-1]), (B, name, "keys not ascending")
            # equal neighbours (the NaN run at the end counts as one tie) come in index order
            same = np.concatenate([body[1:] == body[:-1], np.zeros(min(1, len(body)) if nan.any() else 0, bool),
                                   np.ones(max(int(nan.sum()) - 1, 0), bool)])
            assert len(same) == max(B - 1, 0) and np.all(np.diff(order)[same] > 0), (B, name, "ties out of index order")
            # all of it at once: numpy's stable sort orders NaN last and equal keys (+0 == -0) by index
            assert np.array_equal(order, np.argsort(keys, kind="stable")), (B, name)
