"""Every compiled solve / known-answer kernel at its dispatch boundaries, against the oracle.

The cases, their graphs and the instantiation each one reaches are in tests/synth_graphs.py (the CPU test
tests/test_variant_coverage.py holds that table complete against gik_instances.h).  Per accepted case: the
kernel the library chose (Template.info), cost / egrad / ehess / cost_and_grad / proj on eight points with active
and inactive hinges, the first outer iterations decision for decision against co.rtr_solve / co.cg_solve, and the
end state.  Ragged batches against each problem solved alone; refused shapes name their limit."""
import numpy as np
import pytest

import synth_graphs as sg
from parity_util import assert_prefix_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_graphs = {}


def _graph(cid):
    if cid not in _graphs:
        c = sg.CASES[cid]
        _graphs[cid] = sg.build_graph(c["k"], c["N"], **c["graph"])
    return _graphs[cid]


def _template(k, om, pL, pU, params):
    from graphik_amd.engine import Template
    return Template.from_matrices(om, pL, pU, k=k, use_limits=True, device="cuda:0", params=dict(params))


def _check_info(T, want):
    got = {key: T.info[key] for key in want}
    assert got == want, (got, want)


def _hinge_state(Y, om, pL, pU):
    """(active hinges outside the psi_L == psi_U pairs, smallest relative distance of any hinge to its switch)."""
    d = ((Y[:, None] - Y[None]) ** 2).sum(-1)
    iu = np.triu_indices(len(Y), 1)
    lo = (pL[iu] > 0) & (pL[iu] != pU[iu])
    up = (pU[iu] > 0) & (pL[iu] != pU[iu])
    eqh = (pL[iu] > 0) & (pL[iu] == pU[iu]) & (om[iu] > 0)
    act = int((d[iu][lo] < pL[iu][lo]).sum() + (d[iu][up] > pU[iu][up]).sum())
    gaps = []
    for m, psi in ((lo | eqh, pL[iu]), (up | eqh, pU[iu])):
        gaps.append(np.abs(d[iu][m] - psi[m]) / psi[m])
    return act, float(np.concatenate(gaps).min())


def _kat_points(P, om, pL, pU, seed):
    """Eight points around P: close ones (no hinge active but the psi_L == psi_U pair's), far ones (many active);
    every hinge at least 1e-6 (relative) away from its switch."""
    rng = np.random.RandomState(seed)
    spread = np.abs(P).max()
    Ys, acts = [], []
    for s in (1e-5, 1e-4, 1e-3, 0.03, 0.15, 0.3, 0.6, 1.0):
        for _ in range(50):
            Y = P + s * spread * rng.randn(*P.shape)
            act, gap = _hinge_state(Y, om, pL, pU)
            if gap >= 1e-6:
                break
        assert gap >= 1e-6
        Ys.append(Y)
        acts.append(act)
    assert min(acts) == 0 and max(acts) > 0, acts
    return np.stack(Ys), rng.randn(len(Ys), *P.shape)


ACCEPTED = sorted(sg.CASES)


@pytest.mark.parametrize("cid", ACCEPTED)
def test_known_answers(torch_cuda, cid):
    from oracle import c_oracle as co
    c = sg.CASES[cid]
    om, pL, pU, D, P = _graph(cid)
    T = _template(c["k"], om, pL, pU, c["params"])
    _check_info(T, c["info"])
    n = sg.term_counts(om, pL, pU, c["graph"].get("clique", 0))
    assert T.T == n["T"]
    for key, want in c["counts"].items():
        assert n[key] == want, (key, n[key], want)
    inds = co.limit_inds(om, pL, pU)
    Ys, Ws = _kat_points(P, om, pL, pU, seed=len(cid))
    tg = T.targets_from_D(D)
    c_, g_ = T.cost(Ys, tg).cpu().numpy(), T.grad(Ys, tg).cpu().numpy()
    h_, p_ = T.hess(Ys, Ws, tg).cpu().numpy(), T.proj(Ys, Ws).cpu().numpy()
    cf, gf = T.cost_and_grad(Ys, tg)
    assert np.array_equal(cf.cpu().numpy(), c_) and np.array_equal(gf.cpu().numpy(), g_)
    # the floors of test_cost_grad_hess_proj_known_answers (unit-scale graphs of ~30 terms), times the round-off that
    # grows with the targets' size and the number of terms a sum runs over
    fs = max(1.0, float(np.abs(D).max())) * np.sqrt(max(1.0, T.T / 32.0))
    for m in range(len(Ys)):
        rc = co.lcost(Ys[m], D, om, pL, pU, inds)
        rg = co.lgrad(Ys[m], D, om, pL, pU, inds)
        rh = co.lhess(Ys[m], Ws[m], D, om, pL, pU, inds)
        rp = co.proj(Ys[m], Ws[m])
        assert abs(c_[m] - rc) <= 1e-12 * abs(rc) + fs * 1e-14 * np.sqrt(abs(rc)), (m, c_[m], rc)
        assert np.abs(g_[m] - rg).max() <= 1e-12 * np.abs(rg).max() + fs * 1e-13, m
        assert np.abs(h_[m] - rh).max() <= 1e-12 * np.abs(rh).max() + fs * 1e-13, m
        assert np.abs(p_[m] - rp).max() <= 1e-12 * np.abs(rp).max() + 1e-13, m


def _oracle_kw(params):
    return {key: params[key] for key in ("theta", "kappa", "maxiter") if key in params}


@pytest.mark.parametrize("cid", ACCEPTED)
def test_trajectory_and_end_state(torch_cuda, cid):
    from oracle import c_oracle as co
    c = sg.CASES[cid]
    om, pL, pU, D, P = _graph(cid)
    params = dict(c["params"])
    if "maxiter" in c:
        params["maxiter"] = c["maxiter"]
    T = _template(c["k"], om, pL, pU, params)
    cg = params.get("solver") == "ConjugateGradient"
    planar = c["k"] == 2
    scaled = c["graph"].get("scaled", False)
    rng = np.random.RandomState(17)
    B = 3
    Y0 = P[None] + 0.15 * np.abs(P).max() * rng.randn(B, *P.shape)
    cap = 16
    r = T.solve(Y0, T.targets_from_D(D)[0], trace_cap=cap)
    tr = {key: v.cpu().numpy() for key, v in r["trace"].items()}
    f, its, stop = r["f"].cpu().numpy(), r["iterations"].cpu().numpy(), r["stop"].cpu().numpy()
    kw = _oracle_kw(params)
    for b in range(B):
        if cg:
            o = co.cg_solve(Y0[b], D, om, pL, pU, True, traj_cap=cap, **kw)
            m = min(12, int(its[b]), o["iterations"])
            for key, okey in (("f_before", "f"), ("gradnorm_after", "gradnorm"), ("Delta", "stepsize")):
                assert np.allclose(tr[key][b][:m], o["traj"][okey][:m], rtol=1e-8, atol=0), (b, key)
            assert np.array_equal(tr["numit"][b][:m], o["traj"]["costevals"][:m]), b
            assert m == 12 or int(its[b]) == o["iterations"], (b, its[b], o["iterations"])
            assert (f[b] < 1e-9) == (o["f(x)"] < 1e-9), (b, f[b], o["f(x)"])
            continue
        o = co.rtr_solve(Y0[b], D, om, pL, pU, True, traj_cap=cap, **kw)
        t_b, o_b = {key: v[b] for key, v in tr.items()}, o["traj"]
        if planar:
            # the bar of test_trajectory_planar_identical_to_oracle: every decision while f >= 1e-14 (below it
            # a tCG call hinges on round-off), f to 1e-7, |grad| to 1e-6 -- over 8 outer iterations: these random
            # graphs are floppier than a chain (tCG calls of 100 - 270 inner iterations from the 6th on), and two of
            # them end such a call one inner iteration apart from the oracle at the 9th / 10th
            fo = o_b["f_before"]
            m = min(8, int(its[b]), o["iterations"], int(np.argmax(fo < 1e-14)) if np.any(fo < 1e-14) else len(fo))
            assert m == 8 or int(its[b]) == o["iterations"] or (m < len(fo) and fo[m] < 1e-14), (b, m, its[b])
            for key in ("numit", "stop", "accept", "Delta"):
                assert np.array_equal(t_b[key][:m], o_b[key][:m]), (b, key, t_b[key][:m], o_b[key][:m])
            assert np.allclose(t_b["f_before"][:m], fo[:m], rtol=1e-7, atol=0), b
            assert np.allclose(t_b["gradnorm_after"][:m - 1], o_b["gradnorm_after"][:m - 1], rtol=1e-6, atol=0), b
        else:
            # 3-D: four outer iterations strictly (decisions, f and |grad| to 1e-8); the fifth's decisions too, or the
            # one near-tie of the radius test that test_trajectory_prefix_3d accepts: both exits on the trust-region
            # boundary, one inner iteration apart, same acceptance
            m = min(5, int(its[b]), o["iterations"])
            assert m == 5 or int(its[b]) == o["iterations"], (b, its[b], o["iterations"])
            assert_prefix_equal(t_b, o_b, min(m, 4), rtol=1e-8)
            if m == 5 and not np.array_equal(t_b["numit"][:5], o_b["numit"][:5]):
                assert int(t_b["stop"][4]) in (0, 1) and int(o_b["stop"][4]) in (0, 1), b
                assert abs(int(t_b["numit"][4]) - int(o_b["numit"][4])) == 1, b
                assert int(t_b["accept"][4]) == int(o_b["accept"][4]), b
            else:
                for key in ("numit", "stop", "accept", "Delta"):
                    assert np.array_equal(t_b[key][:m], o_b[key][:m]), (b, key)
        if "maxiter" in c:
            continue
        if scaled:
            assert stop[b] == 0 and o["stop"] == 0 and f[b] > 1e-6, (b, stop[b], f[b])
            assert abs(f[b] - o["f(x)"]) <= 1e-6 * o["f(x)"], (b, f[b], o["f(x)"])
        else:
            assert stop[b] == 0 and f[b] < 1e-9, (b, stop[b], f[b], its[b])


def _solve_np(T, Y, tg):
    r = T.solve(Y, tg)
    keys = ("x", "f", "gradnorm", "iterations", "inner_total", "stop", "n_accept", "stepsize", "flags")
    return {key: r[key].cpu().numpy() for key in keys}


@pytest.mark.parametrize("bid", sorted(sg.BATCH_CASES))
def test_ragged_batch_equals_each_problem_alone(torch_cuda, monkeypatch, bid):
    bc = sg.BATCH_CASES[bid]
    c = sg.CASES[bc["graph"]]
    om, pL, pU, D, P = _graph(bc["graph"])
    params = dict(bc["params"], maxiter=60)
    if "mig" in bc:
        monkeypatch.setenv("GIK_SLICE_CYCLES", "0")      # (read at creation: hand-overs also in short runs)
        params.update(waves_per_cu=8, slice_outer_its=4)
    T = _template(c["k"], om, pL, pU, params)
    n_cu = T.info["n_cu"]
    if "mig" in bc:
        B = 8 * n_cu + 37
        alone = T
    else:
        assert T.info["problems_per_wave"] == 4
        B = 12 * n_cu + bc["quad"]
        # alone: the same kernel -- the four-problem kernel takes a single problem with debug_flags 16384
        alone = _template(c["k"], om, pL, pU, dict(params, debug_flags=16384)) if bc["quad"] > 0 else T
    rng = np.random.RandomState(3)
    Y0 = P[None] + 0.3 * np.abs(P).max() * rng.randn(B, *P.shape)
    tg = T.targets_from_D(D)
    rb = _solve_np(T, Y0, np.repeat(tg, B, axis=0))
    if "mig" in bc:
        moved = (rb["flags"] & 2) != 0
        assert moved.any() == bc["mig"], int(moved.sum())
    for g in sorted({0, 1, 2, 3, B // 2, B - 38, B - 2, B - 1}):
        r1 = _solve_np(alone, Y0[g:g + 1], tg)
        for key in r1:
            if key == "flags":
                continue
            assert np.array_equal(r1[key][0], rb[key][g]), (g, key)


@pytest.mark.parametrize("rid", sorted(sg.REFUSED))
def test_refused_shapes_name_their_limit(torch_cuda, rid):
    rf = sg.REFUSED[rid]
    om, pL, pU, _, _ = sg.build_graph(rf["k"], rf["N"], **rf["graph"])
    with pytest.raises(RuntimeError) as e:
        _template(rf["k"], om, pL, pU, rf["params"])
    assert rf["match"] in str(e.value), str(e.value)
    # the library still builds and solves the next template
    om, pL, pU, D, P = _graph("w3_n21_d9")
    T = _template(3, om, pL, pU, {})
    r = T.solve(P[None] + 1e-3 * np.random.RandomState(0).randn(1, *P.shape), T.targets_from_D(D))
    assert int(r["stop"][0]) == 0 and float(r["f"][0]) < 1e-9
