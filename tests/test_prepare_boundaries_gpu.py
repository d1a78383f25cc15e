"""The six prepare kernels at every size boundary of plan_prepare and of prep_block_kernel (tests/synth_prepare.py; proved
to sit there by tests/test_prepare_boundaries_host.py), each against the host restatement of the same operation --
BatchProblem.assemble, dgp.floyd_warshall_bounds, dgp.gram_from_distance_matrix, dgp.generate_initialization_batch --
never against another kernel.  Then recover_kernel and seed_kernel on the same graphs.  Every figure goes to the report
(parity_util.report; docs/NOTEBOOK.md 36) before it is asserted."""
import numpy as np
import pytest

import synth_prepare as sp
from parity_util import report, wrap_abs
from test_hip_gpu import _classify_init

pytestmark = pytest.mark.gpu

_PROBLEMS = {}      # (case id, GIK_PREP_WAVES_PER_CU) -> BatchProblem: a template per module, the big scenes cost seconds


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _problem(cid, monkeypatch, waves=None):
    """The case's BatchProblem, created under its environment switch (read once, at attach)."""
    if (cid, waves) not in _PROBLEMS:
        from graphik_amd.solvers.riemannian_solver import BatchProblem
        for k, v in sp.CASES[cid]["env"].items():
            monkeypatch.setenv(k, v)
        if waves is not None:
            monkeypatch.setenv("GIK_PREP_WAVES_PER_CU", str(waves))
        _PROBLEMS[(cid, waves)] = BatchProblem(sp.host_reference(cid)["graph"], use_limits=True)
    prob = _PROBLEMS[(cid, waves)]
    c, info = sp.CASES[cid], prob.template.info
    assert prob.device_pipeline
    assert info["prepare_is_block"] == c["is_block"] and info["goals_per_wave"] == c["goals_per_wave"], (cid, info)
    return prob


def _np(*tensors):
    return [t.cpu().numpy() for t in tensors]


@pytest.mark.parametrize("cid", sorted(sp.CASES))
def test_prepare_against_the_host(torch_cuda, monkeypatch, cid):
    """Eight goals of one case (the 40-joint chain with spheres: two).  Targets at 1e-12 max|targets|; lb and ub of
    prepare_debug against floyd_warshall_bounds at 1e-12 max(1, max ub) (a min-plus path sums up to N - 1 lengths, total
    near 100: reordering round-off is at most (N - 1) 2^-53 max ub = 1.4e-14 max ub); the Gram spectrum against eigvalsh
    of the host Gram at 1e-10 max|ev|;
    Gram(Y_init) against the host's at 1e-8 max(1, max|G_h|), K within [dim, N], everything finite.  3-D cases: every
    goal meets that bar (their K comes from 1e-8-sized noise columns, so the near-threshold census would excuse
    everything and is not consulted).  Planar chains: _classify_init with nothing unexplained, at most 1 of 8 goals not
    identical and only one the host itself marks near-threshold.
    Under prepare_debug a quad template runs prep_wave_kernel (PrepPlan::diagnostics): for the quad cases its output is
    held to the bounds only; targets, Y_init and K always come from prepare, the kernel the case names."""
    c, ref = sp.CASES[cid], sp.host_reference(cid)
    N, T = c["N"], _problem(cid, monkeypatch).template
    tg_d, Y_d, K_d = _np(*T.prepare(ref["Tg"], return_K=True))
    fig = {"variant": c["variant"], "path": c["path"], "N": N, "K_device": K_d.tolist(), "K_host": ref["info"]["K"].tolist()}
    fig["targets_rel"] = float(np.abs(tg_d - ref["targets"]).max() / np.abs(ref["targets"]).max())
    dbg = T.prepare_debug(ref["Tg"])
    lb_d, ub_d, eig_d = _np(dbg["lb"], dbg["ub"], dbg["eig"])
    ub_scale = max(1.0, float(ref["ub"][np.isfinite(ref["ub"])].max()))
    fig["lb_rel"] = float(np.abs(lb_d - ref["lb"]).max() / ub_scale)
    fig["ub_rel"] = float(np.abs(ub_d - ref["ub"]).max() / ub_scale)
    quad = c["variant"].startswith("quad")
    if not quad:
        ev_d = np.sort(eig_d[:, 0, :], axis=1)
        fig["gram_ev_rel"] = float(np.abs(ev_d - ref["ev_gram"]).max() / np.abs(ref["ev_gram"]).max())
        assert np.array_equal(_np(dbg["targets"])[0], tg_d)      # (the diagnostics launch is the same kernel)
    G_d, G_h = Y_d @ Y_d.transpose(0, 2, 1), ref["Y"] @ ref["Y"].transpose(0, 2, 1)
    scale = np.maximum(1.0, np.abs(G_h).reshape(len(G_h), -1).max(axis=1))
    fig["init_gram_rel"] = (np.abs(G_d - G_h).reshape(len(G_h), -1).max(axis=1) / scale).tolist()
    cls = _classify_init(Y_d, K_d, ref["Y"], ref["info"])
    same = cls.pop("mask_identical")
    fig["census"] = cls
    report(f"prepare_boundaries/{cid}", fig)

    assert fig["targets_rel"] <= 1e-12
    assert np.all(np.isfinite(lb_d)) and fig["lb_rel"] <= 1e-12 and fig["ub_rel"] <= 1e-12
    if not quad:
        assert fig["gram_ev_rel"] <= 1e-10
    assert np.all(np.isfinite(Y_d)) and np.all(K_d >= c["dim"]) and np.all(K_d <= N)
    if c["family"] != "planar":
        assert max(fig["init_gram_rel"]) <= 1e-8, fig["init_gram_rel"]
    else:
        assert cls["unexplained"] == 0, cls
        assert cls["identical"] >= 7 and np.all(same | sp.near_threshold(ref)), (cls, same)
        assert max(np.asarray(fig["init_gram_rel"])[same]) <= 1e-8


@pytest.mark.parametrize("variant", sp.VARIANTS)
def test_a_workgroup_that_takes_more_than_one_goal(torch_cuda, monkeypatch, variant):
    """One workgroup (wavefront) per CU -- GIK_PREP_WAVES_PER_CU = 1: the launch grid is n_cu -- and n_cu + 5 goals (the
    four-goal kernel: 4 n_cu + 5), the case's eight poses in turn: the goals that open and close the batch and the two
    around the point where the grid wraps come out bit for bit as the same pose prepared alone.  Whatever a workgroup
    carries from one goal to the next shows here: the block kernel's LOWER table, written once per launch and patched
    per goal; the LDS arrays; the slab."""
    cid = sp.MULTI_GOAL[variant]
    ref = sp.host_reference(cid)
    T = _problem(cid, monkeypatch, waves=1).template
    n_cu, per = T.info["n_cu"], max(1, sp.CASES[cid]["goals_per_wave"])
    B = per * n_cu + 5
    Tg = ref["Tg"][np.arange(B) % 8]
    tg, Y, K = _np(*T.prepare(Tg, return_K=True))
    assert np.all(np.isfinite(Y))
    differ = {}
    for g in sorted({0, n_cu - 1, n_cu, per * n_cu - 1, per * n_cu, B - 1}):
        tg1, Y1, K1 = _np(*T.prepare(Tg[g:g + 1], return_K=True))
        bad = [name for name, a, b in (("targets", tg[g], tg1[0]), ("Y_init", Y[g], Y1[0]), ("K", K[g], K1[0]))
               if not np.array_equal(a, b)]
        if bad:
            differ[g] = dict(what=bad, Y_abs=float(np.abs(Y[g] - Y1[0]).max()), K=[int(K[g]), int(K1[0])])
    report(f"prepare_boundaries/multi_goal/{variant}", {"case": cid, "B": B, "grid": n_cu, "differ": differ})
    assert not differ, differ


@pytest.mark.parametrize("rid", sorted(sp.REFUSED))
def test_refused_graphs(torch_cuda, rid):
    """Creation refuses the graph with the message the table pins, and the next template still prepares."""
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    r = sp.REFUSED[rid]
    robot, graph, Tg, _ = sp.build(r)
    with pytest.raises(RuntimeError) as e:
        BatchProblem(graph, use_limits=True)
    assert r["match"] in str(e.value), str(e.value)
    ref = sp.host_reference("planar_n17")
    tg = BatchProblem(ref["graph"], use_limits=True).template.prepare(ref["Tg"])[0].cpu().numpy()
    assert np.abs(tg - ref["targets"]).max() <= 1e-12 * np.abs(ref["targets"]).max()


def _angles_65(ref):
    """65 joint configurations (the second launch block of recover_kernel holds one goal) and their poses."""
    Q = ref["Q"][np.arange(65) % 8] * np.linspace(1.0, 0.5, 65)[:, None]
    return Q, ref["robot"].fk_batch(Q)


@pytest.mark.parametrize("cid", sp.RECOVER_SEED)
def test_recover_kernel_against_the_host(torch_cuda, monkeypatch, cid):
    """recover_kernel on the realizations of 65 configurations, exact and perturbed by 1e-3: joint angles against
    BatchProblem.joint_variables at 1e-9 modulo 2 pi, position errors against pose_errors at 1e-9, rotation errors at
    1e-7 (the bars of test_device_recover_matches_host and of the 216-node scene)."""
    ref = sp.host_reference(cid)
    prob = _problem(cid, monkeypatch)
    Q, Tg = _angles_65(ref)
    Y0 = prob.seed_points(Q)
    fig = {}
    for tag, Y in (("exact", Y0), ("perturbed", Y0 + 1e-3 * np.random.RandomState(1).randn(*Y0.shape))):
        q_d, pe_d, re_d = _np(*prob.template.recover(Y, Tg))
        q_h = np.asarray(prob.joint_variables(Y, Tg), dtype=float)
        pe_h, re_h = prob.pose_errors(q_h, Tg)
        fig[tag] = dict(q=float(wrap_abs(q_d - q_h).max()), pos=float(np.abs(pe_d - pe_h).max()), rot=float(np.abs(re_d - re_h).max()))
        if tag == "exact":
            fig[tag]["q_true"] = float(wrap_abs(q_d - Q).max())
    report(f"prepare_boundaries/recover/{cid}", fig)
    for tag in fig:
        assert fig[tag]["q"] < 1e-9 and fig[tag]["pos"] < 1e-9 and fig[tag]["rot"] < 1e-7, fig


@pytest.mark.parametrize("cid", sp.RECOVER_SEED)
def test_seed_kernel_against_the_host(torch_cuda, monkeypatch, cid):
    """seed_kernel: Y against BatchProblem.seed_points at 1e-12, targets bit-identical to prepare's (the bars of
    test_seed_matches_reference_and_prepare_targets)."""
    ref = sp.host_reference(cid)
    prob = _problem(cid, monkeypatch)
    Q, Tg = _angles_65(ref)
    tg, Y = prob.template.seed(Tg, Q)
    err = float(np.abs(Y.cpu().numpy() - prob.seed_points(Q)).max())
    report(f"prepare_boundaries/seed/{cid}", {"Y_abs": err})
    assert err < 1e-12
    assert torch_cuda.equal(tg, prob.template.prepare(Tg)[0])
