"""The fixed-anchor wavefront kernels at every compiled limit on the MI355X, template-level calls only (Template.cost /
grad / hess / cost_and_grad / solve on the synthetic problems of tests/synth_anchored.py, batches of 8): which kernel ran,
known answers against the plain numpy reference, the solve against its CPU twin, near lists against the full walk bit for
bit, and the refused shapes.  The 20-slot build (rtr_wave_kernel<3, 20, W_THETA1 | W_ANCH>, kat_wave_kernel<3, 20, W_ANCH>) runs in
the cases a10 and a20_full.  Every condition on the inputs is a test of tests/test_anchored_limits_host.py."""
import functools

import numpy as np
import pytest

import synth_anchored as sa
from parity_util import assert_prefix_equal, first_divergence, report
from test_anchored_limits_host import known_answer_bar, reference, stable_prefix, twin

pytestmark = pytest.mark.gpu

STATS = ("x", "f", "gradnorm", "iterations", "inner_total", "stop")
PREFIX = 3          # outer iterations pinned against the twin (5 on the UR10 scene, 4 on synthetic free-free graphs)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _template(cid, dbg=0):
    from graphik_amd.engine import Template
    p = sa.build(cid)
    return Template(p.N, 3, p.ti, p.tj, p.tk, None, params={"debug_flags": dbg} if dbg else None, anchored=sa.anchored_desc(p))


# ---- 1. which kernel ran -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sorted(sa.CASES))
def test_which_kernel_ran(torch_cuda, cid):
    info = _template(cid).info
    assert info["max_terms_per_node"] == sa.CASES[cid]["slots"], info
    assert info["anchored"] == 1 and not info["is_block"], info
    assert sa.CASES[cid]["reaches"] == [f"rtr_wave_kernel<3,{info['max_terms_per_node']},W_THETA1|W_ANCH>",
                                        f"kat_wave_kernel<3,{info['max_terms_per_node']},W_ANCH>"]


# ---- 2. known answers ----------------------------------------------------------------------------------------------
def _known_answers(T, cid):
    """cost, grad, hess of the case's known-answer points as arrays; cost_and_grad equals the separate calls bit for bit."""
    p = sa.build(cid)
    Y, W = sa.known_answer_points(cid)
    f, G, H = _np(T.cost(Y, p.goal.copy())), _np(T.grad(Y, p.goal.copy())), _np(T.hess(Y, W, p.goal.copy()))
    f2, G2 = T.cost_and_grad(Y, p.goal.copy())
    assert np.array_equal(_np(f2), f) and np.array_equal(_np(G2), G)
    assert np.array_equal(_np(T.proj(Y, W)), W)                 # Euclidean: proj is the identity
    return f, G, H


def _assert_known_answers(cid, f, G, H):
    p = sa.build(cid)
    Y, W = sa.known_answer_points(cid)
    bar = known_answer_bar(cid)
    worst = [0.0, 0.0, 0.0]
    for b in range(sa.B):
        fr, Gr, Hr = reference(p, b, Y[b], W[b])
        err = (abs(f[b] - fr) / abs(fr), np.abs(G[b] - Gr).max() / np.abs(Gr).max(), np.abs(H[b] - Hr).max() / np.abs(Hr).max())
        worst = [max(a, float(e)) for a, e in zip(worst, err)]
        print(f"{cid} problem {b}: f {fr:.6e}, errors {err[0]:.2e} {err[1]:.2e} {err[2]:.2e}")
    report(f"anchored_limits/known_answers/{cid}", {"f": worst[0], "egrad": worst[1], "ehess": worst[2], "bar": bar})
    assert max(worst) <= bar, (cid, worst, bar)


@pytest.mark.parametrize("cid", sorted(sa.CASES))
def test_known_answers(torch_cuda, cid):
    """cost / grad / hess / cost_and_grad of the known-answer kernel against the numpy reference at the project's 1e-12:
    relative to |f|, max |G|, max |H|."""
    _assert_known_answers(cid, *_known_answers(_template(cid), cid))


@pytest.mark.parametrize("cid", ["near8", "near9"])
def test_known_answers_twice_on_one_template(torch_cuda, cid):
    """The same evaluation twice in a row on the same template: the second meets whatever the first left behind, answers
    the same bits, and both meet the bar."""
    T = _template(cid)
    first = _known_answers(T, cid)
    second = _known_answers(T, cid)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    _assert_known_answers(cid, *second)


# ---- 3. the solve against its CPU twin -----------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sa.SOLVE_CASES)
def test_solve_against_twin(torch_cuda, cid):
    """Per problem: decisions identical and f, |grad| to 1e-8 with oracle.c_oracle.rtr_solve_anchored over the first
    min(3, n) outer iterations (a wrong slot, pin row, obstacle or goal row shows in the first) -- as far as the twin
    reproduces itself under another summation order (stable_prefix: at least 4 iterations in every case, so all three are
    pinned, but 2 in near8 / near9, whose third iteration from 0.01 away is not reproducible on the CPU either); the
    solve stops by its gradient rule with f < 1e-9, the reference agrees about the returned point, and every masked node
    is outside every sphere up to 1e-4."""
    p = sa.build(cid)
    r = _template(cid).solve(sa.start_points(cid), p.goal.copy(), trace_cap=32)
    tr = {k: _np(v) for k, v in r["trace"].items()}
    x, f, its, stop = _np(r["x"]), _np(r["f"]), _np(r["iterations"]), _np(r["stop"])
    leaves = []
    Z = np.zeros((p.N, 3))
    for b in range(sa.B):
        o = twin(cid, b)
        n = min(32, int(its[b]), o["iterations"])
        hip = {k: tr[k][b] for k in tr}
        assert n >= 1
        assert_prefix_equal(hip, o["traj"], min(PREFIX, n, stable_prefix(cid, b)))
        leaves.append(first_divergence(hip, o["traj"], n))
    report(f"anchored_limits/first_divergence/{cid}", {"hip_leaves_twin_at": leaves, "iterations_hip": its.tolist(),
                                                        "iterations_twin": [twin(cid, b)["iterations"] for b in range(sa.B)]})
    assert np.all(stop == 0) and np.all(f < 1e-9), (cid, stop.tolist(), f.tolist())
    for b in range(sa.B):
        assert reference(p, b, x[b], Z)[0] < 1e-9, (cid, b)
    if len(p.obs):
        assert sa.clearance(x[:, p.mask != 0], p.obs).min() > -1e-4


# ---- 4. near lists -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", sa.NEAR_LIST_CASES)
def test_near_lists_are_bit_identical(torch_cuda, cid):
    """debug_flags 128 (every walk visits every obstacle) against the default (near lists): eight near spheres, nine (the
    overflow), a node that travels into a sphere that was not on its list, and the 20-slot build -- x and the statistics
    bit for bit."""
    p = sa.build(cid)
    Y0 = sa.start_points(cid)
    out = []
    for dbg in (0, 128):
        r = _template(cid, dbg).solve(Y0, p.goal.copy())
        out.append({k: _np(r[k]) for k in STATS})
    for k in STATS:
        assert np.array_equal(out[0][k], out[1][k], equal_nan=True), (cid, k)
    assert int(out[0]["iterations"].min()) >= 1


# ---- 5. refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid", sorted(sa.REFUSED))
def test_refused_shapes(torch_cuda, rid):
    from graphik_amd import _ffi
    from graphik_amd.engine import Template
    (N, ti, tj, tk, desc), match = sa.refused(rid)
    with pytest.raises(_ffi.GikError, match=match):
        Template(N, 3, ti, tj, tk, None, anchored=desc)
