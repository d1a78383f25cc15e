"""The solve loop of the hinge builds on the MI355X against the numpy trust-region twin (tests/anchored_twin.py): the six
cases of tests/test_anchored_hinge_twin_host.py -- one per rtr_wave_kernel build with link hinges, self hinges or
half-spaces -- decision for decision over the pinned prefix, the iterate at the end of it, and the batch of eight against
each problem alone.  Every condition on the inputs is a test of the host file; no seed is excused here.  The scene builds
add no solves: tests/synth_graphs.EXISTING names the tests that hold them bit-identical to their own templates."""
import numpy as np
import pytest

from parity_util import CONTRACT_RTOL, assert_prefix_equal, first_divergence, report
from test_anchored_hinge_twin_host import B, CASES, STABLE, pinned_recorded as pinned, seeds as case_seeds, problem, start, twin

pytestmark = pytest.mark.gpu

STATS = ("x", "f", "iterations", "inner_total", "stop")
X_RTOL = 1e-8       # the trajectory contract's bar, of max |x|


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _np(t):
    return t.detach().cpu().numpy()


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.int64) if x.dtype == np.float64 else x


def _device(case, maxiter=None):
    """The device problem of a case: the build, the slot count and the kernel family are the case table's."""
    robot, graph, ap = problem(case, host_only=False, maxiter=maxiter)
    info = ap.template.info
    assert info["anchored"] == CASES[case]["build"] and info["max_terms_per_node"] == 9 and not info["is_block"], info
    return ap


def _inputs(case):
    seeds = list(case_seeds(case))
    assert len(seeds) == B
    return seeds, np.array([start(case, g)[0] for g in seeds]), np.array([start(case, g)[1] for g in seeds])


@pytest.mark.parametrize("case", sorted(CASES))
def test_solve_against_the_numpy_twin(torch_cuda, case):
    """One solve of the batch of eight: per problem, decisions identical and f, |grad| to 1e-8 with the twin over
    min(4, n, stable_prefix) outer iterations -- which hold rejected steps, active sets that change and feet that move
    (the host file asserts it), so a kernel that reads a rejected trial point's state, drops a hinge share from the trial
    cost or carries a hinge gradient off by 1e-6 fails here (the host file's mutants)."""
    ap = _device(case)
    seeds, Y0, ga = _inputs(case)
    r = ap.template.solve(Y0, ga, trace_cap=32)
    tr = {k: _np(v) for k, v in r["trace"].items()}
    its = _np(r["iterations"])
    leaves, pins = [], []
    for b, g in enumerate(seeds):
        o = twin(case, g)
        hip = {k: tr[k][b] for k in tr}
        n = min(32, int(its[b]), o["iterations"])
        m = min(pinned(case, g), n)
        assert m >= 1
        pins.append(m)
        leaves.append(first_divergence(hip, o["traj"], n))
        print(f"{case} seed {g}: pinned {m}, device leaves the twin at {leaves[-1]} of {n}; accept {hip['accept'][:n].tolist()} "
              f"numit {hip['numit'][:n].tolist()} twin {o['traj']['numit'][:n].tolist()}")
    report(f"hinge_twin/first_divergence/{case}", {"seeds": seeds, "pinned": pins, "hip_leaves_twin_at": leaves,
                                                   "iterations_hip": its.tolist(),
                                                   "iterations_twin": [twin(case, g)["iterations"] for g in seeds],
                                                   "twin_reproduces_itself_for": list(STABLE[case])})
    for b, g in enumerate(seeds):
        assert_prefix_equal({k: tr[k][b] for k in tr}, twin(case, g)["traj"], pins[b], rtol=CONTRACT_RTOL)


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_iterate_at_the_end_of_the_pinned_prefix(torch_cuda, case):
    """params maxiter = m (the pinned length): the x the device returns is the twin's iterate after m outer iterations, to
    1e-8 of max |x| -- the accepted points themselves, not only their f and |grad|.  One template per distinct m."""
    seeds, Y0, ga = _inputs(case)
    m = np.array([pinned(case, g) for g in seeds])
    dist = np.full(B, np.nan)
    for mm in sorted(set(m.tolist())):
        sel = np.flatnonzero(m == mm)
        ap = _device(case, maxiter=mm)
        assert ap.template.params["maxiter"] == mm
        r = ap.template.solve(Y0[sel], ga[sel])
        x, its = _np(r["x"]), _np(r["iterations"])
        for row, b in enumerate(sel):
            o = twin(case, seeds[b])
            assert int(its[row]) == mm or (o["iterations"] < mm and int(its[row]) == o["iterations"]), (case, seeds[b], its[row], mm)
            want = o["traj"]["x"][int(its[row]) - 1]
            dist[b] = np.abs(x[row] - want).max() / np.abs(want).max()
    report(f"hinge_twin/x_at_end_of_prefix/{case}", {"seeds": seeds, "pinned": m.tolist(), "distance": dist.tolist(), "bar": X_RTOL})
    assert np.all(dist <= X_RTOL), (case, dist.tolist())


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_batch_equals_each_problem_alone(torch_cuda, case):
    """Eight launches of one problem: x, f, iterations, inner_total and stop equal the batch's bit for bit (the rule of
    test_ragged_batch_equals_each_problem_alone) -- no hinge state of one problem reaches another."""
    ap = _device(case)
    seeds, Y0, ga = _inputs(case)
    batch = ap.template.solve(Y0, ga)
    batch = {k: _np(batch[k]) for k in STATS}
    assert int(batch["iterations"].min()) >= 1
    for b in range(B):
        one = ap.template.solve(Y0[b:b + 1], ga[b:b + 1])
        for k in STATS:
            assert np.array_equal(_bits(_np(one[k])), _bits(batch[k][b:b + 1])), (case, seeds[b], k)
