"""The nine-slot lone wavefront's tCG loop with its cold block outside the hot loop (docs/NOTEBOOK.md 34): every way out
of the hot loop and back into it, from either of the two role-swapped steps, against the tail-spreading build of the
same kernel, whose loop is the old one (one step = test, cold block and updates in one piece).

64 LWA4D problems under ten parameter sets: the four of test_lone_wave_tail_gpu.py that are off the defaults, and
maxinner 1, 2, 3 with mininner 0 and 2, where the inner iterations run out in the first step (maxinner 1), in the second
(2) and in the first again after one full round (3), and where a step before mininner that meets the residual target
takes the cold block and comes back.  The spread build only runs when the batch is larger than the launch
(gik_plan.h: eight waves on each CU under GIK_WAVES_PER_CU=8), so the 64 problems are repeated to twice that; the same
batch through the default plan (one wave per SIMD) is the lone build.  Hand-overs prove the spread build (there is none
for theta != 1: that set runs the generic-theta lone build, which this loop does not touch, on both sides).

Asked of the CPU oracle first (oracle.c_oracle.rtr_solve with traj_cap 3000 on these 64 problems): (exit code, parity
of numit) -> solves, theta = 1 sets together: every one of the six codes ends solves after an even and
after an odd number of steps -- e.g. mininner4 (5, 0) 139, (5, 1) 152, (3, 0) 4278, (3, 1) 4042; mix (4, 1) 190841;
maxinner5 (4, 0) 191553; maxinner1 (4, 0) 191919; maxinner2 (4, 1) 191742; maxinner3 (4, 0) 191644; (0, 0) / (0, 1) 20-38
in each; (2, 0) 330, (2, 1) 214 in mininner4."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

FIELDS = ("x", "f", "gradnorm", "iterations", "inner_total", "n_accept", "stop")
SETS = {"mininner4": {"mininner": 4}, "mix": {"mininner": 3, "maxinner": 12, "kappa": 0.3},
        "maxinner5": {"maxinner": 5}, "theta2": {"theta": 2.0, "kappa": 0.5}}
for _mx in (1, 2, 3):
    for _mn in (0, 2):
        SETS["maxinner%d-mininner%d" % (_mx, _mn)] = {"maxinner": _mx, "mininner": _mn}
TRACE_CAP = 3000      # maxiter: whole trajectories
PROBLEMS = 64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def batch(B, params):
    """(template, start points, targets): the first 64 start points of tools/solve_digest.py's LWA4D batch, repeated."""
    import torch
    from graphik_amd.engine import Template
    d = load_golden("lwa4d")
    T = Template.from_matrices(d["omega"], d["psi_L"], d["psi_U"], k=int(d["dim"]), use_limits=bool(int(d["use_limits"])),
                               params=params)
    tg = T.targets_from_D(d["D_goal"])
    idx = np.arange(PROBLEMS) % len(d["Y_init"])
    Y0 = d["Y_init"][idx] + 1e-3 * np.random.RandomState(0).randn(PROBLEMS, *d["Y_init"].shape[1:])
    rep = np.arange(B) % PROBLEMS
    return T, Y0[rep], tg[torch.as_tensor(idx[rep], device=tg.device)]


def solved(torch, T, Y0, tg):
    """The per-problem outputs on the host; the two traces that are compared stay on the device (12 M entries each)."""
    r = T.solve(Y0, tg, trace_cap=TRACE_CAP)
    torch.cuda.synchronize()
    out = {k: r[k].cpu().numpy() for k in FIELDS + ("flags",)}
    valid = torch.arange(TRACE_CAP, device=r["iterations"].device)[None, :] < r["iterations"].clamp(max=TRACE_CAP)[:, None]
    return out, valid, r["trace"]["numit"], r["trace"]["stop"]


_runs = {}


def both_builds(torch, monkeypatch, name):
    """The batch through the lone build and through the spread build, once per parameter set: (outputs of the lone build,
    of the spread build, whether the traces' numit / stop agree wherever an iteration ran, the set of (tCG exit code,
    numit & 1) in the lone build's trace)."""
    if name not in _runs:
        T, _, _ = batch(1, SETS[name])
        B = 2 * 8 * T.info["n_cu"]
        assert T.info["hessian_form"] == 1 and T.info["problems_per_wave"] == 1
        assert B <= 6 * 4 * T.info["n_cu"]      # gik_plan.h: the default plan of this batch is one wave per SIMD
        T, Y0, tg = batch(B, SETS[name])
        lone, valid, numit, stop = solved(torch, T, Y0, tg)
        monkeypatch.setenv("GIK_WAVES_PER_CU", "8")      # (read once, at creation)
        Ts, _, _ = batch(1, SETS[name])
        monkeypatch.delenv("GIK_WAVES_PER_CU")
        spread, valid_s, numit_s, stop_s = solved(torch, Ts, Y0, tg)
        same = {"valid": bool(torch.equal(valid, valid_s)), "numit": bool(torch.equal(numit[valid], numit_s[valid])),
                "stop": bool(torch.equal(stop[valid], stop_s[valid]))}
        seen = torch.unique(stop[valid] * 2 + (numit[valid] & 1)).cpu().tolist()
        _runs[name] = (lone, spread, same, {(int(c) >> 1, int(c) & 1) for c in seen})
    return _runs[name]


@pytest.mark.parametrize("name", sorted(SETS))
def test_lone_loop_equals_the_one_piece_loop(torch_cuda, monkeypatch, name):
    lone, spread, same, seen = both_builds(torch_cuda, monkeypatch, name)
    assert not (lone["flags"] & 2).any()      # nothing paused: the plain kernel
    moved = (spread["flags"] & 2) != 0
    print(name, "moved", int(moved.sum()), "iterations", int(lone["iterations"].sum()), "exits", sorted(seen))
    if SETS[name].get("theta", 1.0) == 1.0:
        assert moved.any(), "no problem was handed over: the batch did not run on the tail-spreading build"
    assert int(lone["iterations"].min()) >= 1
    for k in FIELDS:
        assert lone[k].tobytes() == spread[k].tobytes(), k
    assert same == {"valid": True, "numit": True, "stop": True}, same      # the per-iteration trace
    # the repeats of a problem are the same problem
    for k in FIELDS:
        assert np.array_equal(lone[k][:PROBLEMS], lone[k][-PROBLEMS:]), k


def test_every_exit_from_both_steps(torch_cuda, monkeypatch):
    """All six tCG exit codes, each after an even and after an odd number of steps, in the traces compared above (the
    theta = 1 sets: the builds with the restructured loop) -- exit and re-entry ran from both roles."""
    seen = set()
    for name in sorted(SETS):
        if SETS[name].get("theta", 1.0) == 1.0:
            seen |= both_builds(torch_cuda, monkeypatch, name)[3]
    print(sorted(seen))
    assert seen >= {(code, parity) for code in range(6) for parity in (0, 1)}, sorted(seen)
    # the exhausted-inner exit in the first step, in the second, and in the first of the second round
    for name, parity in (("maxinner1-mininner0", 0), ("maxinner2-mininner0", 1), ("maxinner3-mininner0", 0),
                         ("maxinner1-mininner2", 0), ("maxinner2-mininner2", 1), ("maxinner3-mininner2", 0)):
        assert (4, parity) in both_builds(torch_cuda, monkeypatch, name)[3], name
