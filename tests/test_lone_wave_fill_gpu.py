"""The nine-slot lone wavefront's tCG step with the model test taken in the lanes of the distributed sums
(docs/NOTEBOOK.md 38): the state that now lives across the hot loop's back edge -- the two distributed sums wa / wb,
swapped with the other two-set values on the way out of the loop and back in, +inf before a solve's first step -- on
every way into the loop and out of it, against the tail-spreading build of the same kernel, whose loop is the one-piece
`step` with the model values in scalar registers.  (The sets were chosen for a second change as well, the recurrences
:596-597 deferred into the next step's reduction, which was measured slower and is not in the library; they stay: a
first-step exit, an exit in either role right after a cold re-entry, a re-summed beta and a resumed checkpoint are
where a stale or unswapped "previous" sum would show.)

The device of test_lone_wave_loop_gpu.py, whose helpers are imported: 64 LWA4D problems repeated to twice the launch of
the spread build, once through the default plan (one wave per SIMD: the lone build) and once under GIK_WAVES_PER_CU=8
(the spread build; a function of the batch size and the waves per CU alone, gik_plan.h -- hand-overs prove it wherever
the solves are long enough for a tail).  `x`, `f`, `gradnorm`, `iterations`, `inner_total`,
`n_accept`, `stop` and the per-iteration numit / stop trace byte for byte; `inner_executed` byte for byte on the problems
the spread build did not hand over (a handed-over problem loses its tCG checkpoint and may execute more products for the
same bits) and equal across the 64 repeats of a problem in the lone build.  Twelve parameter sets:

  maxinner 1 .. 5 x mininner 0, 2   a solve's first step leaves with +inf as the previous model value (maxinner 1),
                                    the second with one real sum behind it, and so on in either role; with mininner 2 a
                                    step that meets the residual target early takes the cold block and comes back
  resum      kappa 1e-14, maxiter 200   the residual target is out of reach, tCG runs until its Krylov space is exhausted
                                    and <r', r'> collapses: beta_p < 1e-3, the cold block re-sums <r', r'>, replaces beta
                                    and new_r_r, and the step is finished outside the loop before it is entered again
  checkpoints   defaults, maxiter 40   rejections and reruns from the checkpoint (ck_e_Pd2 / ck_d_Pd), the model exits
                                    of the default parameters

Asked of the CPU oracle first (oracle.c_oracle.rtr_solve, traj_cap 3000, these 64 problems; a copy that also counts the
steps whose beta (:592) is below 1e-3): (exit code, parity of numit) -> solves
  resum        (0,0) 31 (0,1) 29 (1,0) 2735 (1,1) 2735 (2,1) 1 (5,0) 2338 (5,1) 2294; 8086 steps with beta < 1e-3, numit to 259
  checkpoints  (0,0) 40 (0,1) 30 (1,0) 728 (1,1) 660 (2,0) 244 (2,1) 283 (3,0) 249 (3,1) 326; 16 steps with beta < 1e-3
  maxinner1    (4,0) 191919 / 191938 (mininner 0 / 2)     maxinner2  (4,1) 191742     maxinner3  (4,0) 191644
  maxinner4    (4,1) 191663                                maxinner5  (4,0) 191553, (3,0) 9-10, (3,1) 2-3
so every one of the six codes ends solves after an even and after an odd number of steps, and none of the 64 problems
converges under a maxinner of 1 .. 5 (192000 outer iterations in each set)."""
import numpy as np
import pytest

from test_lone_wave_loop_gpu import PROBLEMS, TRACE_CAP, batch

pytestmark = pytest.mark.gpu

FIELDS = ("x", "f", "gradnorm", "iterations", "inner_total", "inner_executed", "n_accept", "stop")
SETS = {"resum": {"kappa": 1e-14, "maxiter": 200}, "checkpoints": {"maxiter": 40}}
for _mx in (1, 2, 3, 4, 5):
    for _mn in (0, 2):
        SETS["maxinner%d-mininner%d" % (_mx, _mn)] = {"maxinner": _mx, "mininner": _mn}
# what the oracle's trajectories hold on these inputs (the docstring's table): the device traces must hold it too
ORACLE_EXITS = {"resum": {(0, 0), (0, 1), (1, 0), (1, 1), (5, 0), (5, 1)},
                "checkpoints": {(c, q) for c in range(4) for q in (0, 1)}}
for _mx in (1, 2, 3, 4, 5):
    for _mn in (0, 2):
        ORACLE_EXITS["maxinner%d-mininner%d" % (_mx, _mn)] = {(4, (_mx - 1) & 1)}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def solved(torch, T, Y0, tg):
    r = T.solve(Y0, tg, trace_cap=TRACE_CAP)
    torch.cuda.synchronize()
    out = {k: r[k].cpu().numpy() for k in FIELDS + ("flags",)}
    valid = torch.arange(TRACE_CAP, device=r["iterations"].device)[None, :] < r["iterations"].clamp(max=TRACE_CAP)[:, None]
    return out, valid, r["trace"]["numit"], r["trace"]["stop"]


_runs = {}


def both_builds(torch, monkeypatch, name):
    """(outputs of the lone build, of the spread build, whether the traces agree, the (exit code, numit & 1) pairs of the
    lone build's trace), once per parameter set."""
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
def test_lone_fill_equals_the_one_piece_loop(torch_cuda, monkeypatch, name):
    lone, spread, same, seen = both_builds(torch_cuda, monkeypatch, name)
    assert not (lone["flags"] & 2).any()      # nothing paused: the plain kernel
    moved = (spread["flags"] & 2) != 0
    print(name, "moved", int(moved.sum()), "iterations", int(lone["iterations"].sum()), "inner", int(lone["inner_total"].sum()),
          "executed", int(lone["inner_executed"].sum()), "exits", sorted(seen))
    if "maxiter" not in SETS[name]:      # (whole-length solves: there is a tail to spread)
        assert moved.any(), "no problem was handed over: the batch did not run on the tail-spreading build"
    assert int(lone["iterations"].min()) >= 1
    for k in FIELDS:
        if k != "inner_executed":
            assert lone[k].tobytes() == spread[k].tobytes(), k
    # A handed-over problem resumes without its tCG checkpoint (RtrResume): where it was paused behind a rejected step it
    # runs that tCG solve again instead of answering it from the checkpoint -- the same bits from more products.  So the
    # executed products are compared on the problems that stayed where they were, and may only be more on the others.
    more = spread["inner_executed"] != lone["inner_executed"]
    print(name, "inner_executed differs on", int(more.sum()), "problems,", int((more & ~moved).sum()), "of them not moved")
    assert not (more & ~moved).any()
    assert (spread["inner_executed"] >= lone["inner_executed"]).all()
    assert same == {"valid": True, "numit": True, "stop": True}, same      # the per-iteration trace
    # the repeats of a problem are the same problem
    for k in FIELDS:
        assert np.array_equal(lone[k][:PROBLEMS], lone[k][-PROBLEMS:]), k
    # the exits the oracle reaches on these inputs, in the role it reaches them in
    assert seen >= ORACLE_EXITS[name], (sorted(seen), sorted(ORACLE_EXITS[name]))
    if name == "checkpoints":      # reruns answered from the checkpoint: fewer products executed than counted
        assert int(lone["inner_executed"].sum()) < int(lone["inner_total"].sum())


def test_every_exit_from_both_steps(torch_cuda, monkeypatch):
    """All six tCG exit codes, each after an even and after an odd number of steps, in the traces compared above."""
    seen = set()
    for name in sorted(SETS):
        seen |= both_builds(torch_cuda, monkeypatch, name)[3]
    print(sorted(seen))
    assert seen >= {(code, parity) for code in range(6) for parity in (0, 1)}, sorted(seen)
