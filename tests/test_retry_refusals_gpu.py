"""What the five plain restart exports refuse, and in which order, after they moved into the second host unit and the
driver's loop became the one it shares with the anchored entries (docs/NOTEBOOK.md 31): the return code and the full text
of gik_last_error() of every call of a table (cases) equal tests/golden/retry_refusals_parent.json, which
tools/record_refusals.py --table retry recorded on the MI355X from a checkout of the parent commit with this table.
LWA4D with its pipeline, B = 2, plus one bare template without a pipeline.

gik_retry_select, gik_retry_seeds, gik_retry_merge, gik_ik_batch_retry: each refusal the export has, and cases with two
faults at once, whose message says which one is tested first; every such case is refused on the host before anything is
queued.  gik_retry_ws_bytes returns 0 on a bad handle and sets no message: its cases record the value.  Two calls of the
driver must NOT be refused and record their 0: seeded with retries = 0 and a null workspace (it runs; its outputs are
buffers of its own), and retries = 1 with a null workspace at B = 0.  Left out, as in the anchored table:
  - a capturing stream (tests/test_retry_gpu.py begins a capture for it);
  - gik_retry_select with a null d_stats, d_pos_err or d_rot_err: refused after the memset of d_count;
  - a graph that cannot be seeded on the device (another robot)."""
import ctypes as C
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN, load_golden, make_graph
from test_anchored_refusals_gpu import SIZE, _entry, _p

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "retry_refusals_parent.json")
B = 2
RUNS = "(runs: returns 0)"


@functools.lru_cache(maxsize=None)
def env():
    """The handles and the device buffers every case draws from: the LWA4D template with its pipeline (tpl) and the same
    graph's template without one (bare)."""
    import torch
    from graphik_amd import _ffi
    from graphik_amd.engine import Template
    from graphik_amd.solvers.riemannian_solver import BatchProblem
    assert torch.cuda.is_available(), "these tests need the MI355X"
    robot, graph = make_graph("lwa4d")
    tpl = BatchProblem(graph).template
    d = load_golden("lwa4d")
    bare = Template.from_matrices(d["omega"], d["psi_L"], d["psi_U"], k=3, use_limits=True, device="cuda:0")
    assert tpl.info["has_pipeline"] and not bare.info["has_pipeline"]
    e = SimpleNamespace(torch=torch, ffi=_ffi, lib=_ffi.lib(), robot=robot, tpl=tpl, bare=bare)
    e.T = torch.from_numpy(np.ascontiguousarray(robot.fk_batch(np.zeros((B, robot.n))))).cuda().reshape(B, 16).contiguous()
    e.q0 = torch.zeros(B, robot.n, dtype=torch.float64, device="cuda")
    e.out, e.out_r, e.out_run = (tpl.alloc_ik_buffers(B) for _ in range(3))       # answers, the compact side of a merge, the call that runs
    for o in (e.out, e.out_r, e.out_run):
        o["attempt"] = torch.zeros(B, dtype=torch.int32, device="cuda")
        for v in o.values():
            v.view(torch.int32).fill_(-7)
    e.ws = torch.zeros(int(e.lib.gik_retry_ws_bytes(tpl._h, B)) // 8 + 1, dtype=torch.float64, device="cuda")
    e.idx, e.count = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    e.poses, e.q1 = torch.zeros(B, 16, dtype=torch.float64, device="cuda"), torch.zeros(B, robot.n, dtype=torch.float64, device="cuda")
    e.lo, e.hi = (torch.from_numpy(a).cuda() for a in robot.limits_arrays())
    e.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return e


def cases(e=None):
    """name -> (kind, callable): kind "call" returns the return code of a refused call, kind "size" the size itself, kind
    "runs" the return code of a call that is not refused."""
    e = e or env()
    lib, ffi, tpl, bare = e.lib, e.ffi, e.tpl._h, e.bare._h
    table = {}

    def add(export, make, what, kind="call", **over):
        name = f"{export}: {what}"
        assert name not in table, name
        table[name] = (kind, make(**over))

    def opts(retries=1, lo=True, hi=True, pos_tol=0.01, rot_tol=0.01):
        o = ffi.RetryOpts(retries=retries, seed=1, pos_tol=pos_tol, rot_tol=rot_tol, d_q_lo=_p(e.lo) if lo else None,
                          d_q_hi=_p(e.hi) if hi else None)
        return C.byref(o)

    def buffers(o, suffix=""):
        return {k + suffix: _p(o[k]) for k in ("Y", "stats", "q", "pos_err", "rot_err")}
    o = e.out
    answer = buffers(o)

    # ---- the three steps of a restart
    select = _entry(lib.gik_retry_select, stats=_p(o["stats"]), pos_err=_p(o["pos_err"]), rot_err=_p(o["rot_err"]), B=B, pos_tol=0.01,
                    rot_tol=0.01, idx=_p(e.idx), count=_p(e.count), stream=e.stream)
    for what, over in (("B -1", dict(B=-1)), ("null idx", dict(idx=None)), ("null count", dict(count=None)),
                       ("B -1 + null idx", dict(B=-1, idx=None)), ("B -1 + null count", dict(B=-1, count=None))):
        add("gik_retry_select", select, what, **over)
    seeds = _entry(lib.gik_retry_seeds, t=tpl, T=_p(e.T), idx=_p(e.idx), count=B, seed=1, attempt=1, q_lo=_p(e.lo), q_hi=_p(e.hi),
                   T_out=_p(e.poses), q_out=_p(e.q1), stream=e.stream)
    for what, over in (("null t", dict(t=None)), ("count -1", dict(count=-1)), ("no pipeline", dict(t=bare)),
                       ("attempt -1", dict(attempt=-1)), ("attempt 64", dict(attempt=64)), ("null q_lo", dict(q_lo=None)),
                       ("null q_hi", dict(q_hi=None)), ("null T", dict(T=None)), ("null idx", dict(idx=None)),
                       ("null T_out", dict(T_out=None)), ("null q_out", dict(q_out=None)),
                       ("count -1 + no pipeline", dict(count=-1, t=bare)), ("no pipeline + attempt 64", dict(t=bare, attempt=64)),
                       ("attempt 64 + null q_lo", dict(attempt=64, q_lo=None)), ("null q_hi + null T", dict(q_hi=None, T=None)),
                       ("null q_lo, count 0", dict(q_lo=None, count=0))):
        add("gik_retry_seeds", seeds, what, **over)
    compact = buffers(e.out_r, "_r")
    merge = _entry(lib.gik_retry_merge, t=tpl, idx=_p(e.idx), count=B, attempt=1, pos_tol=0.01, rot_tol=0.01, **compact, **answer,
                   attempt_of=_p(o["attempt"]), stream=e.stream)
    for what, over in (("null t", dict(t=None)), ("count -1", dict(count=-1)), ("no pipeline", dict(t=bare)),
                       ("count -1 + no pipeline", dict(count=-1, t=bare)), ("no pipeline + null idx", dict(t=bare, idx=None))):
        add("gik_retry_merge", merge, what, **over)
    for b in ("idx", *compact, *answer, "attempt_of"):
        add("gik_retry_merge", merge, "null " + b, **{b: None})

    # ---- the driver
    driver = _entry(lib.gik_ik_batch_retry, t=tpl, T=_p(e.T), q_init=None, B=B, opts=opts(), ws=_p(e.ws), targets=_p(o["targets"]),
                    **answer, attempt=_p(o["attempt"]), stream=e.stream)
    for what, over in (("null t", dict(t=None)), ("B -1", dict(B=-1)), ("null opts", dict(opts=None)), ("no pipeline", dict(t=bare)),
                       ("retries 64", dict(opts=opts(retries=64))), ("retries -1", dict(opts=opts(retries=-1))),
                       ("null q_lo", dict(opts=opts(lo=False))), ("null q_hi", dict(opts=opts(hi=False))),
                       ("pos_tol 0", dict(opts=opts(pos_tol=0.0))), ("rot_tol nan", dict(opts=opts(rot_tol=float("nan")))),
                       ("null ws", dict(ws=None)), ("ws off 8-byte alignment", dict(ws=_p(e.ws) + 4)),
                       ("B -1 + no pipeline", dict(B=-1, t=bare)), ("no pipeline + retries 64", dict(t=bare, opts=opts(retries=64))),
                       ("retries 64 + null q_lo", dict(opts=opts(retries=64, lo=False))),
                       ("null q_hi + pos_tol 0", dict(opts=opts(hi=False, pos_tol=0.0))),
                       ("rot_tol 0 + null ws", dict(opts=opts(rot_tol=0.0), ws=None)), ("null ws + null T", dict(ws=None, T=None)),
                       ("ws off 8-byte alignment + null Y", dict(ws=_p(e.ws) + 4, Y=None)),
                       ("no retries, null T", dict(opts=opts(retries=0), T=None)),
                       ("no retries, null q_lo and ws, null attempt", dict(opts=opts(retries=0, lo=False), ws=None, attempt=None)),
                       ("seeded, null targets", dict(q_init=_p(e.q0), targets=None))):
        add("gik_ik_batch_retry", driver, what, **over)
    for b in ("T", "targets", *answer, "attempt"):
        add("gik_ik_batch_retry", driver, "null " + b, **{b: None})
    r = e.out_run
    add("gik_ik_batch_retry", driver, "seeded, retries 0, null ws", kind="runs", q_init=_p(e.q0), opts=opts(retries=0), ws=None,
        targets=_p(r["targets"]), **buffers(r), attempt=_p(r["attempt"]))
    add("gik_ik_batch_retry", driver, "retries 1, null ws, B 0", kind="runs", ws=None, B=0)

    # ---- the size
    size = _entry(lib.gik_retry_ws_bytes, t=tpl, B=B)
    for what, over in (("null t", dict(t=None)), ("no pipeline", dict(t=bare)), ("B -1", dict(B=-1))):
        add("gik_retry_ws_bytes", size, what, kind="size", **over)
    return table


def run(table):
    """name -> {"rc", "message"} of every case, in the table's order"""
    lib = env().lib
    got = {}
    for name, (kind, call) in table.items():
        rc = int(call())
        got[name] = {"rc": rc, "message": {"size": SIZE, "runs": RUNS}.get(kind) or lib.gik_last_error().decode()}
    return got


def test_refusals_equal_the_parents():
    with open(GOLDEN_FILE) as f:
        want = json.load(f)["cases"]
    table = cases()
    assert sorted(want) == sorted(table)
    e = env()
    outputs = {**e.out, "ws": e.ws}
    before = {k: v.clone() for k, v in outputs.items()}
    got = run(table)
    for name, (kind, _) in table.items():
        # no case passes by not having been refused: every recorded call failed (a size, a call that runs: returned 0)
        assert want[name]["message"] and want[name]["rc"] == (-1 if kind == "call" else 0), name
        assert got[name] == want[name], (name, got[name], want[name])
    e.torch.cuda.synchronize()
    assert all(e.torch.equal(v.view(e.torch.int32), before[k].view(e.torch.int32)) for k, v in outputs.items())
    # the call that runs is the seeded call: its answer, and no goal restarted
    ref, r = e.tpl.ik(e.T, q_init=e.q0), e.out_run
    e.torch.cuda.synchronize()
    assert not r["attempt"].any() and e.torch.equal(r["q"], ref["q"])
