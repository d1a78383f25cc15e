"""What the host entry points of the fixed-anchor solve refuse, and in which order, after they were folded onto one attempt
path and one clearance entry (docs/NOTEBOOK.md 30): the return code and the full text of gik_last_error() of every refused
call of a table (cases) equal tests/golden/anchored_refusals_parent.json, which tools/record_refusals.py recorded on the
MI355X from a checkout of the parent commit with this table.  UR10 + table, B = 2.

Every case is refused on the host before anything is queued.  Per export: each refusal it has, and cases with two faults at
once, whose message says which one is tested first.  The three sizes return 0 on a bad pair and set no message: their cases
record the value.  Left out, because they cannot be had without queuing work or without another robot:
  - a capturing stream (the existing tests of each feature begin a capture for it);
  - gik_anchored_retry_select with a null d_stats, d_pos_err, d_rot_err or d_clearance: refused after the memset of d_count;
  - a base graph that cannot be seeded on the device, is planar or has another node count than the template's full_N; link
    hinges that gik_anchored_attach_links cannot build.
The table was recorded again from a checkout of bcb1840 when the exports of the later features joined it -- the half-space and
the self clearance, the sweep with two outputs, the screened seed step and its batch entry, the atlas entries, with their
sizes -- ahead of the fold of the restart entries onto one driver (docs/NOTEBOOK.md 47): the 306 cases it had came out unchanged.
Their handles come from the problems the half-space and the self tests build.
Then the sizes of the three workspaces whose layouts gik_plan.h holds, against the closed forms of tests/test_ws_layouts.py,
and the Python layer's one helper for the restart workspace with a scene set."""
import ctypes as C
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN, make_graph
from test_anchored_halfspaces_gpu import _problem as _half_problem
from test_anchored_halfspaces_host import FLOOR
from test_anchored_links_gpu import _problem
from test_anchored_self_gpu import _problem as _self_problem
from test_ws_layouts import STATS, pad8

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "anchored_refusals_parent.json")
B = 2
ATLAS_ROWS = 16
SIZE = "(a size: 0 on a bad pair, no message)"


def _rs():
    from graphik_amd.solvers import riemannian_solver as rs
    return rs


@functools.lru_cache(maxsize=None)
def env():
    """The handles and the device buffers every case draws from: the UR10 + table template with its link skeleton (tpl),
    the same without links (bare), the robot graph with its pipeline (base: also the handle that is not anchored; tpl is
    the base without a pipeline)."""
    import torch
    from graphik_amd import _ffi
    assert torch.cuda.is_available(), "these tests need the MI355X"
    robot, _, ap = _problem()
    bare = _problem("none")[2].template
    tpl, base = ap.template, ap.base.template
    assert tpl.n_link is not None and bare.n_link is None
    f64 = dict(dtype=torch.float64, device="cuda")
    n = robot.n
    q = np.zeros((B, n))
    e = SimpleNamespace(torch=torch, ffi=_ffi, lib=_ffi.lib(), robot=robot, ap=ap, tpl=tpl, bare=bare, base=base)
    e.T = torch.from_numpy(np.ascontiguousarray(robot.fk_batch(q))).cuda().reshape(B, 16).contiguous()
    e.q0, e.q1 = torch.zeros(B, n, **f64), torch.zeros(B, n, **f64)
    e.out = tpl.alloc_anchored_buffers(base, B, clearance=True)
    e.out_r = tpl.alloc_anchored_buffers(base, B, clearance=True)            # the compact side of a merge
    e.Yf, e.goal = torch.zeros(B, tpl.N * 3, **f64), torch.zeros(B, tpl.n_goal_anchor * 3, **f64)
    e.rws = torch.zeros(int(e.lib.gik_anchored_retry_ws_bytes(tpl._h, base._h, B)) // 8 + B + 2, **f64)      # (ids and slack)
    e.sws = torch.zeros(int(e.lib.gik_anchored_sweep_ws_bytes(tpl._h, base._h, B, 4)) // 8 + 1, **f64)
    e.attempt = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.idx, e.count = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    e.poses = torch.zeros(B, 16, **f64)
    e.lo, e.hi = (torch.from_numpy(a).cuda() for a in robot.limits_arrays())
    e.S = ap.scene_set([ap.obstacles, ap.obstacles + np.array([0.2, 0.0, 0.0, 0.0])])
    e.ids = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    # the handles of the later features, from the problems their own tests build: self pairs on UR10 + table (selft, with
    # its robot graph sbase), a floor under the UR10 with links (half) and without (half_bare)
    sp = _self_problem()[2]
    e.selft, e.sbase = sp.template, sp.base.template
    e.half = _half_problem()[2].template
    e.half_bare = _rs().AnchoredProblem(make_graph("ur10")[1], links=[], halfspaces=[FLOOR]).template
    assert getattr(e.selft, "n_self", None) is not None and getattr(tpl, "n_self", None) is None
    assert e.half.n_half == 1 and e.half.n_link is not None and e.half_bare.n_half == 1 and e.half_bare.n_link is None
    e._problems = (sp,)
    # the screened step's workspace, the larger of the two batch workspaces (4 candidates; one restart), a 16-row atlas
    e.scw = torch.zeros(int(e.lib.gik_anchored_retry_seeds_screened_ws_bytes(tpl._h, base._h, B, 4)) // 8 + 1, **f64)
    e.aws = torch.zeros(max(int(e.lib.gik_anchored_ik_batch_atlas_ws_bytes(tpl._h, base._h, B, 4, 1)),
                            int(e.lib.gik_anchored_ik_batch_retry_screened_ws_bytes(tpl._h, base._h, B, 4))) // 8 + 1, **f64)
    e.keys, e.aq = torch.zeros(6, ATLAS_ROWS, **f64), torch.zeros(ATLAS_ROWS, n, **f64)
    e.nbr, e.dist = torch.zeros(B, 8, dtype=torch.int32, device="cuda"), torch.zeros(B, 8, **f64)
    e.pick, e.pick_cl = torch.zeros(B, dtype=torch.int32, device="cuda"), torch.zeros(B, **f64)
    e.self_out = torch.zeros(B, **f64)
    return e


def _p(t):
    return t.data_ptr()


def _entry(fn, **defaults):
    """make(**overrides) -> a callable that calls fn with the defaults, some of them replaced, in the defaults' order"""
    def make(**over):
        assert set(over) <= set(defaults), set(over) - set(defaults)
        args = list({**defaults, **over}.values())
        return lambda: fn(*args)
    return make


def cases(e=None):
    """name -> (kind, callable): kind "call" returns the return code of a refused call, kind "size" the size itself."""
    e = e or env()
    lib, ffi, tpl, bare, base = e.lib, e.ffi, e.tpl._h, e.bare._h, e.base._h
    table = {}

    def add(export, make, what, kind="call", **over):
        name = f"{export}: {what}"
        assert name not in table, name
        table[name] = (kind, make(**over))

    def scene(n_scene=2, stride=None, obs=True, n_obs=True, ids=True):
        s = ffi.SceneSet(n_scene=n_scene, stride=e.S.stride if stride is None else stride, d_obs=_p(e.S.obs) if obs else None,
                         d_n_obs=_p(e.S.n_obs) if n_obs else None, d_scene_id=_p(e.ids) if ids else None)
        return C.byref(s)
    scene_faults = {"null scene set": None, "n_scene 0": scene(n_scene=0), "stride 129": scene(stride=129),
                    "null d_scene_id with two scenes": scene(ids=False), "null d_n_obs": scene(n_obs=False),
                    "null d_obs": scene(obs=False)}
    given_scene_faults = {what: sc for what, sc in scene_faults.items() if sc is not None}      # (entries whose scene set may be null)
    candidate_faults = (("candidates 0", dict(candidates=0)), ("candidates 17", dict(candidates=17)),
                        ("B * candidates above an int", dict(B=2 ** 30)))

    def opts(retries=1, mode=0, lo=True, hi=True, pos_tol=0.01, rot_tol=0.01, clear_tol=1e-4, spread=0.0):
        o = ffi.AnchoredRetryOpts(retries=retries, clearance_mode=mode, seed=1, pos_tol=pos_tol, rot_tol=rot_tol,
                                  d_q_lo=_p(e.lo) if lo else None, d_q_hi=_p(e.hi) if hi else None, clear_tol=clear_tol, spread=spread)
        return C.byref(o)

    o = e.out
    answer = dict(Y=_p(o["Y"]), stats=_p(o["stats"]), q=_p(o["q"]), pos_err=_p(o["pos_err"]), rot_err=_p(o["rot_err"]))
    pair = (("null anch", dict(anch=None)), ("null base", dict(base=None)), ("B -1", dict(B=-1)),
            ("anch is not anchored", dict(anch=base)), ("base has no pipeline", dict(base=tpl)))

    # ---- the three solve entries and the seed entry
    cold = _entry(lib.gik_anchored_ik_batch, anch=tpl, base=base, T=_p(e.T), B=B, ws=_p(o["ws"]), **answer, stream=e.stream)
    seed = _entry(lib.gik_anchored_seed_batch, anch=tpl, base=base, T=_p(e.T), q_init=_p(e.q0), B=B, ws=_p(o["ws"]), Yf=_p(e.Yf),
                  goal=_p(e.goal), stream=e.stream)
    seeded = _entry(lib.gik_anchored_ik_batch_seeded, anch=tpl, base=base, T=_p(e.T), q_init=_p(e.q0), B=B, ws=_p(o["ws"]), **answer,
                    clearance=_p(o["clearance"]), stream=e.stream)
    scenes = _entry(lib.gik_anchored_ik_batch_scenes, anch=tpl, base=base, T=_p(e.T), q_init=_p(e.q0), B=B, scenes=scene(),
                    ws=_p(o["ws"]), **answer, clearance=_p(o["clearance"]), mode=0, stream=e.stream)
    for export, make, buffers in (("gik_anchored_ik_batch", cold, ("T", "ws", *answer)),
                                  ("gik_anchored_seed_batch", seed, ("T", "ws", "Yf", "goal")),
                                  ("gik_anchored_ik_batch_seeded", seeded, ("T", "ws", *answer)),
                                  ("gik_anchored_ik_batch_scenes", scenes, ("T", "ws", *answer))):
        for what, over in pair:
            add(export, make, what, **over)
        for b in buffers:
            add(export, make, "null " + b, **{b: None})
        add(export, make, "anch is not anchored + null ws", anch=base, ws=None)
        add(export, make, "base has no pipeline + null T", base=tpl, T=None)
        add(export, make, "B -1 + base has no pipeline", B=-1, base=tpl)
    for export, make in (("gik_anchored_seed_batch", seed), ("gik_anchored_ik_batch_seeded", seeded)):
        add(export, make, "null q_init", q_init=None)
        add(export, make, "null q_init + null T", q_init=None, T=None)
        add(export, make, "anch is not anchored + null q_init", anch=base, q_init=None)
    for what, sc in scene_faults.items():
        add("gik_anchored_ik_batch_scenes", scenes, what, scenes=sc)
    add("gik_anchored_ik_batch_scenes", scenes, "cold, base has no pipeline", q_init=None, base=tpl)
    add("gik_anchored_ik_batch_scenes", scenes, "mode 2", mode=2)
    add("gik_anchored_ik_batch_scenes", scenes, "mode -1", mode=-1)
    add("gik_anchored_ik_batch_scenes", scenes, "mode links without links", anch=bare, mode=1)
    add("gik_anchored_ik_batch_scenes", scenes, "mode 2 + without links", anch=bare, mode=2)
    add("gik_anchored_ik_batch_scenes", scenes, "null scene set + mode 2", scenes=None, mode=2)
    add("gik_anchored_ik_batch_scenes", scenes, "anch is not anchored + null scene set", anch=base, scenes=None)
    add("gik_anchored_ik_batch_scenes", scenes, "mode links without links + null T", anch=bare, mode=1, T=None)
    add("gik_anchored_ik_batch_scenes", scenes, "mode 2 + null ws", mode=2, ws=None)

    # ---- the four clearances
    for links in (False, True):
        for with_scenes in (False, True):
            export = "gik_anchored_" + ("link_" if links else "") + "clearance" + ("_scenes" if with_scenes else "")
            d = dict(anch=tpl, Y=_p(o["Y"]), B=B)
            if with_scenes:
                d["scenes"] = scene()
            make = _entry(getattr(lib, export), **d, clearance=_p(o["clearance"]), stream=e.stream)
            add(export, make, "null anch", anch=None)
            add(export, make, "B -1", B=-1)
            add(export, make, "anch is not anchored", anch=base)
            add(export, make, "null Y", Y=None)
            add(export, make, "null clearance", clearance=None)
            add(export, make, "B -1 + anch is not anchored", B=-1, anch=base)
            add(export, make, "anch is not anchored + null Y", anch=base, Y=None)
            if links:
                add(export, make, "without links", anch=bare)
                add(export, make, "without links + null Y", anch=bare, Y=None)
            if with_scenes:
                for what, sc in scene_faults.items():
                    add(export, make, what, scenes=sc)
                add(export, make, "anch is not anchored + null scene set", anch=base, scenes=None)
                add(export, make, "n_scene 0 + null clearance", scenes=scene_faults["n_scene 0"], clearance=None)
            if links and with_scenes:
                add(export, make, "null scene set + without links", anch=bare, scenes=None)

    # ---- the sweep
    sweep = _entry(lib.gik_anchored_sweep_clearance, anch=tpl, base=base, q_a=_p(e.q0), q_b=_p(e.q1), B=B, samples=4, ws=_p(e.sws),
                   clearance=_p(o["clearance"]), stream=e.stream)
    for what, over in pair:
        add("gik_anchored_sweep_clearance", sweep, what, **over)
    for b in ("q_a", "q_b", "ws", "clearance"):
        add("gik_anchored_sweep_clearance", sweep, "null " + b, **{b: None})
    add("gik_anchored_sweep_clearance", sweep, "without links", anch=bare)
    add("gik_anchored_sweep_clearance", sweep, "samples 0", samples=0)
    add("gik_anchored_sweep_clearance", sweep, "B (samples + 1) above an int", samples=2 ** 31 - 1)
    add("gik_anchored_sweep_clearance", sweep, "base has no pipeline + without links", base=tpl, anch=bare)
    add("gik_anchored_sweep_clearance", sweep, "without links + samples 0", anch=bare, samples=0)
    add("gik_anchored_sweep_clearance", sweep, "samples 0 + null q_a", samples=0, q_a=None)

    # ---- the three restart entries that draw their seeds
    for export in ("gik_anchored_ik_batch_retry", "gik_anchored_ik_batch_retry_scenes", "gik_anchored_ik_batch_retry_screened"):
        with_scenes, screened = export.endswith("_scenes"), export.endswith("_screened")
        d = dict(anch=tpl, base=base, T=_p(e.T), q_init=_p(e.q0), B=B, opts=opts())
        if with_scenes:
            d["scenes"] = scene()
        if screened:      # (candidates, then a scene set that may be null)
            d.update(candidates=4, scenes=None)
        make = _entry(getattr(lib, export), **d, ws=_p(e.aws if screened else e.rws), **answer, clearance=_p(o["clearance"]),
                      attempt=_p(e.attempt), stream=e.stream)
        for what, over in pair:
            add(export, make, what, **over)
        add(export, make, "null opts", opts=None)
        for what, op in (("retries 64", opts(retries=64)), ("retries -1", opts(retries=-1)), ("mode 2", opts(mode=2)),
                         ("mode -1, no retries", opts(mode=-1, retries=0)), ("null q_lo", opts(lo=False)), ("null q_hi", opts(hi=False)),
                         ("pos_tol 0", opts(pos_tol=0.0)), ("rot_tol nan", opts(rot_tol=float("nan"))), ("clear_tol 0", opts(clear_tol=0.0)),
                         ("spread -0.1", opts(spread=-0.1)), ("spread nan", opts(spread=float("nan"))),
                         ("retries 64 + mode 2", opts(retries=64, mode=2)), ("mode 2 + null q_lo", opts(mode=2, lo=False)),
                         ("null q_hi + clear_tol 0", opts(hi=False, clear_tol=0.0)), ("pos_tol 0 + spread -0.1", opts(pos_tol=0.0, spread=-0.1))):
            add(export, make, what, opts=op)
        add(export, make, "mode links without links", anch=bare, opts=opts(mode=1))
        add(export, make, "mode links without links, no retries", anch=bare, opts=opts(mode=1, retries=0))
        add(export, make, "mode 2 + without links", anch=bare, opts=opts(mode=2))
        add(export, make, "spread 0.1 from a cold batch", q_init=None, opts=opts(spread=0.1))
        add(export, make, "base has no pipeline + retries 64", base=tpl, opts=opts(retries=64))
        add(export, make, "null clearance", clearance=None)
        add(export, make, "null attempt", attempt=None)
        add(export, make, "null ws", ws=None)
        add(export, make, "ws off 8-byte alignment", ws=_p(e.aws if screened else e.rws) + 4)
        for b in ("T", *answer):
            add(export, make, "null " + b, **{b: None})
        add(export, make, "null clearance + null ws", clearance=None, ws=None)
        add(export, make, "null ws + null T", ws=None, T=None)
        add(export, make, "clear_tol 0 + null attempt", opts=opts(clear_tol=0.0), attempt=None)
        if with_scenes:
            for what, sc in scene_faults.items():
                add(export, make, what, scenes=sc)
            add(export, make, "base has no pipeline + null scene set", base=tpl, scenes=None)
            add(export, make, "null scene set + retries 64", scenes=None, opts=opts(retries=64))
            add(export, make, "stride 129 + mode 2", scenes=scene_faults["stride 129"], opts=opts(mode=2))
        if screened:
            for what, sc in given_scene_faults.items():
                add(export, make, what, scenes=sc)
            for what, over in candidate_faults:
                add(export, make, what, **over)
            add(export, make, "clear_tol 0, no retries", opts=opts(retries=0, clear_tol=0.0))
            add(export, make, "base has no pipeline + n_scene 0", base=tpl, scenes=scene_faults["n_scene 0"])
            add(export, make, "base has no pipeline + candidates 0", base=tpl, candidates=0)
            add(export, make, "n_scene 0 + retries 64", scenes=scene_faults["n_scene 0"], opts=opts(retries=64))
            add(export, make, "stride 129 + mode 2", scenes=scene_faults["stride 129"], opts=opts(mode=2))
            add(export, make, "mode 2 + candidates 0", opts=opts(mode=2), candidates=0)
            add(export, make, "spread -0.1 + candidates 0", opts=opts(spread=-0.1), candidates=0)
            add(export, make, "candidates 0 + null clearance", candidates=0, clearance=None)
            add(export, make, "ws off 8-byte alignment + null T", ws=_p(e.aws) + 4, T=None)

    # ---- the three steps of a restart
    select = _entry(lib.gik_anchored_retry_select, stats=_p(o["stats"]), pos_err=_p(o["pos_err"]), rot_err=_p(o["rot_err"]),
                    clearance=_p(o["clearance"]), B=B, pos_tol=0.01, rot_tol=0.01, clear_tol=1e-4, idx=_p(e.idx), count=_p(e.count),
                    stream=e.stream)
    add("gik_anchored_retry_select", select, "B -1", B=-1)
    add("gik_anchored_retry_select", select, "null idx", idx=None)
    add("gik_anchored_retry_select", select, "null count", count=None)
    add("gik_anchored_retry_select", select, "B -1 + null idx", B=-1, idx=None)
    seeds = _entry(lib.gik_anchored_retry_seeds, base=base, T=_p(e.T), idx=_p(e.idx), count=B, seed=1, attempt=1, q_lo=_p(e.lo),
                   q_hi=_p(e.hi), q_center=_p(e.q0), spread=0.0, T_out=_p(e.poses), q_out=_p(e.q1), stream=e.stream)
    for what, over in (("null base", dict(base=None)), ("count -1", dict(count=-1)), ("base has no pipeline", dict(base=tpl)),
                       ("attempt -1", dict(attempt=-1)), ("attempt 64", dict(attempt=64)), ("null q_lo", dict(q_lo=None)),
                       ("null q_hi", dict(q_hi=None)), ("spread -1", dict(spread=-1.0)), ("spread nan", dict(spread=float("nan"))),
                       ("spread 0.1 without a centre", dict(spread=0.1, q_center=None)), ("null T", dict(T=None)),
                       ("null idx", dict(idx=None)), ("null T_out", dict(T_out=None)), ("null q_out", dict(q_out=None)),
                       ("count -1 + base has no pipeline", dict(count=-1, base=tpl)), ("attempt 64 + null q_lo", dict(attempt=64, q_lo=None)),
                       ("null q_hi + spread -1", dict(q_hi=None, spread=-1.0)), ("spread 0.1 without a centre + null T", dict(spread=0.1, q_center=None, T=None))):
        add("gik_anchored_retry_seeds", seeds, what, **over)
    r = e.out_r
    compact = dict(Y_r=_p(r["Y"]), stats_r=_p(r["stats"]), q_r=_p(r["q"]), pos_err_r=_p(r["pos_err"]), rot_err_r=_p(r["rot_err"]),
                   clearance_r=_p(r["clearance"]))
    merge = _entry(lib.gik_anchored_retry_merge, anch=tpl, base=base, idx=_p(e.idx), count=B, attempt=1, pos_tol=0.01, rot_tol=0.01,
                   clear_tol=1e-4, **compact, **answer, clearance=_p(o["clearance"]), attempt_of=_p(e.attempt), stream=e.stream)
    for what, over in pair:
        add("gik_anchored_retry_merge", merge, what.replace("B -1", "count -1"), **({"count": -1} if "B" in over else over))
    for b in ("idx", *compact, *answer, "clearance", "attempt_of"):
        add("gik_anchored_retry_merge", merge, "null " + b, **{b: None})
    add("gik_anchored_retry_merge", merge, "anch is not anchored + null idx", anch=base, idx=None)
    add("gik_anchored_retry_merge", merge, "count -1 + base has no pipeline", count=-1, base=tpl)

    # ---- gik_anchored_attach_links: refused calls only, so `bare` stays without links
    def links(n_link=2, hinges=0, a=(0, 4), b=(4, 5), radius=(0.0, 0.01), arrays=True):
        keep = [np.asarray(a, dtype=np.int32), np.asarray(b, dtype=np.int32), np.asarray(radius, dtype=np.float64)]
        d = ffi.LinkDesc(n_link=n_link, hinges=hinges, link_a=keep[0].ctypes.data_as(C.POINTER(C.c_int32)) if arrays else None,
                         link_b=keep[1].ctypes.data_as(C.POINTER(C.c_int32)), link_radius=keep[2].ctypes.data_as(C.POINTER(C.c_double)))
        e.__dict__.setdefault("_keep", []).append(keep)
        return C.byref(d)
    attach = _entry(lib.gik_anchored_attach_links, anch=bare, d=links())
    N = e.tpl.full_N
    for what, over in (("null anch", dict(anch=None)), ("null desc", dict(d=None)), ("anch is not anchored", dict(anch=base)),
                       ("links already attached", dict(anch=tpl)), ("hinges 2", dict(d=links(hinges=2))),
                       ("n_link -1", dict(d=links(n_link=-1))), ("n_link 65", dict(d=links(n_link=65))),
                       ("null link_a", dict(d=links(arrays=False))), ("link_a outside", dict(d=links(a=(0, N)))),
                       ("link_b outside", dict(d=links(b=(4, -1)))), ("negative radius", dict(d=links(radius=(0.0, -1e-3)))),
                       ("nan radius", dict(d=links(radius=(float("nan"), 0.0)))), ("infinite radius", dict(d=links(radius=(0.0, float("inf"))))),
                       ("anch is not anchored + hinges 2", dict(anch=base, d=links(hinges=2))),
                       ("links already attached + n_link 65", dict(anch=tpl, d=links(n_link=65))),
                       ("hinges 2 + n_link 65", dict(d=links(hinges=2, n_link=65))),
                       ("link 0 outside + link 1 negative radius", dict(d=links(a=(N, 0), radius=(0.0, -1.0)))),
                       ("link 0 nan radius + link 1 outside", dict(d=links(b=(4, N), radius=(float("nan"), 0.0))))):
        add("gik_anchored_attach_links", attach, what, **over)

    # ---- the half-space and the self clearance, the sweep with two outputs
    selft, sbase, half, half_bare = e.selft._h, e.sbase._h, e.half._h, e.half_bare._h
    ex = "gik_anchored_halfspace_clearance"
    make = _entry(getattr(lib, ex), anch=half, Y=_p(o["Y"]), B=B, links=0, clearance=_p(o["clearance"]), stream=e.stream)
    for what, over in (("null anch", dict(anch=None)), ("B -1", dict(B=-1)), ("anch is not anchored", dict(anch=base)),
                       ("without half-spaces", dict(anch=tpl)), ("links 2", dict(links=2)),
                       ("links 1 without links", dict(anch=half_bare, links=1)), ("null Y", dict(Y=None)),
                       ("null clearance", dict(clearance=None)), ("B -1 + anch is not anchored", dict(B=-1, anch=base)),
                       ("without half-spaces + links 2", dict(anch=tpl, links=2)), ("links 2 + null Y", dict(links=2, Y=None)),
                       ("links 1 without links + null Y", dict(anch=half_bare, links=1, Y=None))):
        add(ex, make, what, **over)
    ex = "gik_anchored_self_clearance"
    make = _entry(getattr(lib, ex), anch=selft, Y=_p(o["Y"]), B=B, clearance=_p(o["clearance"]), stream=e.stream)
    for what, over in (("null anch", dict(anch=None)), ("B -1", dict(B=-1)), ("anch is not anchored", dict(anch=base)),
                       ("without links", dict(anch=bare)), ("without self pairs", dict(anch=tpl)), ("null Y", dict(Y=None)),
                       ("null clearance", dict(clearance=None)), ("B -1 + anch is not anchored", dict(B=-1, anch=base)),
                       ("without links + null clearance", dict(anch=bare, clearance=None)),
                       ("without self pairs + null Y", dict(anch=tpl, Y=None))):
        add(ex, make, what, **over)
    ex = "gik_anchored_sweep_clearances"
    make = _entry(getattr(lib, ex), anch=selft, base=sbase, q_a=_p(e.q0), q_b=_p(e.q1), B=B, samples=4, ws=_p(e.sws),
                  link_out=_p(o["clearance"]), self_out=_p(e.self_out), stream=e.stream)
    for what, over in pair:
        add(ex, make, what, **over)
    for what, over in (("without links", dict(anch=bare)), ("samples 0", dict(samples=0)),
                       ("B (samples + 1) above an int", dict(samples=2 ** 31 - 1)),
                       ("both outputs null", dict(link_out=None, self_out=None)), ("self_out without self pairs", dict(anch=tpl)),
                       ("null q_a", dict(q_a=None)), ("null q_b", dict(q_b=None)), ("null ws", dict(ws=None)),
                       ("base has no pipeline + without links", dict(base=tpl, anch=bare)),
                       ("without links + samples 0", dict(anch=bare, samples=0)),
                       ("samples 0 + both outputs null", dict(samples=0, link_out=None, self_out=None)),
                       ("both outputs null, without self pairs", dict(anch=tpl, link_out=None, self_out=None)),
                       ("self_out without self pairs + null q_a", dict(anch=tpl, q_a=None))):
        add(ex, make, what, **over)

    # ---- the screened seed step and the atlas: the nearest rows, the seed step, the batch entry, its picks
    step_modes = (("mode 2", dict(mode=2)), ("mode -1", dict(mode=-1)), ("mode links without links", dict(anch=bare, mode=1)))
    step_ws = (("null ws", dict(ws=None)), ("ws off 8-byte alignment", dict(ws=_p(e.scw) + 4)))
    step_out = dict(ws=_p(e.scw), T_out=_p(e.poses), q_out=_p(e.q1), pick=_p(e.pick), pick_clearance=_p(e.pick_cl), stream=e.stream)
    ex = "gik_anchored_retry_seeds_screened"
    make = _entry(getattr(lib, ex), anch=tpl, base=base, T=_p(e.T), idx=_p(e.idx), B=B, seed=1, attempt=1, q_lo=_p(e.lo),
                  q_hi=_p(e.hi), q_center=_p(e.q0), spread=0.0, candidates=4, mode=0, clear_tol=1e-4, scenes=None, **step_out)
    for what, over in (*pair, *((w, dict(scenes=sc)) for w, sc in given_scene_faults.items()), *step_modes,
                       ("attempt -1", dict(attempt=-1)), ("attempt 64", dict(attempt=64)), ("null q_lo", dict(q_lo=None)),
                       ("null q_hi", dict(q_hi=None)), ("spread -1", dict(spread=-1.0)), ("spread nan", dict(spread=float("nan"))),
                       ("spread 0.1 without a centre", dict(spread=0.1, q_center=None)), *candidate_faults,
                       ("clear_tol 0", dict(clear_tol=0.0)), ("clear_tol nan", dict(clear_tol=float("nan"))), *step_ws,
                       ("null T", dict(T=None)), ("null idx", dict(idx=None)), ("null T_out", dict(T_out=None)),
                       ("null q_out", dict(q_out=None)),
                       ("base has no pipeline + n_scene 0", dict(base=tpl, scenes=scene_faults["n_scene 0"])),
                       ("anch is not anchored + mode 2", dict(anch=base, mode=2)),
                       ("base has no pipeline + candidates 0", dict(base=tpl, candidates=0)),
                       ("stride 129 + mode 2", dict(scenes=scene_faults["stride 129"], mode=2)),
                       ("mode 2 + attempt 64", dict(mode=2, attempt=64)), ("attempt 64 + null q_lo", dict(attempt=64, q_lo=None)),
                       ("null q_hi + spread -1", dict(q_hi=None, spread=-1.0)),
                       ("spread 0.1 without a centre + candidates 0", dict(spread=0.1, q_center=None, candidates=0)),
                       ("candidates 0 + clear_tol 0", dict(candidates=0, clear_tol=0.0)),
                       ("clear_tol 0 + null ws", dict(clear_tol=0.0, ws=None)), ("null ws + null T", dict(ws=None, T=None)),
                       ("ws off 8-byte alignment + null T", dict(ws=_p(e.scw) + 4, T=None))):
        add(ex, make, what, **over)
    ex = "gik_atlas_nearest"
    make = _entry(getattr(lib, ex), base=base, keys=_p(e.keys), atlas_count=ATLAS_ROWS, T=_p(e.T), idx=_p(e.idx), B=B, K=4,
                  nbr=_p(e.nbr), dist=_p(e.dist), stream=e.stream)
    for what, over in (("null base", dict(base=None)), ("B -1", dict(B=-1)), ("base has no pipeline", dict(base=tpl)),
                       ("K 0", dict(K=0)), ("K 65", dict(K=65)), ("atlas_count 0", dict(atlas_count=0)),
                       ("atlas_count above 2^30", dict(atlas_count=2 ** 30 + 1)), ("B * K above an int", dict(B=2 ** 30)),
                       ("null keys", dict(keys=None)), ("null T", dict(T=None)), ("null nbr", dict(nbr=None)),
                       ("B -1 + base has no pipeline", dict(B=-1, base=tpl)), ("base has no pipeline + K 0", dict(base=tpl, K=0)),
                       ("K 0 + atlas_count 0", dict(K=0, atlas_count=0)), ("atlas_count 0 + null keys", dict(atlas_count=0, keys=None)),
                       ("null keys + null T", dict(keys=None, T=None))):
        add(ex, make, what, **over)
    ex = "gik_anchored_atlas_seeds"
    make = _entry(getattr(lib, ex), anch=tpl, base=base, atlas_q=_p(e.aq), atlas_count=ATLAS_ROWS, T=_p(e.T), idx=_p(e.idx), B=B,
                  nbr=_p(e.nbr), nbr_stride=8, first=0, candidates=4, mode=0, clear_tol=1e-4, scenes=None, **step_out)
    for what, over in (*pair, *((w, dict(scenes=sc)) for w, sc in given_scene_faults.items()), *step_modes, *candidate_faults,
                       ("atlas_count 0", dict(atlas_count=0)), ("atlas_count above 2^30", dict(atlas_count=2 ** 30 + 1)),
                       ("first -1", dict(first=-1)), ("nbr_stride 0", dict(nbr_stride=0)), ("first 5 of 8 ranks", dict(first=5)),
                       ("clear_tol 0", dict(clear_tol=0.0)), ("null atlas_q", dict(atlas_q=None)), *step_ws,
                       ("null T", dict(T=None)), ("null nbr", dict(nbr=None)), ("null T_out", dict(T_out=None)),
                       ("null q_out", dict(q_out=None)),
                       ("base has no pipeline + n_scene 0", dict(base=tpl, scenes=scene_faults["n_scene 0"])),
                       ("anch is not anchored + mode 2", dict(anch=base, mode=2)),
                       ("base has no pipeline + candidates 0", dict(base=tpl, candidates=0)),
                       ("stride 129 + mode 2", dict(scenes=scene_faults["stride 129"], mode=2)),
                       ("mode 2 + candidates 0", dict(mode=2, candidates=0)),
                       ("candidates 0 + atlas_count 0", dict(candidates=0, atlas_count=0)),
                       ("atlas_count 0 + first -1", dict(atlas_count=0, first=-1)),
                       ("first -1 + clear_tol 0", dict(first=-1, clear_tol=0.0)),
                       ("clear_tol 0 + null atlas_q", dict(clear_tol=0.0, atlas_q=None)),
                       ("null atlas_q + null ws", dict(atlas_q=None, ws=None)), ("null ws + null T", dict(ws=None, T=None)),
                       ("ws off 8-byte alignment + null T", dict(ws=_p(e.scw) + 4, T=None))):
        add(ex, make, what, **over)
    ex = "gik_anchored_ik_batch_atlas"
    make = _entry(getattr(lib, ex), anch=tpl, base=base, T=_p(e.T), q_init=_p(e.q0), B=B, opts=opts(), candidates=4,
                  atlas_keys=_p(e.keys), atlas_q=_p(e.aq), atlas_count=ATLAS_ROWS, scenes=None, ws=_p(e.aws), **answer,
                  clearance=_p(o["clearance"]), attempt=_p(e.attempt), stream=e.stream)
    for what, over in (*pair, ("null opts", dict(opts=None)), *((w, dict(scenes=sc)) for w, sc in given_scene_faults.items()),
                       ("mode 2", dict(opts=opts(mode=2))), ("mode -1, no retries", dict(opts=opts(mode=-1, retries=0))),
                       ("mode links without links", dict(anch=bare, opts=opts(mode=1))),
                       ("retries 64", dict(opts=opts(retries=64))), ("retries -1", dict(opts=opts(retries=-1))), *candidate_faults,
                       ("K 68 above 64", dict(opts=opts(retries=16))), ("atlas_count 0", dict(atlas_count=0)),
                       ("atlas_count above 2^30", dict(atlas_count=2 ** 30 + 1)),
                       ("B * K above an int", dict(B=2 ** 30, candidates=1)), ("K 8 above atlas_count 7", dict(atlas_count=7)),
                       ("pos_tol 0", dict(opts=opts(pos_tol=0.0))), ("rot_tol nan", dict(opts=opts(rot_tol=float("nan")))),
                       ("clear_tol 0, no retries", dict(opts=opts(clear_tol=0.0, retries=0))),
                       ("spread 0.1", dict(opts=opts(spread=0.1))), ("spread -0.1", dict(opts=opts(spread=-0.1))),
                       ("null atlas_keys", dict(atlas_keys=None)), ("null atlas_q", dict(atlas_q=None)),
                       ("null clearance", dict(clearance=None)), ("null attempt", dict(attempt=None)), ("null ws", dict(ws=None)),
                       ("ws off 8-byte alignment", dict(ws=_p(e.aws) + 4)), *(("null " + b, {b: None}) for b in ("T", *answer)),
                       ("base has no pipeline + n_scene 0", dict(base=tpl, scenes=scene_faults["n_scene 0"])),
                       ("anch is not anchored + mode 2", dict(anch=base, opts=opts(mode=2))),
                       ("base has no pipeline + candidates 0", dict(base=tpl, candidates=0)),
                       ("stride 129 + mode 2", dict(scenes=scene_faults["stride 129"], opts=opts(mode=2))),
                       ("mode 2 + retries 64", dict(opts=opts(mode=2, retries=64))),
                       ("retries 64 + candidates 0", dict(opts=opts(retries=64), candidates=0)),
                       ("candidates 0 + atlas_count 0", dict(candidates=0, atlas_count=0)),
                       ("atlas_count 0 + pos_tol 0", dict(atlas_count=0, opts=opts(pos_tol=0.0))),
                       ("K 8 above atlas_count 7 + clear_tol 0", dict(atlas_count=7, opts=opts(clear_tol=0.0))),
                       ("clear_tol 0 + null atlas_q", dict(opts=opts(clear_tol=0.0), atlas_q=None)),
                       ("spread 0.1 + null atlas_keys", dict(opts=opts(spread=0.1), atlas_keys=None)),
                       ("null atlas_q + null clearance", dict(atlas_q=None, clearance=None)),
                       ("null clearance + null ws", dict(clearance=None, ws=None)), ("null ws + null T", dict(ws=None, T=None)),
                       ("ws off 8-byte alignment + null T", dict(ws=_p(e.aws) + 4, T=None))):
        add(ex, make, what, **over)
    ex = "gik_anchored_atlas_picks"
    make = _entry(getattr(lib, ex), anch=tpl, base=base, B=B, candidates=4, retries=1, ws=_p(e.aws), attempt=_p(e.attempt),
                  atlas_pick=_p(e.pick), stream=e.stream)
    for what, over in (*pair, ("retries -1", dict(retries=-1)), ("retries 64", dict(retries=64)), *candidate_faults,
                       ("K 68 above 64", dict(retries=16)), ("null ws", dict(ws=None)),
                       ("ws off 8-byte alignment", dict(ws=_p(e.aws) + 4)), ("null attempt", dict(attempt=None)),
                       ("null atlas_pick", dict(atlas_pick=None)), ("B -1 + base has no pipeline", dict(B=-1, base=tpl)),
                       ("base has no pipeline + retries 64", dict(base=tpl, retries=64)),
                       ("retries 64 + candidates 0", dict(retries=64, candidates=0)),
                       ("candidates 0 + null ws", dict(candidates=0, ws=None)), ("null ws + null attempt", dict(ws=None, attempt=None))):
        add(ex, make, what, **over)

    # ---- the sizes of the screened and the atlas workspaces
    for ex, d in (("gik_anchored_retry_seeds_screened_ws_bytes", dict(candidates=4)),
                  ("gik_anchored_ik_batch_retry_screened_ws_bytes", dict(candidates=4)),
                  ("gik_anchored_atlas_seeds_ws_bytes", dict(candidates=4)),
                  ("gik_anchored_ik_batch_atlas_ws_bytes", dict(candidates=4, retries=1))):
        make = _entry(getattr(lib, ex), anch=tpl, base=base, B=B, **d)
        for what, over in (*pair, *candidate_faults):
            add(ex, make, what, kind="size", **over)
    atlas_bytes = _entry(lib.gik_anchored_ik_batch_atlas_ws_bytes, anch=tpl, base=base, B=B, candidates=4, retries=1)
    for what, over in (("retries -1", dict(retries=-1)), ("retries 64", dict(retries=64)), ("K 68 above 64", dict(retries=16)),
                       ("B * K above an int", dict(B=2 ** 30, candidates=1))):
        add("gik_anchored_ik_batch_atlas_ws_bytes", atlas_bytes, what, kind="size", **over)

    # ---- the three sizes
    ws_doubles = _entry(lib.gik_anchored_ws_doubles, anch=tpl, base=base, B=B)
    retry_bytes = _entry(lib.gik_anchored_retry_ws_bytes, anch=tpl, base=base, B=B)
    sweep_bytes = _entry(lib.gik_anchored_sweep_ws_bytes, anch=tpl, base=base, B=B, samples=4)
    for export, make in (("gik_anchored_ws_doubles", ws_doubles), ("gik_anchored_retry_ws_bytes", retry_bytes),
                         ("gik_anchored_sweep_ws_bytes", sweep_bytes)):
        for what, over in pair[:4]:
            add(export, make, what, kind="size", **over)
    for export, make in (("gik_anchored_retry_ws_bytes", retry_bytes), ("gik_anchored_sweep_ws_bytes", sweep_bytes)):
        add(export, make, "base has no pipeline", kind="size", base=tpl)
    add("gik_anchored_sweep_ws_bytes", sweep_bytes, "samples 0", kind="size", samples=0)
    add("gik_anchored_sweep_ws_bytes", sweep_bytes, "B (samples + 1) above an int", kind="size", samples=2 ** 31 - 1)
    return table


def run(table):
    """name -> {"rc", "message"} of every case, in the table's order"""
    lib = env().lib
    got = {}
    for name, (kind, call) in table.items():
        rc = int(call())
        got[name] = {"rc": rc, "message": SIZE if kind == "size" else lib.gik_last_error().decode()}
    return got


def test_refusals_equal_the_parents():
    with open(GOLDEN_FILE) as f:
        want = json.load(f)["cases"]
    table = cases()
    assert sorted(want) == sorted(table)
    e = env()
    outputs = {**e.out, "attempt": e.attempt, "rws": e.rws}
    before = {k: v.clone() for k, v in outputs.items()}
    got = run(table)
    for name, (kind, _) in table.items():
        # no case passes by not having been refused: every recorded call failed (a size: returned 0) and left a message
        assert want[name]["message"] and want[name]["rc"] == (0 if kind == "size" else -1), name
        assert got[name] == want[name], (name, got[name], want[name])
    e.torch.cuda.synchronize()
    assert all(e.torch.equal(v.view(e.torch.int32), before[k].view(e.torch.int32)) for k, v in outputs.items())
    assert e.bare.n_link is None and int(e.lib.gik_anchored_link_clearance(e.bare._h, None, 0, None, e.stream)) != 0      # still none


@pytest.mark.parametrize("nb", [0, 1, 5])
def test_workspace_sizes_equal_the_closed_forms(nb):
    """gik_retry_ws_bytes, gik_anchored_retry_ws_bytes and gik_anchored_sweep_ws_bytes (samples = 2) on the UR10 pair
    against the layout comments' closed forms (tests/test_ws_layouts.py), and the Python layer's helper on top."""
    e = env()
    lib, tpl, base = e.lib, e.tpl, e.base
    n, K = base.n_joints, base.k
    pose_w = base.n_ee * (K + 1) * (K + 1)
    assert (n, K, pose_w) == (e.robot.n, 3, 16) and base.info["has_pipeline"] and tpl.info["anchored"] and tpl.full_N == base.N
    assert int(lib.gik_retry_ws_bytes(base._h, nb)) == \
        8 + pad8(4 * nb) + 8 * nb * (pose_w + n + base.T + base.N * K) + STATS * nb + 8 * nb * (n + 2)
    scratch = nb * (base.T + 3 * base.N + 3 * tpl.N + 3 * tpl.n_goal_anchor)
    assert int(lib.gik_anchored_ws_doubles(tpl._h, base._h, nb)) == scratch
    plain = 8 * scratch + 8 + pad8(4 * nb) + 8 * nb * (pose_w + 2 * n + 3 * tpl.full_N) + STATS * nb + 8 * nb * (n + 3)
    assert int(lib.gik_anchored_retry_ws_bytes(tpl._h, base._h, nb)) == plain
    M = nb * (2 + 1)
    assert int(lib.gik_anchored_sweep_ws_bytes(tpl._h, base._h, nb, 2)) == 8 * M * (n + pose_w + base.T + 3 * tpl.full_N + 1)
    assert tpl.anchored_retry_ws_bytes(base, nb) == tpl.anchored_retry_ws_bytes(base, nb, scenes=False) == plain
    assert tpl.anchored_retry_ws_bytes(base, nb, scenes=True) == plain + 4 * nb
