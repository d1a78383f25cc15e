"""The synthetic fixed-anchor problems of tests/synth_anchored.py, checked on the CPU before anything runs on a GPU
(tests/test_anchored_limits_gpu.py): every case sits exactly on the boundary it claims (counts re-derived from the term
lists), the plain numpy reference agrees with a 50-digit mpmath evaluation (its own rounding floor), the known-answer
points exercise every class of terms, the CPU twin of the solve converges from every start point and does so stably,
and the case table covers the compiled anchored kernels.  No GPU needed."""
import copy
import functools
import re

import numpy as np
import pytest

import synth_anchored as sa
import synth_graphs as sg
from parity_util import anchored_numpy_terms, first_divergence, report
from synth_graphs import EQ, LOWER, UPPER

ANCH_MAXN, ANCH_MAXDEG, ANCH_MAXA, ANCH_PMAX, ANCH_MAXOBS = 21, 20, 16, 8, 128       # gik_wave.hip.h / gik_host.hip
KERNEL_BAR = 1e-12              # the project's bar for cost / egrad / ehess (test_anchored_kernel_known_answers)


# ---- 1. boundaries ---------------------------------------------------------------------------------------------------
def counts(p):
    """What the term lists of a problem say: busiest free-free degree, pins per node, rows, goal rows, obstacles."""
    deg = np.bincount(np.concatenate([p.ti, p.tj]), minlength=p.N)
    per_node = np.bincount([q[0] for q in p.pins], minlength=p.N)
    return dict(N=p.N, busiest=int(deg.max()), pins=int(per_node.max()), n_anchor=len(p.anchor_pos),
                n_goal=p.goal.shape[1] // 3, n_obs=len(p.obs))


def near_list(point, obs):
    """Indices of the spheres within NEAR_TAU of a point, ascending: the near list a full walk builds."""
    return np.flatnonzero(sa.clearance(point, obs) < sa.NEAR_TAU).tolist()


def check_boundary(cid, p, Y0):
    """Every count of CASES[cid], re-derived from the problem p (and its start points): raises AssertionError."""
    c = sa.CASES[cid]
    n = counts(p)
    for key in ("N", "busiest", "pins", "n_anchor", "n_goal", "n_obs"):
        assert n[key] == c[key], (cid, key, n[key], c[key])
    deg = np.bincount(np.concatenate([p.ti, p.tj]), minlength=p.N)
    assert int((deg == deg.max()).sum()) == 1 or p.N == 2                 # one busiest node, the hub
    assert c["slots"] == (9 if n["busiest"] <= 9 else 20)                  # the smallest compiled slot count that holds it
    assert 3 * p.N <= 64 and n["busiest"] <= ANCH_MAXDEG and n["n_anchor"] <= ANCH_MAXA and n["n_obs"] <= ANCH_MAXOBS
    # pinned terms: by (node, row, kind); three equality pins to distinct rows at every node; `pins` at one node only
    key = [(q[0], q[1], q[2]) for q in p.pins]
    assert key == sorted(set(key)) and all(0 <= q[1] < n["n_anchor"] for q in p.pins)
    per_node = np.bincount([q[0] for q in p.pins], minlength=p.N)
    assert per_node.min() >= 3 and per_node.max() <= ANCH_PMAX
    if n["n_anchor"] >= 3:
        for i in range(p.N):
            assert len({q[1] for q in p.pins if q[0] == i and q[2] == EQ}) >= 3, (cid, i)
    if c["pins"] > 3:
        assert int((per_node == c["pins"]).sum()) == 1 and per_node[p.pins_node] == c["pins"]
        assert {q[2] for q in p.pins if q[0] == p.pins_node} == {EQ, LOWER, UPPER}
    assert {q[1] for q in p.pins} == set(range(n["n_anchor"]))            # every row is used, the last included
    # goal rows are the last rows; the problems differ in them
    assert p.goal.shape == (sa.B, 3 * c["n_goal"]) and len(np.unique(p.goal.round(12), axis=0)) == sa.B
    assert np.all(p.anchor_pos[n["n_anchor"] - n["n_goal"]:] == 0.0)
    # the tip group hangs on the body by hinges only
    for i, j, k in zip(p.ti, p.tj, p.tk):
        if (i in p.tips) != (j in p.tips):
            assert k != EQ, (cid, i, j)
    # obstacles: every hidden point 4 mm outside, one node off the mask, one hinge per (masked node, sphere)
    assert int((p.mask == 0).sum()) == 1 and p.mask[p.off_node] == 0
    node, pos, tgt, kind = sa.anchor_terms(p, 0)
    assert len(node) == len(p.pins) + int(p.mask.sum()) * n["n_obs"]
    assert p.off_node not in node[len(p.pins):].tolist() and np.all(kind[len(p.pins):] == LOWER)
    if n["n_obs"]:
        assert sa.clearance(p.P, p.obs).min() >= sa.MIN_CLEAR
    if c.get("near"):
        want = sa.NEAR_IDX[c["near"]]
        for pt in [p.P[b, p.near_node] for b in range(sa.B)] + [Y0[b, p.near_node] for b in range(sa.B)]:
            assert near_list(pt, p.obs) == want, (cid, near_list(pt, p.obs))
        assert len(want) == c["near"] and p.mask[p.near_node] and p.mask[p.near_node2]
        for pt in [p.P[b, p.near_node2] for b in range(sa.B)] + [Y0[b, p.near_node2] for b in range(sa.B)]:
            assert near_list(pt, p.obs) == sa.NEAR2_IDX
        # sphere 127: list position 3 (byte 3 of idx[0]) at near_node2, position 7 (byte 3 of idx[1]) where eight are near
        assert sa.NEAR2_IDX.index(127) == 3 and n["n_obs"] - 1 == 127
        assert want.index(127) == (7 if c["near"] == 8 else 8)
    if c.get("crossing"):
        k, i = p.cross_sphere, p.cross_node
        assert p.mask[i] and k == n["n_obs"] - 1
        for b in range(sa.B):
            assert sa.clearance(Y0[b, i], p.obs)[k] >= 0.1                 # not on the near list at the start ...
            assert sa.clearance(0.5 * (Y0[b, i] + p.P[b, i]), p.obs)[k] < 0  # ... and in the way


@pytest.mark.parametrize("cid", sorted(sa.CASES))
def test_case_sits_on_its_boundary(cid):
    from graphik_amd.engine import build_terms
    p = sa.build(cid)
    check_boundary(cid, p, sa.start_points(cid))
    # the term list is engine.build_terms' of the dense matrices: what the twin reads is what the template gets
    ti, tj, tk, tv = build_terms(p.omega, p.psi_L, p.psi_U, True)
    assert np.array_equal(ti, p.ti) and np.array_equal(tj, p.tj) and np.array_equal(tk, p.tk)
    assert np.array_equal(np.where(np.isnan(tv), p.D[ti, tj], tv), p.target)
    d = sa.anchored_desc(p)
    assert np.allclose(d["obs"][:, 3], p.obs[:, 3] ** 2) and d["full_N"] == p.N + len(p.anchor_pos)


def test_a_case_moved_off_its_boundary_fails():
    """check_boundary notices one term, pin, anchor row or sphere more or less (and a near sphere moved away)."""
    cid = "near8"
    base, Y0 = sa.build(cid), sa.start_points(cid)
    check_boundary(cid, base, Y0)

    def broken(**kw):
        p = copy.copy(base)
        for k, v in kw.items():
            setattr(p, k, v)
        with pytest.raises(AssertionError):
            check_boundary(cid, p, Y0)

    hub = base.hub
    other = next(v for v in range(base.N) if v != hub and v not in base.tips and not np.any((base.ti == min(v, hub)) & (base.tj == max(v, hub))))
    broken(ti=np.append(base.ti, min(other, hub)), tj=np.append(base.tj, max(other, hub)), tk=np.append(base.tk, EQ))     # a term more
    drop = np.flatnonzero((base.ti == hub) | (base.tj == hub))[-1]
    broken(ti=np.delete(base.ti, drop), tj=np.delete(base.tj, drop), tk=np.delete(base.tk, drop))                           # a term less
    broken(pins=sorted(base.pins + [(0, 3, LOWER, 1.0)]))                                                                  # a pin more
    broken(pins=base.pins[1:])                                                                                             # a pin less
    broken(anchor_pos=np.concatenate([np.ones((1, 3)), base.anchor_pos]))                                                  # a row more
    broken(obs=base.obs[:-1])                                                                                              # a sphere less
    broken(obs=np.concatenate([base.obs, [[9.0, 9.0, 9.0, 0.1]]]))                                                         # a sphere more
    far = np.array(base.obs)
    far[sa.NEAR_IDX[8][0], :3] += 5.0
    broken(obs=far)                                                                                                        # seven near
    near = np.array(base.obs)
    k = next(k for k in range(len(near)) if k not in sa.NEAR_IDX[8] and k not in sa.NEAR2_IDX)
    near[k] = [*(base.P[0, base.near_node] + np.array([0.0, 0.0, 0.03 + 0.01])), 0.03]
    broken(obs=near)                                                                                                       # nine near
    p20 = sa.build("a20_full")
    with pytest.raises(AssertionError):
        check_boundary("a10", p20, sa.start_points("a20_full"))


@pytest.mark.parametrize("rid", sorted(sa.REFUSED))
def test_refused_shape_is_one_past_its_limit(rid):
    (N, ti, tj, tk, d), match = sa.refused(rid)
    deg = int(np.bincount(np.concatenate([ti, tj]), minlength=N).max())
    per_node = np.bincount(d["pin_node"], minlength=N)
    got = dict(N=N, busiest=deg, n_anchor=len(d["anchor_pos"]), n_goal=d["n_goal_anchor"], n_obs=len(d["obs"]),
               pins=int(per_node.max()), row=int(max(d["pin_anchor"])))
    past = {"r_n22": ("N", ANCH_MAXN + 1), "r_busiest21": ("busiest", ANCH_MAXDEG + 1), "r_anchors17": ("n_anchor", ANCH_MAXA + 1),
            "r_goal_beyond_anchors": ("n_goal", got["n_anchor"] + 1), "r_obs129": ("n_obs", ANCH_MAXOBS + 1),
            "r_pins9": ("pins", ANCH_PMAX + 1), "r_pin_row": ("row", got["n_anchor"])}[rid]
    assert got[past[0]] == past[1], (rid, got)
    inside = dict(N=got["N"] <= ANCH_MAXN, busiest=deg <= ANCH_MAXDEG, n_anchor=got["n_anchor"] <= ANCH_MAXA,
                  n_goal=got["n_goal"] <= got["n_anchor"], n_obs=got["n_obs"] <= ANCH_MAXOBS, pins=got["pins"] <= ANCH_PMAX,
                  row=got["row"] < got["n_anchor"])
    assert [k for k, ok in inside.items() if not ok] == [past[0]]          # nothing else is wrong with it
    with open(sg.INSTANCES_H.replace("gik_instances.h", "gik_host.hip")) as f:
        assert re.search(match, f.read()), match                           # the phrase is the library's


# ---- 2. the plain reference against 50 digits --------------------------------------------------------------------------
def reference(p, b, Y, W):
    """cost, egrad, ehess of problem b at (Y, W): parity_util.anchored_numpy_terms on the explicit term lists."""
    return anchored_numpy_terms(sa.free_terms(p), sa.anchor_terms(p, b), Y, W)


def mp_reference(p, b, Y, W, digits=50):
    """The same in mpmath at `digits` digits.  A hinge that fp64 finds inactive by more than 1e-9 (squared metres) is
    inactive at any precision and contributes exactly zero: only the others are evaluated."""
    import mpmath as mp
    mp.mp.dps = digits
    N = p.N
    f = mp.mpf(0)
    G = [[mp.mpf(0)] * 3 for _ in range(N)]
    H = [[mp.mpf(0)] * 3 for _ in range(N)]
    Ym = [[mp.mpf(float(v)) for v in row] for row in Y]
    Wm = [[mp.mpf(float(v)) for v in row] for row in W]
    zero = [mp.mpf(0)] * 3

    def term(i, yj, wj, j, tgt, kind):
        nonlocal f
        y = [Ym[i][c] - yj[c] for c in range(3)]
        w = [Wm[i][c] - wj[c] for c in range(3)]
        d = y[0] * y[0] + y[1] * y[1] + y[2] * y[2]
        u = mp.mpf(float(tgt)) - d
        if not (kind == EQ or (kind == LOWER and u > 0) or (kind == UPPER and u < 0)):
            return
        cc = -u
        yw = y[0] * w[0] + y[1] * w[1] + y[2] * w[2]
        f += u * u
        for c in range(3):
            g, h = 2 * cc * y[c], 2 * (2 * yw * y[c] + cc * w[c])
            G[i][c] += g
            H[i][c] += h
            if j is not None:
                G[j][c] -= g
                H[j][c] -= h
    for i, j, k_, t in zip(*sa.free_terms(p)):
        term(int(i), Ym[j], Wm[j], int(j), t, int(k_))
    node, pos, tgt, kind = sa.anchor_terms(p, b)
    u64 = tgt - ((Y[node] - pos) ** 2).sum(axis=1)
    maybe = (kind == EQ) | ((kind == LOWER) & (u64 > -1e-9)) | ((kind == UPPER) & (u64 < 1e-9))
    for t in np.flatnonzero(maybe):
        term(int(node[t]), [mp.mpf(float(v)) for v in pos[t]], zero, None, tgt[t], int(kind[t]))
    return f, G, H


@functools.lru_cache(maxsize=None)
def reference_floor(cid):
    """Largest relative distance (f to |f|, egrad to max |G|, ehess to max |H|) between the numpy reference and the
    50-digit evaluation over the case's known-answer points: the reference's own rounding floor."""
    import mpmath as mp
    p = sa.build(cid)
    Y, W = sa.known_answer_points(cid)
    worst = [0.0, 0.0, 0.0]
    for b in range(sa.B):
        f, G, H = reference(p, b, Y[b], W[b])
        fm, Gm, Hm = mp_reference(p, b, Y[b], W[b])
        gmax = max(abs(v) for row in Gm for v in row)
        hmax = max(abs(v) for row in Hm for v in row)
        worst[0] = max(worst[0], float(abs(mp.mpf(float(f)) - fm) / abs(fm)))
        worst[1] = max(worst[1], max(float(abs(mp.mpf(float(G[i, c])) - Gm[i][c]) / gmax) for i in range(p.N) for c in range(3)))
        worst[2] = max(worst[2], max(float(abs(mp.mpf(float(H[i, c])) - Hm[i][c]) / hmax) for i in range(p.N) for c in range(3)))
    return tuple(worst)


def known_answer_bar(cid):
    """The bar of the GPU comparison: the project's 1e-12 wherever the reference's floor is at least ten times below it
    (every case, asserted below), ten times the floor otherwise."""
    return max(KERNEL_BAR, 10.0 * max(reference_floor(cid)))


@pytest.mark.parametrize("cid", sorted(sa.CASES))
def test_reference_against_50_digits(cid):
    floor = reference_floor(cid)
    report(f"anchored_limits/reference_floor/{cid}", {"f": floor[0], "egrad": floor[1], "ehess": floor[2]})
    # measured: at most 4.9e-15 (a_min's egrad; docs/NOTEBOOK.md); 1e-13 keeps the GPU bar at the project's 1e-12 in every case
    assert max(floor) <= 0.1 * KERNEL_BAR, (cid, floor)
    assert known_answer_bar(cid) == KERNEL_BAR


# ---- 3. the known-answer points exercise every class of terms ---------------------------------------------------------
def class_counts(p, Y):
    """(free-free | pinned | obstacle, kind) -> [active, inactive] over the B known-answer points, decided as the
    reference decides (an equality is active while its residual is not zero)."""
    cls = {}
    npin = len(p.pins)
    for b in range(sa.B):
        d = ((Y[b][p.ti] - Y[b][p.tj]) ** 2).sum(axis=1)
        node, pos, tgt, kind = sa.anchor_terms(p, b)
        da = ((Y[b][node] - pos) ** 2).sum(axis=1)
        for name, kk, tt, dd in (("free-free", p.tk, p.target, d), ("pinned", kind[:npin], tgt[:npin], da[:npin]),
                                 ("obstacle", kind[npin:], tgt[npin:], da[npin:])):
            for k in (EQ, LOWER, UPPER):
                m = kk == k
                if m.any():
                    u = tt[m] - dd[m]
                    act = (u != 0) if k == EQ else (u > 0) if k == LOWER else (u < 0)
                    c = cls.setdefault((name, k), [0, 0])
                    c[0] += int(act.sum())
                    c[1] += int((~act).sum())
    return cls


@pytest.mark.parametrize("cid", sorted(sa.CASES))
def test_known_answer_points_exercise_every_class(cid):
    c, p = sa.CASES[cid], sa.build(cid)
    Y, W = sa.known_answer_points(cid)
    cls = class_counts(p, Y)
    want = {("free-free", EQ), ("pinned", EQ)}
    if c["busiest"] > 2:
        want |= {("free-free", LOWER), ("free-free", UPPER)}
    if c["pins"] > 3 or c["n_anchor"] == 1:
        want |= {("pinned", LOWER), ("pinned", UPPER)}
    if c["n_obs"]:
        want |= {("obstacle", LOWER)}
    assert set(cls) == want, (cid, sorted(cls))
    for key, (act, inact) in cls.items():
        assert act > 0, (cid, key)
        assert inact > 0 or key[1] == EQ, (cid, key)        # (an equality has no inactive side)
    # ... and the reference sees them: switching the active obstacle hinges off changes its cost
    if c["n_obs"]:
        f_all = reference(p, 0, Y[0], W[0])[0]
        node, pos, tgt, kind = sa.anchor_terms(p, 0)
        f_pins = anchored_numpy_terms(sa.free_terms(p), (node[:len(p.pins)], pos[:len(p.pins)], tgt[:len(p.pins)],
                                                         kind[:len(p.pins)]), Y[0], W[0])[0]
        assert f_all >= f_pins


# ---- 4. the CPU twin ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def twin(cid, b, jitter=0):
    """oracle.c_oracle.rtr_solve_anchored on problem b of a case from its start point (jitter: + 1e-9 randn)."""
    from oracle import c_oracle as co
    p = sa.build(cid)
    Y0 = sa.start_points(cid)[b]
    if jitter:
        Y0 = Y0 + 1e-9 * np.random.RandomState(100 * jitter + b).randn(p.N, 3)
    return co.rtr_solve_anchored(Y0, p.D, p.omega, p.psi_L, p.psi_U, *sa.anchor_terms(p, b), traj_cap=32)


STABLE_RTOL = 1e-9              # ten times below the 1e-8 at which the GPU is compared with the twin
N_RENDERINGS = 6


@functools.lru_cache(maxsize=None)
def stable_prefix(cid, b):
    """Number of leading outer iterations over which the twin reproduces ITSELF (identical decisions, f and |grad| to
    1e-9) when only its rounding changes: the point-to-anchor terms summed in another order (reversed, five random
    permutations), the start point moved by 1e-15 randn (a few ulps: the backward error of any other summation order), the
    strict and the FMA build of the same source in turn.  Beyond it the reference does not reproduce itself and nothing
    else can be asked to (parity_util.stable_prefix); the GPU comparison pins min(3, n, this)."""
    from oracle import c_oracle as co
    p = sa.build(cid)
    Y0 = sa.start_points(cid)[b]
    at = sa.anchor_terms(p, b)
    o = twin(cid, b)
    k = o["iterations"]
    for r in range(N_RENDERINGS):
        rng = np.random.RandomState(r)
        perm = np.arange(len(at[0]))[::-1] if r == 0 else rng.permutation(len(at[0]))
        y = Y0 if r == 0 else Y0 + 1e-15 * rng.randn(p.N, 3)
        q = co.rtr_solve_anchored(y, p.D, p.omega, p.psi_L, p.psi_U, *[a[perm] for a in at], traj_cap=32, fast=r % 2 == 0)
        k = min(k, first_divergence(q["traj"], o["traj"], min(o["iterations"], q["iterations"]), rtol=STABLE_RTOL))
    return k


def start_point_faults(cid, b):
    """What is wrong with problem b's start point, or nothing: the conditions under which it is kept (a start point that
    fails one is replaced by another seed in synth_anchored.Y0_SEEDS, never excused on the GPU)."""
    p = sa.build(cid)
    faults = []
    if not reference(p, b, p.P[b], np.zeros((p.N, 3)))[0] < 1e-20:
        faults.append("the hidden point costs something")
    o = twin(cid, b)
    if not (o["stop"] == 0 and o["f(x)"] < 1e-9 and 1 <= o["iterations"] < 32):
        faults.append(f"the twin stops with stop {o['stop']}, f {o['f(x)']:.1e} after {o['iterations']} iterations")
    for jitter in (1, 2):
        o2 = twin(cid, b, jitter)
        if not (o2["stop"] == 0 and o2["f(x)"] < 1e-9 and abs(o2["iterations"] - o["iterations"]) <= 1):
            faults.append(f"from 1e-9 away: stop {o2['stop']}, f {o2['f(x)']:.1e}, {o2['iterations']} against {o['iterations']} iterations")
    want = min(STABLE_WANT[cid], o["iterations"])
    if stable_prefix(cid, b) < want:
        faults.append(f"the twin reproduces itself for {stable_prefix(cid, b)} iterations, {want} wanted")
    return faults


# Iterations the twin must reproduce: one more than the three the GPU comparison pins.  The near cases start 0.01 from the
# solution and their third iteration already solves its trust-region model to a tight tolerance, 20 to 40 tCG steps on a
# 36-dimensional problem: there the twin reproduces two iterations, three for a rare start point (measured over 400
# seeds per problem and 12 graphs: docs/NOTEBOOK.md), so two are wanted and two are pinned on the GPU.
STABLE_WANT = {cid: 2 if sa.CASES[cid].get("near") else 4 for cid in sa.CASES}


@pytest.mark.parametrize("cid", sa.SOLVE_CASES)
def test_twin_converges_from_every_start_point(cid):
    """Per problem: the hidden point costs nothing (below 1e-20), the twin stops by its gradient rule with f < 1e-9, does
    so again from two start points 1e-9 away with the same outer-iteration count +- 1, and reproduces its own first
    iterations when only its rounding changes (stable_prefix)."""
    for b in range(sa.B):
        assert not start_point_faults(cid, b), (cid, b, start_point_faults(cid, b))
    report(f"anchored_limits/twin/{cid}", {"iterations": [twin(cid, b)["iterations"] for b in range(sa.B)],
                                           "reproduces_itself_for": [stable_prefix(cid, b) for b in range(sa.B)]})


# ---- 5. coverage -------------------------------------------------------------------------------------------------------
def test_the_case_table_covers_the_anchored_kernels():
    cov = sg.coverage()
    assert not any("ANCH" in k or re.search(r"wave_kernel<3,\d+,[^>]*W_ANCH", k) for k in sg.OUT_OF_SCOPE)
    assert all(why for why in sg.OUT_OF_SCOPE.values())
    group = sg.group_members("GIK_KERNELS_ANCH")
    assert len(group) == 4
    for inst in group:
        by_case = [c for c in cov[inst] if c.startswith("anchored:")]
        assert by_case, inst
        slots = int(inst.split(",")[1])
        assert all(sa.CASES[c.split(":")[1]]["slots"] == slots for c in by_case)
    # the link-hinge group is in the table and covered
    compiled = sg.compiled_instances()
    for inst in ("rtr_wave_kernel<3,9,W_THETA1|W_ANCH|W_LINKS>", "kat_wave_kernel<3,9,W_ANCH|W_LINKS>"):
        assert compiled.count(inst) == 1 and cov.get(inst), inst
