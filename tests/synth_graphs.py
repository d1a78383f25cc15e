"""Seeded synthetic problem graphs at the dispatch boundaries of gik_template_create, and the table of
which compiled kernel instantiation (graphik_amd/csrc/gik_instances.h) each boundary case reaches.

Plain module (numpy only at import): tests/test_variant_coverage.py reads the table without torch or a
GPU, tests/test_variant_matrix_gpu.py parametrizes from the same table, so the two cannot disagree.

A graph is a term list over N nodes: equality terms (target = squared distance of a random point set
P, or that times a per-pair factor when `scaled`), lower and upper hinges (thresholds below / above
the squared distance of P, so P satisfies them).  One pair carries an equality with psi_L == psi_U
on top (kept: both hinges apply), one pair carries psi_L == psi_U alone (dropped by build_terms and
by the oracle's limit_inds alike).
"""
import os
import re

import numpy as np

EQ, LOWER, UPPER = 1, 2, 3          # GIK_TERM_* (include/graphik_amd.h)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INSTANCES_H = os.path.join(REPO, "graphik_amd", "csrc", "gik_instances.h")


# ---- the graph builder --------------------------------------------------------------------------
class _Terms:
    def __init__(self, N):
        self.N = N
        self.kinds = {}                 # (i, j), i < j -> set of kinds

    def has(self, i, j, kind):
        return kind in self.kinds.get((min(i, j), max(i, j)), ())

    def add(self, i, j, kind):
        assert i != j
        s = self.kinds.setdefault((min(i, j), max(i, j)), set())
        assert kind not in s
        s.add(kind)

    def count(self, v, pred=lambda i, j, kind: True):
        return sum(1 for (i, j), s in self.kinds.items() if v in (i, j) for kd in s if pred(i, j, kd))


def build_graph(k, N, *, seed=0, busiest=None, clique=0, outside=None, carriers=None, per_node=None,
                scaled=False):
    """(omega, psi_L, psi_U, D, P) of a seeded synthetic graph.

    k, N      dimension and node count.
    busiest   exact number of terms at the busiest node (a hub node gets terms to every nearby node).
    clique    size of a rigid equality clique on nodes 0 .. clique-1 (0: none).
    outside   exact number of terms outside the clique (every term but the clique's equalities).
    carriers  exact number of nodes that carry such terms (the node-per-lane kernel's direction rows).
    per_node  exact number of such terms at the busiest non-clique node (its gather list).
    scaled    each equality target times its own factor in [0.9, 1.1]: no exact solution.
    The counts are asserted by the caller through term_counts (engine.build_terms)."""
    rng = np.random.RandomState(seed)
    P = 0.5 * rng.randn(N, k)            # (robot scale: targets of order 1, as in the fixtures)
    tm = _Terms(N)
    C = clique
    for a in range(C):
        for b in range(a + 1, C):
            tm.add(a, b, EQ)
    chain0 = C if C else 1
    for v in range(chain0, N):          # a chain through the other nodes, tied to the clique's last node
        tm.add(v - 1, v, EQ)
    # psi_L == psi_U on top of an equality (kept) on the first chain pair outside the clique
    eq_pair = (chain0, chain0 + 1) if chain0 + 1 < N else (chain0 - 1, chain0)
    tm.add(*eq_pair, LOWER)
    tm.add(*eq_pair, UPPER)
    equal_pairs = {eq_pair}
    for a, kind in ((chain0 + 2, LOWER), (chain0 + 3, UPPER)):      # plain hinges next to it
        if a + 1 < N:
            tm.add(a, a + 1, kind)
    # psi_L == psi_U alone (dropped): a pair that carries nothing else
    lone = None
    for a in range(chain0, N):
        for b in range(a + 2, N):
            if (a, b) not in tm.kinds and not (a < C and b < C):
                lone = (a, b)
                break
        if lone:
            break

    def slot(i, j, kind):
        return not (kind == EQ and i < C and j < C)

    def n_slot_terms():
        return sum(1 for (i, j), s in tm.kinds.items() for kd in s if slot(i, j, kd))

    def carrier_set():
        return {v for (i, j), s in tm.kinds.items() for kd in s if slot(i, j, kd) for v in (i, j)}

    hub = None
    if carriers is not None:
        assert C >= 2
        free = [c for c in range(C - 1) if c not in carrier_set()][::-1]
        need = carriers - len(carrier_set())
        assert 0 <= need <= len(free), (need, len(free))
        while need >= 2:
            a, b = free.pop(), free.pop()
            tm.add(a, b, LOWER)
            need -= 2
        if need:
            tm.add(free.pop(), C - 1, LOWER)
    if per_node is not None:            # a hub among the other nodes: exactly per_node slot terms
        hub = C + (N - C) // 2
        _fill_hub(tm, hub, per_node, [v for v in _by_distance(hub, N) if v >= C], cap=per_node - 1)
    if busiest is not None:
        hub = N // 2
        _fill_hub(tm, hub, busiest, _by_distance(hub, N), cap=busiest)
    if outside is not None:
        have = carrier_set()
        cap = (per_node - 1) if per_node is not None else 12
        pool = [(a, a + s) for s in (1, 2, 3, 4) for a in sorted(have) if a + s < N and a + s in have]
        pool = [(a, b) for a, b in pool if (a, b) not in equal_pairs and (a, b) != lone and not (a < C and b < C)]
        for kind in (LOWER, UPPER, EQ):
            for a, b in pool:
                if n_slot_terms() >= outside:
                    break
                if tm.has(a, b, kind) or a == hub or b == hub or tm.count(a, slot) >= cap or tm.count(b, slot) >= cap:
                    continue
                if kind == EQ and (a < C or b < C):
                    continue
                tm.add(a, b, kind)
        assert n_slot_terms() == outside, (n_slot_terms(), outside)

    Dp = ((P[:, None, :] - P[None, :, :]) ** 2).sum(-1)
    omega, psi_L, psi_U = np.zeros((N, N)), np.zeros((N, N)), np.zeros((N, N))
    for (i, j), s in tm.kinds.items():
        for kind in s:
            if kind == EQ:
                omega[i, j] = omega[j, i] = 1.0
            elif (i, j) in equal_pairs:
                psi_L[i, j] = psi_L[j, i] = psi_U[i, j] = psi_U[j, i] = Dp[i, j]
            elif kind == LOWER:
                psi_L[i, j] = psi_L[j, i] = Dp[i, j] * rng.uniform(0.4, 0.8)
            else:
                psi_U[i, j] = psi_U[j, i] = Dp[i, j] * rng.uniform(1.25, 2.0)
    if lone is not None:
        a, b = lone
        psi_L[a, b] = psi_L[b, a] = psi_U[a, b] = psi_U[b, a] = 1.1 * Dp[a, b]
    D = Dp.copy()
    if scaled:
        S = rng.uniform(0.9, 1.1, size=(N, N))
        D = Dp * np.triu(S, 1) + (Dp * np.triu(S, 1)).T
    return omega, psi_L, psi_U, D, P


def _by_distance(hub, N):
    return sorted((v for v in range(N) if v != hub), key=lambda v: (abs(v - hub), v))


def _fill_hub(tm, hub, want, others, cap):
    """Terms hub - v, v nearest first, kinds EQ, LOWER, UPPER per pair, until the hub has `want`;
    no other node is taken beyond `cap` terms."""
    for v in others:
        for kind in (EQ, LOWER, UPPER):
            if tm.count(hub) >= want:
                return
            if not tm.has(hub, v, kind) and tm.count(v) < cap:
                tm.add(hub, v, kind)
    assert tm.count(hub) == want, (tm.count(hub), want)


def term_counts(omega, psi_L, psi_U, clique=0):
    """What engine.build_terms makes of a graph: terms, busiest node, terms outside the clique
    (everything but the clique's equalities), nodes that carry them, and their busiest node."""
    from graphik_amd.engine import build_terms
    ti, tj, tk, _ = build_terms(omega, psi_L, psi_U, True)
    N = omega.shape[0]
    deg = np.bincount(np.concatenate([ti, tj]), minlength=N)
    out = ~((tk == EQ) & (ti < clique) & (tj < clique))
    sdeg = np.bincount(np.concatenate([ti[out], tj[out]]), minlength=N)
    return {"T": len(ti), "busiest": int(deg.max()), "outside": int(out.sum()), "carriers": int((sdeg > 0).sum()),
            "per_node": int(sdeg[clique:].max()) if N > clique else 0, "pairs": set(zip(ti.tolist(), tj.tolist()))}


# ---- the boundary cases ----------------------------------------------------------------------
def _info(kind, **kw):
    base = {"wave3": dict(is_block=0, node_per_lane=0, problems_per_wave=1, hessian_form=1),
            "wave3c": dict(is_block=0, node_per_lane=0, problems_per_wave=1, hessian_form=0),
            "wave2": dict(is_block=0, node_per_lane=0, problems_per_wave=1, hessian_form=0),
            "quad": dict(is_block=0, node_per_lane=0, problems_per_wave=4, hessian_form=0),
            "block": dict(is_block=1, max_terms_per_node=0, node_per_lane=0, problems_per_wave=0, hessian_form=1),
            "npt2": dict(is_block=1, max_terms_per_node=0, node_per_lane=2, problems_per_wave=0, hessian_form=1),
            "npt1": dict(is_block=1, max_terms_per_node=0, node_per_lane=1, problems_per_wave=0, hessian_form=1),
            "npt4": dict(is_block=1, max_terms_per_node=0, node_per_lane=4, problems_per_wave=0, hessian_form=1)}[kind]
    return dict(base, **kw)


def _strict(D):
    return [f"rtr_wave_kernel<3,{D},W_THETA1|W_PER_EDGE>", f"kat_wave_kernel<3,{D},W_PER_EDGE>"]


def _column(D):
    return [f"rtr_wave_kernel<3,{D},W_THETA1>", f"kat_wave_kernel<3,{D}>"]


CASES = {}


def _case(cid, k, N, graph, info, reaches, params=None, counts=None, **extra):
    assert cid not in CASES
    CASES[cid] = dict(k=k, N=N, graph=graph, info=info, reaches=reaches, params=params or {}, counts=counts or {},
                      **extra)


# k = 3, one unknown per lane: N * k <= 64, busiest node 9 / 10 slots (11: the workgroup kernels)
for D in (9, 10):
    mt = dict(max_terms_per_node=D)
    _case(f"w3_n21_d{D}", 3, 21, dict(busiest=D), _info("wave3", **mt), _strict(D), counts=dict(busiest=D))
    _case(f"w3_n21_d{D}_column", 3, 21, dict(busiest=D), _info("wave3c", **mt), _column(D),
          params={"hessian_form": "column"}, counts=dict(busiest=D))
    _case(f"w3_d{D}_cg", 3, 21, dict(busiest=D), _info("wave3c", **mt), [f"rcg_wave_kernel<3,{D}>", f"kat_wave_kernel<3,{D}>"],
          params={"solver": "ConjugateGradient"}, counts=dict(busiest=D))
    for th, ka, tag in ((0.5, 0.2, "theta05"), (2.0, 0.5, "theta2")):
        _case(f"w3_d{D}_{tag}", 3, 21, dict(busiest=D, seed=3), _info("wave3", **mt),
              [f"rtr_wave_kernel<3,{D},W_PER_EDGE>", f"kat_wave_kernel<3,{D},W_PER_EDGE>"],
              params={"theta": th, "kappa": ka}, counts=dict(busiest=D))
        _case(f"w3_d{D}_column_{tag}", 3, 21, dict(busiest=D, seed=3), _info("wave3c", **mt),
              [f"rtr_wave_kernel<3,{D},0>", f"kat_wave_kernel<3,{D}>"],
              params={"theta": th, "kappa": ka, "hessian_form": "column"}, counts=dict(busiest=D))
_case("w3_n21_d9_scaled", 3, 21, dict(busiest=9, scaled=True, seed=5), _info("wave3", max_terms_per_node=9), _strict(9),
      counts=dict(busiest=9))
_case("w3_n21_d11", 3, 21, dict(busiest=11), _info("block"), ["rtr_block_kernel<3>", "kat_block_kernel<3>"],
      counts=dict(busiest=11))

# k = 3 beyond one wavefront: the node-per-lane kernel (TrustRegions, theta = 1) or the workgroup kernels
_case("b3_n22", 3, 22, dict(), _info("npt2"), ["rtr_npt_kernel<1,1,2,false>", "kat_npt_kernel<1,1,2,false>"])
_case("b3_n22_cg", 3, 22, dict(), _info("block"), ["rcg_block_kernel<3>", "kat_block_kernel<3>"],
      params={"solver": "ConjugateGradient", "maxiter": 400})
_case("b3_n22_theta2", 3, 22, dict(), _info("block"), ["rtr_block_kernel<3>", "kat_block_kernel<3>"],
      params={"theta": 2.0, "kappa": 0.5})
_case("b3_n127", 3, 127, dict(outside=140), _info("npt2"), ["rtr_npt_kernel<4,1,2,false>", "kat_npt_kernel<4,1,2,false>"],
      counts=dict(outside=140, carriers=127))
_case("b3_n128", 3, 128, dict(outside=140), _info("block"), ["rtr_block_kernel<3>", "kat_block_kernel<3>"],
      counts=dict(outside=140, carriers=128))
for N in (127, 128):
    _case(f"b3_n{N}_clq", 3, N, dict(clique=100), _info("npt2", n_clique=100),
          ["rtr_npt_kernel<1,1,2,false>", "kat_npt_kernel<1,1,2,false>"], counts=dict(carriers=N - 99))
_case("b3_n129_clq", 3, 129, dict(clique=100), _info("npt4", n_clique=100),
      ["rtr_npt_kernel<1,1,4,true>", "kat_npt_kernel<1,1,4,true>"], counts=dict(carriers=30), maxiter=40)
_case("b3_n255_clq", 3, 255, dict(clique=200, outside=120), _info("npt4", n_clique=200),
      ["rtr_npt_kernel<4,1,4,true>", "kat_npt_kernel<4,1,4,true>"], counts=dict(outside=120, carriers=56), maxiter=40)

# node-per-lane limits on N = 100 (clique of 40: 61 busy nodes, no helper lanes): terms outside the clique (TL 1 -> 4 at
# 65, refused beyond 256), per node (16), direction rows (127); debug_flags 2048: one wavefront, two nodes per lane
_NPL = dict(clique=40)
for out, var in ((64, "<1,1,2,false>"), (65, "<4,1,2,false>"), (256, "<4,1,2,false>")):
    for forced in (0, 2):
        _case(f"npt_out{out}" + ("_forced" if forced else ""), 3, 100, dict(_NPL, outside=out), _info("npt2", n_clique=40),
              [f"rtr_npt_kernel{var}", f"kat_npt_kernel{var}"], params={"force_block_path": forced} if forced else {},
              counts=dict(outside=out))
_case("npt_out257", 3, 100, dict(_NPL, outside=257), _info("block", n_clique=40), ["rtr_block_kernel<3>", "kat_block_kernel<3>"],
      counts=dict(outside=257))
_case("npt_per_node16", 3, 100, dict(_NPL, per_node=16), _info("npt2", n_clique=40),
      ["rtr_npt_kernel<1,1,2,false>", "kat_npt_kernel<1,1,2,false>"], counts=dict(per_node=16))
_case("npt_per_node17", 3, 100, dict(_NPL, per_node=17), _info("block", n_clique=40),
      ["rtr_block_kernel<3>", "kat_block_kernel<3>"], counts=dict(per_node=17))
_case("npt_rows127", 3, 128, dict(_NPL, carriers=127), _info("npt2", n_clique=40),
      ["rtr_npt_kernel<4,1,2,false>", "kat_npt_kernel<4,1,2,false>"], counts=dict(carriers=127))
_case("npt_rows128", 3, 128, dict(_NPL, carriers=128), _info("block", n_clique=40),
      ["rtr_block_kernel<3>", "kat_block_kernel<3>"], counts=dict(carriers=128))
_case("npt_2048_out64", 3, 100, dict(_NPL, outside=64), _info("npt1", n_clique=40),
      ["rtr_npt_kernel<1,2,1,false>", "kat_npt_kernel<1,2,1,false>"], params={"debug_flags": 2048}, counts=dict(outside=64))
_case("npt_2048_out65", 3, 100, dict(_NPL, outside=65), _info("npt1", n_clique=40),
      ["rtr_npt_kernel<4,2,1,false>", "kat_npt_kernel<4,2,1,false>"], params={"debug_flags": 2048}, counts=dict(outside=65))
_case("npt_force1", 3, 100, dict(_NPL, outside=64), _info("block", n_clique=40), ["rtr_block_kernel<3>", "kat_block_kernel<3>"],
      params={"force_block_path": 1}, counts=dict(outside=64))

# k = 2: N * k <= 64 and N <= 32; slot counts 6 / 16 / 31 (32: the workgroup kernels); the four-problem kernel up to 16 nodes
for D, slots, N in ((6, 6, 17), (7, 16, 24), (16, 16, 24), (17, 31, 32), (31, 31, 32)):
    _case(f"w2_d{D}", 2, N, dict(busiest=D), _info("wave2", max_terms_per_node=slots),
          [f"rtr_wave_kernel<2,{slots},W_THETA1>", f"kat_wave_kernel<2,{slots}>"], counts=dict(busiest=D))
_case("w2_d32", 2, 32, dict(busiest=32), _info("block"), ["rtr_block_kernel<2>", "kat_block_kernel<2>"], counts=dict(busiest=32))
_case("w2_n32", 2, 32, dict(busiest=6), _info("wave2", max_terms_per_node=6), ["rtr_wave_kernel<2,6,W_THETA1>", "kat_wave_kernel<2,6>"],
      counts=dict(busiest=6))
_case("w2_n33", 2, 33, dict(busiest=6), _info("block"), ["rtr_block_kernel<2>", "kat_block_kernel<2>"], counts=dict(busiest=6))
_case("w2_n33_cg", 2, 33, dict(busiest=6), _info("block"), ["rcg_block_kernel<2>", "kat_block_kernel<2>"],
      params={"solver": "ConjugateGradient"}, counts=dict(busiest=6))
_case("w2_n16_quad", 2, 16, dict(busiest=6), _info("quad", max_terms_per_node=6), ["rtr_quad_kernel<6>", "kat_quad_kernel<6>"],
      params={"debug_flags": 16384}, counts=dict(busiest=6))
_case("w2_n16_wave", 2, 16, dict(busiest=6), _info("wave2", max_terms_per_node=6), ["rtr_wave_kernel<2,6,W_THETA1>", "kat_wave_kernel<2,6>"],
      params={"debug_flags": 8192}, counts=dict(busiest=6))
_case("w2_d16_scaled", 2, 24, dict(busiest=16, scaled=True, seed=5), _info("wave2", max_terms_per_node=16),
      ["rtr_wave_kernel<2,16,W_THETA1>", "kat_wave_kernel<2,16>"], counts=dict(busiest=16))
for D, N in ((6, 17), (16, 24), (31, 32)):
    mt = dict(max_terms_per_node=D)
    _case(f"w2_d{D}_cg", 2, N, dict(busiest=D), _info("wave2", **mt), [f"rcg_wave_kernel<2,{D}>", f"kat_wave_kernel<2,{D}>"],
          params={"solver": "ConjugateGradient"}, counts=dict(busiest=D))
    for th, ka, tag in ((0.5, 0.2, "theta05"), (2.0, 0.5, "theta2")):
        _case(f"w2_d{D}_{tag}", 2, N, dict(busiest=D, seed=3), _info("wave2", **mt),
              [f"rtr_wave_kernel<2,{D},0>", f"kat_wave_kernel<2,{D}>"], params={"theta": th, "kappa": ka},
              counts=dict(busiest=D))

# ragged batches, every sampled problem against itself alone.  Tail spreading (the *_mig builds): more problems than
# resident waves at more than four waves per CU -- waves_per_cu = 8, B = 8 * n_cu + 37; debug_flags 512 turns it off.
# The four-problem kernel: below / above its batch-size switch (12 problems per CU).
BATCH_CASES = {
    "mig_d9": dict(graph="w3_n21_d9", params={}, reaches=["rtr_wave_kernel<3,9,W_THETA1|W_SPREAD|W_PER_EDGE>"], mig=True),
    "mig_d9_column": dict(graph="w3_n21_d9_column", params={"hessian_form": "column"},
                          reaches=["rtr_wave_kernel<3,9,W_THETA1|W_SPREAD>"], mig=True),
    "mig_d10": dict(graph="w3_n21_d10", params={}, reaches=["rtr_wave_kernel<3,10,W_THETA1|W_SPREAD|W_PER_EDGE>"], mig=True),
    # (<3, 10> has no column-form tail-spreading build: the same batch runs on the plain one, nothing moves)
    "mig_d10_column": dict(graph="w3_n21_d10_column", params={"hessian_form": "column"}, reaches=_column(10)[:1], mig=False),
    "mig_d10_off": dict(graph="w3_n21_d10", params={"debug_flags": 512}, reaches=_strict(10)[:1], mig=False),
    "quad_below": dict(graph="w2_n16_quad", params={}, reaches=["rtr_wave_kernel<2,6,W_THETA1>"], quad=-1),
    "quad_above": dict(graph="w2_n16_quad", params={}, reaches=["rtr_quad_kernel<6>"], quad=3),
}

# refused shapes: (graph of a case or explicit, params, a phrase of the error)
REFUSED = {
    "r_n256": dict(k=3, N=256, graph=dict(clique=200), params={}, match="N must be in"),
    "r_k2_n129": dict(k=2, N=129, graph=dict(busiest=6), params={}, match="more than 128 nodes run on the node-per-lane kernel only"),
    "r_n129_cg": dict(k=3, N=129, graph=dict(clique=100), params={"solver": "ConjugateGradient"},
                      match="more than 128 nodes run on the node-per-lane kernel only"),
    "r_n129_theta": dict(k=3, N=129, graph=dict(clique=100), params={"theta": 0.5},
                         match="more than 128 nodes run on the node-per-lane kernel only"),
    "r_n129_force1": dict(k=3, N=129, graph=dict(clique=100), params={"force_block_path": 1},
                          match="more than 128 nodes run on the node-per-lane kernel only"),
    "r_n200_out257": dict(k=3, N=200, graph=dict(clique=100, outside=257), params={},
                          match="at most 256 terms outside the rigid clique"),
    "r_n129_noclq": dict(k=3, N=129, graph=dict(outside=140), params={}, match="at most 127 nodes that carry such terms"),
    "r_force2_out257": dict(k=3, N=100, graph=dict(_NPL, outside=257), params={"force_block_path": 2},
                            match="at most 256 terms outside the rigid clique"),
    "r_force2_per_node17": dict(k=3, N=100, graph=dict(_NPL, per_node=17), params={"force_block_path": 2},
                                match="at most 16 per lane"),
    "r_force2_rows128": dict(k=3, N=128, graph=dict(_NPL, carriers=128), params={"force_block_path": 2},
                             match="node-per-lane kernel: k = 3"),
}

# instantiations that the existing suite reaches (anchored formulation, prepare kernels): named, not re-tested
_PREP_HOST = "tests/test_prepare_boundaries_gpu.py::test_prepare_against_the_host"
_PREP_MULTI = "tests/test_prepare_boundaries_gpu.py::test_a_workgroup_that_takes_more_than_one_goal"
_HINGE_TWIN = "tests/test_anchored_hinge_twin_gpu.py::test_solve_against_the_numpy_twin"
_SELF_SCENES = "tests/test_anchored_self_hinges_gpu.py::test_scenes_are_bit_identical_to_their_own_templates"
_HALF_SCENES = "tests/test_anchored_halfspaces_gpu.py::test_scenes_are_bit_identical_to_their_own_templates"
EXISTING = {
    "rtr_wave_kernel<3,9,W_THETA1|W_ANCH>": ["tests/test_hip_gpu.py::test_anchored_trajectory_against_oracle",
                                             "tests/test_hip_gpu.py::test_anchored_pipeline"],
    "kat_wave_kernel<3,9,W_ANCH>": ["tests/test_hip_gpu.py::test_anchored_kernel_known_answers"],
    # ... with link hinges (UR10 + table, AnchoredProblem(link_hinges=True))
    "rtr_wave_kernel<3,9,W_THETA1|W_ANCH|W_LINKS>": [_HINGE_TWIN,
                                                     "tests/test_anchored_link_hinges_gpu.py::test_the_blind_spot_closes",
                                                     "tests/test_anchored_link_hinges_gpu.py::test_the_new_kernel_group_is_what_the_hinge_template_runs"],
    "kat_wave_kernel<3,9,W_ANCH|W_LINKS>": ["tests/test_anchored_link_hinges_gpu.py::test_link_hinge_known_answers"],
    # ... the scene entries: the synthetic cases near9 / a20_full of tests/synth_anchored_scenes.py (9 and 20 slots, asserted
    # there through info), and UR10 with hinges
    "rtr_wave_scene_kernel<3,9,W_THETA1|W_ANCH>": ["tests/test_anchored_scenes_gpu.py::test_template_level_bit_identity",
                                                   "tests/test_anchored_scenes_gpu.py::test_a_wave_changes_scene_between_problems"],
    "rtr_wave_scene_kernel<3,20,W_THETA1|W_ANCH>": ["tests/test_anchored_scenes_gpu.py::test_template_level_bit_identity",
                                                    "tests/test_anchored_scenes_gpu.py::test_a_wave_changes_scene_between_problems"],
    "rtr_wave_scene_kernel<3,9,W_THETA1|W_ANCH|W_LINKS>": ["tests/test_anchored_scenes_gpu.py::test_ur10_three_scenes"],
    # the self-hinge and half-space groups (GIK_KERNELS_ANCH_SELF, GIK_KERNELS_ANCH_HALF): the solve
    # builds against the numpy trust-region twin (HINGE_TWIN_CASES below names the cases), the known-answer builds against
    # numpy, the scene builds bit-identical to their own templates
    "rtr_wave_kernel<3,9,W_THETA1|W_ANCH|W_SELF>": [_HINGE_TWIN],
    "rtr_wave_kernel<3,9,W_THETA1|W_ANCH|W_LINKS|W_SELF>": [_HINGE_TWIN],
    "rtr_wave_kernel<3,9,W_THETA1|W_ANCH|W_HALF>": [_HINGE_TWIN],
    "rtr_wave_kernel<3,9,W_THETA1|W_ANCH|W_LINKS|W_HALF>": [_HINGE_TWIN],
    "kat_wave_kernel<3,9,W_ANCH|W_SELF>": ["tests/test_anchored_self_hinges_gpu.py::test_self_hinge_known_answers"],
    "kat_wave_kernel<3,9,W_ANCH|W_LINKS|W_SELF>": ["tests/test_anchored_self_hinges_gpu.py::test_self_hinge_known_answers"],
    "kat_wave_kernel<3,9,W_ANCH|W_HALF>": ["tests/test_anchored_halfspaces_gpu.py::test_halfspace_known_answers"],
    "kat_wave_kernel<3,9,W_ANCH|W_LINKS|W_HALF>": ["tests/test_anchored_halfspaces_gpu.py::test_halfspace_known_answers"],
    "rtr_wave_scene_kernel<3,9,W_THETA1|W_ANCH|W_SELF>": [_SELF_SCENES],
    "rtr_wave_scene_kernel<3,9,W_THETA1|W_ANCH|W_LINKS|W_SELF>": [_SELF_SCENES],
    "rtr_wave_scene_kernel<3,9,W_THETA1|W_ANCH|W_HALF>": [_HALF_SCENES],
    "rtr_wave_scene_kernel<3,9,W_THETA1|W_ANCH|W_LINKS|W_HALF>": [_HALF_SCENES],
    # the prepare kernels: against the host restatement at every size boundary (the case table of tests/synth_prepare.py,
    # tests/test_prepare_boundaries_host.py keeps it complete), and the older kernel-against-kernel comparisons
    "prep_block_kernel<true>": [_PREP_HOST, _PREP_MULTI, "tests/test_hip_gpu.py::test_block_prepare_kernel_equals_wave_kernel"],
    "prep_block_kernel<false>": [_PREP_HOST, _PREP_MULTI, "tests/test_hip_gpu.py::test_block_prepare_kernel_equals_wave_kernel"],
    "prep_block_kernel<false,PREP_BIGN>": [_PREP_HOST, _PREP_MULTI,
                                           "tests/test_hip_gpu.py::test_scene_with_200_spheres_beyond_128_nodes"],
    "prep_quad_kernel<13>": [_PREP_HOST, _PREP_MULTI, "tests/test_hip_gpu.py::test_quad_prepare_kernel_against_wave_kernel"],
    "prep_quad_kernel<0>": [_PREP_HOST, _PREP_MULTI,
                            "tests/test_hip_gpu.py::test_planar_chains_of_other_sizes_on_the_quad_kernels"],
}
# the solve builds with hinges -> the cases of tests/test_anchored_hinge_twin_host.py that pin them against the numpy twin
HINGE_TWIN_CASES = {
    "rtr_wave_kernel<3,9,W_THETA1|W_ANCH|W_LINKS>": ["links"],
    "rtr_wave_kernel<3,9,W_THETA1|W_ANCH|W_SELF>": ["self"],
    "rtr_wave_kernel<3,9,W_THETA1|W_ANCH|W_LINKS|W_SELF>": ["self_links"],
    "rtr_wave_kernel<3,9,W_THETA1|W_ANCH|W_HALF>": ["half", "half8"],
    "rtr_wave_kernel<3,9,W_THETA1|W_ANCH|W_LINKS|W_HALF>": ["half_links"],
}
# compiled but outside this matrix on purpose, with the reason (none at present: the 20-slot anchored kernels are
# reached through tests/synth_anchored.py's case table)
OUT_OF_SCOPE = {}


def coverage():
    """instantiation -> the case ids (or existing tests) that reach it."""
    cov = {}
    for cid, c in CASES.items():
        for inst in c["reaches"]:
            cov.setdefault(inst, []).append(cid)
    for cid, c in BATCH_CASES.items():
        for inst in c["reaches"]:
            cov.setdefault(inst, []).append(cid)
    import synth_anchored       # (here: it imports this module's builder)
    for cid, c in synth_anchored.CASES.items():
        for inst in c["reaches"]:
            cov.setdefault(inst, []).append("anchored:" + cid)
    for inst, tests in EXISTING.items():
        cov.setdefault(inst, []).extend(tests)
    for inst, why in OUT_OF_SCOPE.items():
        cov.setdefault(inst, []).append("out of scope: " + why)
    return cov


def macro_body(name, text=None):
    """The replacement text of `#define <name>(X) ...` in gik_instances.h (or `text`), continuation lines included."""
    if text is None:
        with open(INSTANCES_H) as f:
            text = f.read()
    m = re.search(rf"#define\s+{name}\(X\)((?:[^\n]*\\\n)*[^\n]*)", text)
    assert m, name + " not found"
    return m.group(1)


def group_members(name, text=None):
    """The instantiations of the group `#define <name>(X)`, in its order and without blanks:
    'rtr_wave_kernel<3,9,W_THETA1>' etc."""
    return [re.sub(r"\s+", "", s) for s in re.findall(r"X\(\s*void\s+(\w+\s*<[^>]*>)\s*\(", macro_body(name, text))]


def compiled_instances(text=None):
    """The instantiations GIK_ALL_KERNELS expands to (gik_instances.h): the members of every group it names."""
    out = []
    for g in re.findall(r"(GIK_KERNELS_\w+)\(X\)", macro_body("GIK_ALL_KERNELS", text)):
        out += group_members(g, text)
    return out
