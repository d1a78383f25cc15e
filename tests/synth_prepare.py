"""Problem graphs at every size boundary of the device prepare (plan_prepare in graphik_amd/csrc/gik_plan.h, and the two
size rules inside prep_block_kernel), and the table of which prepare kernel and which in-kernel path each one reaches.

Plain module (numpy at import, the host layer inside the builders; no torch, no GPU): tests/test_prepare_boundaries_host.py
proves on the CPU that every graph sits where its row says, tests/test_prepare_boundaries_gpu.py runs the same rows on the
device against host_reference() below -- the host restatement, never another kernel.

Three families.
  planar L   a planar chain of L links of lengths 0.5 + 0.1 (i mod 7), limits +-pi/2: N = L + 3 nodes, three anchors.  The
             Gram matrix of its D_rand has numerical rank N - 1, so N = 65 is the range compression at its cap (r = 64 =
             PREP_RMAX) and N = 66 the fallback behind it (range_basis_blk returns -1).  MDS's 1e-8 threshold is absolute:
             the lengths are not to be rescaled.
  ur10 S     UR10 with S spheres of radius 0.1: N = 16 + S nodes, 4 + S anchors, Gram rank min(N - 1, 23).
  chain40 S  the 40-joint 3-D chain of tests/test_hip_gpu.py (N = 84) with S spheres: two goals.

The boundaries (BOUNDARIES below) and what is unreachable from Python:
  * N = 129 on a planar chain (126 links): template creation refuses a 2-D graph of more than 128 nodes, so the planar
    family stops at the five-matrix slab; N = 129 and beyond are reached by the sphere scenes alone.
  * prep_block_kernel<false, PREP_BIGN>'s refusal of more than 128 MDS columns (K_out = -1, Y_init = NaN): the one graph
    of more than 128 nodes with a Gram rank above 64 that creation accepts, a 40-joint 3-D chain with 45 spheres
    (N = 129, "chain40_n129": rank 113 and 120, the slow full decomposition behind the compression), has 57 and 61
    columns, about half its rank as on every graph here; the solve side takes at most 127 nodes outside the rigid clique
    of such a graph, so no input with more than 128 columns is known.
  * n_anchor > 32 at N <= 32 cannot occur (anchors are nodes, two more are the goal's).
"""
import numpy as np

# what the kernels compile in (gik_args.h, gik_prep.hip.h); tests/test_prepare_boundaries_host.py reads the headers
# and asserts these are still their values
PREPQ_MAXN, WAVE_MAXN, PREP_COMPRESS_MIN_N, PREP_RMAX, PREP_MAXN, PREP_BIGN = 16, 32, 48, 64, 128, 256
LDS_MAXN = 123                    # largest N whose work matrix fits in LDS next to the kernel's static arrays

VARIANTS = ["quad13", "quad", "wave", "block_lds", "block", "block_big"]      # enum class Prep, in its order
KERNEL = {"quad13": "prep_quad_kernel<13>", "quad": "prep_quad_kernel<0>", "wave": "prep_wave_kernel",
          "block_lds": "prep_block_kernel<true>", "block": "prep_block_kernel<false>",
          "block_big": "prep_block_kernel<false,PREP_BIGN>"}
ENV_FACT = {"GIK_NO_PREP_QUAD": "env_no_quad", "GIK_PREP_NO_COMPRESS": "env_no_compress", "GIK_PREP_A_GLOBAL": "env_a_global"}

# every size named by the issue of this table: the first / last graph of a kernel or of a path inside one
BOUNDARIES = {
    17: "the first graph of prep_wave_kernel", 32: "the last wave graph", 33: "the first block graph",
    47: "the last graph without the range compression", 48: "the compression switches on",
    65: "the rank reaches PREP_RMAX", 66: "the rank exceeds PREP_RMAX: fallback",
    123: "the last work matrix in LDS", 124: "the work matrix moves to the global slab",
    128: "the last five-matrix slab, LDS arrays of 128 rows", 129: "six matrices, LDS arrays of 256 rows",
    255: "the last accepted graph", 256: "the first refused graph",
}

CASES = {}        # accepted graphs
REFUSED = {}      # graphs that creation refuses: the message, and what is unreachable because of it


def _path(family, N, variant, env):
    """The in-kernel path of an accepted case: 'plain' (full decomposition by size or by switch), 'compressed r=...'
    or 'fallback' (the compression ran, found more than PREP_RMAX directions and handed the matrix back)."""
    if not variant.startswith("block"):
        return "plain"
    compresses = variant == "block_big" or (variant == "block_lds" and N >= PREP_COMPRESS_MIN_N and
                                            "GIK_PREP_NO_COMPRESS" not in env)
    if not compresses:
        return "plain"
    if family == "chain40":
        return "fallback"      # (rank 113 and 120: tests/test_prepare_boundaries_host.py)
    rank = N - 1 if family == "planar" else min(N - 1, 23)
    return f"compressed r={rank}" if rank <= PREP_RMAX else "fallback"


def _case(family, size, variant, env=()):
    N = size + {"planar": 3, "ur10": 16, "chain40": 84}[family]
    env = {k: "1" for k in env}
    cid = f"{family}_n{N}" + "".join("_" + k.split("_", 1)[1].lower() for k in sorted(env))
    assert cid not in CASES
    CASES[cid] = dict(family=family, size=size, N=N, env=env, variant=variant, path=_path(family, N, variant, env),
                      dim=2 if family == "planar" else 3, n_anchor=3 if family == "planar" else 4 + size,
                      is_block=int(variant.startswith("block")),
                      goals_per_wave=0 if variant.startswith("block") else (4 if variant.startswith("quad") else 1))


_case("planar", 10, "quad13")
_case("planar", 13, "quad")
_case("ur10", 0, "quad")
for _N in (17, 32):
    _case("planar", _N - 3, "wave")
    _case("ur10", _N - 16, "wave")
_case("planar", 13, "wave", env=["GIK_NO_PREP_QUAD"])
for _N in (33, 47, 48, 65, 66, 123):
    _case("planar", _N - 3, "block_lds")
for _N in (33, 48, 123):
    _case("ur10", _N - 16, "block_lds")
_case("planar", 62, "block_lds", env=["GIK_PREP_NO_COMPRESS"])
for _N in (124, 128):
    _case("planar", _N - 3, "block")
    _case("ur10", _N - 16, "block")
_case("planar", 62, "block", env=["GIK_PREP_A_GLOBAL"])
_case("ur10", 107, "block", env=["GIK_PREP_A_GLOBAL"])
for _N in (129, 255):
    _case("ur10", _N - 16, "block_big")
_case("chain40", 45, "block_big")
# N K = 63 and 66 entries of Y_init on a 3-D graph: the last that one pass of a wavefront's 64 lanes writes, and the first
# that takes two (prep_wave_kernel wrote the first 64 only until these cases and "ur10_n32" found it)
_case("ur10", 5, "wave")
_case("ur10", 6, "wave")

REFUSED["ur10_n256"] = dict(family="ur10", size=240, N=256, dim=3, match="N must be in [2, 255]",
                            unreachable="nothing: 256 is the first size beyond every kernel")
REFUSED["planar_n129"] = dict(family="planar", size=126, N=129, dim=2,
                              match="graphs of more than 128 nodes run on the node-per-lane kernel only",
                              unreachable="N >= 129 on a planar chain (rank N - 1 beyond 128 nodes)")

# one case per variant at its largest N: a workgroup (wavefront) that takes more than one goal
MULTI_GOAL = {"quad13": "planar_n13", "quad": "planar_n16", "wave": "planar_n32", "block_lds": "planar_n123",
              "block": "planar_n128", "block_big": "ur10_n255"}
# the kernels on the other side of the solve (recover_kernel, seed_kernel) on the same graphs
RECOVER_SEED = ["planar_n17", "planar_n33", "planar_n128", "ur10_n17", "ur10_n129", "ur10_n255"]


def gaps(cases=None):
    """What the table fails to cover: prepare variants without a case, boundary sizes without an accepted (256: a
    refused) case, variants without a multi-goal case.  Empty when the table is complete."""
    cases = CASES if cases is None else cases
    out = [f"variant {v}" for v in VARIANTS if not any(c["variant"] == v for c in cases.values())]
    for N in sorted(BOUNDARIES):
        pool = REFUSED if N == 256 else cases
        if not any(c["N"] == N and not c.get("env") for c in pool.values()):      # (on the default plan, no switch)
            out.append(f"boundary N = {N}")
    for N, path in ((65, f"compressed r={PREP_RMAX}"), (66, "fallback"), (47, "plain")):
        if not any(c["N"] == N and c["path"] == path and not c["env"] for c in cases.values()):
            out.append(f"path {path} at N = {N}")
    out += [f"multi-goal {v}" for v in VARIANTS if MULTI_GOAL.get(v) not in cases or cases[MULTI_GOAL[v]]["variant"] != v]
    return out


def coverage():
    """kernel instantiation -> the case ids that reach it (synth_graphs.coverage's form)."""
    cov = {}
    for cid, c in CASES.items():
        cov.setdefault(KERNEL[c["variant"]], []).append("prepare:" + cid)
    return cov


# ---- the builders ---------------------------------------------------------------------------------
def planar_chain(links):
    from graphik_amd.graphs import ProblemGraphPlanar
    from graphik_amd.robots import RobotPlanar
    from graphik_amd.utils import list_to_variable_dict
    lim = 0.5 * np.pi * np.ones(links)
    robot = RobotPlanar({"link_lengths": list_to_variable_dict(0.5 + 0.1 * (np.arange(links) % 7)),
                         "theta": list_to_variable_dict(np.zeros(links)),
                         "joint_limits_upper": list_to_variable_dict(lim),
                         "joint_limits_lower": list_to_variable_dict(-lim), "num_joints": links})
    return robot, ProblemGraphPlanar(robot)


def _add_spheres(graph, rs, count):
    for i in range(count):
        graph.add_spherical_obstacle(f"o{i}", np.array([1.5, 0, 0]) + rs.rand(3) * np.array([0.5, 3, 2]) - np.array([0, 1.5, 0]), 0.1)


def chain40():
    """The 40-joint 3-D chain of test_chain_with_more_than_31_joints_through_the_device_pipeline (N = 84)."""
    from graphik_amd.graphs import ProblemGraphRevolute
    from graphik_amd.robots import RobotRevolute
    n = 40
    rs = np.random.RandomState(0)
    names = [f"p{i}" for i in range(1, n + 1)]
    params = {"a": dict(zip(names, 0.1 + 0.2 * rs.rand(n))), "alpha": dict(zip(names, rs.choice([0, np.pi / 2, -np.pi / 2], n))),
              "d": dict(zip(names, 0.1 * rs.rand(n))), "theta": dict(zip(names, np.zeros(n))), "modified_dh": False,
              "num_joints": n}
    robot = RobotRevolute(params)
    return robot, ProblemGraphRevolute(robot)


def build(c):
    """(robot, graph, T_goal [8, d + 1, d + 1]) of a case or refused row: the seeds and the order of the draws are part
    of the table (spheres first, then the goals, from RandomState(size))."""
    rs = np.random.RandomState(c["size"])
    if c["family"] == "planar":
        robot, graph = planar_chain(c["size"])
        lb, ub = robot.limits_arrays()
        Q = lb + (ub - lb) * rs.rand(8, c["size"])
    elif c["family"] == "ur10":
        from graphik_amd.utils.roboturdf import load_ur10
        robot, graph = load_ur10()
        _add_spheres(graph, rs, c["size"])
        Q = -np.pi + 2 * np.pi * rs.rand(8, robot.n)
    else:
        robot, graph = chain40()
        _add_spheres(graph, rs, c["size"])
        lb, ub = robot.limits_arrays()
        Q = lb + (ub - lb) * rs.rand(2, robot.n)
    assert graph.number_of_nodes() == c["N"], (graph.number_of_nodes(), c["N"])
    return robot, graph, robot.fk_batch(Q), Q


_REF = {}


def host_reference(cid):
    """The host restatement of prepare for a case's eight goals, computed once per process and left unchanged:
    BatchProblem(host_only).assemble -> floyd_warshall_bounds -> gram_from_distance_matrix -> generate_initialization_batch
    (canonical signs, with info).  Cases that differ in the environment switch only share one entry."""
    c = CASES[cid]
    key = (c["family"], c["size"])
    if key not in _REF:
        from graphik_amd.solvers.riemannian_solver import BatchProblem
        from graphik_amd.utils import dgp
        robot, graph, Tg, Q = build(c)
        prob = BatchProblem(graph, use_limits=True, host_only=True)
        D, lo, up = prob.assemble(Tg)
        lb, ub = map(np.stack, zip(*(dgp.floyd_warshall_bounds(lo[g], up[g]) for g in range(len(Tg)))))   # (N^3 doubles a goal)
        G = dgp.gram_from_distance_matrix((lb + 0.9 * (ub - lb)) ** 2)
        Y, info = dgp.generate_initialization_batch(lb, ub, graph.dim, prob.omega, canonical=True, return_info=True)
        ref = dict(robot=robot, graph=graph, prob=prob, Tg=Tg, Q=Q, D=D, targets=prob.targets_from_D(D), lb=lb, ub=ub, gram=G,
                   ev_gram=np.linalg.eigvalsh(G), Y=Y, info=info, n_anchor=len(prob.anchor_nodes))
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def gram_rank(ref):
    """Per goal: the numerical rank of the host Gram matrix at 1e-13 |B|_F (eigenvalues by magnitude), and the ratio of
    the smallest counted eigenvalue to that threshold."""
    ev = np.abs(ref["ev_gram"])
    thr = 1e-13 * np.linalg.norm(ref["gram"], axis=(1, 2))
    counted = ev > thr[:, None]
    return counted.sum(axis=1), np.where(counted, ev, np.inf).min(axis=1) / thr


def leading_gap(ref, m):
    """Per goal: the ratio of the m-th largest eigenvalue (by magnitude) of the host Gram matrix to 1e-13 |B|_F."""
    ev = np.sort(np.abs(ref["ev_gram"]), axis=1)[:, ::-1]
    return ev[:, m - 1] / (1e-13 * np.linalg.norm(ref["gram"], axis=(1, 2)))


def near_threshold(ref):
    """The goals whose MDS column count the host itself takes from an eigenvalue within a factor 4 of 1e-8
    (tests/test_hip_gpu.py: _classify_init)."""
    ev = ref["info"]["ev_rank"]
    return np.any((ev > 0.25e-8) & (ev < 4e-8), axis=1)
