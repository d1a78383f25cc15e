"""Drop-in front end for GraphIK's Riemannian solver
(graphik/solvers/riemannian_solver.py), running on the MI355X engine.

    from graphik_amd.solvers.riemannian_solver import solve_with_riemannian, RiemannianSolver

`solve_with_riemannian(graph, T_goal, use_jit=True)` and `RiemannianSolver(graph, params)
.solve(D_goal, omega, use_limits, bounds, Y_init, jit, output_log)` keep the reference's
signatures and return shapes; `jit` / `use_jit` are accepted and ignored (there is exactly one
implementation: the HIP kernels -- no CPU fallback).  `solve_batch` is the batched entry point
the engine is built for.
"""
import collections
import hashlib
import time

import numpy as np
import torch

from ..engine import (RETRY_CANDIDATE_STEP, Template, _alloc_stats, _decode_stats, anchored_call_plan, build_terms,
                      check_atlas_args, check_atlas_k, check_clearance_mode, check_retry_args, check_retry_candidates,
                      workspace)
from ..utils import dgp
from ..utils.constants import POS
from ..utils.lie import as_matrix

_STOP_REASONS = {0: "Terminated - min grad norm reached", 1: "Terminated - max iterations reached",
                 2: "Terminated - NaN encountered", 3: "Terminated - min stepsize reached"}
# riemannian_solver.py:24-26 (indexable like pymanopt's make_enum: BetaTypes[3] == "HagerZhang")
BetaTypes = ["FletcherReeves", "PolakRibiere", "HestenesStiefel", "HagerZhang"]


# Templates behind the create_cost / create_cost_limits closures: least-recently-used, bounded like
# _PROBLEM_CACHE (a Template owns device tables and a HIP handle), keyed by the device as well, and
# emptied by clear_problem_cache()
_closure_templates = collections.OrderedDict()
_CLOSURE_TEMPLATES_MAX = 8


def _cost_closures(D_goal, omega, psi_L, psi_U, use_limits):
    """The closure triple of create_cost / create_cost_limits on the default device, reference
    solver defaults; one cached Template per (k, masks)."""
    omega = np.asarray(omega, dtype=float)
    psi_L = None if psi_L is None else np.asarray(psi_L, dtype=float)
    psi_U = None if psi_U is None else np.asarray(psi_U, dtype=float)
    D_goal = np.asarray(D_goal, dtype=float)
    state = {}

    def tpl(Y):
        k = int(np.asarray(Y).shape[-1])
        if state.get("k") != k:
            dev = torch.cuda.current_device() if torch.cuda.is_available() else -1
            key = (dev, k, use_limits, omega.tobytes(), None if psi_L is None else psi_L.tobytes(),
                   None if psi_U is None else psi_U.tobytes())
            if key not in _closure_templates:
                _closure_templates[key] = Template.from_matrices(omega, psi_L, psi_U, k=k, use_limits=use_limits)
                while len(_closure_templates) > _CLOSURE_TEMPLATES_MAX:
                    _closure_templates.popitem(last=False)
            else:
                _closure_templates.move_to_end(key)
            state["k"], state["T"] = k, _closure_templates[key]
            state["tg"] = state["T"].targets_from_D(D_goal)
        return state["T"], state["tg"]

    def cost(Y):
        T, tg = tpl(Y)
        return float(T.cost(Y, tg)[0])

    def egrad(Y):
        T, tg = tpl(Y)
        return T.grad(Y, tg)[0].cpu().numpy()

    def ehess(Y, Z):
        T, tg = tpl(Y)
        return T.hess(Y, Z, tg)[0].cpu().numpy()

    return cost, egrad, ehess


class RiemannianSolver:
    def __init__(self, graph, params={}):
        self.params = params
        self.graph = graph
        self.dim = graph.dim
        self.N = graph.number_of_nodes()
        solver_type = params.get("solver", "TrustRegions")
        if solver_type == "TrustRegions":
            # riemannian_solver.py:44-50
            self.tr_params = {"mingradnorm": params.get("mingradnorm", 0.5 * 1e-9),
                              "maxiter": int(params.get("maxiter", 3000)),
                              "theta": params.get("theta", 1.0), "kappa": params.get("kappa", 0.1)}
        elif solver_type == "ConjugateGradient":
            # riemannian_solver.py:51-59: pymanopt's ConjugateGradient (HagerZhang, adaptive line
            # search), on the device like the trust-region solver (rcg_* kernels)
            beta = params.get("beta_type", 3)
            if isinstance(beta, str):
                beta = BetaTypes.index(beta)
            self.tr_params = {"solver": "ConjugateGradient",
                              "mingradnorm": params.get("mingradnorm", 1e-9),
                              "maxiter": int(params.get("maxiter", 10e4)),
                              "minstepsize": params.get("minstepsize", 1e-10),
                              "orth_value": params.get("orth_value", 10e10), "beta_type": int(beta)}
        else:
            raise ValueError("params[\"solver\"] must be one of 'ConjugateGradient', 'TrustRegions'")
        for k in ("maxinner", "mininner", "rho_prime", "rho_regularization", "planar_proj_exact",
                  "force_block_path", "waves_per_cu", "slice_outer_its", "debug_flags",
                  "clique_closed_form", "hessian_form"):
            if k in params:
                self.tr_params[k] = params[k]
        self.device = params.get("device", None)
        self._templates = {}

    # -- statics kept for API parity -----------------------------------------------------------
    @staticmethod
    def generate_initialization(bounds, dim, omega, psi_L=None, psi_U=None):
        """riemannian_solver.py:67-75"""
        return dgp.generate_initialization(bounds, dim, omega)

    def _template(self, omega, psi_L, psi_U, use_limits):
        key = (use_limits, omega.tobytes(), None if psi_L is None else psi_L.tobytes(),
               None if psi_U is None else psi_U.tobytes())
        if key not in self._templates:
            self._templates[key] = Template.from_matrices(
                omega, psi_L, psi_U, k=self.dim, use_limits=use_limits, device=self.device,
                params=self.tr_params)
        return self._templates[key]

    @staticmethod
    def create_cost(D_goal, omega, jit=True):
        """(cost, egrad, ehess) closures like riemannian_solver.py:77-119 (a @staticmethod there too:
        callable on the class), evaluated on the GPU.  The embedding dimension is taken from the
        first point the closures see (Y.shape[1]); templates are cached per process."""
        return _cost_closures(D_goal, omega, None, None, False)

    @staticmethod
    def create_cost_limits(D_goal, omega, psi_L, psi_U, jit=True):
        """riemannian_solver.py:121-176"""
        return _cost_closures(D_goal, omega, psi_L, psi_U, True)

    # -- solve ----------------------------------------------------------------------------------
    def solve(self, D_goal, omega, use_limits=False, bounds=None, Y_init=None, jit=True,
              output_log=True):
        """riemannian_solver.py:178-218.  D_goal / Y_init / bounds may carry a leading batch
        axis; the return value is then a dict of arrays instead of a single final_values dict."""
        omega = np.asarray(omega, dtype=float)
        D_goal = np.asarray(D_goal, dtype=float)
        batched = D_goal.ndim == 3
        if use_limits:
            psi_L, psi_U = self.graph.distance_bound_matrices()
        else:
            psi_L, psi_U = None, None
        if bounds is not None:  # bounds take precedence over Y_init (:197-198)
            lb, ub = np.asarray(bounds[0], dtype=float), np.asarray(bounds[1], dtype=float)
            if lb.ndim == 2:
                Y_init = dgp.generate_initialization((lb, ub), self.dim, omega)
            else:
                Y_init = dgp.generate_initialization_batch(lb, ub, self.dim, omega)
        elif Y_init is None:
            raise Exception("If not using bounds, provide an initialization!")
        T = self._template(omega, psi_L, psi_U, use_limits)
        t0 = time.time()
        res = T.solve(Y_init, T.targets_from_D(D_goal))
        torch.cuda.synchronize(T.device)
        dt = time.time() - t0
        x = res["x"].cpu().numpy()
        B = x.shape[0]
        info = {"x": x, "f(x)": res["f"].cpu().numpy(), "time": np.full(B, dt / B),
                "gradnorm": res["gradnorm"].cpu().numpy(),
                "iterations": res["iterations"].cpu().numpy(),
                "inner_iterations": res["inner_total"].cpu().numpy(),
                "stop": res["stop"].cpu().numpy()}
        if T.solver == "ConjugateGradient":      # pymanopt's final_values carry the last step size
            info["costevals"] = info.pop("inner_iterations")
            info["stepsize"] = res["stepsize"].cpu().numpy()
        if not batched:
            info = {k: (v[0] if k == "x" else v[0].item()) for k, v in info.items()}
            info["stop_reason"] = _STOP_REASONS[int(info["stop"])]
        return info if output_log else info["x"]


# ---------------------------------------------------------------------------------------------
GOAL_KINDS = ("pose", "position")


def goal_kinds(goal, n_ee):
    """The goal= argument -> one kind per end effector: "pose" or "position", or a sequence of those with one entry
    per robot.end_effectors.  ValueError for anything else."""
    kinds = (goal,) * n_ee if isinstance(goal, str) else tuple(goal) if isinstance(goal, (list, tuple, np.ndarray)) else None
    if kinds is None:
        raise ValueError(f"goal must be 'pose', 'position' or a sequence of those, got {goal!r}")
    if len(kinds) != n_ee:
        raise ValueError(f"goal has {len(kinds)} entries for {n_ee} end effector{'s' if n_ee != 1 else ''}")
    for kind in kinds:
        if not isinstance(kind, str) or kind not in GOAL_KINDS:
            raise ValueError(f"unknown goal kind {kind!r}: a goal is 'pose' or 'position'")
    return tuple(str(kind) for kind in kinds)


def goal_poses(goals, kinds, dim, lead=1):
    """The goal array of a problem with position goals as pose arrays, the layout of the device buffers.  `lead` leading
    axes ([B], or [B, L] of a path).  When every end effector is a position: positions [..., d] or [..., n_ee, d], packed
    into identity-rotation poses; pose arrays [..., d+1, d+1] / [..., n_ee, d+1, d+1] are taken as they are (of a position
    end effector's pose only the translation column is read).  ValueError for any other shape."""
    G = np.asarray(goals, dtype=float)
    n_ee, d = len(kinds), dim
    head, tail = G.shape[:lead], G.shape[lead:]
    pose_tails = [(n_ee, d + 1, d + 1)] + ([(d + 1, d + 1)] if n_ee == 1 else [])
    if G.ndim >= lead and tail in pose_tails:
        return G
    if all(kind == "position" for kind in kinds):
        if G.ndim >= lead and tail in [(n_ee, d)] + ([(d,)] if n_ee == 1 else []):
            P = G.reshape(head + (n_ee, d))
            T = np.broadcast_to(np.identity(d + 1), head + (n_ee, d + 1, d + 1)).copy()
            T[..., :d, d] = P
            return T if len(tail) == 2 else T[..., 0, :, :]
    axes = "B, L, " if lead == 2 else "B, "
    want = f"poses [{axes}{f'{n_ee}, ' if n_ee > 1 else ''}{d + 1}, {d + 1}]"
    if all(kind == "position" for kind in kinds):
        want = f"positions [{axes}{d}] or [{axes}{n_ee}, {d}], or " + want
    raise ValueError(f"goal array of shape {list(G.shape)}: expected {want}")


class BatchProblem:
    """Goal-independent data of solve_with_riemannian for one problem graph, prepared once:
    edge template, which squared distances depend on the goal, anchors, limits."""

    def __init__(self, graph, use_limits=True, params=None, device=None, force_block_prepare=False,
                 host_only=False, goal="pose"):
        """host_only: only the goal-independent host data (edge pattern, anchors, limits); no device
        handle is created (term-set construction can then be inspected without a GPU).

        goal: "pose" -- a goal pins p_e and q_e (planar: the end effector and its parent), graph.from_pose -- or
        "position": it pins the point p_e alone, the reference's graph.from_pos({p_e: xyz}); the orientation is free,
        no T_final correction applies to that end effector's last angle and its rotation error is reported as 0.  A
        sequence with one entry per robot.end_effectors mixes the kinds on a tree."""
        self.force_block_prepare = force_block_prepare
        self.graph = graph
        self.robot = graph.robot
        self.dim = graph.dim
        self.use_limits = use_limits
        N = graph.number_of_nodes()
        n = self.robot.n
        self.end_effectors = list(self.robot.end_effectors)
        self.multi_ee = len(self.end_effectors) > 1
        self.goal_kinds = goal_kinds(goal, len(self.end_effectors))
        is_pose = [kind == "pose" for kind in self.goal_kinds]
        ee = self.end_effectors[0]
        # goal nodes and how their positions follow from the goal pose (_pose_goal); a robot with
        # several end effectors (3-D trees) has a (p, q) pair per end effector and takes goals
        # [B, n_ee, 4, 4] in the order of robot.end_effectors.  A position goal pins p_e only.
        if self.dim == 3:
            self.goal_nodes = [graph.index(c + e[1:]) for e, pose in zip(self.end_effectors, is_pose) for c in ("pq" if pose else "p")]
            self._goal_keep = [2 * e_i + s for e_i, pose in enumerate(is_pose) for s in ((0, 1) if pose else (0,))]
        else:
            # planar (graph_planar.py:136-145): a goal pose pins its end effector and the end effector's
            # parent; two end effectors of a tree may share that parent (one goal node then)
            self.goal_nodes, self._goal_src = [], []
            for e_i, e in enumerate(self.end_effectors):
                for is_parent, name in ((0, e), (1, self.robot.parent[e]))[:2 if is_pose[e_i] else 1]:
                    if graph.index(name) not in self.goal_nodes:
                        self.goal_nodes.append(graph.index(name))
                        self._goal_src.append((e_i, is_parent, graph.dist[graph.index(self.robot.parent[e]),
                                                                            graph.index(e)]))
        self.anchor_nodes = [i for i, name in enumerate(graph.node_ids)
                             if POS in graph.nodes[name] and i not in self.goal_nodes]
        self.anchor_pos = np.array([graph.nodes[graph.node_ids[i]][POS] for i in self.anchor_nodes],
                                   dtype=float)
        # a goal instance with a dummy pose gives the complete edge pattern (omega)
        q0 = self.robot.zero_configuration()
        if all(is_pose):
            G0 = graph.from_pose({e: self.robot.pose(q0, e) for e in self.end_effectors})
        else:      # from_pos of what the goals pin: (p_e, q_e) of a pose, p_e of a position
            pinned = {}
            for e, pose in zip(self.end_effectors, is_pose):
                T_e = self.robot.pose(q0, e)
                pinned.update(graph._pose_goal({e: T_e}) if pose else {e: as_matrix(T_e)[:self.dim, self.dim]})
            G0 = graph.from_pos(pinned)
        self.omega = dgp.adjacency_matrix_from_graph(G0)
        self.base_D = dgp.distance_matrix_from_graph(G0)
        self.base_lower = np.where(G0.edge, G0.lower, np.nan)
        self.base_upper = np.where(G0.edge, G0.upper, np.nan)
        if use_limits:
            self.psi_L, self.psi_U = graph.distance_bound_matrices()
        else:
            self.psi_L = self.psi_U = None
        self.N = N
        self.terms = build_terms(self.omega, self.psi_L, self.psi_U, use_limits)   # (i, j, kind, static target)
        if host_only:
            self.template, self.device_pipeline = None, False
            return
        self.template = Template.from_matrices(self.omega, self.psi_L, self.psi_U, k=self.dim,
                                               use_limits=use_limits, device=device, params=params)
        self._attach_device_pipeline()
        # claim order of the solve kernels (gik_template_set_claim_key): the robot's data names its key, params
        # {"claim_order": "on" | "off"} overrides; the library decides per call whether it orders
        mode = (params or {}).get("claim_order", "auto")
        if mode == "on" or (mode == "auto" and getattr(self.robot, "claim_key", None) == "reach"):
            terms = self.claim_key_terms()
            if terms:
                self.template.set_claim_key(terms, np.ones(len(terms)))

    def claim_key_nodes(self):
        """The goal nodes whose distance to the base origin p0 is the goal's reach: the end effectors' points p_e."""
        return [self.graph.index(e) for e in self.end_effectors] if self.dim == 3 else []

    def claim_key_terms(self):
        """Indices of the goal-dependent equality terms (p0, p_e) between the base anchor and the goal nodes of
        claim_key_nodes: their targets are the squared reach of the goal."""
        ti, tj, tk, _ = self.terms
        p0 = self.graph.index("p0")
        pairs = {(min(p0, g), max(p0, g)) for g in self.claim_key_nodes()}
        return [t for t in range(len(ti)) if tk[t] == 1 and (int(ti[t]), int(tj[t])) in pairs]

    def _attach_device_pipeline(self):
        """Hand the goal-independent pre/post-processing data to the device handle."""
        g, T = self.graph, self.template
        n = self.robot.n
        if len(self.anchor_nodes) > 256 or self.N > (255 if self.dim == 3 else 128) or len(self.end_effectors) > 8:
            # beyond the device prepare / recover kernels (N <= 128, 3-D graphs 255; <= 8 end effectors):
            # host pre/post-processing around the device solve
            self.device_pipeline = False
            return
        # Device goal slots: two per end effector.  3-D: (p_e, q_e) = self.goal_nodes in order.  Planar (round 6: trees
        # too): (the end effector, its parent); a parent that an earlier end effector's pose pins already gets an inert
        # slot (-1) -- _pose_goal / BatchProblem keep the first definition.  A position goal: (p_e, -1) in either dimension.
        is_pose = [kind == "pose" for kind in self.goal_kinds]
        position_mask = sum(1 << e for e, pose in enumerate(is_pose) if not pose)
        if self.dim == 3:
            dev_slots = [g.index(c + e[1:]) if c == "p" or pose else -1 for e, pose in zip(self.end_effectors, is_pose) for c in "pq"]
        else:
            dev_slots, seen = [], set()
            for e, pose in zip(self.end_effectors, is_pose):
                for name in (e, self.robot.parent[e]):
                    node = g.index(name)
                    pinned = pose or name == e
                    dev_slots.append(node if pinned and node not in seen else -1)
                    if pinned:
                        seen.add(node)
            if any(dev_slots[2 * e] < 0 for e in range(len(self.end_effectors))):
                self.device_pipeline = False       # (an end effector that is another one's parent: host path)
                return
        goal_slot = {node: sl for sl, node in enumerate(dev_slots) if node >= 0}
        goalset = set(self.goal_nodes)
        slot = {a: s for s, a in enumerate(self.anchor_nodes)}
        G = len(dev_slots)                           # 2 per end effector
        # goal nodes of different end effectors that the goal graph ties by an equality edge
        live = sorted(goal_slot.values())
        pairs = [(a, b) for ia, a in enumerate(live) for b in live[ia + 1:]
                 if self.omega[dev_slots[a], dev_slots[b]] != 0 and np.isnan(g.dist[dev_slots[a], dev_slots[b]])]
        pair_slot = {(dev_slots[a], dev_slots[b]): q for q, (a, b) in enumerate(pairs)}
        term_src = np.full(T.T, -1, dtype=np.int32)
        for t in range(T.T):
            i, j = int(T.term_i[t]), int(T.term_j[t])
            if T.term_kind[t] != 1:
                continue
            for a, gnode in ((i, j), (j, i)):
                if gnode in goalset and a in slot:
                    term_src[t] = slot[a] * G + goal_slot[gnode]
            if (i, j) in pair_slot or (j, i) in pair_slot:
                term_src[t] = G * len(self.anchor_nodes) + pair_slot.get((i, j), pair_slot.get((j, i)))
        static = np.where(np.isnan(T.targets_static), self.base_D[T.term_i, T.term_j],
                          T.targets_static)
        lower = self.base_lower.copy()
        upper = self.base_upper.copy()
        for a in self.anchor_nodes:   # goal edges are re-created per goal on the device
            for gnode in self.goal_nodes:
                lower[a, gnode] = lower[gnode, a] = np.nan
                upper[a, gnode] = upper[gnode, a] = np.nan
        for a, b in pairs:
            ga, gb = dev_slots[a], dev_slots[b]
            lower[ga, gb] = lower[gb, ga] = upper[ga, gb] = upper[gb, ga] = np.nan
        I, J = np.nonzero(np.triu(self.omega))
        T0 = self.robot.T0_array()
        ee_path = np.full((len(self.end_effectors), n + 1), -1, dtype=np.int32)
        for e, ee in enumerate(self.end_effectors):
            path = [int(name[1:]) for name in self.robot.kinematic_map["p0"][ee]]
            ee_path[e, :len(path)] = path
        ee_len, point_axis = None, {}
        if self.dim == 3:
            p_idx = [g.index(f"p{i}") for i in range(n + 1)]
            q_idx = [g.index(f"q{i}") for i in range(n + 1)]
            along_z = 0                                   # one bit per end effector (:314)
            for e, ee in enumerate(self.end_effectors):
                path = [int(name[1:]) for name in self.robot.kinematic_map["p0"][ee]]
                rel_last = np.linalg.inv(T0[path[-2]]) @ T0[path[-1]]
                if is_pose[e] and np.linalg.norm(np.cross(rel_last[:3, 3], [0, 0, 1])) < 1e-10:
                    along_z |= 1 << e      # (a position goal has no T_final: the correction does not apply)
            goal_len = g.axis_length
            # a position goal behind a last link along z: the residues the point formula takes its angle from (point_axis_offset)
            from ..graphs.graph_revolute import point_axis_offset
            for e, ee in enumerate(self.end_effectors):
                if not is_pose[e] and point_axis_offset(g, ee) is not None:
                    point_axis[e] = point_axis_offset(g, ee)[:2]
        else:
            p_idx = [g.index(f"p{i}") for i in range(n + 1)]
            q_idx = None
            along_z = 0
            ee_len = [g.dist[g.index(self.robot.parent[e]), g.index(e)] for e in self.end_effectors]
            goal_len = ee_len[0]
        T.attach_pipeline(T0=T0, p_index=p_idx, q_index=q_idx, x_index=g.index("x"),
                          y_index=g.index("y"), axis_length=g.axis_length,
                          goal_nodes=dev_slots[:2], goal_len=goal_len, base_lower=lower,
                          base_upper=upper, anchor_index=self.anchor_nodes,
                          anchor_pos=self.anchor_pos, pair_i=I, pair_j=J, term_src=term_src,
                          term_static=static, last_link_along_z=along_z, position_goal_mask=position_mask, point_axis=point_axis,
                          force_block_prepare=self.force_block_prepare,
                          ee_goal_nodes=dev_slots if self.multi_ee else None, ee_path=ee_path, ee_goal_len=ee_len,
                          goal_pair_a=[a for a, _ in pairs], goal_pair_b=[b for _, b in pairs])
        self.device_pipeline = True

    def goal_poses(self, goals, lead=1):
        """Goal arrays as this problem's entries take them -> pose arrays (goal_poses above): positions, where every
        end effector has a position goal, are packed into identity-rotation poses."""
        return goal_poses(goals, self.goal_kinds, self.dim, lead)

    def goal_positions(self, T_goals):
        """[B,d+1,d+1] poses -> positions of the goal nodes [B,2,d]  (_pose_goal; a position goal: p_e alone)."""
        T = np.asarray(T_goals, dtype=float)
        d = self.dim
        if d == 3:
            if T.ndim == 3:
                T = T[:, None]                           # one end effector
            p = T[:, :, :3, 3]
            q = p + T[:, :, :3, 2] * self.graph.axis_length
            gp = np.stack((p, q), axis=2).reshape(T.shape[0], -1, 3)   # p_e, q_e per end effector
            return gp if len(self._goal_keep) == gp.shape[1] else gp[:, self._goal_keep]
        if T.ndim == 3:
            T = T[:, None]                               # one end effector
        return np.stack([T[:, e_i, :2, 2] - (T[:, e_i, :2, 0] * dist if is_parent else 0.0)
                         for e_i, is_parent, dist in self._goal_src], axis=1)

    def assemble(self, T_goals):
        """D_goal, LOWER, UPPER [B,N,N] for a batch of goals (from_pose + graph_complete_edges)."""
        gp = self.goal_positions(T_goals)
        B = gp.shape[0]
        D = np.broadcast_to(self.base_D, (B, self.N, self.N)).copy()
        lo = np.broadcast_to(self.base_lower, (B, self.N, self.N)).copy()
        up = np.broadcast_to(self.base_upper, (B, self.N, self.N)).copy()
        for gi, g in enumerate(self.goal_nodes):
            dist = np.linalg.norm(gp[:, gi, None, :] - self.anchor_pos[None], axis=-1)  # [B,A]
            for ai, a in enumerate(self.anchor_nodes):
                D[:, a, g] = D[:, g, a] = dist[:, ai] ** 2
                lo[:, a, g] = lo[:, g, a] = dist[:, ai]
                up[:, a, g] = up[:, g, a] = dist[:, ai]
            for hi in range(gi + 1, len(self.goal_nodes)):   # goal nodes of DIFFERENT end effectors
                h = self.goal_nodes[hi]
                if self.omega[g, h] != 0 and np.isnan(self.graph.dist[g, h]):
                    dd = np.linalg.norm(gp[:, gi] - gp[:, hi], axis=-1)
                    D[:, g, h] = D[:, h, g] = dd ** 2
                    lo[:, g, h] = lo[:, h, g] = dd
                    up[:, g, h] = up[:, h, g] = dd
        return D, lo, up

    def prepare(self, T_goals, chunk=None, workers=None):
        """Host pre-processing for a batch: targets [B,T] and Y_init [B,N,k].  Chunks of goals are
        smoothed and initialised on a thread pool (numpy releases the GIL in its loops and in
        LAPACK); for graphs the device prepare kernel covers (N <= 32) this path is only the mirror
        the tests compare it with."""
        import os
        from concurrent.futures import ThreadPoolExecutor
        D, lo, up = self.assemble(T_goals)
        B = D.shape[0]
        if chunk is None:
            chunk = 512 if self.N <= 32 else 8
        spans = [(s, min(s + chunk, B)) for s in range(0, B, chunk)]

        def one(span):
            lb, ub = dgp.floyd_warshall_bounds(lo[span[0]:span[1]], up[span[0]:span[1]])
            return dgp.generate_initialization_batch(lb, ub, self.dim, self.omega)

        workers = workers or min(len(spans), max(1, (os.cpu_count() or 1) // 2))
        if workers <= 1 or len(spans) == 1:
            Ys = [one(sp) for sp in spans]
        else:
            with ThreadPoolExecutor(workers) as ex:
                Ys = list(ex.map(one, spans))
        return self.targets_from_D(D), np.concatenate(Ys, axis=0)

    def _seed_recipe(self):
        """How graph.realization places each node (graph_base.py:112-120 through _pose_goal): the
        joints' parents along the end-effector paths in root-first order, T0[parent]^-1 T0[j], and
        per node the frame it is read from (-1: its POS) and the coefficient of the frame axis
        (z for 3-D, x for planar) added to the frame's translation."""
        if getattr(self, "_recipe", None) is not None:
            return self._recipe
        g, d, N = self.graph, self.dim, self.N
        T0 = self.robot.T0_array()
        parent, order = {}, []
        for ee in self.end_effectors:                   # get_all_poses' order (robot_base.py:185-193)
            path = [int(name[1:]) for name in self.robot.kinematic_map["p0"][ee]]
            for k, j in enumerate(path):
                if j not in parent:
                    parent[j] = path[k - 1] if k else -1
                    order.append(j)
        Trel = np.zeros_like(T0)
        for j in order:
            if parent[j] >= 0:
                Trel[j] = np.linalg.inv(T0[parent[j]]) @ T0[j]
        frame, coef = np.full(N, -1, dtype=np.int64), np.zeros(N)
        for j in order:
            if d == 3:                                  # graph_revolute.py:243-249
                frame[g.index(f"p{j}")] = frame[g.index(f"q{j}")] = j
                coef[g.index(f"q{j}")] = g.axis_length
            elif parent[j] >= 0:                        # graph_planar.py:136-145: the last child wins
                u, v = g.index(f"p{j}"), g.index(f"p{parent[j]}")
                frame[u], coef[u] = j, 0.0
                frame[v], coef[v] = j, -g.dist[v, u]
        pos = np.full((N, d), np.nan)
        for i, name in enumerate(g.node_ids):
            if POS in g.nodes[name]:
                pos[i] = g.nodes[name][POS]
        self._recipe = (T0, parent, order, Trel, frame, coef, pos)
        return self._recipe

    def seed_points(self, q):
        """Joint angles [B,n] (or [n]) -> their graph realizations [B,N,k] in node order: the
        reference's warm start pos_from_graph(graph.realization(q)) (the Y_init of
        experiments/simple_ik_examples/test_chain_2d_new.py:46-59), batched.  The host mirror of
        gik_seed_batch."""
        T0, parent, order, Trel, frame, coef, pos = self._seed_recipe()
        Q = np.atleast_2d(np.asarray(q, dtype=float))
        B, d = Q.shape[0], self.dim
        F = np.zeros((B,) + T0.shape)
        for j in order:
            if parent[j] < 0:
                F[:, j] = T0[j]
                continue
            c, s = np.cos(Q[:, j - 1]), np.sin(Q[:, j - 1])
            Rz = np.broadcast_to(np.identity(d + 1), (B, d + 1, d + 1)).copy()
            Rz[:, 0, 0], Rz[:, 0, 1], Rz[:, 1, 0], Rz[:, 1, 1] = c, -s, s, c
            F[:, j] = F[:, parent[j]] @ Rz @ Trel[j]
        axis = 2 if d == 3 else 0
        Y = np.broadcast_to(pos, (B, self.N, d)).copy()
        on = frame >= 0
        Fn = F[:, frame[on]]                             # [B, nodes, d+1, d+1]
        Y[:, on] = Fn[:, :, :d, d] + coef[on][None, :, None] * Fn[:, :, :d, axis]
        return Y

    def targets_from_D(self, D):
        """[B,N,N] squared-distance matrices -> [B,T] per-term targets (Template.targets_from_D without
        a device handle)."""
        ti, tj, tk, tv = self.terms
        D = np.asarray(D, dtype=np.float64)
        tg = D[:, ti, tj].copy()
        hinge = tk != 1
        tg[:, hinge] = tv[hinge]
        return tg

    def joint_variables(self, Y, T_goals):
        from ..graphs.graph_revolute import joint_variables_revolute_batch
        from ..graphs.graph_planar import joint_variables_planar_batch
        if self.dim == 3:
            T = np.asarray(T_goals, dtype=float)
            if "position" in self.goal_kinds:      # T_final only for the end effectors whose goal is a pose
                T = T if T.ndim == 4 else T[:, None]
                T = {e: T[:, i] for i, e in enumerate(self.end_effectors) if self.goal_kinds[i] == "pose"} or None
            elif T.ndim == 4:
                T = {e: T[:, i] for i, e in enumerate(self.end_effectors)}
            return joint_variables_revolute_batch(self.graph, Y, T)
        return joint_variables_planar_batch(self.graph, Y)

    def pose_errors(self, q, T_goals):
        """EE position / rotation error of FK(q) against the goals (the metric of
        experiments/simple_ik_examples/test_chain_2d_new.py:62-66)."""
        T_goals = np.asarray(T_goals, dtype=float)
        if "position" in self.goal_kinds:      # a position goal has no rotation error: 0, and no part in the maximum
            T4 = T_goals if T_goals.ndim == 4 else T_goals[:, None]
            errs = [BatchProblem._pose_err(self.robot.fk_batch(q, int(e[1:])), T4[:, i], self.dim)
                    for i, e in enumerate(self.end_effectors)]
            rot = [r for (_, r), kind in zip(errs, self.goal_kinds) if kind == "pose"]
            return np.max([e[0] for e in errs], axis=0), np.max(rot, axis=0) if rot else np.zeros(len(T4))
        if T_goals.ndim == 4:        # several end effectors: the worst of them
            errs = [BatchProblem._pose_err(self.robot.fk_batch(q, int(e[1:])), T_goals[:, i], self.dim)
                    for i, e in enumerate(self.end_effectors)]
            return np.max([e[0] for e in errs], axis=0), np.max([e[1] for e in errs], axis=0)
        return BatchProblem._pose_err(self.robot.fk_batch(q), T_goals, self.dim)

    @staticmethod
    def _pose_err(T_sol, T_goals, d):
        pos = np.linalg.norm(T_goals[:, :d, d] - T_sol[:, :d, d], axis=1)
        Rrel = T_goals[:, :d, :d] @ np.swapaxes(T_sol[:, :d, :d], 1, 2)
        if d == 3:
            c = np.clip(0.5 * np.trace(Rrel, axis1=1, axis2=2) - 0.5, -1.0, 1.0)
            rot = np.arccos(c)
        else:
            rot = np.abs(np.arctan2(Rrel[:, 1, 0], Rrel[:, 0, 0]))
        return pos, rot


# ---- the pair geometry of AnchoredProblem's numpy mirrors, once (the device side: csrc/gik_anch_pairs.h) ----------------
# Elementwise float64 numpy on arrays of ends [..., 3]: the operations of the device pair functions in their order, every
# product and sum rounded on its own, whether the arrays hold a batch (the clearances) or one pair (the *_host feet).
def _dot3(x, y):
    return x[..., 0] * y[..., 0] + x[..., 1] * y[..., 1] + x[..., 2] * y[..., 2]


def _clamp01(x):
    x = np.where(x > 0.0, x, 0.0)
    return np.where(x < 1.0, x, 1.0)


def _nan_min(x, axis):
    """The minimum along axis (an int or a tuple); a NaN among the values gives NaN."""
    return np.where(np.isnan(x).any(axis=axis), np.nan, np.where(np.isnan(x), np.inf, x).min(axis=axis))


def _link_foot(a, b, c):
    """A link from a to b against a centre c -> (d, L2, u, t): d = b - a, L2 = d.d, u = c - a and the foot parameter
    t = min(max(u.d / L2, 0), 1), 0 for a zero-length link.  What link_clearance and link_foot_host share; their vectors
    (u - t d and ((1 - t) a + t b) - c) round differently, as on the device, and both sets of bits are pinned by tests."""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = b - a
        L2 = _dot3(d, d)
        u = c - a
        t = np.where(L2 > 0.0, _clamp01(_dot3(u, d) / L2), 0.0)
    return d, L2, u, t


def _segment_feet(a1, b1, a2, b2):
    """The closest points of the segments a1 -> b1 and a2 -> b2 -> (s, t, v, d): they are a1 + s d1 and a2 + t d2,
    v = (a1 + s d1) - (a2 + t d2) and d = v.v.  With d1 = b1 - a1, d2 = b2 - a2, r = a1 - a2, a = d1.d1, e = d2.d2,
    f = d2.r, c = d1.r, b = d1.d2, den = a e - b b:  s = clamp((b f - c e) / den, 0, 1) where a > 0 and den > 0, else 0;
    t = (b s + f) / e where e > 0, else the t < 0 branch is taken;  where t < 0: t = 0, s = clamp(-c / a, 0, 1);  where
    t > 1: t = 1, s = clamp((b - c) / a, 0, 1) (0 where a == 0).  A NaN coordinate reaches v -- through s d1 or t d2 even
    where s or t is 0 -- so d is NaN without a guard of its own."""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d1, d2, r = b1 - a1, b2 - a2, a1 - a2
        a, e, f, c, b = _dot3(d1, d1), _dot3(d2, d2), _dot3(d2, r), _dot3(d1, r), _dot3(d1, d2)
        den = a * e - b * b
        s = np.where((a > 0.0) & (den > 0.0), _clamp01((b * f - c * e) / den), 0.0)
        t = np.where(e > 0.0, (b * s + f) / e, -1.0)          # (a zero-length second link: the t = 0 branch)
        s_lo = np.where(a > 0.0, _clamp01(-c / a), 0.0)
        s_hi = np.where(a > 0.0, _clamp01((b - c) / a), 0.0)
        s = np.where(t < 0.0, s_lo, np.where(t > 1.0, s_hi, s))
        t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
        v = (a1 + s[..., None] * d1) - (a2 + t[..., None] * d2)
        return s, t, v, _dot3(v, v)


class AnchoredProblem:
    """Opt-in "intended" obstacle semantics.  graph_base.py:182-211 ties every
    node with a known position -- base frame, goal nodes, obstacle centres -- to the others by
    equality edges and means to add robot<->obstacle lower-bound hinges (:205-211; the TYPE
    comparison at :207 never fires, so the reference creates none, and that observable behaviour
    stays the default everywhere else in this package).  Here those nodes are CONSTANTS instead of
    rows of Y and the hinges exist: UR10 + table_environment() becomes a 10-node problem with 100
    point-to-obstacle hinges per p-node on the wavefront kernel, instead of N = 116 / 5612 terms on
    the workgroup kernel.  The anchors fix the gauge, so the search space is Euclidean.

    graph: a ProblemGraphRevolute (chain) with its obstacles added (either spelling of
    add_spherical_obstacle).  The initial point is the robot graph's own (bound smoothing + MDS
    without obstacles) fitted to the world frame by its anchors."""

    def __init__(self, graph, params=None, device=None, host_only=False, links=None, link_radius=0.0, link_hinges=False,
                 goal="pose", self_pairs=None, self_hinges=False, halfspaces=None, halfspace_margin=None):
        """host_only: derive the term set only (no device handles) -- what tests/test_host_layer.py
        compares with the reference's own edge construction (tests/golden/ur10_table_intended.npz).

        links: the segments whose clearance link_clearance / clearance_mode="links" measure, as (name_a, name_b)
        pairs of robot-graph nodes.  None: the chain's skeleton p0->p1, ..., p(n-1)->pn, base and end-effector rows
        included (the last link is real geometry even though its end is a constant of the goal).  [] attaches none.
        link_radius: the capsule radius of the links in metres, >= 0, a scalar or one entry per link.
        link_hinges: False -- the links are measured only, the solve sees the joint points (the node hinges) -- or True:
        the solve kernel also carries a hinge per (link, sphere) on the distance from the sphere's centre to the link's
        SEGMENT (gik_anchored_attach_links with hinges = 1; link_hinge_terms_host is the numpy mirror of the terms), so
        every solve, restart and tracked waypoint of this problem pushes whole links out of the spheres.  The node
        hinges stay.  Needs a link set; chains on the 9-slot anchored kernel.
        self_pairs: the link pairs whose mutual distance self_clearance / clearance_mode="links+self" measure (link
        against link: the robot against itself).  None: nothing is attached.  "auto": every pair of the links that share
        no end row, l < m in link order -- ten pairs for UR10's skeleton.  Or a sequence of (l, m) indices into
        self.link_names; a pair of links that share a row is refused (its distance is 0 in every configuration).  The
        links are capsules of link_radius around SEGMENTS: with thick capsules around the short wrist links "auto" reports
        overlaps the real geometry does not have -- links 2 and 4 of UR10 are joined by a link of 11.5 cm, so at a radius
        of 6 cm they touch in every configuration -- and such a robot wants an explicit list.  self.self_pairs is the
        [P, 2] int array (None: not attached).
        self_hinges: False -- the pairs are measured only: nothing in the cost acts on the self clearance, a restart
        finds a self-clear answer by landing elsewhere -- or True: the solve kernel also carries a hinge per pair on the
        distance between the two SEGMENTS (gik_anchored_attach_self_hinges; self_hinge_terms_host is the numpy mirror of the
        terms), so every solve, restart, scene and tracked waypoint of this problem pushes the robot's own links apart.
        Needs self_pairs, at most 16 of them; chains on the 9-slot anchored kernel; with or without link_hinges.
        halfspaces: floors and walls, an array-like [H, 4] of (nx, ny, nz, d0) rows, H within 1 .. 8: the allowed side of
        row h is n.p - d0 >= 0 (each row is divided by |n| here; self.halfspaces holds the result).  Every masked free node i
        then carries the hinge max(0, margin_i - (n.Y_i - d0))^2 per half-space in the solve
        (gik_anchored_attach_halfspaces; halfspace_terms_host is the numpy mirror), and every clearance the device reports
        -- solve, restarts, scenes, tracking, sweeps -- is the minimum of the spheres' and halfspace_clearance.  With scenes
        the half-spaces stay the problem's: the room.  None: nothing is attached, the problem runs what it ran.
        halfspace_margin: None -- each masked free node gets the largest link_radius among the attached links that end at
        it (0 without), which keeps whole capsules on the allowed side: a linear function on a segment takes its minimum at
        an end --, or a scalar, or one entry per free node (self.free_names), metres, >= 0.  self.halfspace_margin holds it.
        Chains on the 9-slot anchored kernel; with or without link_hinges; not together with self_hinges."""
        import copy
        from ..utils.constants import OBSTACLE, ROBOT, TYPE, MAIN_PREFIX
        from .. import _ffi
        if graph.dim != 3 or not graph.robot.is_chain:
            raise NotImplementedError("the fixed-anchor formulation covers 3-D chains")
        if goal_kinds(goal, len(graph.robot.end_effectors)) != ("pose",):
            # (q_n is a constant row of the goal there; with a position goal it would become a free node)
            raise NotImplementedError("the fixed-anchor formulation takes pose goals: goal='position' is not supported")
        if not isinstance(link_hinges, (bool, np.bool_)):      # (before any device call)
            raise ValueError(f"link_hinges must be a bool, got {link_hinges!r}")
        if link_hinges and links is not None and len(links) == 0:
            raise ValueError("link_hinges=True needs a link set: links=[] attaches none")
        self.link_hinges = bool(link_hinges)
        if not isinstance(self_hinges, (bool, np.bool_)):      # (before any device call)
            raise ValueError(f"self_hinges must be a bool, got {self_hinges!r}")
        if self_hinges and self_pairs is None:
            raise ValueError("self_hinges=True needs self pairs: self_pairs=None attaches none")
        self.self_hinges = bool(self_hinges)
        self.halfspaces = self._check_halfspaces(halfspaces, halfspace_margin, self.self_hinges)      # (before any device call)
        self.graph, self.robot = graph, graph.robot
        obstacles = [n for n in graph.node_ids if graph.nodes[n].get(TYPE) == OBSTACLE]
        bare = copy.deepcopy(graph)
        bare.clear_obstacles()
        if links is None:
            links = [(f"p{i}", f"p{i + 1}") for i in range(self.robot.n)]
        links = [tuple(l) for l in links]
        for l in links:
            if len(l) != 2 or any(name not in bare.node_ids for name in l):
                raise ValueError(f"link {l!r}: a link is a pair of node names of the robot graph")
        self.link_names = links
        self.link_rows = np.array([[bare.index(a), bare.index(b)] for a, b in links], dtype=np.int32).reshape(-1, 2)
        rho = np.asarray(link_radius, dtype=np.float64)
        if rho.ndim == 0:
            rho = np.full(len(links), float(rho))
        if rho.shape != (len(links),):
            raise ValueError(f"link_radius must be a scalar or have one entry per link ({len(links)}), got shape {list(rho.shape)}")
        if not np.all(np.isfinite(rho) & (rho >= 0)):
            raise ValueError("link_radius must be finite and at least 0")
        self.link_radius = np.ascontiguousarray(rho)
        self.self_pairs = self._check_self_pairs(self_pairs, self.link_rows)
        if self.self_hinges and len(self.self_pairs) > _ffi.SELF_HINGE_MAX_PAIRS:
            raise ValueError(f"self_hinges=True takes at most {_ffi.SELF_HINGE_MAX_PAIRS} self pairs, got {len(self.self_pairs)}")
        self.base = BatchProblem(bare, use_limits=True, params=params, device=device, host_only=host_only)
        if not host_only and not self.base.device_pipeline:
            raise NotImplementedError("robot graph beyond the device pipeline")
        bp = self.base
        N = bp.N
        goal = list(bp.goal_nodes)
        anchors = list(bp.anchor_nodes) + goal               # constant rows first, goal rows last
        free = [i for i in range(N) if i not in anchors]
        fidx = {n: f for f, n in enumerate(free)}
        om, pL, pU, D = bp.omega, bp.psi_L, bp.psi_U, bp.base_D
        sub = np.ix_(free, free)
        ti, tj, tk, tv = build_terms(om[sub], pL[sub], pU[sub], True)
        Dff = D[sub]
        target = np.where(np.isnan(tv), Dff[ti, tj], tv)
        pin = []
        for i in free:
            for r, a in enumerate(anchors):
                if om[i, a] != 0:
                    pin.append((fidx[i], r, _ffi.TERM_EQ, D[i, a]))
                if pL[i, a] != 0:
                    pin.append((fidx[i], r, _ffi.TERM_LOWER, pL[i, a]))
                if pU[i, a] != 0:
                    pin.append((fidx[i], r, _ffi.TERM_UPPER, pU[i, a]))
        self.obstacles = np.array([[*np.asarray(graph.nodes[o]["pos"], dtype=float), float(graph.nodes[o]["radius"])]
                                   for o in obstacles], dtype=float).reshape(-1, 4)
        self.obstacle_names = obstacles
        obs = self.obstacles.copy()
        obs[:, 3] = obs[:, 3] ** 2                            # LOWER = radius  ->  psi_L = radius^2
        names = [bare.node_ids[i] for i in free]
        # graph_base.py:205-211 as written: every node whose TYPE holds ROBOT and whose name starts
        # with MAIN_PREFIX gets [BELOW], LOWER = radius towards the obstacle -- pinned to the
        # reference's own lines by tools/capture_golden_intended.py (700 edges for UR10 + table: p0..p6
        # x 100; p0 and p6 are constants here, so 5 x 100 hinges act on unknowns)
        mask = [int(n[0] == MAIN_PREFIX and ROBOT in bare.nodes[n].get(TYPE, [])) for n in names]
        pos = np.zeros((len(anchors), 3))
        pos[:len(bp.anchor_nodes)] = bp.anchor_pos
        self.free, self.anchors, self.pin = free, anchors, pin
        self.anchor_pos, self.n_goal_anchor = pos, len(goal)      # (goal rows: zeros, filled per problem)
        self.free_names = names
        self.free_terms = (ti, tj, tk, target)
        self.obs_mask = np.array(mask, dtype=np.int32)
        self.halfspace_margin = self._halfspace_margins(halfspace_margin)
        if host_only:
            self.template = None
            return
        self.template = Template(
            len(free), 3, ti, tj, tk, None, device=device, params=params,
            anchored=dict(anchor_pos=pos, n_goal_anchor=len(goal), term_target=target,
                          pin_node=[p[0] for p in pin], pin_anchor=[p[1] for p in pin],
                          pin_kind=[p[2] for p in pin], pin_target=[p[3] for p in pin],
                          obs=obs, obs_node_mask=mask, full_N=N, free_full_index=free,
                          anchor_full_index=anchors, axis_length=graph.axis_length))
        if len(links):
            self.template.attach_links(self.link_rows[:, 0], self.link_rows[:, 1], self.link_radius, hinges=self.link_hinges)
        if self.self_pairs is not None:
            self.template.attach_self_pairs(self.self_pairs[:, 0], self.self_pairs[:, 1])
        if self.self_hinges:
            self.template.attach_self_hinges()
        if self.halfspaces is not None:      # (last: it re-resolves the kernels of the form the calls above left)
            self.template.attach_halfspaces(self.halfspaces, self.halfspace_margin)

    @staticmethod
    def _check_halfspaces(halfspaces, halfspace_margin, self_hinges):
        """halfspaces of __init__ -> [H, 4] float64 with unit normals (None: none), checked on the host: ValueError for a
        shape other than [H, 4], H outside 1 .. 8, a zero or non-finite normal, a non-finite offset, a margin without
        half-spaces, and self_hinges=True together with halfspaces."""
        from .. import _ffi
        if halfspaces is None:
            if halfspace_margin is not None:
                raise ValueError("halfspace_margin needs halfspaces: halfspaces=None attaches none")
            return None
        if self_hinges:
            raise ValueError("halfspaces together with self_hinges=True is not supported: the solve has no such build")
        try:
            h = np.array(halfspaces, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("halfspaces must be an array-like of shape [H, 4]: rows (nx, ny, nz, d0)") from None
        if h.ndim != 2 or h.shape[1] != 4:
            raise ValueError(f"halfspaces must have shape [H, 4] (rows nx, ny, nz, d0), got {list(h.shape)}")
        if not 1 <= len(h) <= _ffi.HALF_MAX:
            raise ValueError(f"halfspaces takes 1 .. {_ffi.HALF_MAX} rows, got {len(h)}")
        if not np.all(np.isfinite(h)):
            raise ValueError("halfspaces has non-finite entries")
        norm = np.sqrt(_dot3(h, h))
        if not np.all(np.isfinite(norm) & (norm > 0.0)):
            raise ValueError("halfspaces: a normal (nx, ny, nz) is zero or overflows")
        return np.ascontiguousarray(h / norm[:, None])      # (| |n|^2 - 1 | is then a few ulp: the C entry asks for 1e-12)

    def _halfspace_margins(self, halfspace_margin):
        """halfspace_margin of __init__ -> [len(free)] float64 (None without half-spaces): the default from the link radii,
        a scalar broadcast, or one entry per free node; ValueError for another shape and for a negative or non-finite entry."""
        if self.halfspaces is None:
            return None
        Nf = len(self.free)
        if halfspace_margin is None:
            mu = np.zeros(Nf)
            for (ra, rb), rho in zip(np.asarray(self.link_rows).tolist(), self.link_radius):
                for r in (ra, rb):
                    if r in self.free:
                        f = self.free.index(r)
                        mu[f] = max(mu[f], float(rho))
            return np.where(self.obs_mask == 1, mu, 0.0)
        try:
            mu = np.array(halfspace_margin, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("halfspace_margin must be None, a scalar or one entry per free node") from None
        if mu.ndim == 0:
            mu = np.full(Nf, float(mu))
        if mu.shape != (Nf,):
            raise ValueError(f"halfspace_margin must be a scalar or have one entry per free node ({Nf}), got shape {list(mu.shape)}")
        if not np.all(np.isfinite(mu) & (mu >= 0)):
            raise ValueError("halfspace_margin must be finite and at least 0")
        return np.ascontiguousarray(mu)

    @staticmethod
    def _halfspace_s(P, h):
        """s_h(P) = ((nx x + ny y) + nz z) - d0 for points P [..., 3] against rows h [H, 4] -> [..., H]: every product and
        sum rounded on its own, the bits of anch_half_clearance_kernel."""
        P = P[..., None, :]
        return ((h[:, 0] * P[..., 0] + h[:, 1] * P[..., 1]) + h[:, 2] * P[..., 2]) - h[:, 3]

    def halfspace_clearance(self, Y_full, links=False):
        """min over (masked free node i, half-space h) of s_h(Y_i) - margin_i per goal, or with links=True over (link l,
        both of its end rows, h) of s_h(P) - link_radius[l]: the host mirror of gik_anchored_halfspace_clearance, the same
        operations in the same order.  Y_full [B, N_robot, 3] (numpy).  >= 0: every measured point keeps its margin to
        every plane; with the default margins the node value bounds the link value over the links with a free end.  No
        half-spaces, no masked node or no link: +inf; a NaN coordinate of a measured row: NaN for that goal."""
        Y = np.asarray(Y_full, dtype=np.float64)
        if Y.ndim == 2:
            Y = Y[None]
        B = Y.shape[0]
        if self.halfspaces is None:
            return np.full(B, np.inf)
        if links:
            rows = np.asarray(self.link_rows, dtype=np.int64).reshape(-1, 2)
            if len(rows) == 0:
                return np.full(B, np.inf)
            P = Y[:, rows]                                                          # [B, n_link, 2, 3]
            with np.errstate(invalid="ignore"):
                val = self._halfspace_s(P, self.halfspaces) - np.asarray(self.link_radius)[None, :, None, None]
            return _nan_min(val, axis=(1, 2, 3))
        nodes = [self.free[i] for i in range(len(self.free)) if self.obs_mask[i] == 1]
        if not nodes:
            return np.full(B, np.inf)
        mu = self.halfspace_margin[self.obs_mask == 1]
        with np.errstate(invalid="ignore"):
            val = self._halfspace_s(Y[:, nodes], self.halfspaces) - mu[None, :, None]
        return _nan_min(val, axis=(1, 2))

    def halfspace_terms_host(self, Y_free, W, frozen_active=None):
        """(f, G, H) of the half-space hinges alone at one point: Y_free, W [Nf, 3], in the conventions of
        link_hinge_terms_host (f = sum res^2, G = 1/2 grad f, H = 1/2 Hess f [W]).  Per (masked free node i, half-space h):
            res = margin_i - (n.Y_i - d0),  active <=> res > 0
            f += res^2;  G_i += -res n;  H_i += (n . W_i) n
        H is exact wherever the active set does not change.  Unmasked nodes carry nothing; the anchors are constants.
        frozen_active: a set of (free node, half-space) to take as the active set instead of this point's (what a finite
        difference of the gradient across a boundary needs); this point's own comes back in self.last_half_active."""
        Y, W = np.asarray(Y_free, dtype=np.float64), np.asarray(W, dtype=np.float64)
        f, G, H = 0.0, np.zeros_like(Y), np.zeros_like(Y)
        self.last_half_active = set()
        if self.halfspaces is None:
            return f, G, H
        for i in range(len(self.free)):
            if self.obs_mask[i] != 1:
                continue
            for h, (nx, ny, nz, d0) in enumerate(self.halfspaces):
                n = np.array([nx, ny, nz])
                res = self.halfspace_margin[i] - (float(n @ Y[i]) - d0)
                if res > 0.0:
                    self.last_half_active.add((i, h))
                if not ((i, h) in frozen_active if frozen_active is not None else res > 0.0):
                    continue
                f += res * res
                G[i] += -res * n
                H[i] += float(n @ W[i]) * n
        return f, G, H

    @staticmethod
    def _check_self_pairs(self_pairs, link_rows):
        """self_pairs of __init__ -> [P, 2] int32 (None: none), checked on the host: ValueError for pairs without links, an
        index outside the links, l == m, and an explicit pair whose links share an end row."""
        if self_pairs is None:
            return None
        n_link = len(link_rows)
        if n_link == 0:
            raise ValueError("self_pairs needs a link set: links=[] attaches none")
        shares = lambda l, m: bool(set(link_rows[l].tolist()) & set(link_rows[m].tolist()))      # noqa: E731
        if isinstance(self_pairs, str):
            if self_pairs != "auto":
                raise ValueError(f"self_pairs must be None, 'auto' or a sequence of (l, m) link indices, got {self_pairs!r}")
            pairs = [(l, m) for l in range(n_link) for m in range(l + 1, n_link) if not shares(l, m)]
        else:
            pairs = []
            for pr in self_pairs:
                if len(pr) != 2 or any(isinstance(i, (bool, np.bool_)) or int(i) != i for i in pr):
                    raise ValueError(f"self pair {pr!r}: a pair is two link indices (l, m)")
                l, m = int(pr[0]), int(pr[1])
                if not (0 <= l < n_link and 0 <= m < n_link):
                    raise ValueError(f"self pair {pr!r}: a link index is outside [0, {n_link})")
                if l == m:
                    raise ValueError(f"self pair {pr!r}: l == m names one link twice")
                if shares(l, m):
                    raise ValueError(f"self pair {pr!r}: the two links share an end row, their distance is 0 in every configuration")
                pairs.append((l, m))
        from .. import _ffi
        if len(pairs) > _ffi.SELF_MAX_PAIRS:
            raise ValueError(f"at most {_ffi.SELF_MAX_PAIRS} self pairs, got {len(pairs)}")
        return np.array(pairs, dtype=np.int32).reshape(-1, 2)

    def goal_anchors(self, T_goals):
        """[B,4,4] -> [B, 2*3]: p_n, q_n world positions (graph_revolute.py:243-249)."""
        return self.base.goal_positions(T_goals).reshape(len(T_goals), -1)

    def seed_points(self, q):
        """Joint angles [B,n] (or [n]) -> the anchored start point [B, len(free), 3]: the free rows of
        the robot graph's realization (BatchProblem.seed_points), which is already in the world frame.
        The host mirror of gik_anchored_seed_batch's Y_free."""
        return self.base.seed_points(q)[:, self.free]

    def scene_set(self, scenes):
        """Per-goal obstacle scenes for solve(..., scenes=) and solve_trajectory: a sequence of [m_s, 4] arrays of
        (centre x, y, z, radius), numpy or torch, at most 128 spheres each; an empty scene is an array of shape [0, 4].
        They are uploaded once; the returned engine.SceneSet holds the device tensors (obs with the radii squared by one
        rounded product, the bits of this problem's own obs[:, 3] ** 2; n_obs), the counts, the stride and the host
        copies.  ValueError before any device call: more than 128 spheres in a scene, a radius that is negative or not
        finite, a centre that is not finite, a shape that is not [m, 4].  The problem's own obstacles play no part in a
        solve that is given scenes; its masked nodes, links and link radii apply to every scene."""
        from ..engine import SceneSet, pack_scenes
        scenes = list(scenes)
        pack_scenes(scenes)      # (the checks, before the template -- a device object -- is touched)
        if self.template is None:
            raise ValueError("a host-only problem has no device to upload scenes to")
        return SceneSet(scenes, self.template.device)

    def seed_atlas(self, size=65536, seed=0, q_limits=None, clearance_mode="nodes", clear_tol=1e-4):
        """A SeedAtlas of this problem: the rows of retry_seeds_host(seed, arange(size), 0, lo, hi) -- uniform inside
        q_limits, default the robot's limits_arrays() -- whose realization is clear of the room,
        candidate_clearance_host(q, clearance_mode) >= -clear_tol, with their keys (base.seed_points, the goal rows).
        Host numpy, about a second for 65536 rows; the device is touched only by the upload at the end (not at all on a
        host-only problem)."""
        if isinstance(size, (bool, np.bool_)) or int(size) != size or size < 1:
            raise ValueError(f"size must be a positive integer, got {size!r}")
        if not clear_tol > 0:
            raise ValueError("clear_tol must be positive")
        check_clearance_mode(clearance_mode, len(self.link_names) > 0, self.self_pairs is not None)
        lo, hi = self.robot.limits_arrays() if q_limits is None else q_limits
        q = retry_seeds_host(seed, np.arange(int(size)), 0, lo, hi)
        return SeedAtlas.from_configurations(self, q, clearance_mode, clear_tol, keep_clear_only=True)

    def _check_atlas(self, atlas):
        """atlas of a call -> itself: a SeedAtlas whose key width is this problem's base template's, uploaded."""
        if not isinstance(atlas, SeedAtlas):
            raise TypeError("atlas must be a SeedAtlas (AnchoredProblem.seed_atlas, SeedAtlas.from_configurations)")
        width = 3 * len(self.base.goal_nodes)
        if atlas.width != width:
            raise ValueError(f"the atlas has keys of width {atlas.width}, this problem's goals have {width}")
        if atlas.q.shape[1] != self.robot.n:
            raise ValueError(f"the atlas has rows of {atlas.q.shape[1]} angles, the robot has {self.robot.n} joints")
        return atlas

    def atlas_nearest(self, T_goals, atlas, k):
        """Goal poses [B, 4, 4] -> device (idx [B, k] int32, dist [B, k]): the k (1 .. 64) rows of `atlas` whose key lies
        nearest to each goal's (gik_atlas_nearest on the robot graph's template), ascending in (distance, row); -1 / +inf
        where fewer than k rows have a finite distance.  atlas_nearest_host(atlas.keys, goal_anchors(T_goals), k) is the
        mirror, equal in idx and in the bits of dist."""
        self._check_atlas(atlas)
        k = check_atlas_k(k, None)
        if self.template is None:
            raise ValueError("a host-only problem has no device: atlas_nearest_host is the mirror")
        if atlas.d_keys is None:
            atlas.upload(self.template.device)
        return self.base.template.atlas_nearest(atlas, np.asarray(T_goals, dtype=float), k)

    def atlas_seeds_host(self, T_goals, atlas, candidates, first=0, clearance_mode="nodes", clear_tol=1e-4, obstacles=None):
        """The numpy mirror of the atlas seed step (gik_anchored_atlas_seeds over all goals): candidate c of goal g is the
        atlas row of rank first + c among the goal's nearest (atlas_nearest_host; a missing rank is a NaN row), each
        measured by candidate_clearance_host, and retry_pick_host's choice among them.  obstacles: as screened_seeds_host
        (None, one [m, 4] scene, or one per goal).  Returns (q [G, n] the picked angles, pick [G] int, clearance [G] of
        the pick); self.last_atlas = (rows [C, G] the candidates' atlas rows, q_c [C, G, n], clearance_c [C, G])."""
        self._check_atlas(atlas)
        C = check_retry_candidates(candidates)
        if isinstance(first, (bool, np.bool_)) or int(first) != first or first < 0:
            raise ValueError(f"first must be a non-negative integer, got {first!r}")
        first = int(first)
        check_atlas_k(first + C, None, "first + candidates")
        if not clear_tol > 0:
            raise ValueError("clear_tol must be positive")
        T = np.asarray(T_goals, dtype=float)
        G = len(T)
        nbr, _ = atlas_nearest_host(atlas.keys, self.goal_anchors(T), first + C)
        rows = np.ascontiguousarray(nbr[:, first:first + C].T)                      # [C, G]
        q_c = np.where((rows >= 0)[..., None], atlas.q[np.maximum(rows, 0)], np.nan)
        per_goal = obstacles is not None and not (isinstance(obstacles, np.ndarray) and obstacles.ndim == 2)
        if per_goal:
            obstacles = [np.asarray(o, dtype=np.float64).reshape(-1, 4) for o in obstacles]
            if len(obstacles) != G:
                raise ValueError(f"obstacles must be one [m, 4] array or one per goal ({G}), got {len(obstacles)}")
            cl = np.empty((C, G))
            for g in range(G):
                cl[:, g] = self.candidate_clearance_host(q_c[:, g], clearance_mode, obstacles[g])
        else:
            cl = self.candidate_clearance_host(q_c.reshape(C * G, -1), clearance_mode, obstacles).reshape(C, G)
        pick = retry_pick_host(cl, clear_tol)
        self.last_atlas = (rows, q_c, cl)
        cols = np.arange(G)
        return q_c[pick, cols], pick, cl[pick, cols]

    def solve(self, T_goals, q_init=None, clearance=False, retries=0, retry_seed=0, pos_tol=0.01, rot_tol=0.01,
              clear_tol=1e-4, retry_spread=0.0, q_limits=None, clearance_mode="nodes", scenes=None, scene_id=None,
              retry_candidates=1, atlas=None, atlas_candidates=1):
        """Goal poses -> dict of device tensors (x [B, N_robot, 3], q, pos_err, rot_err, stats).

        q_init (warm start): joint angles [B,n] or [n]; the solve then starts from the realization of
        its seed (gik_anchored_ik_batch_seeded) instead of bound smoothing + MDS, the goal nodes still
        where the goal puts them.  clearance: add "clearance" [B], the device twin of
        self.clearance(x) -- always there for a seeded solve and with retries > 0.

        clearance_mode: "nodes" -- "clearance" is that of the joint points (self.clearance), which does not see a
        link that crosses a sphere between two of them -- or "links": it is that of whole links
        (self.link_clearance; the problem must have links), with retries=0 too.  On a problem built with
        link_hinges=True the solve itself carries link hinges, so clearance_mode="links" then has hinges behind it: the
        rule reads a clearance the cost acts on.  "links+self" (the problem must have self_pairs): the minimum of the
        link clearance and self.self_clearance of the same points -- an answer whose links pass through each other has
        failed the rule like one whose links pass through a sphere.  Nothing in the cost acts on the self clearance unless the
        problem was built with self_hinges=True.

        retries > 0 (gik_anchored_ik_batch_retry): a goal that fails -- stop != 0, pos_err > pos_tol, rot_err >
        rot_tol or clearance < -clear_tol, so an answer on its goal with a joint point (clearance_mode="nodes") or
        any part of a link ("links") inside a sphere has failed -- is solved again up to `retries` (<= 63) times from joint angles inside q_limits (default: the robot's
        limits_arrays()), and the better answer is kept; "attempt" [B] int32 says which one each goal holds.
        retry_spread == 0: the angles are uniform inside the limits, retry_seeds_host(retry_seed, [g], attempt,
        lo, hi) are goal g's.  retry_spread > 0 (radians, needs q_init): they lie within retry_spread of q_init
        (retry_seeds_host(..., center=q_init[g:g+1], spread=retry_spread)), for a tracked waypoint that
        should stay on its IK branch.

        scenes (scene_set(...)) with scene_id ([B] ints within [0, S), numpy or a device tensor; optional with one
        scene): goal b is solved among the spheres of scene scene_id[b] instead of the problem's own -- one launch over
        the whole batch, whatever the mix -- and "clearance" is measured against them.  Every other keyword combines with
        it.  Goal b's answer is, bit for bit, that of an AnchoredProblem built with scene scene_id[b]'s spheres.

        retry_candidates (an int within 1 .. 16; above 1 needs retries > 0): a restart draws that many candidate seeds per
        failed goal instead of one, measures the robot as each candidate places it with the clearance the rule reads
        (clearance_mode, half-spaces, the goal's scene) and starts from the first that is clear -- or, where none is, from
        the one with the largest clearance.  screened_seeds_host is the numpy mirror of the choice; a goal with
        "attempt" = a > 0 holds what solve(T[g:g+1], q_init=that pick) returns.  1 (the default): one blind seed, the
        call as it was.

        atlas (a SeedAtlas: seed_atlas, SeedAtlas.from_configurations) with atlas_candidates = C (1 .. 16): a seed that
        knows the goal (gik_anchored_ik_batch_atlas).  Without q_init attempt 0 starts from the pick -- the first clear
        one, as above -- among the C atlas rows whose end effector lies nearest to the goal's; restart a of a failed goal
        starts from the pick among ranks [a C, (a + 1) C).  With q_init attempt 0 starts there and the restarts alone
        take atlas rows.  Combines with clearance_mode and scenes / scene_id; retry_seed and q_limits are not read.
        ValueError before any device call: retry_spread > 0, retry_candidates > 1, (retries + 1) C above 64 or above
        atlas.count, an atlas whose key width is not this problem's.  A goal with "attempt" = a holds what
        solve(T[g:g+1], q_init=atlas_seeds_host(T, atlas, C, first=a C, ...)[0][g:g+1]) returns; "atlas_pick" [B] int32
        names the atlas row it started from (-1: from q_init).  None (the default): the call as it was."""
        T = np.asarray(T_goals, dtype=float)
        check_clearance_mode(clearance_mode, len(self.link_names) > 0, self.self_pairs is not None)
        extra = {}
        if atlas is not None:
            self._check_atlas(atlas)
            extra = dict(atlas=atlas, atlas_candidates=check_atlas_args(atlas, atlas_candidates, retries, retry_candidates,
                                                                        retry_spread, spread_first=True))
        elif atlas_candidates != 1:
            raise ValueError("atlas_candidates needs atlas=")
        retry = self._retry_args(retries, retry_seed, pos_tol, rot_tol, clear_tol, retry_spread, q_limits, q_init is not None,
                                 retry_candidates)
        if q_init is not None:
            q_init = _seed_angles(q_init, T.shape[0], self.robot.n)
        if atlas is not None:
            if not retry:      # (attempt 0 alone still runs on the atlas entry, under the call's tolerances)
                retry = dict(pos_tol=pos_tol, rot_tol=rot_tol, clear_tol=clear_tol)
            if atlas.d_keys is None:
                atlas.upload(self.template.device)
        return self.template.anchored_ik(self.base.template, T, q_init=q_init, clearance=clearance or q_init is not None,
                                         clearance_mode=clearance_mode, scenes=scenes, scene_id=scene_id, **retry, **extra)

    def _retry_args(self, retries, retry_seed, pos_tol, rot_tol, clear_tol, retry_spread, q_limits, has_center=True,
                    retry_candidates=1):
        """The restart arguments of solve / solve_trajectory, checked here before any device call, as the keywords
        Template.anchored_ik takes ({} with retries == 0); q_limits defaults to the robot's limits_arrays().
        retry_candidates is among them only above 1."""
        retry_candidates = check_retry_candidates(retry_candidates, retries)
        q_limits = self.robot.limits_arrays() if retries and q_limits is None else q_limits
        kw = _retry_kwargs(retries, retry_seed, pos_tol, rot_tol, q_limits, self.robot.n, has_center, clear_tol=clear_tol,
                           retry_spread=retry_spread)
        if retry_candidates > 1:
            kw["retry_candidates"] = retry_candidates
        return kw

    def candidate_clearance_host(self, q, clearance_mode="nodes", obstacles=None):
        """Joint angles [M, n] -> [M]: the clearance a screened restart measures a candidate seed with -- that of the
        robot graph's realization of q (BatchProblem.seed_points: every row where the configuration puts it, the end
        effector included) in clearance_mode, the half-spaces folded in: the minimum of the existing mirrors, NaN if any
        part is NaN.  obstacles: [m, 4] to measure against instead of the problem's own (a scene)."""
        check_clearance_mode(clearance_mode, len(self.link_names) > 0, self.self_pairs is not None)
        Y = self.base.seed_points(np.asarray(q, dtype=np.float64))
        with np.errstate(invalid="ignore"):
            if clearance_mode == "nodes":
                none = len(self.obstacles if obstacles is None else np.reshape(obstacles, (-1, 4))) == 0
                parts = [np.full(len(Y), np.inf) if none else self.clearance(Y, obstacles=obstacles)]
            else:
                parts = [self.link_clearance(Y, obstacles=obstacles)]
                if clearance_mode == "links+self":
                    parts.append(self.self_clearance(Y))
            if self.halfspaces is not None:
                parts.append(self.halfspace_clearance(Y, links=clearance_mode != "nodes"))
        return _nan_min(np.stack(parts, axis=0), axis=0)

    def screened_seeds_host(self, seed, goals, attempt, candidates, q_lo, q_hi, center=None, spread=0.0, clearance_mode="nodes",
                            clear_tol=1e-4, obstacles=None):
        """The numpy mirror of the screened seed step (gik_anchored_retry_seeds_screened): for every goal index in `goals`,
        `candidates` seeds -- candidate c is retry_seeds_host((seed + c * 0xD1342543DE82EF95) mod 2^64, goals, attempt,
        ...), so candidate 0 is the unscreened seed --, each measured by candidate_clearance_host, and retry_pick_host's
        choice among them.  center [len(goals), n]: as retry_seeds_host.  obstacles: None -- the problem's own -- or
        [m, 4], one scene for every goal, or a sequence of one [m_g, 4] per goal in `goals`.
        Returns (q [G, n] the picked angles, pick [G] int, clearance [G] of the pick); the whole table is left in
        self.last_screen = (q_c [C, G, n], clearance_c [C, G])."""
        C = check_retry_candidates(candidates)
        if not clear_tol > 0:
            raise ValueError("clear_tol must be positive")
        goals = np.asarray(goals, dtype=np.int64).reshape(-1)
        G = len(goals)
        q_c = np.stack([retry_seeds_host((int(seed) + c * RETRY_CANDIDATE_STEP) & (2 ** 64 - 1), goals, attempt, q_lo, q_hi,
                                         center=center, spread=spread) for c in range(C)], axis=0)
        per_goal = obstacles is not None and not (isinstance(obstacles, np.ndarray) and obstacles.ndim == 2)
        if per_goal:
            obstacles = [np.asarray(o, dtype=np.float64).reshape(-1, 4) for o in obstacles]
            if len(obstacles) != G:
                raise ValueError(f"obstacles must be one [m, 4] array or one per goal ({G}), got {len(obstacles)}")
            cl = np.empty((C, G))
            for g in range(G):
                cl[:, g] = self.candidate_clearance_host(q_c[:, g], clearance_mode, obstacles[g])
        else:
            cl = self.candidate_clearance_host(q_c.reshape(C * G, -1), clearance_mode, obstacles).reshape(C, G)
        pick = retry_pick_host(cl, clear_tol)
        self.last_screen = (q_c, cl)
        cols = np.arange(G)
        return q_c[pick, cols], pick, cl[pick, cols]

    def solve_trajectory(self, T_path, q_start, return_Y=False, retries=0, retry_seed=0, pos_tol=0.01, rot_tol=0.01,
                         clear_tol=1e-4, retry_spread=0.0, q_limits=None, clearance_mode="nodes", sweep=None, scenes=None,
                         scene_id=None, retry_candidates=1):
        """Path tracking among the obstacles: B paths of L waypoints, T_path [B, L, 4, 4].  Waypoint 0
        is seeded by q_start ([B,n] or [n]), waypoint l by the joint angles recovered at waypoint l-1,
        which never leave the device: L calls of gik_anchored_ik_batch_seeded on one stream, one
        workspace, one synchronisation at the end.  With retries=0 a waypoint that fails still seeds the
        next one (no retry): check info["stop"], info["f(x)"] and info["clearance"].

        retries > 0: every waypoint is a solve(T[:, l], q_init=previous angles, retries=..., ...) -- a failed
        waypoint (the rule of solve(), clearance included) is solved again before it seeds the next one, and
        the rescued angles are what the next waypoint starts from.  retry_spread > 0 keeps the restarts within
        that many radians of the previous waypoint's angles.  The stream then synchronises once per attempt
        and waypoint; info["attempt"] [B, L] int32 says which attempt each waypoint holds.  retry_candidates (1 .. 16;
        above 1 needs retries > 0) is passed on to every waypoint's solve: its restarts screen that many candidate seeds.

        clearance_mode: as in solve() -- which clearance info["clearance"] holds and the rule reads; with
        link_hinges=True clearance_mode="links" has hinges behind it at every waypoint.
        sweep=S (an integer >= 1; the problem must have links): adds info["sweep_clearance"] [B, L], the minimum link
        clearance over S + 1 joint-space samples between waypoint l-1's answer (q_start for waypoint 0) and waypoint
        l's (sweep_clearance(q[:, l-1], q[:, l], S)), one gik_anchored_sweep_clearance call per waypoint on the rows
        already on the device.  It is sampled, not conservative -- pick S from the joint step between waypoints --
        and it is reported only: the restart rule does not read it.  With clearance_mode="links+self" the same call
        (gik_anchored_sweep_clearances, one realization of the samples) also gives info["sweep_self_clearance"] [B, L].

        scenes (scene_set(...)) with scene_id: [B] ints -- a scene per path -- or [B, L] -- a scene per waypoint, which
        is a moving obstacle: waypoint l of path b is solved among the spheres of scene scene_id[b, l].  Optional with
        one scene.  sweep= together with scenes= is refused (the sweep clearance reads the problem's own obstacles).

        Returns q [B, L, n], Y [B, L, N_robot, 3] (None unless return_Y), and info with [B, L] arrays
        iterations, inner_iterations, stop, f(x), gradnorm, pos_err, rot_err, clearance, plus
        solve_time (seconds, whole path)."""
        T = np.asarray(T_path, dtype=float)
        B = T.shape[0]
        q0 = _seed_angles(q_start, B, self.robot.n, "q_start")
        check_clearance_mode(clearance_mode, len(self.link_names) > 0, self.self_pairs is not None)
        if sweep is not None and scenes is not None:
            raise ValueError("sweep= with scenes= is not supported: the sweep clearance measures the problem's own obstacles")
        ids = None      # [L, B] int32 on the device: waypoint-major, a row per step
        if scenes is not None:
            L = T.shape[1]
            shape = np.shape(scene_id) if scene_id is not None else ()
            per_waypoint = len(shape) == 2
            ids = scenes.ids(scene_id, (B, L) if per_waypoint else (B,))
            if ids is not None:
                ids = ids.T.contiguous() if per_waypoint else ids[None].expand(L, B).contiguous()
        elif scene_id is not None:
            raise ValueError("scene_id needs scenes=")
        if sweep is not None:
            sweep = self._check_samples(sweep, "sweep")
            if not len(self.link_names):
                raise ValueError("sweep needs a link set: this problem was built without links")
        retry = self._retry_args(retries, retry_seed, pos_tol, rot_tol, clear_tol, retry_spread, q_limits,
                                 retry_candidates=retry_candidates)
        tpl, base = self.template, self.base.template
        planes, shared, nbytes = ["clearance"], {}, None
        plan = anchored_call_plan(True, True, clearance_mode, scenes is not None, retries, retry.get("retry_candidates", 1))
        if plan.restart:
            # one restart workspace for all waypoints, sized by the plan every waypoint's anchored_ik runs on: it holds the
            # anchored scratch too; without restarts it serves attempt 0 of the restart entry alone
            nbytes = tpl.anchored_plan_ws_bytes(base, B, plan)
        else:
            shared["ws"] = tpl.alloc_anchored_buffers(base, B)["ws"]
        if retry:
            planes.append("attempt")
        sweep_self = bool(sweep) and clearance_mode == "links+self"
        if sweep:      # one workspace for all waypoints
            planes.append("sweep_clearance")
            if sweep_self:
                planes.append("sweep_self_clearance")
            sweep_ws = workspace(tpl.anchored_sweep_ws_bytes(base, B, sweep), tpl.device)

        waypoint = iter(range(T.shape[1]))

        def step(T_l, q_prev, out):
            l = next(waypoint)
            tpl.anchored_ik(base, T_l, q_init=q_prev, out=out, clearance=True, clearance_mode=clearance_mode, scenes=scenes,
                            scene_id=None if ids is None else ids[l], scene_id_checked=True, **retry)
            if sweep_self:
                tpl.anchored_sweep_clearances(base, q_prev, out["q"], sweep, link_out=out["sweep_clearance"],
                                              self_out=out["sweep_self_clearance"], ws=sweep_ws)
            elif sweep:
                tpl.anchored_sweep_clearance(base, q_prev, out["q"], sweep, out=out["sweep_clearance"], ws=sweep_ws)

        return _track(tpl, T, q0, (tpl.full_N, 3), return_Y, planes, step, shared, nbytes, retry.get("q_limits"))

    @staticmethod
    def _check_samples(samples, name="samples"):
        if isinstance(samples, bool) or int(samples) != samples or samples < 1:
            raise ValueError(f"{name} must be an integer of at least 1, got {samples!r}")
        return int(samples)

    def link_clearance(self, Y_full, obstacles=None):
        """min over (link, obstacle) of the distance from the sphere to the link's capsule per goal: the host mirror of
        gik_anchored_link_clearance, the same operations in the same order.  Y_full [B, N_robot, 3] (numpy).  For a
        link from a to b and a sphere (c, r):  d = b - a, L2 = d.d, u = c - a, t = L2 > 0 ? min(max(u.d / L2, 0), 1) : 0,
        v = u - t d, value = |v| - r - link_radius.  >= 0: no part of a link is inside a sphere.  With radius 0 and the
        skeleton it is <= clearance(Y_full, include_goal=True).  No link or no obstacle: +inf; a NaN coordinate of a
        link end: NaN for that goal.  obstacles: [m, 4] (centre, radius) to measure against instead of the problem's own
        (a scene of scene_set)."""
        Y = np.asarray(Y_full, dtype=np.float64)
        if Y.ndim == 2:
            Y = Y[None]
        B = Y.shape[0]
        obstacles = self.obstacles if obstacles is None else np.asarray(obstacles, dtype=np.float64).reshape(-1, 4)
        if len(self.link_rows) == 0 or len(obstacles) == 0:
            return np.full(B, np.inf)
        a = Y[:, self.link_rows[:, 0], None, :]                    # [B, n_link, 1, 3]
        b = Y[:, self.link_rows[:, 1], None, :]
        c = obstacles[None, None, :, :3]                          # [1, 1, n_obs, 3]
        r2 = obstacles[:, 3] ** 2                                 # (what the template holds: the squared radius)
        d, L2, u, t = _link_foot(a, b, c)                         # (L2 [B, n_link, 1], t [B, n_link, n_obs])
        with np.errstate(invalid="ignore"):
            v = u - t[..., None] * d
            val = np.sqrt(_dot3(v, v)) - np.sqrt(r2)[None, None, :] - self.link_radius[None, :, None]
            val = np.where(np.isnan(L2), np.nan, val)
        return _nan_min(val, axis=(1, 2))

    def self_clearance(self, Y_full):
        """min over the self pairs (l, m) of the distance between the capsules of links l and m per goal: the host mirror
        of gik_anchored_self_clearance, the same operations in the same order.  Y_full [B, N_robot, 3] (numpy).  With
        link l from a1 to b1, link m from a2 to b2 and d of _segment_feet(a1, b1, a2, b2):  value = sqrt(d) - rho_l - rho_m.
        >= 0: no two measured links overlap.  No pair: +inf; a NaN coordinate of a measured link's end: NaN for that
        goal.  Reads self.link_rows, self.link_radius and self.self_pairs only."""
        Y = np.asarray(Y_full, dtype=np.float64)
        if Y.ndim == 2:
            Y = Y[None]
        B = Y.shape[0]
        pairs = None if self.self_pairs is None else np.asarray(self.self_pairs, dtype=np.int64).reshape(-1, 2)
        if pairs is None or len(pairs) == 0:
            return np.full(B, np.inf)
        rows, rho = np.asarray(self.link_rows), np.asarray(self.link_radius, dtype=np.float64)
        l, m = pairs[:, 0], pairs[:, 1]
        a1, b1 = Y[:, rows[l, 0]], Y[:, rows[l, 1]]                # [B, P, 3]
        a2, b2 = Y[:, rows[m, 0]], Y[:, rows[m, 1]]
        with np.errstate(invalid="ignore"):
            return _nan_min(np.sqrt(_segment_feet(a1, b1, a2, b2)[3]) - rho[l][None, :] - rho[m][None, :], axis=1)

    def sweep_self_clearance_host(self, q_a, q_b, samples):
        """The numpy mirror of sweep_self_clearance: self_clearance of BatchProblem.seed_points at every sample, the
        minimum over the samples, NaN if any sample is NaN."""
        return self._sweep_min_host(q_a, q_b, samples, self.self_clearance)

    def sweep_self_clearance(self, q_a, q_b, samples):
        """Joint angles q_a, q_b [B, n] -> device tensor [B]: the minimum self clearance over the samples + 1
        configurations of sweep_clearance (gik_anchored_sweep_clearances; the problem must have self_pairs).  Like it, the
        sweep is SAMPLED, NOT CONSERVATIVE: two links can meet and part between two samples.
        sweep_self_clearance_host is the numpy mirror."""
        S = self._check_samples(samples)
        if self.self_pairs is None:
            raise ValueError("sweep_self_clearance needs self pairs: this problem was built without self_pairs")
        return self.template.anchored_sweep_clearances(self.base.template, q_a, q_b, S, link=False)[1]

    @staticmethod
    def link_foot_host(a, b, c):
        """One (link, sphere centre) pair -> (t, m, d): the foot parameter of link_clearance, m = (1 - t) a + t b - c and
        d = m.m -- the operations of the device pair function (anch_link_foot) in its order."""
        a, b, c = (np.asarray(x, dtype=np.float64) for x in (a, b, c))
        t = _link_foot(a, b, c)[3]
        m = ((1.0 - t) * a + t * b) - c
        return float(t), m, float(_dot3(m, m))

    def link_ends_host(self, Y_free, W, goal_anchor):
        """Per link: ((A, W_A, i_A), (B, W_B, i_B)) -- position, direction and free-node index of either end at the point
        Y_free [Nf, 3]; a constant end (base anchor, or goal anchor from goal_anchor [n_goal * 3]) has W = 0 and index None."""
        Y, W = np.asarray(Y_free, dtype=np.float64), np.asarray(W, dtype=np.float64)
        apos = np.array(self.anchor_pos, dtype=np.float64)
        if self.n_goal_anchor:
            apos[len(apos) - self.n_goal_anchor:] = np.asarray(goal_anchor, dtype=np.float64).reshape(-1, 3)
        fidx = {n: f for f, n in enumerate(self.free)}
        aidx = {n: r for r, n in enumerate(self.anchors)}
        end = lambda r: (Y[fidx[r]], W[fidx[r]], fidx[r]) if r in fidx else (apos[aidx[r]], np.zeros(3), None)   # noqa: E731
        return [(end(int(ra)), end(int(rb))) for ra, rb in self.link_rows]

    def link_hinge_terms_host(self, Y_free, W, goal_anchor, frozen_t=None):
        """(f, G, H) of the link hinges alone at one point: Y_free, W [Nf, 3], goal_anchor [n_goal * 3], in the
        conventions of the anchored kernels' known answers (f = sum res^2, G = 1/2 grad f, H = 1/2 Hess f [W]).  Per
        (link, sphere), with A, B the link's ends, R = r + rho and (t, m, d) of link_foot_host:
            res = R^2 - d,  active <=> res > 0,  c = d - R^2
            f += res^2;  G_A += (1 - t) 2 c m;  G_B += t 2 c m
            w = (1 - t) W_A + t W_B;  H_A += (1 - t) 2 (2 (m.w) m + c w);  H_B += t 2 (2 (m.w) m + c w)
        Contributions to a constant end are dropped; a link with two constant ends has no hinge.  The gradient is exact
        (envelope theorem), H is the frozen-t model the solve kernel uses.  The full reference of a point is the
        free-free and anchor terms plus this.  frozen_t: {(link, obstacle): t} to evaluate at instead of the foot
        parameters of this point (what a finite difference of the frozen-t gradient needs); active pairs' t come back
        in self.last_link_t."""
        Y = np.asarray(Y_free, dtype=np.float64)
        f, G, H = 0.0, np.zeros_like(Y), np.zeros_like(Y)
        self.last_link_t = {}
        for l, ((A, WA, ia), (B, WB, ib)) in enumerate(self.link_ends_host(Y, W, goal_anchor)):
            if ia is None and ib is None:
                continue
            rho = float(self.link_radius[l])
            for o, (cx, cy, cz, r) in enumerate(self.obstacles):
                C = (cx, cy, cz)
                t, m, d = self.link_foot_host(A, B, C)
                if frozen_t is not None:
                    if (l, o) not in frozen_t:
                        continue
                    t = frozen_t[(l, o)]
                    m = ((1.0 - t) * A + t * B) - np.array(C)
                    d = float(m[0] * m[0] + m[1] * m[1] + m[2] * m[2])
                R = float(np.sqrt(r * r)) + rho      # (the template holds r^2)
                res = R * R - d
                if not res > 0.0 and frozen_t is None:
                    continue
                self.last_link_t[(l, o)] = t
                c = -res
                f += res * res
                om = (1.0 - t) * WA + t * WB
                hv = 2.0 * (2.0 * (m @ om) * m + c * om)
                if ia is not None:
                    G[ia] += (1.0 - t) * 2.0 * c * m
                    H[ia] += (1.0 - t) * hv
                if ib is not None:
                    G[ib] += t * 2.0 * c * m
                    H[ib] += t * hv
        return f, G, H

    @staticmethod
    def self_feet_host(a1, b1, a2, b2):
        """One (link, link) pair -> (s, t, v, d): the foot parameters of self_clearance, v = (a1 + s d1) - (a2 + t d2)
        and d = v.v -- the operations of the device pair function (anch_self_feet) in its order, and the function
        self_clearance takes its distance from."""
        s, t, v, d = _segment_feet(*(np.asarray(p, dtype=np.float64) for p in (a1, b1, a2, b2)))
        return float(s), float(t), v, float(d)

    def self_hinge_terms_host(self, Y_free, W, goal_anchor, frozen_st=None):
        """(f, G, H) of the self hinges alone at one point: Y_free, W [Nf, 3], goal_anchor [n_goal * 3], in the
        conventions of link_hinge_terms_host (f = sum res^2, G = 1/2 grad f, H = 1/2 Hess f [W]).  Per self pair (l, m),
        with A1, B1 the ends of link l, A2, B2 those of link m, R = rho_l + rho_m and (s, t, v, d) of self_feet_host:
            res = R^2 - d,  active <=> res > 0,  c = -res,  w = (1 - s, s, -(1 - t), -t) on (A1, B1, A2, B2)
            f += res^2;  G_P += w_P 2 c v;  om = sum_Q w_Q W_Q;  H_P += w_P 2 (2 (v.om) v + c om)
        Contributions to a constant end are dropped (its W is 0); a pair whose four ends are constants adds to f alone.
        The gradient is exact wherever the closest points are unique (envelope theorem), H is the frozen-(s, t) model
        the solve kernel uses.  frozen_st: {pair: (s, t)} to evaluate at instead of the feet of this point (what a
        finite difference of the frozen gradient needs); active pairs' (s, t) come back in self.last_self_st."""
        Y = np.asarray(Y_free, dtype=np.float64)
        f, G, H = 0.0, np.zeros_like(Y), np.zeros_like(Y)
        self.last_self_st = {}
        if self.self_pairs is None:
            return f, G, H
        ends = self.link_ends_host(Y, W, goal_anchor)
        for p, (l, m) in enumerate(np.asarray(self.self_pairs).tolist()):
            (A1, W1, i1), (B1, X1, j1) = ends[l]
            (A2, W2, i2), (B2, X2, j2) = ends[m]
            s, t, v, d = self.self_feet_host(A1, B1, A2, B2)
            if frozen_st is not None:
                if p not in frozen_st:
                    continue
                s, t = frozen_st[p]
                v = (A1 + s * (B1 - A1)) - (A2 + t * (B2 - A2))
                d = float(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            R = float(self.link_radius[l]) + float(self.link_radius[m])
            res = R * R - d
            if not res > 0.0 and frozen_st is None:
                continue
            self.last_self_st[p] = (s, t)
            c = -res
            f += res * res
            w = (1.0 - s, s, -(1.0 - t), -t)
            om = w[0] * W1 + w[1] * X1 + w[2] * W2 + w[3] * X2
            hv = 2.0 * (2.0 * (v @ om) * v + c * om)
            for wP, iP in zip(w, (i1, j1, i2, j2)):
                if iP is not None:
                    G[iP] += wP * 2.0 * c * v
                    H[iP] += wP * hv
        return f, G, H

    def sweep_points(self, q_a, q_b, samples):
        """The samples + 1 configurations of a sweep, [samples + 1, B, n]: q_s = (1 - w) q_a + w q_b with w = s / samples
        (two rounded products, one rounded sum -- the bits the device writes; s = 0 is q_a and s = samples is q_b)."""
        S = self._check_samples(samples)
        qa, qb = np.asarray(q_a, dtype=np.float64), np.asarray(q_b, dtype=np.float64)
        if qa.ndim != 2 or qa.shape != qb.shape:
            raise ValueError("q_a and q_b must both have shape [B, n]")
        w = np.arange(S + 1, dtype=np.float64)[:, None, None] / np.float64(S)
        return (1.0 - w) * qa[None] + w * qb[None]

    def sweep_clearance_host(self, q_a, q_b, samples):
        """The numpy mirror of sweep_clearance: link_clearance of BatchProblem.seed_points at every sample, the minimum
        over the samples, NaN if any sample is NaN."""
        return self._sweep_min_host(q_a, q_b, samples, self.link_clearance)

    def _sweep_min_host(self, q_a, q_b, samples, clearance):
        """clearance (a mirror: full point matrices -> [B]) of BatchProblem.seed_points at every sample of a sweep, and
        the minimum over the samples."""
        qs = self.sweep_points(q_a, q_b, samples)
        S1, B, n = qs.shape
        return _nan_min(clearance(self.base.seed_points(qs.reshape(S1 * B, n))).reshape(S1, B), axis=0)

    def sweep_clearance(self, q_a, q_b, samples):
        """Joint angles q_a, q_b [B, n] -> device tensor [B]: the minimum link clearance over the samples + 1
        configurations q_s = (1 - s / samples) q_a + (s / samples) q_b, s = 0 .. samples, each realized by forward
        kinematics (gik_anchored_sweep_clearance; the problem must have links).  The sweep is SAMPLED, NOT
        CONSERVATIVE: a link can pass through a sphere between two samples.  Pick `samples` from the joint step -- a
        link of length L turning by dq moves its far end by about L dq, so samples >= L max|q_b - q_a| / tolerance
        keeps what is missed below the tolerance.  sweep_clearance_host is the numpy mirror."""
        S = self._check_samples(samples)
        if not len(self.link_names):
            raise ValueError("sweep_clearance needs a link set: this problem was built without links")
        return self.template.anchored_sweep_clearance(self.base.template, q_a, q_b, S)

    def clearance(self, Y_full, include_goal=False, obstacles=None):
        """min over (p-node of the robot, obstacle) of |p - centre| - radius per goal (>= 0: no joint point
        inside a sphere, the sense of graph_base.py:205-211; a link BETWEEN two joint points can still cross
        one -- link_clearance).  Y_full [B, N_robot, 3] (numpy).
        The end effector p_n sits where the goal puts it (a constant of the problem), so it only
        counts with include_goal=True.  obstacles: [m, 4] (centre, radius) to measure against instead of the problem's
        own (a scene of scene_set); none: +inf."""
        g = self.base.graph
        pn = [g.index(f"p{i}") for i in range(1, self.robot.n + (1 if include_goal else 0))]
        P = np.asarray(Y_full)[:, pn]                                            # [B, n, 3]
        if obstacles is None:
            obstacles = self.obstacles
        else:
            obstacles = np.asarray(obstacles, dtype=np.float64).reshape(-1, 4)
            if len(obstacles) == 0:
                return np.full(len(P), np.inf)
        d = np.linalg.norm(P[:, :, None, :] - obstacles[None, None, :, :3], axis=-1)
        return (d - obstacles[None, None, :, 3]).min(axis=(1, 2))


# BatchProblem objects (device handles) of recent solve_batch / solve_with_riemannian calls.  The
# reference re-reads the graph on every call (riemannian_solver.py:220-234), so the key is the
# CONTENT a BatchProblem is built from -- edge pattern, distances, limits, anchor positions, robot
# frames -- not the identity of the graph object: a graph mutated in place (clear_obstacles +
# add_spherical_obstacle, set_limits, ...) gets a fresh problem.  Least recently used entries are
# dropped (their device handles are freed by Template.__del__).
_PROBLEM_CACHE = collections.OrderedDict()
_PROBLEM_CACHE_MAX = 8


def graph_fingerprint(graph):
    """Content hash of everything BatchProblem reads from a problem graph."""
    h = hashlib.blake2b(digest_size=16)
    h.update(repr((type(graph).__name__, graph.dim, graph.number_of_nodes(), tuple(graph.node_ids),
                   float(getattr(graph, "axis_length", 0.0)))).encode())
    for a in (graph.edge, graph.dist, graph.lower, graph.upper):
        h.update(np.ascontiguousarray(a).tobytes())
    if hasattr(graph, "bounded"):
        h.update(repr(graph.bounded).encode() if not isinstance(graph.bounded, np.ndarray)
                 else np.ascontiguousarray(graph.bounded).tobytes())
    for name in graph.node_ids:
        pos = graph.nodes[name].get(POS)
        h.update(b"-" if pos is None else np.asarray(pos, dtype=float).tobytes())
    h.update(np.ascontiguousarray(graph.robot.T0_array()).tobytes())
    lb, ub = graph.robot.limits_arrays()
    h.update(np.asarray(lb, dtype=float).tobytes() + np.asarray(ub, dtype=float).tobytes())
    return h.hexdigest()


def _problem_for(graph, use_limits=True, params=None, device=None, goal="pose"):
    kinds = goal_kinds(goal, len(graph.robot.end_effectors))
    key = (graph_fingerprint(graph), bool(use_limits),
           None if not params else tuple(sorted(params.items())), None if device is None else str(device), kinds)
    prob = _PROBLEM_CACHE.get(key)
    if prob is None:
        prob = _PROBLEM_CACHE[key] = BatchProblem(graph, use_limits, params, device, goal=kinds)
        while len(_PROBLEM_CACHE) > _PROBLEM_CACHE_MAX:
            _PROBLEM_CACHE.popitem(last=False)
    else:
        _PROBLEM_CACHE.move_to_end(key)
        prob.graph = graph      # same content, possibly another object: recover through the caller's
    return prob


def clear_problem_cache():
    _PROBLEM_CACHE.clear()
    _closure_templates.clear()


def _seed_angles(q_init, B, n, name="q_init"):
    """[B,n] or [n] (broadcast) finite joint angles -> [B,n] float array; ValueError otherwise."""
    q = q_init.detach().cpu().numpy() if isinstance(q_init, torch.Tensor) else np.asarray(q_init, dtype=float)
    q = np.asarray(q, dtype=float)
    if q.shape == (n,):
        q = np.broadcast_to(q, (B, n))
    if q.shape != (B, n):
        raise ValueError(f"{name} must have shape [{B}, {n}] or [{n}], got {list(q.shape)}")
    if not np.all(np.isfinite(q)):
        raise ValueError(f"{name} has non-finite entries")
    return np.ascontiguousarray(q)


def _retry_kwargs(retries, retry_seed, pos_tol, rot_tol, q_limits, n, has_center=True, **anchored):
    """The restart keywords of one call, checked here before any device call: {} with retries == 0, else what
    Template.ik takes -- retries, retry_seed, pos_tol, rot_tol and q_limits as the checked (lo, hi) -- and, for
    Template.anchored_ik, its own two: anchored = clear_tol and retry_spread (has_center: the call has a q_init)."""
    if not retries:
        return {}
    retries, lo, hi = check_retry_args(retries, pos_tol, rot_tol, q_limits, n, has_center=has_center, **anchored)
    return dict(retries=retries, retry_seed=retry_seed, pos_tol=pos_tol, rot_tol=rot_tol, q_limits=(lo, hi), **anchored)


def retry_uniform_host(seed, goals, attempt, n):
    """The restart generator's uniform numbers in [0, 1), [len(goals), n]: splitmix64's finaliser over the
    counter of (goal, attempt, joint) in uint64 arithmetic -- bit for bit what retry_seed_kernel draws
    (include/graphik_amd.h)."""
    if not 0 <= int(attempt) <= 63 or not 0 < int(n) <= 125:
        raise ValueError("attempt must be within 0 .. 63 and n within 1 .. 125")
    u64 = np.uint64
    g = np.asarray(goals, dtype=np.int64).reshape(-1)
    if np.any(g < 0):
        raise ValueError("goal indices must not be negative")
    with np.errstate(over="ignore"):
        c = (g.astype(u64)[:, None] * u64(64) + u64(int(attempt))) * u64(128) + np.arange(n, dtype=u64)[None, :] + u64(1)
        z = u64(int(seed) & (2 ** 64 - 1)) + u64(0x9E3779B97F4A7C15) * c
        z ^= z >> u64(30)
        z *= u64(0xBF58476D1CE4E5B9)
        z ^= z >> u64(27)
        z *= u64(0x94D049BB133111EB)
        z ^= z >> u64(31)
    return (z >> u64(11)).astype(np.float64) * 2.0 ** -53


def retry_seeds_host(seed, goals, attempt, q_lo, q_hi, center=None, spread=0.0):
    """Host mirror of gik_retry_seeds: the joint angles [len(goals), n] that restart `attempt` of goals
    `goals` starts from, q = q_lo + u (q_hi - q_lo) with u from retry_uniform_host.  A function of
    (seed, goal, attempt, joint) alone; the same bits as the device draws.

    spread > 0 (local mode of gik_anchored_retry_seeds): center [len(goals), n] holds the centre row of
    each goal in `goals`, and q = min(max(center + spread (2u - 1), q_lo), q_hi) with the same u."""
    lo, hi = np.asarray(q_lo, dtype=np.float64), np.asarray(q_hi, dtype=np.float64)
    u = retry_uniform_host(seed, goals, attempt, len(lo))
    if not spread >= 0:
        raise ValueError("spread must be at least 0")
    if spread == 0:
        return lo[None, :] + u * (hi - lo)[None, :]
    if center is None:
        raise ValueError("spread > 0 needs the centre rows")
    c = np.asarray(center, dtype=np.float64)
    if c.shape != u.shape:
        raise ValueError(f"center must have shape {list(u.shape)}, got {list(c.shape)}")
    t = 2.0 * u - 1.0                                   # exact: u is a 53-bit fraction
    return np.minimum(np.maximum(c + np.float64(spread) * t, lo[None, :]), hi[None, :])


def retry_pick_host(clearance, clear_tol=1e-4):
    """Host mirror of retry_pick (gik_retry.hip.h): clearance [C, G] of C candidates per goal -> [G] the picked
    candidate.  The first c with clearance >= -clear_tol (+inf qualifies); none: the c of the largest clearance, the
    lowest on a tie, a NaN never winning; all NaN: 0."""
    cl = np.asarray(clearance, dtype=np.float64)
    if cl.ndim == 1:
        cl = cl[:, None]
    with np.errstate(invalid="ignore"):
        clear = cl >= -clear_tol
        largest = (cl == np.where(np.isnan(cl), -np.inf, cl).max(axis=0)[None, :]) & ~np.isnan(cl)
    # (argmax takes the first True; a column without one -- all NaN -- gives 0)
    return np.where(clear.any(axis=0), clear.argmax(axis=0), largest.argmax(axis=0)).astype(np.int64)


def atlas_nearest_host(keys, goal_keys, K, chunk=64):
    """Host mirror of gik_atlas_nearest: keys [M, W] (one row per atlas row), goal_keys [G, W] -> (nbr [G, K] int32,
    dist [G, K]): per goal the K rows with the smallest (d, m), ascending, d = (...((t0 t0 + t1 t1) + t2 t2) ...) with
    t_c = goal_keys[g, c] - keys[m, c] -- every difference, product and sum rounded on its own, in column order, so the
    bits of the device's --, by a stable sort.  A NaN or infinite d is never listed; where fewer than K rows are listed
    the rest is -1 / +inf.  chunk: goals per pass (the table of distances is [chunk, M])."""
    keys = np.asarray(keys, dtype=np.float64)
    g = np.asarray(goal_keys, dtype=np.float64)
    if keys.ndim != 2 or g.ndim != 2 or keys.shape[1] != g.shape[1]:
        raise ValueError(f"keys [M, W] and goal_keys [G, W] must share W, got {list(keys.shape)} and {list(g.shape)}")
    K = check_atlas_k(K, None, "K")
    G, M, W = g.shape[0], keys.shape[0], keys.shape[1]
    nbr = np.full((G, K), -1, dtype=np.int32)
    dist = np.full((G, K), np.inf)
    take = min(K, M)
    for s in range(0, G, chunk):
        gs = g[s:s + chunk]
        with np.errstate(invalid="ignore", over="ignore"):
            t = gs[:, None, 0] - keys[None, :, 0]
            d = t * t
            for c in range(1, W):
                t = gs[:, None, c] - keys[None, :, c]
                d = d + t * t
        d = np.where(np.isfinite(d), d, np.inf)
        order = np.argsort(d, axis=1, kind="stable")[:, :take]
        dk = np.take_along_axis(d, order, axis=1)
        nbr[s:s + chunk, :take] = np.where(np.isfinite(dk), order, -1)
        dist[s:s + chunk, :take] = dk
    return nbr, dist


class SeedAtlas:
    """A configuration atlas for goal-aware seeds of the anchored solve (AnchoredProblem.solve(..., atlas=)): joint
    configurations that are clear of the room, each with its key -- the positions its end effector's goal nodes take.
    Holds q [M, n], keys [M, W] and clearance [M] as numpy arrays, count = M, width = W and, once uploaded, the device
    tensors d_q [M, n] and d_keys [W, M] (component-major, what gik_atlas_nearest reads).  Built on the host by
    AnchoredProblem.seed_atlas or from_configurations; the upload is the only device work."""

    def __init__(self, q, keys, clearance, device=None):
        self.q, self.keys, self.clearance = (np.array(a, dtype=np.float64, order="C") for a in (q, keys, clearance))      # (copies)
        if self.q.ndim != 2 or self.keys.ndim != 2 or len(self.keys) != len(self.q) or self.clearance.shape != (len(self.q),):
            raise ValueError("a SeedAtlas takes q [M, n], keys [M, W] and clearance [M]")
        if len(self.q) == 0:
            raise ValueError("the atlas is empty: no configuration passed the clearance filter")
        self.count, self.width = int(self.keys.shape[0]), int(self.keys.shape[1])
        self.d_q = self.d_keys = None
        if device is not None:
            self.upload(device)

    def upload(self, device):
        """Copy q and the component-major keys to `device` (once; a later call moves them)."""
        self.d_q = torch.from_numpy(self.q).to(device)
        self.d_keys = torch.from_numpy(np.array(self.keys.T, order="C")).to(device)
        return self

    @classmethod
    def from_configurations(cls, problem, q, clearance_mode="nodes", clear_tol=1e-4, keep_clear_only=False, obstacles=None):
        """The atlas of the caller's own rows q [M, n] -- the answers of an earlier batch, say -- for the AnchoredProblem
        `problem`: keys from its robot graph's realization (base.seed_points, the goal rows), clearance from
        candidate_clearance_host(q, clearance_mode, obstacles).  keep_clear_only: keep the rows with clearance >=
        -clear_tol only (the default keeps every row).  Uploaded unless the problem is host-only."""
        q = np.atleast_2d(np.asarray(q, dtype=np.float64))
        if q.ndim != 2 or q.shape[1] != problem.robot.n:
            raise ValueError(f"q must have shape [M, {problem.robot.n}], got {list(q.shape)}")
        if not clear_tol > 0:
            raise ValueError("clear_tol must be positive")
        rows = 8192      # per pass: the mirrors form [rows, links, obstacles, 3] arrays
        cl = np.concatenate([problem.candidate_clearance_host(q[s:s + rows], clearance_mode, obstacles) for s in range(0, len(q), rows)])
        if keep_clear_only:
            with np.errstate(invalid="ignore"):
                keep = cl >= -clear_tol
            q, cl = q[keep], cl[keep]
        goal_rows = problem.base.goal_nodes
        keys = np.concatenate([problem.base.seed_points(q[s:s + rows])[:, goal_rows].reshape(-1, 3 * len(goal_rows))
                               for s in range(0, len(q), rows)]) if len(q) else np.zeros((0, 3 * len(goal_rows)))
        return cls(q, keys, cl, None if problem.template is None else problem.template.device)


def anchored_retry_failed(stop, pos_err, rot_err, clearance, pos_tol=0.01, rot_tol=0.01, clear_tol=1e-4):
    """Host mirror of the failure rule of gik_anchored_ik_batch_retry (include/graphik_amd.h), on arrays."""
    stop, pos_err, rot_err, clearance = (np.asarray(a) for a in (stop, pos_err, rot_err, clearance))
    with np.errstate(invalid="ignore"):
        return (stop != 0) | ~(pos_err <= pos_tol) | ~(rot_err <= rot_tol) | ~(clearance >= -clear_tol)


def anchored_retry_score(pos_err, rot_err, clearance, pos_tol=0.01, rot_tol=0.01, clear_tol=1e-4):
    """... of the score: max(pos_err / pos_tol, rot_err / rot_tol, max(0, -clearance) / clear_tol), +inf for a NaN."""
    pos_err, rot_err, clearance = (np.asarray(a, dtype=np.float64) for a in (pos_err, rot_err, clearance))
    with np.errstate(invalid="ignore"):
        s = np.maximum(np.maximum(pos_err / pos_tol, rot_err / rot_tol), np.maximum(0.0, -clearance) / clear_tol)
    return np.where(np.isnan(s), np.inf, s)          # (np.maximum propagates NaN)


def anchored_retry_better(new, old, pos_tol=0.01, rot_tol=0.01, clear_tol=1e-4):
    """... of the merge order: new / old = (stop, pos_err, rot_err, clearance) arrays -> does `new` replace `old`?
    A success beats a failure, within a class the smaller score wins, a NaN never wins, a tie keeps `old`."""
    tol = (pos_tol, rot_tol, clear_tol)
    ok_n, ok_o = ~anchored_retry_failed(*new, *tol), ~anchored_retry_failed(*old, *tol)
    return (ok_n & ~ok_o) | ((ok_n == ok_o) & (anchored_retry_score(*new[1:], *tol) < anchored_retry_score(*old[1:], *tol)))


def solve_batch(graph, T_goals, use_limits=True, params=None, device=None, Y_init=None, q_init=None,
                retries=0, retry_seed=0, pos_tol=0.01, rot_tol=0.01, goal="pose"):
    """Batched solve_with_riemannian.  T_goals: [B,d+1,d+1] array or list of poses.
    Returns (q [B,n], Y [B,N,k], info dict of arrays).

    goal: "pose" (the default), "position", or a sequence of those with one entry per robot.end_effectors.  A position
    goal pins the end effector's point and leaves its orientation free -- the reference's graph.from_pos({p_e: xyz}) with
    joint_variables(G_sol) without T_final; info["rot_err"] leaves such an end effector out (0.0 when all are
    positions), so the restart rule's rot_tol never fires for it.  When every end effector is a position, T_goals holds
    positions [B, d] or [B, n_ee, d] (pose arrays are accepted too: only their translations are read); with mixed kinds
    it holds poses as for "pose".  q_init, retries and every other argument combine with it unchanged.

    q_init (warm start): joint angles [B,n] or [n] (one seed for all goals), columns in
    robot.q_to_array order.  Each solve then starts from the realization of its seed -- the
    reference's RiemannianSolver.solve(D_goal, omega, Y_init=pos_from_graph(graph.realization(q_init)),
    bounds=None) -- instead of from bound smoothing + MDS; on the device pipeline that is one
    gik_ik_batch_seeded call, otherwise the host realization (BatchProblem.seed_points) feeds the
    device solve.  Y_init and q_init exclude each other.

    retries > 0 (restarts, device pipeline only): a goal that fails -- stop != 0, pos_err > pos_tol or
    rot_err > rot_tol -- is solved again up to `retries` (<= 63) times from joint angles drawn uniformly
    inside graph.robot.limits_arrays() (retry_seeds_host(retry_seed, [g], attempt, lo, hi) are goal g's),
    and the better answer is kept; info["attempt"] [B] int32 is the attempt each goal's answer comes
    from (0: the first).  With q_init the first attempt is seeded and the later ones are random.  Y_init
    cannot be combined with retries, and a graph off the device pipeline has none: ValueError."""
    T = np.stack([as_matrix(t) for t in T_goals]) if not isinstance(T_goals, np.ndarray) \
        else np.asarray(T_goals, dtype=float)
    if not (isinstance(goal, str) and goal == "pose"):
        T = goal_poses(T, goal_kinds(goal, len(graph.robot.end_effectors)), graph.dim)
    if q_init is not None:
        if Y_init is not None:
            raise ValueError("pass Y_init or q_init, not both")
        q_init = _seed_angles(q_init, T.shape[0], graph.robot.n)
    if retries and Y_init is not None:
        raise ValueError("retries > 0 cannot be combined with Y_init (pass q_init, or no start at all)")
    retry = _retry_kwargs(retries, retry_seed, pos_tol, rot_tol, graph.robot.limits_arrays() if retries else None, graph.robot.n)
    prob = _problem_for(graph, use_limits, params, device, goal)
    if retries and not prob.device_pipeline:
        raise ValueError("retries > 0 needs the device pipeline, which this graph is outside of")
    tpl = prob.template
    on_device = prob.device_pipeline and Y_init is None
    t0 = time.time()
    if on_device:
        # everything on the device: prepare or seed -> solve (with restarts) -> recover (gik_ik_batch[_seeded | _retry])
        res = tpl.ik(T, q_init=q_init, **retry)
    else:
        # the host prepares and recovers around the device solve; the clock starts after the preparation
        if q_init is not None:
            targets, Y0 = prob.targets_from_D(prob.assemble(T)[0]), prob.seed_points(q_init)
        else:
            targets, Y0 = prob.prepare(T)
            if Y_init is not None:
                Y0 = np.asarray(Y_init, dtype=float)
        t0 = time.time()
        res = tpl.solve(Y0, targets)
    torch.cuda.synchronize(tpl.device)
    dt = time.time() - t0
    Y = res["x"].cpu().numpy()
    if on_device:
        q, pos, rot = (res[key].cpu().numpy() for key in ("q", "pos_err", "rot_err"))
    else:
        q = prob.joint_variables(Y, T)
        pos, rot = prob.pose_errors(q, T)
    info = {"x": Y, "f(x)": res["f"].cpu().numpy(), "gradnorm": res["gradnorm"].cpu().numpy(),
            "iterations": res["iterations"].cpu().numpy(),
            "inner_iterations": res["inner_total"].cpu().numpy(),
            "stop": res["stop"].cpu().numpy(), "time": np.full(len(Y), dt / max(len(Y), 1)),
            "solve_time": dt, "pos_err": pos, "rot_err": rot,
            "attempt": res["attempt"].cpu().numpy() if retries else np.zeros(len(Y), dtype=np.int32)}
    return q, Y, info


def solve_trajectory(graph, T_path, q_start, use_limits=True, params=None, device=None, return_Y=False,
                     retries=0, retry_seed=0, pos_tol=0.01, rot_tol=0.01, goal="pose"):
    """Path tracking: B paths of L waypoints, each waypoint a warm-started solve_batch.

    T_path: [B, L, d+1, d+1] goal poses ([B, L, n_ee, 4, 4] for robots with several end effectors).
    Waypoint 0 is seeded by q_start ([B,n] or [n]); waypoint l by the joint angles recovered at
    waypoint l-1.  On the device pipeline those angles never leave the device: the L calls of
    gik_ik_batch_seeded are queued on one stream without a host synchronisation in between.  A
    waypoint whose solve fails (stop != 0, or a large pos_err) still seeds the next one; by default
    there is no retry -- check info["stop"] / info["pos_err"].

    goal: as in solve_batch; with position goals T_path holds positions [B, L, d] or [B, L, n_ee, d].

    retries > 0: every waypoint is a solve_batch(..., q_init=previous angles, retries=...) -- a failed
    waypoint is solved again from random joint angles (see solve_batch), and a rescued waypoint seeds
    the next one with its rescued angles.  Each waypoint then synchronises the stream once per attempt.

    Returns q [B, L, n], Y [B, L, N, k] (None unless return_Y), and info with [B, L] arrays
    iterations, inner_iterations, stop, f(x), gradnorm, pos_err, rot_err, attempt, plus solve_time
    (seconds, whole path)."""
    T = np.asarray(T_path, dtype=float)
    if not (isinstance(goal, str) and goal == "pose"):
        T = goal_poses(T, goal_kinds(goal, len(graph.robot.end_effectors)), graph.dim, lead=2)
    B, L = T.shape[:2]
    n = graph.robot.n
    q0 = _seed_angles(q_start, B, n, "q_start")
    retry = _retry_kwargs(retries, retry_seed, pos_tol, rot_tol, graph.robot.limits_arrays() if retries else None, n)
    prob = _problem_for(graph, use_limits, params, device, goal)
    if not prob.device_pipeline:
        qs, Ys, infos, dt = [], [], [], 0.0
        q_prev = q0
        own = {key: v for key, v in retry.items() if key != "q_limits"}      # (solve_batch reads the robot's limits itself)
        for l in range(L):
            q_prev, Y, info = solve_batch(graph, T[:, l], use_limits, params, device, q_init=q_prev, goal=goal, **own)
            qs.append(q_prev)
            Ys.append(Y)
            infos.append(info)
            dt += info["solve_time"]
        out = {key: np.stack([i[key] for i in infos], axis=1)
               for key in ("iterations", "inner_iterations", "stop", "f(x)", "gradnorm", "pos_err", "rot_err",
                           "attempt")}
        out["solve_time"] = dt
        return np.stack(qs, axis=1), (np.stack(Ys, axis=1) if return_Y else None), out
    tpl = prob.template
    shared = {"targets": torch.empty(B, tpl.T, dtype=torch.float64, device=tpl.device)}
    nbytes = tpl.retry_ws_bytes(B) if retry else None

    def step(T_l, q_prev, out):
        tpl.ik(T_l, out=out, q_init=q_prev, **retry)

    return _track(tpl, T, q0, (tpl.N, tpl.k), return_Y, ["attempt"], step, shared, nbytes, retry.get("q_limits"))


def _track(tpl, T, q0, Y_shape, return_Y, planes, step, shared, retry_ws_bytes=None, q_limits=None):
    """The tracking loop of both solve_trajectory functions: B paths of L waypoints T [B, L, ...] from the start angles
    q0 [B, n], on tpl's device.  step(T_l, q_prev, out) makes waypoint l's calls: goal poses T_l [B, ...], the angles
    q_prev [B, n] that seed it (q0, then waypoint l-1's answer -- they never leave the device), and `out`, its rows of
    the result storage: "Y" (row 0 every time unless return_Y), "stats", "q", "pos_err", "rot_err", one [B] row per
    name in `planes` ("attempt": int32, zero where no call writes it; the others float64) and what the waypoints
    share: `shared`, with retry_ws_bytes (the caller's restart workspace size in bytes) one restart workspace "retry_ws"
    and with q_limits = (q_lo, q_hi) one upload of the limits "q_lo" / "q_hi".  One synchronisation after the last
    waypoint.  Returns q [B, L, n], Y [B, L, *Y_shape] (None unless return_Y) and info: [B, L] arrays of the stats
    and the planes, plus solve_time."""
    B, L = T.shape[:2]
    dev = tpl.device
    f64 = dict(dtype=torch.float64, device=dev)
    Tw = torch.from_numpy(np.ascontiguousarray(np.swapaxes(T, 0, 1))).to(dev)     # [L, B, ...]: waypoint-major
    q_all = torch.empty(L, B, q0.shape[1], **f64)
    Y_all = torch.empty(L if return_Y else 1, B, Y_shape[0] * Y_shape[1], **f64)
    stats = _alloc_stats(L * B, dev)
    stats = stats.reshape(L, B, stats.shape[1])      # (no -1: B may be 0)
    rows ={name: torch.zeros(L, B, dtype=torch.int32, device=dev) if name == "attempt" else torch.empty(L, B, **f64)
            for name in ("pos_err", "rot_err", *planes)}
    shared = dict(shared)
    if retry_ws_bytes is not None:
        shared["retry_ws"] = workspace(retry_ws_bytes, dev)
    if q_limits is not None:
        shared.update(q_lo=torch.from_numpy(q_limits[0]).to(dev), q_hi=torch.from_numpy(q_limits[1]).to(dev))
    q_prev = torch.from_numpy(q0).to(dev)      # (its own tensor: the start angles outlive waypoint 0's solve)
    torch.cuda.synchronize(dev)
    t0 = time.time()
    for l in range(L):
        step(Tw[l], q_prev, {"Y": Y_all[l if return_Y else 0], "stats": stats[l], "q": q_all[l],
                             **{name: plane[l] for name, plane in rows.items()}, **shared})
        q_prev = q_all[l]
    torch.cuda.synchronize(dev)
    dt = time.time() - t0
    st = _decode_stats(stats.reshape(L * B, stats.shape[2]))
    info = {"iterations": st["iterations"], "inner_iterations": st["inner_total"], "stop": st["stop"],
            "f(x)": st["f"], "gradnorm": st["gradnorm"], **{name: plane.reshape(-1) for name, plane in rows.items()}}
    info = {key: v.reshape(L, B).T.cpu().numpy() for key, v in info.items()}
    info["solve_time"] = dt
    q = q_all.permute(1, 0, 2).cpu().numpy()
    Y = Y_all.reshape(L, B, *Y_shape).permute(1, 0, 2, 3).cpu().numpy() if return_Y else None
    return q, Y, info


def solve_with_riemannian(graph, T_goal, use_jit=True, jit=None):
    """riemannian_solver.py:220-234 on the GPU engine (B = 1).  `jit=` is accepted as an alias of
    `use_jit=` because the reference's README spells it that way (README.md:45)."""
    if isinstance(T_goal, dict):     # several end effectors: {end effector: pose}
        T = np.stack([as_matrix(T_goal[e]) for e in graph.robot.end_effectors])[None]
    else:
        T = as_matrix(T_goal)[None]
    q, Y, info = solve_batch(graph, T)
    q_sol = graph.robot.array_to_q(q[0])
    broken = graph.check_distance_limits(graph.realization(q_sol), tol=1e-6)
    if len(broken) > 0:
        return None, None
    return q_sol, Y[0]
