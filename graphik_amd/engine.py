"""Device-side engine objects: a problem-graph template + batched kernels over HBM buffers.

`Template` plays the role of the closures returned by RiemannianSolver.create_cost_limits /
create_cost (graphik/solvers/riemannian_solver.py:77-176): it fixes the index pairs and which
of omega / psi_L / psi_U apply to each, and exposes batched cost / egrad / ehess / proj and the
trust-region solve on the GPU.  All array arguments are torch tensors on the HIP device
(fp64, contiguous); numpy inputs are copied to the device for convenience.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _ffi


def build_terms(omega, psi_L=None, psi_U=None, use_limits=True):
    """Residual terms in the order the reference's loops visit them.

    Index pairs follow riemannian_solver.py:122-124 (limits) / :79 (no limits): row-major
    nonzeros of the upper triangles; per pair the loops of costs.py:80-207 apply an equality
    term if omega != 0, a lower hinge if psi_L != 0 and an upper hinge if psi_U != 0.
    Returns (term_i, term_j, term_kind, targets_static) where targets_static holds psi_L / psi_U
    for hinge terms and NaN for equality terms (filled per goal from D_goal).
    """
    omega = np.asarray(omega, dtype=float)
    N = omega.shape[0]
    if use_limits:
        psi_L = np.asarray(psi_L, dtype=float)
        psi_U = np.asarray(psi_U, dtype=float)
        diff = psi_L != psi_U
        inds = np.nonzero(np.triu(omega) + np.triu(diff * (psi_L > 0)) + np.triu(diff * (psi_U > 0)))
    else:
        psi_L = np.zeros((N, N))
        psi_U = np.zeros((N, N))
        inds = np.nonzero(np.triu(omega))
    ti, tj, tk, tv = [], [], [], []
    for i, j in zip(*inds):
        if omega[i, j] != 0:
            ti.append(i); tj.append(j); tk.append(_ffi.TERM_EQ); tv.append(np.nan)
        if psi_L[i, j] != 0:
            ti.append(i); tj.append(j); tk.append(_ffi.TERM_LOWER); tv.append(psi_L[i, j])
        if psi_U[i, j] != 0:
            ti.append(i); tj.append(j); tk.append(_ffi.TERM_UPPER); tv.append(psi_U[i, j])
    return (np.array(ti, dtype=np.int32), np.array(tj, dtype=np.int32),
            np.array(tk, dtype=np.int32), np.array(tv, dtype=np.float64))


def _dev(x, device):
    if isinstance(x, torch.Tensor):
        t = x
    else:
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    t = t.to(device=device, dtype=torch.float64)
    return t.contiguous()


def _alloc_stats(B, device):
    """[B] gik_stats records as a [B, sizeof(gik_stats) / 8] fp64 buffer."""
    assert _ffi.STATS_BYTES % 8 == 0
    return torch.zeros(B, _ffi.STATS_BYTES // 8, dtype=torch.float64, device=device)


def _decode_stats(stats):
    """Views of the gik_stats fields (layout taken from _ffi.Stats, i.e. from the header)."""
    ints = stats.view(torch.int32)
    out = {name: stats[:, col] for name, col in _ffi.STATS_F64.items()}      # f, gradnorm, stepsize
    for name in ("iterations", "inner_total", "stop", "n_accept", "inner_executed", "flags"):
        out[name] = ints[:, _ffi.STATS_I32[name]]
    return out


def _result(out, x_shape, extras=()):
    """What Template.ik / anchored_ik return, from the buffers `out` the call wrote: "x" (the point matrices "Y" as
    x_shape = [B, rows, k]), "q", "pos_err", "rot_err", the call's extras (clearance, attempt, keep-alive entries) and
    the decoded stats."""
    res = {"x": out["Y"].reshape(x_shape), "q": out["q"], "pos_err": out["pos_err"], "rot_err": out["rot_err"]}
    res.update(extras)
    res.update(_decode_stats(out["stats"]))
    return res


RETRY_MAX = 63          # attempts share 6 bits of the seed generator's counter (include/graphik_amd.h)
RETRY_MAX_JOINTS = 125


def check_retry_args(retries, pos_tol, rot_tol, q_limits, n, clear_tol=None, retry_spread=0.0, has_center=True):
    """Arguments of a solve with restarts, checked on the host before any device call: retries within
    0 .. 63, positive tolerances, joint limits (q_lo [n], q_hi [n]) finite and ordered.  Returns
    (retries, q_lo, q_hi) with the limits as contiguous float64 arrays; ValueError otherwise.

    The anchored solve adds clear_tol (positive; None: the rule has no clearance part) and retry_spread
    (>= 0 radians; > 0 needs a centre: has_center says whether the call has a q_init)."""
    if int(retries) != retries or not 0 <= int(retries) <= RETRY_MAX:
        raise ValueError(f"retries must be an integer within 0 .. {RETRY_MAX}, got {retries!r}")
    if not (pos_tol > 0 and rot_tol > 0):
        raise ValueError("pos_tol and rot_tol must be positive")
    if clear_tol is not None and not clear_tol > 0:
        raise ValueError("clear_tol must be positive")
    if not retry_spread >= 0:
        raise ValueError(f"retry_spread must be at least 0 (radians), got {retry_spread!r}")
    if retry_spread > 0 and not has_center:
        raise ValueError("retry_spread > 0 needs q_init: local restarts are drawn around the seed, a cold solve has none")
    if n > RETRY_MAX_JOINTS:
        raise ValueError(f"restarts cover robots of at most {RETRY_MAX_JOINTS} joints")
    if q_limits is None:
        raise ValueError("retries > 0 needs q_limits=(q_lo, q_hi): the seeds are drawn inside them")
    lo, hi = (np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in q_limits)
    if lo.shape != (n,) or hi.shape != (n,):
        raise ValueError(f"q_limits must be two arrays of shape [{n}], got {list(lo.shape)} and {list(hi.shape)}")
    if not (np.all(np.isfinite(lo)) and np.all(np.isfinite(hi))):
        raise ValueError("q_limits has non-finite entries: random seeds need finite joint limits")
    if np.any(lo > hi):
        raise ValueError("q_limits: a lower limit exceeds its upper limit")
    return int(retries), lo, hi


RETRY_MAX_CANDIDATES = 16                        # GIK_RETRY_MAX_CANDIDATES (include/graphik_amd.h)
RETRY_CANDIDATE_STEP = 0xD1342543DE82EF95        # candidate c draws under the seed (seed + c * this) mod 2^64


def check_retry_candidates(retry_candidates, retries=None, what="retry_candidates"):
    """retry_candidates of an anchored solve, checked on the host before any device call: an int within 1 .. 16, and
    above 1 only with retries > 0 (retries=None: the stand-alone step, which has no retries).  ValueError otherwise.
    what: the keyword's name in the message (atlas_candidates takes the same range)."""
    if isinstance(retry_candidates, (bool, np.bool_)) or not isinstance(retry_candidates, (int, np.integer)) or \
            not 1 <= int(retry_candidates) <= RETRY_MAX_CANDIDATES:
        raise ValueError(f"{what} must be an integer within 1 .. {RETRY_MAX_CANDIDATES}, got {retry_candidates!r}")
    if retries is not None and int(retry_candidates) > 1 and not retries:
        raise ValueError("retry_candidates > 1 needs retries > 0: the candidates are drawn for the restarts")
    return int(retry_candidates)


ATLAS_MAX_NEIGHBOURS = 64                        # GIK_ATLAS_MAX_NEIGHBOURS (include/graphik_amd.h)


def check_atlas_k(k, count, what="k"):
    """A neighbour count of the atlas entries, checked on the host before any device call: an int within 1 .. 64 and,
    where `count` (the atlas's rows) is given, at most that.  ValueError otherwise."""
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= ATLAS_MAX_NEIGHBOURS:
        raise ValueError(f"{what} must be an integer within 1 .. {ATLAS_MAX_NEIGHBOURS}, got {k!r}")
    if count is not None and int(k) > count:
        raise ValueError(f"{what} = {int(k)} exceeds the atlas's {count} rows")
    return int(k)


def _retry_opts(retries, retry_seed, pos_tol, rot_tol, q_lo, q_hi, mode=None, clear_tol=None, retry_spread=0.0):
    """Checked restart arguments -> the options record of the restart entries: gik_retry_opts (Template.ik), or with
    `mode` (the clearance mode, from check_clearance_mode) and clear_tol gik_anchored_retry_opts (Template.anchored_ik).
    q_lo / q_hi: the limits on the device.  retries == 0 -- attempt 0 alone, the merged clearance of "links+self" --
    draws no seeds: the seed, the limits and the spread stay zero whatever was passed."""
    opts = _ffi.RetryOpts() if mode is None else _ffi.AnchoredRetryOpts(clearance_mode=mode, clear_tol=float(clear_tol))
    opts.retries, opts.pos_tol, opts.rot_tol = int(retries), float(pos_tol), float(rot_tol)
    if retries:
        opts.seed, opts.d_q_lo, opts.d_q_hi = int(retry_seed) & (2 ** 64 - 1), q_lo.data_ptr(), q_hi.data_ptr()
        if mode is not None:
            opts.spread = float(retry_spread)
    return opts


def workspace(nbytes, device):
    """A device buffer of at least nbytes bytes (what a gik_*_ws_bytes query reported) as float64, never empty."""
    return torch.empty(max((nbytes + 7) // 8, 1), dtype=torch.float64, device=device)


def check_clearance_mode(clearance_mode, has_links=True, has_self=True):
    """clearance_mode of an anchored solve -> gik_anchored_retry_opts.clearance_mode (0 nodes, 1 links, 2 links+self),
    checked on the host before any device call: ValueError for another word, for "links" where no links are attached and
    for "links+self" where no self pairs are."""
    if not isinstance(clearance_mode, str) or clearance_mode not in _ffi.CLEARANCE_MODES:
        raise ValueError(f"clearance_mode must be 'nodes', 'links' or 'links+self', got {clearance_mode!r}")
    if clearance_mode != "nodes" and not has_links:
        raise ValueError(f"clearance_mode={clearance_mode!r} needs a link set: this problem was built without links")
    if clearance_mode == "links+self" and not has_self:
        raise ValueError("clearance_mode='links+self' needs self pairs: this problem was built without self_pairs")
    return _ffi.CLEARANCE_MODES[clearance_mode]


def check_atlas_args(atlas, atlas_candidates, retries, retry_candidates, retry_spread, spread_first=False):
    """The atlas keywords of an anchored solve (Template.anchored_ik; AnchoredProblem.solve, whose order is spread_first),
    checked on the host before any device call: atlas_candidates within 1 .. 16, retry_candidates 1, no retry_spread,
    (retries + 1) * atlas_candidates within 1 .. 64 and atlas.count.  Returns atlas_candidates as an int; ValueError otherwise."""
    cand = check_retry_candidates(atlas_candidates, what="atlas_candidates")
    spread = "atlas= with retry_spread > 0 is not supported: the restarts take atlas rows, not draws around q_init"
    if spread_first and retry_spread > 0:
        raise ValueError(spread)
    if check_retry_candidates(retry_candidates) > 1:
        raise ValueError("atlas= with retry_candidates > 1 is not supported: the restarts take atlas rows, not draws")
    if retry_spread > 0:
        raise ValueError(spread)
    if int(retries) == retries and 0 <= int(retries) <= RETRY_MAX:
        check_atlas_k((int(retries) + 1) * cand, atlas.count, "(retries + 1) * atlas_candidates")
    return cand


AnchoredCallPlan = collections.namedtuple("AnchoredCallPlan", "entry ws_query ws_ints args after restart")


def anchored_call_plan(seeded, clearance, clearance_mode, scenes, retries, retry_candidates=1, atlas_candidates=None):
    """The C entry of one Template.anchored_ik call from its checked keywords alone -- no tensor, no library call: seeded (a
    q_init is given), clearance (as passed), clearance_mode (the word), scenes (a set is given), retries, retry_candidates,
    atlas_candidates (None: no atlas).  Returns the entry's name; ws_query, the export that sizes its workspace, and ws_ints,
    that query's integers behind (anch, base, B); args, the names of the entry's arguments between the goal poses and the
    stream ("answer": the five answer pointers; "null": the seeded entry's clearance where `after` measures instead); after,
    the clearance export to launch behind an entry that does not measure the call's clearance itself; restart: a restart
    entry, whose workspace "retry_ws" holds the scratch "ws" too -- with retries > 0, with an atlas, and in "links+self"
    with a clearance and neither restarts nor scenes, which is attempt 0 of gik_anchored_ik_batch_retry alone."""
    def plan(entry, ws_query, ws_ints, middle, after=None):
        restart = ws_query != "gik_anchored_ws_doubles"
        args = ("q_init", "B", "opts", *middle, "ws", "answer", "clearance", "attempt") if restart else middle
        return AnchoredCallPlan("gik_anchored_ik_batch" + entry, ws_query, ws_ints, args, after, restart)
    if atlas_candidates is not None:
        return plan("_atlas", "gik_anchored_ik_batch_atlas_ws_bytes", (atlas_candidates, int(retries)),
                    ("candidates", "atlas_keys", "atlas_q", "atlas_count", "scenes"))
    if retry_candidates > 1:      # (one entry with a nullable scene set)
        return plan("_retry_screened", "gik_anchored_ik_batch_retry_screened_ws_bytes", (retry_candidates,), ("candidates", "scenes"))
    if retries or (clearance_mode == "links+self" and clearance and not scenes):
        return plan("_retry_scenes" if scenes else "_retry", "gik_anchored_retry_ws_bytes", (), ("scenes",) if scenes else ())
    if scenes:      # one call: cold or seeded, the clearance of either mode behind it
        return plan("_scenes", "gik_anchored_ws_doubles", (), ("q_init", "B", "scenes", "ws", "answer", "clearance", "mode"))
    links = "gik_anchored_link_clearance" if clearance and clearance_mode == "links" else None
    if not seeded:
        return plan("", "gik_anchored_ws_doubles", (), ("B", "ws", "answer"), links or ("gik_anchored_clearance" if clearance else None))
    # (the seeded call measures the joint points itself; whole links are measured after it)
    return plan("_seeded", "gik_anchored_ws_doubles", (), ("q_init", "B", "ws", "answer", "null" if links else "clearance"), links)


def pack_scenes(scenes, stride=None):
    """A sequence of [m_s, 4] arrays of (centre x, y, z, radius), numpy or torch -> what gik_scene_set points at, on the
    host: (obs [S, stride, 4] float64 with the radius SQUARED -- one rounded product, the bits of AnchoredProblem's own
    obs[:, 3] ** 2 -- and NaN in the padding rows, which no kernel reads; n_obs [S] int32; stride).  stride defaults to
    the largest count.  ValueError, before any device call: no scene, more than 128 spheres in one, a shape that is not
    [m, 4], a centre that is not finite, a radius that is negative or not finite, a stride below a count or above 128."""
    rows = []
    for s, sc in enumerate(scenes):
        a = sc.detach().cpu().numpy() if isinstance(sc, torch.Tensor) else np.asarray(sc)
        a = np.asarray(a, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError(f"scene {s}: expected an array of shape [m, 4] (centre x, y, z, radius), got {list(a.shape)}")
        if a.shape[0] > _ffi.SCENE_MAX_SPHERES:
            raise ValueError(f"scene {s}: {a.shape[0]} spheres, at most {_ffi.SCENE_MAX_SPHERES} per scene")
        if not np.all(np.isfinite(a[:, :3])):
            raise ValueError(f"scene {s}: a centre is not finite")
        if not np.all(np.isfinite(a[:, 3]) & (a[:, 3] >= 0)):
            raise ValueError(f"scene {s}: a radius is negative or not finite")
        rows.append(a)
    if not rows:
        raise ValueError("a scene set needs at least one scene (an empty scene is an array of shape [0, 4])")
    n_obs = np.array([len(a) for a in rows], dtype=np.int32)
    if stride is None:
        stride = int(n_obs.max())
    if int(stride) != stride or not int(n_obs.max()) <= stride <= _ffi.SCENE_MAX_SPHERES:
        raise ValueError(f"stride must be an integer within {int(n_obs.max())} (the largest scene) .. {_ffi.SCENE_MAX_SPHERES}, got {stride!r}")
    obs = np.full((len(rows), int(stride), 4), np.nan)
    for s, a in enumerate(rows):
        obs[s, :len(a), :3] = a[:, :3]
        obs[s, :len(a), 3] = a[:, 3] ** 2
    return obs, n_obs, int(stride)


class SceneSet:
    """Per-goal obstacle scenes of the anchored solve (gik_scene_set), uploaded once: `scenes` is a sequence of [m_s, 4]
    arrays of (centre, radius).  Holds the device tensors obs [S, stride, 4] (squared radii) and n_obs [S] int32, and on
    the host scenes (the arrays as given, float64), obs_host, counts, stride, n_scene.  An argument of
    Template.solve / anchored_ik and of AnchoredProblem.solve / solve_trajectory, together with scene_id."""

    def __init__(self, scenes, device, stride=None):
        scenes = list(scenes)
        self.obs_host, self.counts, self.stride = pack_scenes(scenes, stride)
        self.n_scene = len(self.counts)
        self.scenes = [np.asarray(sc.detach().cpu().numpy() if isinstance(sc, torch.Tensor) else sc, dtype=np.float64).reshape(-1, 4)
                       for sc in scenes]
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device(f"cuda:{torch.cuda.current_device()}")
        self.obs = torch.from_numpy(self.obs_host).to(self.device)
        self.n_obs = torch.from_numpy(self.counts).to(self.device)

    def ids(self, scene_id, shape, checked=False):
        """scene_id -> a contiguous int32 device tensor of `shape` ([B], or [B, L]), or None where there is one scene and
        no ids (every goal uses scene 0).  ValueError for a missing id array with several scenes, a wrong shape, an id
        that is not an integer or lies outside [0, n_scene); a device tensor is checked with one reduction.
        checked: scene_id is what an earlier ids() returned, or a row of it -- nothing is looked at again."""
        if checked:
            return scene_id
        if scene_id is None:
            if self.n_scene != 1:
                raise ValueError(f"scene_id is required with {self.n_scene} scenes: [B] ints, the scene of each goal")
            return None
        if isinstance(scene_id, torch.Tensor) and scene_id.device.type != "cpu":
            t = scene_id
            if t.dtype not in (torch.int32, torch.int64):
                raise ValueError("scene_id must hold integers")
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f"scene_id must have shape {list(shape)}, got {list(t.shape)}")
            if t.numel() and bool(((t < 0) | (t >= self.n_scene)).any()):
                raise ValueError(f"scene_id has entries outside [0, {self.n_scene})")
            return t.to(device=self.device, dtype=torch.int32).contiguous()
        a = np.asarray(scene_id.numpy() if isinstance(scene_id, torch.Tensor) else scene_id)
        if a.dtype.kind not in "iu":
            if a.dtype.kind != "f" or not np.all(a == np.floor(a)):
                raise ValueError("scene_id must hold integers")
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"scene_id must have shape {list(shape)}, got {list(a.shape)}")
        if a.size and (a.min() < 0 or a.max() >= self.n_scene):
            raise ValueError(f"scene_id has entries outside [0, {self.n_scene})")
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)

    def desc(self, ids):
        """The gik_scene_set of one call: ids [B] int32 on the device (from ids()), or None."""
        return _ffi.SceneSet(n_scene=self.n_scene, stride=self.stride, d_obs=self.obs.data_ptr() if self.stride else None,
                             d_n_obs=self.n_obs.data_ptr(), d_scene_id=None if ids is None else ids.data_ptr())


class Template:
    """Goal-independent part of an IK problem family, resident on one GPU."""

    def __init__(self, N, k, term_i, term_j, term_kind, targets_static=None, device=None,
                 params=None, anchored=None):
        """anchored: None, or the fixed-anchor data of gik_anchored_desc as a dict (anchor_pos
        [A,3], n_goal_anchor, term_target [T], pin_node / pin_anchor / pin_kind / pin_target,
        obs [n_obs,4] (x, y, z, r^2), obs_node_mask [N], full_N, free_full_index,
        anchor_full_index, axis_length) -- see include/graphik_amd.h."""
        self.lib = _ffi.lib()
        if not torch.cuda.is_available():
            raise _ffi.GikError("no HIP device visible: graphik_amd needs an AMD GPU (gfx950)")
        self.device = torch.device(device if device is not None else
                                   f"cuda:{torch.cuda.current_device()}")
        self.N, self.k = int(N), int(k)
        self.term_i = np.ascontiguousarray(term_i, dtype=np.int32)
        self.term_j = np.ascontiguousarray(term_j, dtype=np.int32)
        self.term_kind = np.ascontiguousarray(term_kind, dtype=np.int32)
        self.T = len(self.term_i)
        self.targets_static = None if targets_static is None else \
            np.ascontiguousarray(targets_static, dtype=np.float64)
        d = _ffi.TemplateDesc()
        params = dict(params or {})
        self.solver = params.pop("solver", "TrustRegions")
        self.claim_order = params.pop("claim_order", "auto")      # "off": set_claim_key keeps index order
        if self.claim_order not in ("auto", "on", "off"):
            raise ValueError("params[\"claim_order\"] must be one of 'auto', 'on', 'off'")
        if self.solver == "ConjugateGradient":      # riemannian_solver.py:51-59
            self.lib.gik_default_cg_params(C.byref(d))
        elif self.solver == "TrustRegions":
            self.lib.gik_default_params(C.byref(d))
        else:
            raise ValueError("params[\"solver\"] must be one of 'ConjugateGradient', 'TrustRegions'")
        d.N, d.k, d.n_terms = self.N, self.k, self.T
        d.term_i = self.term_i.ctypes.data_as(C.POINTER(C.c_int32))
        d.term_j = self.term_j.ctypes.data_as(C.POINTER(C.c_int32))
        d.term_kind = self.term_kind.ctypes.data_as(C.POINTER(C.c_int32))
        alias = {"minstepsize": "cg_minstepsize", "orth_value": "cg_orth_value", "beta_type": "cg_beta_type"}
        for key, val in params.items():
            key = alias.get(key, key)
            if not hasattr(d, key):
                raise KeyError(f"unknown solver parameter {key!r}")
            if key == "clique_closed_form" and isinstance(val, str):
                val = {"auto": _ffi.CLIQUE_AUTO, "off": _ffi.CLIQUE_OFF, "dense": _ffi.CLIQUE_DENSE}[val]
            if key == "hessian_form" and isinstance(val, str):
                val = {"column": _ffi.HESS_COLUMN, "per_edge": _ffi.HESS_PER_EDGE, "auto": _ffi.HESS_AUTO}[val]
            setattr(d, key, int(val) if key in ("maxiter", "cg_beta_type", "clique_closed_form", "hessian_form") else val)
        self.params = {f: getattr(d, f) for f in ("mingradnorm", "maxiter", "maxinner", "mininner",
                                                   "theta", "kappa", "rho_prime",
                                                   "rho_regularization", "planar_proj_exact",
                                                   "force_block_path", "waves_per_cu",
                                                   "slice_outer_its", "debug_flags", "cg_minstepsize",
                                                   "cg_orth_value", "cg_beta_type", "clique_closed_form", "hessian_form")}
        self.params["solver"] = self.solver
        h = C.c_void_p()
        self.anchored = anchored is not None
        if anchored is None:
            self._call("gik_template_create", C.byref(d), C.byref(h))
        else:
            ad, keep = _ffi.AnchoredDesc(), {}

            def arr(name, dt):
                keep[name] = np.ascontiguousarray(anchored[name], dtype=dt)
                return keep[name].ctypes.data_as(C.POINTER(C.c_double if dt == np.float64 else C.c_int32))

            ad.anchor_pos = arr("anchor_pos", np.float64)
            ad.n_anchor = len(keep["anchor_pos"])
            ad.n_goal_anchor = int(anchored["n_goal_anchor"])
            ad.term_target = arr("term_target", np.float64)
            assert len(keep["term_target"]) == self.T
            ad.pin_node, ad.pin_anchor = arr("pin_node", np.int32), arr("pin_anchor", np.int32)
            ad.pin_kind, ad.pin_target = arr("pin_kind", np.int32), arr("pin_target", np.float64)
            ad.n_pin = len(keep["pin_node"])
            ad.obs = arr("obs", np.float64)
            ad.n_obs = len(keep["obs"])
            ad.obs_node_mask = arr("obs_node_mask", np.int32)
            ad.full_N = int(anchored["full_N"])
            ad.free_full_index = arr("free_full_index", np.int32)
            ad.anchor_full_index = arr("anchor_full_index", np.int32)
            ad.axis_length = float(anchored["axis_length"])
            self.n_goal_anchor, self.full_N = ad.n_goal_anchor, ad.full_N
            self._call("gik_template_create_anchored", C.byref(d), C.byref(ad), C.byref(h))
        self._h = h
        self.n_link = None      # (attach_links)
        self.link_hinges = False
        self.n_self = None      # (attach_self_pairs)
        self.self_hinges = False
        self.n_half = 0         # (attach_halfspaces)
        self._read_info()
        deg = np.bincount(np.concatenate([self.term_i, self.term_j]), minlength=self.N).max()
        # compiled slot count of the wavefront variant the library chose (or the raw degree: workgroup / node-per-lane paths)
        self.maxdeg = int(self.info["max_terms_per_node"]) if not self.info["is_block"] else int(deg)

    def _read_info(self):
        """What the library decided for this handle (gik_template_get_info); read again after attach_pipeline,
        which decides the prepare kernel."""
        info = _ffi.TemplateInfo()
        self._call("gik_template_get_info", self._h, C.byref(info))
        self.info = {f: getattr(info, f) for f, _ in _ffi.TemplateInfo._fields_ if f != "reserved"}

    @classmethod
    def from_matrices(cls, omega, psi_L=None, psi_U=None, k=3, use_limits=True, **kw):
        ti, tj, tk, tv = build_terms(omega, psi_L, psi_U, use_limits)
        return cls(np.asarray(omega).shape[0], k, ti, tj, tk, tv, **kw)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self.lib.gik_template_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def set_claim_key(self, terms, weights):
        """The template's claim key (gik_template_set_claim_key): solves hand their problems out in ascending order of
        sum_i weights[i] * targets[:, terms[i]].  No terms, or params["claim_order"] = "off": index order."""
        terms = np.ascontiguousarray(terms, dtype=np.int32).reshape(-1)
        w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
        if len(terms) != len(w):
            raise ValueError("one weight per term")
        n = 0 if self.claim_order == "off" else len(terms)
        self._call("gik_template_set_claim_key", self._h, n, terms.ctypes.data_as(C.POINTER(C.c_int32)),
                   w.ctypes.data_as(C.POINTER(C.c_double)))
        self._read_info()

    def claim_order_of(self, keys):
        """keys [B] float32 (device tensor or array) -> the indices in ascending key order as the solve would use them
        (gik_claim_order_sort): stable, NaN last."""
        k = torch.as_tensor(keys, dtype=torch.float32).to(self.device).contiguous()
        order = torch.full((k.numel(),), -1, dtype=torch.int32, device=self.device)
        self._call("gik_claim_order_sort", k.data_ptr(), k.numel(), order.data_ptr(), self._stream())
        return order

    def claim_keys(self, targets):
        """targets [B,T] -> the claim keys [B] float32 of this template (gik_claim_order_keys)."""
        t = _dev(targets, self.device)
        keys = torch.empty(t.shape[0], dtype=torch.float32, device=self.device)
        self._call("gik_claim_order_keys", self._h, t.data_ptr(), t.shape[0], keys.data_ptr(), self._stream())
        return keys

    # -- helpers ------------------------------------------------------------------------------
    def targets_from_D(self, D_goal):
        """[B,N,N] (or [N,N]) squared-distance matrices -> [B,T] per-term targets."""
        D = np.asarray(D_goal, dtype=np.float64)
        if D.ndim == 2:
            D = D[None]
        tg = D[:, self.term_i, self.term_j].copy()
        if self.targets_static is not None:
            hinge = self.term_kind != _ffi.TERM_EQ
            tg[:, hinge] = self.targets_static[hinge]
        return tg

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, name, *args):
        """Every call of an export that returns a status code: `name` is looked up in the library and called with `args`
        while this template's device is the current one; a status other than 0 raises GikError with gik_last_error().
        (The size queries -- gik_*_ws_bytes, gik_anchored_ws_doubles -- return sizes and launch nothing: they are called
        directly.)"""
        with torch.cuda.device(self.device):
            _ffi.check(getattr(self.lib, name)(*args))

    def _vec(self, Y):
        Y = _dev(Y, self.device)
        if Y.dim() == 2:
            Y = Y[None]
        B = Y.shape[0]
        return Y.reshape(B, self.N * self.k).contiguous(), B

    def _tg(self, targets, B):
        t = _dev(targets, self.device)
        if t.dim() == 1:
            t = t[None]
        if t.shape[0] == 1 and B > 1:
            t = t.expand(B, -1).contiguous()
        width = self.T if not self.anchored else 3 * self.n_goal_anchor   # anchored: goal anchors
        assert t.shape == (B, width), (t.shape, (B, width))
        return t

    # -- costgrd twins ------------------------------------------------------------------------
    def cost(self, Y, targets):
        Y, B = self._vec(Y)
        t = self._tg(targets, B)
        out = torch.empty(B, dtype=torch.float64, device=self.device)
        self._call("gik_cost", self._h, Y.data_ptr(), t.data_ptr(), B, out.data_ptr(), self._stream())
        return out

    def grad(self, Y, targets):
        Y, B = self._vec(Y)
        t = self._tg(targets, B)
        out = torch.empty_like(Y)
        self._call("gik_grad", self._h, Y.data_ptr(), t.data_ptr(), B, out.data_ptr(), self._stream())
        return out.reshape(B, self.N, self.k)

    def cost_and_grad(self, Y, targets):
        """lcost_and_grad / jcost_and_grad (costs.py:126-169, 61-77): (f [B], G [B,N,k]) in one pass."""
        Y, B = self._vec(Y)
        t = self._tg(targets, B)
        f = torch.empty(B, dtype=torch.float64, device=Y.device)
        out = torch.empty_like(Y)
        self._call("gik_cost_and_grad", self._h, Y.data_ptr(), t.data_ptr(), B, f.data_ptr(), out.data_ptr(), self._stream())
        return f, out.reshape(B, self.N, self.k)

    def hess(self, Y, W, targets):
        Y, B = self._vec(Y)
        W, _ = self._vec(W)
        t = self._tg(targets, B)
        out = torch.empty_like(Y)
        self._call("gik_hess", self._h, Y.data_ptr(), W.data_ptr(), t.data_ptr(), B, out.data_ptr(), self._stream())
        return out.reshape(B, self.N, self.k)

    def proj(self, Y, Z):
        Y, B = self._vec(Y)
        Z, _ = self._vec(Z)
        out = torch.empty_like(Y)
        self._call("gik_proj", self._h, Y.data_ptr(), Z.data_ptr(), B, out.data_ptr(), self._stream())
        return out.reshape(B, self.N, self.k)

    # -- device pre/post-processing ----------------------------------------------------------
    def attach_pipeline(self, *, T0, p_index, q_index, x_index, y_index, axis_length, goal_nodes,
                        goal_len, base_lower, base_upper, anchor_index, anchor_pos, pair_i, pair_j,
                        term_src, term_static, last_link_along_z, jacobi_sweeps=0,
                        force_block_prepare=False, ee_goal_nodes=None, ee_path=None,
                        goal_pair_a=(), goal_pair_b=(), ee_goal_len=None, position_goal_mask=0, point_axis=None):
        """Give the handle what it needs to run from_pose + bound_smoothing +
        generate_initialization and joint_variables on the device (gik_pipeline_attach).
        position_goal_mask: bit e -- end effector e has a position goal (gik_pipeline_desc::position_goal_mask): its odd
        goal slot (goal_nodes[1], ee_goal_nodes[2 e + 1]) is -1 and its bit of last_link_along_z clear.
        point_axis: {e: (x, y)} for gik_pipeline_set_point_axis (position goals behind a last link along z)."""
        keep = {}

        def arr(name, a, dt):
            keep[name] = np.ascontiguousarray(a, dtype=dt)
            ct = C.c_double if dt == np.float64 else C.c_int32
            return keep[name].ctypes.data_as(C.POINTER(ct))

        d = _ffi.PipelineDesc()
        T0 = np.asarray(T0, dtype=np.float64)
        d.n_joints = T0.shape[0] - 1
        d.T0 = arr("T0", T0, np.float64)
        d.p_index = arr("p", p_index, np.int32)
        d.q_index = arr("q", q_index if q_index is not None else p_index, np.int32)
        d.x_index, d.y_index = int(x_index), int(y_index)
        d.axis_length = float(axis_length)
        d.goal_node0, d.goal_node1 = int(goal_nodes[0]), int(goal_nodes[1])
        d.goal_len = float(goal_len)
        d.base_lower = arr("lo", base_lower, np.float64)
        d.base_upper = arr("up", base_upper, np.float64)
        d.n_anchor = len(anchor_index)
        d.anchor_index = arr("ai", anchor_index, np.int32)
        d.anchor_pos = arr("ap", anchor_pos, np.float64)
        d.n_pairs = len(pair_i)
        d.pair_i = arr("pi", pair_i, np.int32)
        d.pair_j = arr("pj", pair_j, np.int32)
        d.term_src = arr("ts", term_src, np.int32)
        d.term_static = arr("tv", term_static, np.float64)
        d.last_link_along_z = int(last_link_along_z)       # one bit per end effector
        d.position_goal_mask = int(position_goal_mask)     # likewise
        d.jacobi_sweeps = int(jacobi_sweeps)
        d.force_block_prepare = int(bool(force_block_prepare))
        self.n_ee = 1
        if ee_goal_nodes is not None and len(ee_goal_nodes) > 2:     # several end effectors
            self.n_ee = len(ee_goal_nodes) // 2
            d.n_ee = self.n_ee
            d.ee_goal_nodes = arr("eg", ee_goal_nodes, np.int32)
            d.ee_path = arr("ep", ee_path, np.int32)
            d.n_goal_pairs = len(goal_pair_a)
            d.goal_pair_a = arr("ga", goal_pair_a, np.int32)
            d.goal_pair_b = arr("gb", goal_pair_b, np.int32)
            if ee_goal_len is not None:                  # planar trees: the link parent(e) -> e per end effector
                d.ee_goal_len = arr("el", ee_goal_len, np.float64)
        self._call("gik_pipeline_attach", self._h, C.byref(d))
        for e, (x, y) in (point_axis or {}).items():
            self._call("gik_pipeline_set_point_axis", self._h, int(e), float(x), float(y))
        self.n_joints = int(d.n_joints)
        self.goal_slots = (int(d.goal_node0), int(d.goal_node1))      # (-1: the inert odd slot of a position goal)
        self.has_pipeline = True
        self._read_info()

    def _poses(self, T_goal):
        T = _dev(T_goal, self.device)
        B = T.shape[0]
        width = getattr(self, "n_ee", 1) * (self.k + 1) ** 2
        assert T.numel() == B * width, (tuple(T.shape), width)
        T = T.reshape(B, width).contiguous()      # [B][n_ee][(k+1)^2]
        return T, B

    def prepare(self, T_goal, return_K=False):
        """goal poses [B,k+1,k+1] -> (targets [B,T], Y_init [B,N,k]) on the device."""
        T, B = self._poses(T_goal)
        targets = torch.empty(B, self.T, dtype=torch.float64, device=self.device)
        Y0 = torch.empty(B, self.N * self.k, dtype=torch.float64, device=self.device)
        Kc = torch.zeros(B, dtype=torch.int32, device=self.device) if return_K else None
        self._call("gik_prepare_batch", self._h, T.data_ptr(), B, targets.data_ptr(), Y0.data_ptr(),
                   Kc.data_ptr() if return_K else None, self._stream())
        Y0 = Y0.reshape(B, self.N, self.k)
        return (targets, Y0, Kc) if return_K else (targets, Y0)

    def prepare_debug(self, T_goal):
        """prepare() plus the intermediate results the reference computes on the way: dict with
        targets, Y_init, K (MDS column count), lb, ub [B,N,N] (bound_smoothing) and eig [B,3,N]
        (spectra of the Gram matrix, of MDS's rank matrix and of the scatter matrix)."""
        T, B = self._poses(T_goal)
        f64 = dict(dtype=torch.float64, device=self.device)
        out = {"targets": torch.empty(B, self.T, **f64), "Y_init": torch.empty(B, self.N * self.k, **f64),
               "K": torch.zeros(B, dtype=torch.int32, device=self.device),
               "lb": torch.empty(B, self.N, self.N, **f64), "ub": torch.empty(B, self.N, self.N, **f64),
               "eig": torch.empty(B, 3, self.N, **f64)}
        dg = _ffi.PrepareDiag(out["lb"].data_ptr(), out["ub"].data_ptr(), out["eig"].data_ptr())
        self._call("gik_prepare_batch_debug", self._h, T.data_ptr(), B, out["targets"].data_ptr(), out["Y_init"].data_ptr(),
                   out["K"].data_ptr(), C.byref(dg), self._stream())
        out["Y_init"] = out["Y_init"].reshape(B, self.N, self.k)
        return out

    def recover(self, Y, T_goal):
        """points + goal poses -> (q [B,n], pos_err [B], rot_err [B]) on the device."""
        Y, B = self._vec(Y)
        T, _ = self._poses(T_goal)
        q = torch.empty(B, self.n_joints, dtype=torch.float64, device=self.device)
        pe = torch.empty(B, dtype=torch.float64, device=self.device)
        re = torch.empty(B, dtype=torch.float64, device=self.device)
        self._call("gik_recover_batch", self._h, Y.data_ptr(), T.data_ptr(), B, q.data_ptr(), pe.data_ptr(), re.data_ptr(),
                   self._stream())
        return q, pe, re

    def _seed_angles(self, q_init, B):
        q = _dev(q_init, self.device)
        if q.dim() == 1:
            q = q[None].expand(B, -1)
        assert q.shape == (B, self.n_joints), (tuple(q.shape), (B, self.n_joints))
        return q.contiguous()

    def seed(self, T_goal, q_init):
        """goal poses + seed joint angles [B,n] (or [n]) -> (targets [B,T], Y_init [B,N,k]) on the
        device (gik_seed_batch): the prepare kernels' targets and graph.realization(q_init)."""
        T, B = self._poses(T_goal)
        q = self._seed_angles(q_init, B)
        targets = torch.empty(B, self.T, dtype=torch.float64, device=self.device)
        Y0 = torch.empty(B, self.N * self.k, dtype=torch.float64, device=self.device)
        self._call("gik_seed_batch", self._h, T.data_ptr(), q.data_ptr(), B, targets.data_ptr(), Y0.data_ptr(),
                   self._stream())
        return targets, Y0.reshape(B, self.N, self.k)

    def ik(self, T_goal, out=None, q_init=None, retries=0, retry_seed=0, pos_tol=0.01, rot_tol=0.01, q_limits=None):
        """Whole solve_with_riemannian pipeline for a batch of goal poses, one stream, no host
        round trip: prepare -> solve -> recover.  With q_init (seed joint angles [B,n] or [n], a
        device tensor may be out["q"] itself) the initial point is the realization of q_init instead
        of the bound-smoothing + MDS one: seed -> solve -> recover (gik_ik_batch_seeded).  Returns a
        dict of device tensors.

        retries > 0 (gik_ik_batch_retry): goals that fail -- stop != 0, pos_err > pos_tol or rot_err >
        rot_tol -- are solved again, up to `retries` times, from joint angles drawn uniformly inside
        q_limits = (q_lo [n], q_hi [n]) by a generator keyed on (retry_seed, goal, attempt), and the
        better answer is kept; "attempt" [B] int32 says which one each goal holds.  That call
        synchronises the stream once per attempt.  `out` may carry "attempt" [B] int32, "retry_ws" (a
        buffer of gik_retry_ws_bytes) and "q_lo" / "q_hi" device tensors to reuse between calls."""
        if retries:
            if not getattr(self, "has_pipeline", False):
                raise _ffi.GikError("no pipeline attached (attach_pipeline): restarts need the device pipeline")
            retries, lo, hi = check_retry_args(retries, pos_tol, rot_tol, q_limits, self.n_joints)
        T, B = self._poses(T_goal)
        if out is None:
            out = self.alloc_ik_buffers(B)
        q0 = None if q_init is None else self._seed_angles(q_init, B)
        answer = [out[key].data_ptr() for key in ("targets", "Y", "stats", "q", "pos_err", "rot_err")]
        extras = {}
        if retries:
            attempt, ws, q_lo, q_hi = self._retry_buffers(out, B, self.retry_ws_bytes(B), lo, hi)
            opts = _retry_opts(retries, retry_seed, pos_tol, rot_tol, q_lo, q_hi)
            self._call("gik_ik_batch_retry", self._h, T.data_ptr(), None if q0 is None else q0.data_ptr(), B, C.byref(opts),
                       ws.data_ptr(), *answer, attempt.data_ptr(), self._stream())
            extras = {"attempt": attempt, "_retry_ws": ws}      # (the workspace lives as long as the result)
        elif q0 is None:
            self._call("gik_ik_batch", self._h, T.data_ptr(), B, *answer, self._stream())
        else:
            self._call("gik_ik_batch_seeded", self._h, T.data_ptr(), q0.data_ptr(), B, *answer, self._stream())
        return _result(out, (B, self.N, self.k), extras)

    def _retry_buffers(self, out, B, nbytes, lo, hi, limits=True):
        """The restart buffers of one call with retries > 0, taken from `out` where it carries them: ("attempt" [B] int32,
        "retry_ws" of at least nbytes -- what the call's gik_*retry_ws_bytes reported --, "q_lo", "q_hi" on the device);
        a missing one is allocated, or uploaded from the checked limits lo / hi."""
        attempt = out.get("attempt")
        if attempt is None:
            attempt = torch.empty(B, dtype=torch.int32, device=self.device)
        ws = out.get("retry_ws")
        if ws is None or ws.numel() * ws.element_size() < nbytes:
            ws = workspace(nbytes, self.device)
        if not limits:      # (a call with retries = 0 draws no seeds)
            return attempt, ws, None, None
        q_lo = out["q_lo"] if "q_lo" in out else _dev(lo, self.device)
        q_hi = out["q_hi"] if "q_hi" in out else _dev(hi, self.device)
        return attempt, ws, q_lo, q_hi

    def retry_ws_bytes(self, B):
        """Bytes of the restart workspace ("retry_ws") of one ik call of B goals with retries > 0 (gik_retry_ws_bytes)."""
        return int(self.lib.gik_retry_ws_bytes(self._h, B))

    def anchored_sweep_ws_bytes(self, base, B, samples):
        """Bytes of the workspace ("ws") of one anchored_sweep_clearance[s] call of B rows and `samples` samples
        (gik_anchored_sweep_ws_bytes)."""
        return int(self.lib.gik_anchored_sweep_ws_bytes(self._h, base._h, B, samples))

    def anchored_retry_ws_bytes(self, base, B, scenes=False):
        """Bytes of the restart workspace ("retry_ws") of one anchored_ik call of B goals with retries > 0:
        gik_anchored_retry_ws_bytes, a multiple of 8, and with a scene set behind it the compact batch's scene ids,
        [B] int32 (gik_anchored_ik_batch_retry_scenes)."""
        nbytes = int(self.lib.gik_anchored_retry_ws_bytes(self._h, base._h, B))
        return (nbytes + 7) // 8 * 8 + 4 * B if scenes else nbytes

    def anchored_plan_ws_bytes(self, base, B, plan):
        """Bytes of the workspace of one anchored_ik call of B goals on `plan`: "retry_ws" if plan.restart, else "ws"."""
        if plan.ws_query == "gik_anchored_retry_ws_bytes":
            return self.anchored_retry_ws_bytes(base, B, scenes="scenes" in plan.args)
        size = int(getattr(self.lib, plan.ws_query)(self._h, base._h, B, *plan.ws_ints))
        return 8 * size if plan.ws_query == "gik_anchored_ws_doubles" else size

    def anchored_retry_seeds_screened(self, base, T_goal, idx, retry_seed, attempt, candidates, q_limits, center=None, spread=0.0,
                                      clearance_mode="nodes", clear_tol=1e-4, scenes=None, scene_id=None):
        """The screened seed step of the anchored restarts alone (gik_anchored_retry_seeds_screened): for compact slot r,
        goal g = idx[r] of the goal poses T_goal [B, 4, 4], `candidates` seeds of (retry_seed, g, attempt) are drawn
        inside q_limits = (q_lo [n], q_hi [n]) -- around center [B, n] (by goal) with spread > 0 --, realized and measured
        in clearance_mode, against scene scene_id[g] ([B], by goal) where scenes is given, and the first clear one is
        picked (AnchoredProblem.screened_seeds_host is the numpy mirror).  Returns device tensors: "q" [count, n] the
        picked angles, "T" [count, 4, 4] the pose rows, "pick" [count] int32 and "clearance" [count]."""
        def source(T, B, idx):      # the draws' arguments around (T_goal, idx, count)
            n = base.n_joints
            lo, hi = (_dev(np.ascontiguousarray(a, dtype=np.float64), self.device) for a in q_limits)
            assert idx is not None and lo.numel() == n and hi.numel() == n
            ctr = None
            if center is not None:      # (a NaN centre row is allowed: it gives a NaN seed, as the device entry says)
                ctr = center if isinstance(center, torch.Tensor) else np.ascontiguousarray(center, dtype=np.float64)
                ctr = _dev(ctr, self.device).contiguous()
                assert tuple(ctr.shape) == (B, n), (tuple(ctr.shape), (B, n))
            return (), (int(retry_seed) & (2 ** 64 - 1), int(attempt), lo.data_ptr(), hi.data_ptr(),
                        None if ctr is None else ctr.data_ptr(), float(spread)), (lo, hi, ctr)
        return self._screened_step("gik_anchored_retry_seeds_screened", base, T_goal, idx, candidates, clearance_mode, clear_tol, scenes,
                                   scene_id, source, spread, center is not None)

    def _idx(self, idx):
        """Goal indices of compact slots (a sequence, an array or a tensor) -> a contiguous [count] int32 device tensor."""
        if not isinstance(idx, torch.Tensor):
            idx = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int32))
        idx = idx.to(device=self.device, dtype=torch.int32).contiguous()
        assert idx.dim() == 1
        return idx

    def _screened_step(self, name, base, T_goal, idx, candidates, clearance_mode, clear_tol, scenes, scene_id, source, spread=0.0,
                       has_center=True):
        """The body of anchored_retry_seeds_screened and anchored_atlas_seeds: the checks they share, the outputs, the
        workspace (name + "_ws_bytes") and the call of the export `name`.  source(T, B, idx) returns the entry's arguments
        in front of and behind (T_goal, idx, count), and the tensors those point into; spread: that of the draws."""
        assert self.anchored and base.has_pipeline
        mode = check_clearance_mode(clearance_mode, getattr(self, "n_link", None) is not None,
                                    getattr(self, "n_self", None) is not None)
        candidates = check_retry_candidates(candidates)
        if not clear_tol > 0:
            raise ValueError("clear_tol must be positive")
        if not spread >= 0:
            raise ValueError(f"spread must be at least 0 (radians), got {spread!r}")
        if spread > 0 and not has_center:
            raise ValueError("spread > 0 needs the centre rows")
        T, B = base._poses(T_goal)
        idx = None if idx is None else self._idx(idx)
        front, behind, keep = source(T, B, idx)      # (keep: the source's device tensors, alive until the call is queued)
        count = B if idx is None else idx.numel()
        sc, ids = self._scene_desc(scenes, scene_id, B)
        f64 = dict(dtype=torch.float64, device=self.device)
        q = torch.empty(count, base.n_joints, **f64)
        T_out = torch.empty(count, T.numel() // max(B, 1), **f64)
        pick = torch.empty(count, dtype=torch.int32, device=self.device)
        cl = torch.empty(count, **f64)
        ws = workspace(int(getattr(self.lib, name + "_ws_bytes")(self._h, base._h, count, candidates)), self.device)
        self._call(name, self._h, base._h, *front, T.data_ptr(), None if idx is None else idx.data_ptr(), count, *behind, candidates,
                   mode, float(clear_tol), None if sc is None else C.byref(sc), ws.data_ptr(), T_out.data_ptr(), q.data_ptr(),
                   pick.data_ptr(), cl.data_ptr(), self._stream())
        return {"q": q, "T": T_out.reshape(count, 4, 4), "pick": pick, "clearance": cl, "_ws": ws, "_scene_id": ids}

    def atlas_key_width(self):
        """Doubles per atlas key on this robot-graph template (gik_atlas_nearest): 6 -- p_e and q_e of a pose goal --, or 3,
        the p_e of a position goal."""
        return 3 * sum(1 for g in self.goal_slots if g >= 0)

    def atlas_nearest(self, atlas, T_goal, k, idx=None, dist=True):
        """The k (1 .. 64) atlas rows nearest to each goal, on this robot-graph template (gik_atlas_nearest): `atlas` holds
        the device tensors keys [W, M] (component-major) and count = M; T_goal [B, 4, 4]; idx (optional, [count] int32):
        slot r is goal idx[r].  Returns device tensors (nbr [count, k] int32, dist [count, k] or None): ascending in
        (distance, row), -1 / +inf where fewer than k rows have a finite distance.
        riemannian_solver.atlas_nearest_host is the numpy mirror."""
        check_atlas_k(k, None)
        if atlas.width != self.atlas_key_width():
            raise ValueError(f"the atlas has keys of width {atlas.width}, this template's goals have {self.atlas_key_width()}")
        T, B = self._poses(T_goal)
        idx = None if idx is None else self._idx(idx)
        count = B if idx is None else idx.numel()
        nbr = torch.empty(count, int(k), dtype=torch.int32, device=self.device)
        d = torch.empty(count, int(k), dtype=torch.float64, device=self.device) if dist else None
        self._call("gik_atlas_nearest", self._h, atlas.d_keys.data_ptr(), atlas.count, T.data_ptr(),
                   None if idx is None else idx.data_ptr(), count, int(k), nbr.data_ptr(), None if d is None else d.data_ptr(),
                   self._stream())
        return nbr, d

    def anchored_atlas_seeds(self, base, atlas, T_goal, nbr, candidates, first=0, idx=None, clearance_mode="nodes", clear_tol=1e-4,
                             scenes=None, scene_id=None):
        """The screened seed step with the atlas as its candidate source (gik_anchored_atlas_seeds): candidate c of slot r
        (goal g = idx[r], or r) is atlas row nbr[g, first + c]; nbr [B, K] int32 on the device, indexed by goal (what
        base.atlas_nearest returns without idx).  Returns what anchored_retry_seeds_screened returns
        (AnchoredProblem.atlas_seeds_host is the numpy mirror)."""
        def source(T, B, idx):      # the table in front of (T_goal, idx, count), the ranks behind
            assert nbr.dtype == torch.int32 and nbr.dim() == 2 and nbr.shape[0] == B and nbr.is_contiguous()
            return (atlas.d_q.data_ptr(), atlas.count), (nbr.data_ptr(), int(nbr.shape[1]), int(first)), None
        return self._screened_step("gik_anchored_atlas_seeds", base, T_goal, idx, candidates, clearance_mode, clear_tol, scenes, scene_id,
                                   source)

    def alloc_anchored_buffers(self, base, B, clearance=False, ws=True):
        """The buffers of one anchored_ik call of B goals (its `out`): the scratch "ws" (ws=False leaves it out: a call
        with retries > 0 keeps that scratch in its restart workspace), the full point matrix "Y" [B, full_N*3], "stats",
        "q", "pos_err", "rot_err" and, if asked for, "clearance"."""
        f64 = dict(dtype=torch.float64, device=self.device)
        out = {"Y": torch.empty(B, self.full_N * 3, **f64),
               "stats": _alloc_stats(B, self.device), "q": torch.empty(B, base.n_joints, **f64),
               "pos_err": torch.empty(B, **f64), "rot_err": torch.empty(B, **f64)}
        if ws:
            out["ws"] = torch.empty(max(int(self.lib.gik_anchored_ws_doubles(self._h, base._h, B)), 1), **f64)
        if clearance:
            out["clearance"] = torch.empty(B, **f64)
        return out

    def anchored_seed(self, base, T_goal, q_init):
        """Goal poses + seed joint angles [B,n] (or [n]) -> the anchored start point on the device
        (gik_anchored_seed_batch): (Y_free [B,N,3], goal [B,n_goal*3]).  Y_free holds the free rows of
        base.seed(T_goal, q_init)'s realization, copied; goal is computed from the goal poses."""
        assert self.anchored and base.has_pipeline
        T, B = base._poses(T_goal)
        q = base._seed_angles(q_init, B)
        f64 = dict(dtype=torch.float64, device=self.device)
        ws = torch.empty(max(int(self.lib.gik_anchored_ws_doubles(self._h, base._h, B)), 1), **f64)
        Y_free = torch.empty(B, self.N * 3, **f64)
        goal = torch.empty(B, self.n_goal_anchor * 3, **f64)
        self._call("gik_anchored_seed_batch", self._h, base._h, T.data_ptr(), q.data_ptr(), B, ws.data_ptr(),
                   Y_free.data_ptr(), goal.data_ptr(), self._stream())
        return Y_free.reshape(B, self.N, 3), goal

    def anchored_clearance(self, Y_full, scenes=None, scene_id=None):
        """Full point matrices [B, full_N, 3] -> clearance [B] on the device (gik_anchored_clearance): the
        minimum of |Y_i - centre| - radius over the free nodes that carry the obstacle hinges and the
        obstacles; +inf without obstacles.  scenes (a SceneSet) / scene_id [B]: goal b against the spheres of its
        scene instead of the template's own (gik_anchored_clearance_scenes)."""
        assert self.anchored
        return self._clearance_of("gik_anchored_clearance", Y_full, scenes, scene_id)

    def _clearance_of(self, name, Y_full, scenes=None, scene_id=None):
        """Full point matrices [B, full_N, 3] (or [full_N, 3]) as a contiguous [B, full_N*3] buffer -> the [B] of the
        export `name`, or with a scene set of `name`_scenes."""
        Y = _dev(Y_full, self.device)
        if Y.dim() == 2:
            Y = Y[None]
        B = Y.shape[0]
        assert Y.numel() == B * self.full_N * 3, (tuple(Y.shape), (B, self.full_N, 3))
        sc, ids = self._scene_desc(scenes, scene_id, B)
        Y = Y.reshape(B, self.full_N * 3).contiguous()
        out = torch.empty(B, dtype=torch.float64, device=self.device)
        if sc is None:
            self._call(name, self._h, Y.data_ptr(), B, out.data_ptr(), self._stream())
        else:
            self._call(name + "_scenes", self._h, Y.data_ptr(), B, C.byref(sc), out.data_ptr(), self._stream())
        return out

    def _scene_desc(self, scenes, scene_id, B, checked=False):
        """(gik_scene_set, ids tensor) of a call of B goals -- checked on the host before any device call -- or
        (None, None) without scenes.  The caller keeps `ids` alive until its call is queued."""
        if scenes is None:
            if scene_id is not None:
                raise ValueError("scene_id needs scenes=")
            return None, None
        if not isinstance(scenes, SceneSet):
            raise TypeError("scenes must be a SceneSet (AnchoredProblem.scene_set, engine.SceneSet)")
        if not self.anchored:
            raise ValueError("scenes belong to the fixed-anchor solve: this template is not anchored")
        if scenes.device != self.device:
            raise ValueError(f"the scene set lives on {scenes.device}, the template on {self.device}")
        ids = scenes.ids(scene_id, (B,), checked)
        return scenes.desc(ids), ids

    def attach_links(self, link_a, link_b, link_radius, hinges=False):
        """The link set of an anchored template (gik_anchored_attach_links), once: link l is the segment between rows
        link_a[l] and link_b[l] of the full point matrix, a capsule of radius link_radius[l] >= 0 (metres).
        hinges=True: the solve carries link hinges (gik_link_desc.hinges = 1) -- every later call on this template, the
        known-answer entry points included, runs the link builds of its kernels; self.link_hinges and
        self.info["anchored"] == 3 say so."""
        if not isinstance(hinges, (bool, np.bool_)):
            raise TypeError(f"hinges must be a bool, got {hinges!r}")
        assert self.anchored
        a = np.ascontiguousarray(link_a, dtype=np.int32).reshape(-1)
        b = np.ascontiguousarray(link_b, dtype=np.int32).reshape(-1)
        r = np.ascontiguousarray(link_radius, dtype=np.float64).reshape(-1)
        if not len(a) == len(b) == len(r):
            raise ValueError("link_a, link_b and link_radius must have one entry per link")
        d = _ffi.LinkDesc(n_link=len(a), hinges=int(hinges), link_a=a.ctypes.data_as(C.POINTER(C.c_int32)),
                          link_b=b.ctypes.data_as(C.POINTER(C.c_int32)),
                          link_radius=r.ctypes.data_as(C.POINTER(C.c_double)))
        self._call("gik_anchored_attach_links", self._h, C.byref(d))
        self.n_link = len(a)
        self.link_hinges = bool(hinges)
        self._read_info()      # (hinges: other kernels, LDS bytes and occupancy)

    def anchored_link_clearance(self, Y_full, scenes=None, scene_id=None):
        """Full point matrices [B, full_N, 3] -> link clearance [B] on the device (gik_anchored_link_clearance): the
        minimum over the attached links and the obstacles of the distance from the sphere to the link's capsule;
        +inf without obstacles or links.  scenes / scene_id: as anchored_clearance (gik_anchored_link_clearance_scenes)."""
        assert self.anchored
        return self._clearance_of("gik_anchored_link_clearance", Y_full, scenes, scene_id)

    def attach_self_pairs(self, pair_l, pair_m):
        """The link pairs of the self clearance (gik_anchored_attach_self_pairs), once, after attach_links: pair p is
        links pair_l[p] and pair_m[p] of the attached set."""
        assert self.anchored
        l = np.ascontiguousarray(pair_l, dtype=np.int32).reshape(-1)
        m = np.ascontiguousarray(pair_m, dtype=np.int32).reshape(-1)
        if len(l) != len(m):
            raise ValueError("pair_l and pair_m must have one entry per pair")
        self._call("gik_anchored_attach_self_pairs", self._h, len(l), l.ctypes.data_as(C.POINTER(C.c_int32)),
                   m.ctypes.data_as(C.POINTER(C.c_int32)))
        self.n_self = len(l)

    def attach_self_hinges(self):
        """Self hinges (gik_anchored_attach_self_hinges), once, after attach_self_pairs: the attached pairs (at most 16)
        become terms of the solve -- every later call on this template, the known-answer entry points included, runs
        the self builds of its kernels; self.self_hinges and bit 4 of self.info["anchored"] (5, with link hinges 7) say so."""
        assert self.anchored
        self._call("gik_anchored_attach_self_hinges", self._h)
        self.self_hinges = True
        self._read_info()      # (other kernels, LDS bytes and occupancy)

    def anchored_self_clearance(self, Y_full):
        """Full point matrices [B, full_N, 3] -> self clearance [B] on the device (gik_anchored_self_clearance): the
        minimum over the attached link pairs of the distance between the two capsules; +inf without pairs."""
        assert self.anchored
        return self._clearance_of("gik_anchored_self_clearance", Y_full)

    def attach_halfspaces(self, halfspaces, node_margin):
        """Half-space obstacles (gik_anchored_attach_halfspaces), once and last -- after attach_links / attach_self_pairs:
        halfspaces [H, 4] rows (nx, ny, nz, d0) with |n| = 1, H within 1 .. 8, the allowed side n.p - d0 >= 0;
        node_margin [N] metres per free node (read where obs_node_mask is 1).  Every later call on this template, the
        known-answer entry points included, runs the half-space builds of its kernels, and every clearance it reports is
        the minimum of the spheres' and anchored_halfspace_clearance; self.n_half and bit 8 of self.info["anchored"]
        (9, with link hinges 11) say so."""
        assert self.anchored
        h = np.ascontiguousarray(halfspaces, dtype=np.float64)
        m = np.ascontiguousarray(node_margin, dtype=np.float64).reshape(-1)
        if h.ndim != 2 or h.shape[1] != 4:
            raise ValueError(f"halfspaces must have shape [H, 4], got {list(h.shape)}")
        if len(m) != self.N:
            raise ValueError(f"node_margin must have one entry per free node ({self.N}), got {len(m)}")
        self._call("gik_anchored_attach_halfspaces", self._h, len(h), h.ctypes.data_as(C.POINTER(C.c_double)),
                   m.ctypes.data_as(C.POINTER(C.c_double)))
        self.n_half = len(h)
        self._read_info()      # (other kernels, LDS bytes and occupancy)

    def anchored_halfspace_clearance(self, Y_full, links=False):
        """Full point matrices [B, full_N, 3] -> [B] on the device (gik_anchored_halfspace_clearance): the minimum over the
        masked free nodes and the half-spaces of n.Y_i - d0 - margin_i, or with links=True over both end rows of every
        attached link of n.P - d0 - link_radius.  What anchored_clearance / anchored_link_clearance fold into theirs."""
        assert self.anchored
        if not isinstance(links, (bool, np.bool_)):
            raise TypeError(f"links must be a bool, got {links!r}")
        Y = _dev(Y_full, self.device)
        if Y.dim() == 2:
            Y = Y[None]
        B = Y.shape[0]
        assert Y.numel() == B * self.full_N * 3, (tuple(Y.shape), (B, self.full_N, 3))
        Y = Y.reshape(B, self.full_N * 3).contiguous()
        out = torch.empty(B, dtype=torch.float64, device=self.device)
        self._call("gik_anchored_halfspace_clearance", self._h, Y.data_ptr(), B, int(links), out.data_ptr(), self._stream())
        return out

    def anchored_sweep_clearances(self, base, q_a, q_b, samples, link_out=None, self_out=None, ws=None, link=True, self_=True):
        """anchored_sweep_clearance with two outputs from one realization of the samples (gik_anchored_sweep_clearances):
        returns (link [B] or None, self [B] or None) -- link / self_ say which are wanted; link_out / self_out [B] and
        `ws` may be handed in to reuse.  Sampled, not conservative."""
        return tuple(self._sweep("gik_anchored_sweep_clearances", base, q_a, q_b, samples, (link, self_), (link_out, self_out), ws))

    def anchored_sweep_clearance(self, base, q_a, q_b, samples, out=None, ws=None):
        """Joint angles q_a, q_b [B,n] (device tensors or arrays) -> [B]: the minimum link clearance over the samples + 1
        configurations on the joint-space line from q_a to q_b (gik_anchored_sweep_clearance).  Sampled, not
        conservative: pick `samples` from the joint step.  `out` [B] and `ws` (gik_anchored_sweep_ws_bytes, as float64)
        may be handed in to reuse."""
        return self._sweep("gik_anchored_sweep_clearance", base, q_a, q_b, samples, (True,), (out,), ws)[0]

    def _sweep(self, name, base, q_a, q_b, samples, wanted, outs, ws):
        """The body of both sweep methods: the checks of samples, q_a and q_b, one [B] output per entry of `wanted` -- the
        caller's tensor from `outs`, a new one where that is None, NULL where it is not wanted --, the workspace, and the
        call of the export `name`.  Returns the outputs as a list, None for one not wanted."""
        assert self.anchored and base.has_pipeline
        if int(samples) != samples or samples < 1:
            raise ValueError(f"samples must be an integer of at least 1, got {samples!r}")
        qa, qb = _dev(q_a, self.device), _dev(q_b, self.device)
        n = base.n_joints
        if qa.dim() != 2 or qa.shape[1] != n or qa.shape != qb.shape:
            raise ValueError(f"q_a and q_b must both have shape [B, {n}], got {list(qa.shape)} and {list(qb.shape)}")
        qa, qb = qa.contiguous(), qb.contiguous()
        B, S = qa.shape[0], int(samples)
        res = []
        for want, out in zip(wanted, outs):
            if want and out is None:
                out = torch.empty(B, dtype=torch.float64, device=self.device)
            assert out is None or (out.is_contiguous() and out.numel() == B)
            res.append(out if want else None)
        nbytes = self.anchored_sweep_ws_bytes(base, B, S)
        if ws is None or ws.numel() * ws.element_size() < nbytes:
            ws = workspace(nbytes, self.device)
        self._call(name, self._h, base._h, qa.data_ptr(), qb.data_ptr(), B, S, ws.data_ptr(),
                   *(None if o is None else o.data_ptr() for o in res), self._stream())
        return res      # (ws goes back to the allocator of this stream, behind the kernels that use it)

    def anchored_ik(self, base, T_goal, q_init=None, out=None, clearance=False, retries=0, retry_seed=0, pos_tol=0.01,
                    rot_tol=0.01, clear_tol=1e-4, retry_spread=0.0, q_limits=None, clearance_mode="nodes", scenes=None,
                    scene_id=None, scene_id_checked=False, retry_candidates=1, atlas=None, atlas_candidates=1):
        """Whole pipeline through the fixed-anchor solve: `base` is the robot graph's Template (no
        obstacles) with its pipeline attached.  Without q_init the start point is the robot graph's bound
        smoothing + MDS one fitted to the anchors (gik_anchored_ik_batch); with q_init (seed joint angles
        [B,n] or [n]; a device tensor may be out["q"] itself) it is the realization of q_init
        (gik_anchored_ik_batch_seeded).  clearance: also the device clearance of the answer.  `out`: the
        buffers of alloc_anchored_buffers, to reuse between calls.  Returns device tensors: x [B, full_N, 3]
        (all robot-graph nodes, anchors included), q, pos_err, rot_err (+ clearance) + stats.

        retries > 0 (gik_anchored_ik_batch_retry): goals that fail -- stop != 0, pos_err > pos_tol, rot_err >
        rot_tol or clearance < -clear_tol -- are solved again, up to `retries` times, from joint angles drawn
        inside q_limits = (q_lo [n], q_hi [n]) by the generator of Template.ik, keyed on (retry_seed, goal,
        attempt): uniformly with retry_spread == 0, within retry_spread radians of q_init otherwise (which
        q_init must then be there for).  The better answer is kept; "attempt" [B] int32 says which one each
        goal holds, and "clearance" is always returned.  That call synchronises the stream once per attempt.
        `out` may carry "attempt" [B] int32, "retry_ws" (gik_anchored_retry_ws_bytes) and "q_lo" / "q_hi", and needs
        no "ws": the restart workspace holds that scratch.

        clearance_mode: "nodes" (the joint points, gik_anchored_clearance), "links" (whole links,
        gik_anchored_link_clearance; needs attach_links) or "links+self" (the minimum of that and
        gik_anchored_self_clearance; needs attach_self_pairs): which clearance comes back and the restart rule reads.
        "links+self" without retries or scenes is gik_anchored_ik_batch_retry with retries = 0 -- attempt 0 and the merged
        clearance, nothing else -- on the restart workspace (`out` may carry "retry_ws").

        scenes (a SceneSet) with scene_id ([B] ints; optional with one scene): goal b is solved among the spheres of
        scene scene_id[b] instead of the template's own, and its clearance is measured against them
        (gik_anchored_ik_batch_scenes, gik_anchored_ik_batch_retry_scenes); everything else combines with it unchanged.
        scene_id_checked: scene_id is a row of an id array SceneSet.ids() has already checked (solve_trajectory).

        retry_candidates (1 .. 16; above 1 needs retries > 0): every restart draws that many candidate seeds per failed
        goal, measures their realizations in clearance_mode and starts from the first one that is clear
        (gik_anchored_ik_batch_retry_screened, with or without scenes).  1: the entries above, one blind seed.

        atlas (an object with the device tensors d_keys [W, M], d_q [M, n] and count = M: riemannian_solver.SeedAtlas) with
        atlas_candidates = C (1 .. 16): gik_anchored_ik_batch_atlas -- attempt 0 starts from the pick among the C atlas rows
        nearest to the goal (from q_init where that is given), restart a from the pick among ranks [a C, (a + 1) C); no
        seed is drawn, so retry_seed and q_limits are not read and retry_spread must be 0.  (retries + 1) C is at most 64
        and at most atlas.count.  Adds "atlas_pick" [B] int32: the atlas row the answer each goal holds started from, -1
        where it started from q_init.  None (the default): the call as it was."""
        assert self.anchored and base.has_pipeline
        retry_candidates = check_retry_candidates(retry_candidates, retries)
        # 1. the checks
        if atlas is not None:
            atlas_candidates = check_atlas_args(atlas, atlas_candidates, retries, retry_candidates, retry_spread)
            if atlas.width != base.atlas_key_width():
                raise ValueError(f"the atlas has keys of width {atlas.width}, the base template's goals have {base.atlas_key_width()}")
            if retries and q_limits is None:      # (not read: no seed is drawn)
                q_limits = (np.zeros(base.n_joints), np.zeros(base.n_joints))
        mode = check_clearance_mode(clearance_mode, getattr(self, "n_link", None) is not None,
                                    getattr(self, "n_self", None) is not None)
        lo = hi = None
        if retries:
            retries, lo, hi = check_retry_args(retries, pos_tol, rot_tol, q_limits, base.n_joints, clear_tol=clear_tol,
                                               retry_spread=retry_spread, has_center=q_init is not None)
        # 2. the plan: retries = 0 on a restart entry is attempt 0 alone -- the call, the link clearance, the self clearance merged
        plan = anchored_call_plan(q_init is not None, clearance, clearance_mode, scenes is not None, retries, retry_candidates,
                                  None if atlas is None else atlas_candidates)
        clearance = bool(clearance or retries or atlas is not None)      # (it always comes back then, whatever `clearance` says)
        # 3. the pointers and the call
        T, B = base._poses(T_goal)
        sc, ids = self._scene_desc(scenes, scene_id, B, scene_id_checked)
        if out is None:      # (the restart workspace holds the scratch "ws")
            out = self.alloc_anchored_buffers(base, B, clearance, ws=not plan.restart)
        q0 = None if q_init is None else base._seed_angles(q_init, B)
        cl = None
        if clearance:
            cl = out["clearance"] if "clearance" in out else torch.empty(B, dtype=torch.float64, device=self.device)
        seed_ptr, cl_ptr = (None if t is None else t.data_ptr() for t in (q0, cl))
        val = dict(q_init=seed_ptr, B=B, scenes=None if sc is None else C.byref(sc), clearance=cl_ptr, null=None, mode=mode,
                   candidates=retry_candidates)
        if plan.restart:
            attempt, ws, q_lo, q_hi = self._retry_buffers(out, B, self.anchored_plan_ws_bytes(base, B, plan), lo, hi,
                                                          limits=bool(retries) and atlas is None)
            opts = _retry_opts(retries if atlas is None else 0, retry_seed, pos_tol, rot_tol, q_lo, q_hi, mode, clear_tol, retry_spread)
            if atlas is not None:      # (no seed, no limits, no spread: the options of attempt 0 with the retry count)
                opts.retries = int(retries)
                val.update(candidates=atlas_candidates, atlas_keys=atlas.d_keys.data_ptr(), atlas_q=atlas.d_q.data_ptr(), atlas_count=atlas.count)
            val.update(opts=C.byref(opts), attempt=attempt.data_ptr())
            extras = {"clearance": cl, "attempt" if retries else "_attempt": attempt, "_retry_ws": ws}
        else:
            ws = out["ws"]
            assert ws.numel() >= int(self.lib.gik_anchored_ws_doubles(self._h, base._h, B))
            extras = {"_ws": ws, "clearance": cl} if clearance else {"_ws": ws}
        val["ws"] = ws.data_ptr()
        answer = [out[key].data_ptr() for key in ("Y", "stats", "q", "pos_err", "rot_err")]
        args = [v for name in plan.args for v in (answer if name == "answer" else [val[name]])]
        if retries or sc is not None:
            extras["_scene_id"] = ids      # (read by the kernel: lives as long as the result; None without scenes)
        self._call(plan.entry, self._h, base._h, T.data_ptr(), *args, self._stream())
        if plan.after:      # the clearance of an entry that does not measure it itself
            self._call(plan.after, self._h, out["Y"].data_ptr(), B, cl_ptr, self._stream())
        if atlas is not None:
            extras["atlas_pick"] = torch.empty(B, dtype=torch.int32, device=self.device)
            extras["_atlas"] = atlas      # (its tensors are read by the kernels: lives as long as the result)
            self._call("gik_anchored_atlas_picks", self._h, base._h, B, atlas_candidates, int(retries), ws.data_ptr(),
                       attempt.data_ptr(), extras["atlas_pick"].data_ptr(), self._stream())
        return _result(out, (B, self.full_N, 3), extras)

    def alloc_ik_buffers(self, B):
        f64 = dict(dtype=torch.float64, device=self.device)
        return {"targets": torch.empty(B, self.T, **f64), "Y": torch.empty(B, self.N * self.k, **f64),
                "stats": _alloc_stats(B, self.device), "q": torch.empty(B, self.n_joints, **f64),
                "pos_err": torch.empty(B, **f64), "rot_err": torch.empty(B, **f64)}

    # -- trust-region solve -------------------------------------------------------------------
    def solve(self, Y_init, targets, trace_cap=0, scenes=None, scene_id=None):
        """Batched TrustRegions.solve.  Returns dict of device tensors:
        x [B,N,k], f, gradnorm, iterations, inner_total, stop, n_accept (+ trace arrays).
        scenes (a SceneSet) / scene_id [B], anchored templates: problem b among the spheres of its scene instead of the
        template's own (gik_solve_batch_scenes)."""
        Y, B = self._vec(Y_init)
        t = self._tg(targets, B)
        sc, ids = self._scene_desc(scenes, scene_id, B)
        out = torch.empty_like(Y)
        stats = _alloc_stats(B, self.device)
        tr = None
        keep = {}
        if trace_cap > 0:
            tr = _ffi.Trace()
            tr.cap = trace_cap
            for name, dt in (("Delta", torch.float64), ("numit", torch.int32),
                             ("stop", torch.int32), ("f_before", torch.float64),
                             ("gradnorm_after", torch.float64), ("accept", torch.int32)):
                fill = float("nan") if dt == torch.float64 else -9
                keep[name] = torch.full((B, trace_cap), fill, dtype=dt, device=self.device)
                setattr(tr, "d_" + name, keep[name].data_ptr())
        args = (self._h, Y.data_ptr(), t.data_ptr(), B, out.data_ptr(), stats.data_ptr(), C.byref(tr) if tr is not None else None)
        if sc is None:
            self._call("gik_solve_batch", *args, self._stream())
        else:
            self._call("gik_solve_batch_scenes", *args, C.byref(sc), self._stream())
        res = {"x": out.reshape(B, self.N, self.k)}
        if ids is not None:
            res["_scene_id"] = ids      # (read by the kernel: lives as long as the result)
        res.update(_decode_stats(stats))
        if tr is not None:
            res["trace"] = keep
        return res
