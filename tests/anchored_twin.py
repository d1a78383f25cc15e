"""A numpy twin of the fixed-anchor trust-region solve that knows the three hinge families (link hinges, self hinges,
half-spaces): the loop of oracle/gik_oracle.c (tcg, gik_o_rtr_solve_anchored with at != NULL) restated line for line, driven
by a callable terms(Y, W) -> (f, G, H W) in the mirrors' convention (f = sum res^2, G = 1/2 grad f, H W = 1/2 Hess f [W]).
The C twin knows point-to-anchor terms only; this one takes whatever the callable sums.

Plain module (numpy only): tests/test_anchored_hinge_twin_host.py holds it against the C twin and asserts every condition on
its inputs, tests/test_anchored_hinge_twin_gpu.py compares the device with it.  The space is Euclidean: no retraction, no
projection.  The Hessian of a hinge is the frozen-foot model of the kernels; evaluating it at the kept point x for every
tCG product of an outer iteration is the same thing as freezing the feet when x was accepted."""
import numpy as np

from parity_util import TRAJ_KEYS, anchored_numpy, anchored_terms

# trust_region.py:68-75, the codes of the C twin and of the device trace
NEGATIVE_CURVATURE, EXCEEDED_TR, REACHED_TARGET_LINEAR, REACHED_TARGET_SUPERLINEAR, MAX_INNER_ITER, MODEL_INCREASED = range(6)
# gik_o_default_params; Delta_bar = 10 + k with k = 3, Delta0 = Delta_bar / 8
DEFAULTS = dict(mingradnorm=0.5 * 1e-9, maxinner=10000, mininner=1, theta=1.0, kappa=0.1, rho_prime=0.1,
                rho_regularization=1e3, Delta_bar=13.0, Delta0=13.0 / 8.0)
EPS = 2.220446049250313e-16


def _dot(a, b):
    """dot() of the C twin: one running sum over the N * k entries in storage order."""
    s = 0.0
    for u, v in zip(a.ravel().tolist(), b.ravel().tolist()):
        s += u * v
    return s


def _call(terms, Y, W, role):
    """terms(Y, W); a callable with takes_role is also told which call of the loop this is ("start", "hess", "trial",
    "accept") -- what the planted faults of HingeTerms key on."""
    if getattr(terms, "takes_role", False):
        return terms(Y, W, role=role)
    return terms(Y, W)


def tcg_numpy(terms, x, fgradx, Delta, p):
    """tcg() of oracle/gik_oracle.c -> (eta, Heta, numit, stop_tCG)."""
    Z = np.zeros_like(x)
    eta, Heta, r = Z.copy(), Z.copy(), fgradx.copy()
    e_Pe = 0.0
    r_r = _dot(r, r)
    norm_r = np.sqrt(r_r)
    norm_r0 = norm_r
    z_r = _dot(r, r)
    d_Pd = z_r
    delta = -r
    e_Pd = 0.0
    model_value = 0.0
    stop_tCG = MAX_INNER_ITER
    j = 0
    maxinner = int(p["maxinner"])
    while j < maxinner:
        Hdelta = _call(terms, x, delta, "hess")[2]
        d_Hd = _dot(delta, Hdelta)
        with np.errstate(divide="ignore", invalid="ignore"):
            alpha = np.float64(z_r) / np.float64(d_Hd)
        e_Pe_new = e_Pe + 2.0 * alpha * e_Pd + alpha * alpha * d_Pd
        if d_Hd <= 0 or e_Pe_new >= Delta * Delta:
            tau = (-e_Pd + np.sqrt(e_Pd * e_Pd + d_Pd * (Delta * Delta - e_Pe))) / d_Pd
            eta = eta + tau * delta
            Heta = Heta + tau * Hdelta
            stop_tCG = NEGATIVE_CURVATURE if d_Hd <= 0 else EXCEEDED_TR
            break
        e_Pe = e_Pe_new
        new_eta = eta + alpha * delta
        new_Heta = Heta + alpha * Hdelta
        new_model_value = _dot(new_eta, fgradx) + 0.5 * _dot(new_eta, new_Heta)
        if new_model_value >= model_value:
            stop_tCG = MODEL_INCREASED
            break
        eta, Heta = new_eta, new_Heta
        model_value = new_model_value
        r = r + alpha * Hdelta
        r_r = _dot(r, r)
        norm_r = np.sqrt(r_r)
        if j >= p["mininner"] and norm_r <= norm_r0 * min(norm_r0 ** p["theta"], p["kappa"]):
            stop_tCG = REACHED_TARGET_LINEAR if p["kappa"] < norm_r0 ** p["theta"] else REACHED_TARGET_SUPERLINEAR
            break
        zold_rold = z_r
        z_r = _dot(r, r)
        beta = z_r / zold_rold
        delta = -r + beta * delta
        e_Pd = beta * (e_Pd + alpha * d_Pd)
        d_Pd = z_r + beta * beta * d_Pd
        j += 1
    if j >= maxinner:
        j = maxinner - 1
    return eta, Heta, j, stop_tCG


def rtr_numpy(terms, Y0, maxiter=3000, trace_cap=32, **params):
    """gik_o_rtr_solve_anchored on terms(Y, W) from Y0 [N, 3].  Returns a dict: x, f, gradnorm, iterations, inner_total,
    stop (0: gradient rule, 1: maxiter), and "traj" with the keys of parity_util.TRAJ_KEYS (the first trace_cap outer
    iterations) plus
      x      the iterate after every outer iteration (x[k]: after k + 1 of them),
      state  terms.last_state at every accepted point, the start point first (None for a callable without one),
      at     the outer iteration that accepted it (-1: the start point)."""
    p = dict(DEFAULTS)
    unknown = set(params) - set(p)
    assert not unknown, unknown
    p.update(params)
    x = np.array(Y0, dtype=np.float64)
    Z = np.zeros_like(x)
    Delta_bar, Delta = p["Delta_bar"], p["Delta0"]
    kiter = 0
    fx, fgradx, _ = _call(terms, x, Z, "start")
    fgradx = np.array(fgradx)
    norm_grad = np.sqrt(_dot(fgradx, fgradx))
    inner_total, stop = 0, 1
    traj = {k: [] for k in TRAJ_KEYS}
    traj.update(x=[], state=[getattr(terms, "last_state", None)], at=[-1])
    while True:
        eta, Heta, numit, stop_inner = tcg_numpy(terms, x, fgradx, Delta, p)
        inner_total += numit + 1
        rec = len(traj["Delta"]) < trace_cap
        if rec:
            traj["Delta"].append(Delta); traj["numit"].append(numit); traj["stop"].append(stop_inner); traj["f_before"].append(fx)
        x_prop = x + eta
        fx_prop = _call(terms, x_prop, Z, "trial")[0]
        rhonum = fx - fx_prop
        rhoden = -_dot(fgradx, eta) - 0.5 * _dot(eta, Heta)
        rho_reg = max(1.0, abs(fx)) * EPS * p["rho_regularization"]
        rhonum = rhonum + rho_reg
        rhoden = rhoden + rho_reg
        model_decreased = rhoden >= 0
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = np.float64(rhonum) / np.float64(rhoden)
        if rho < 1.0 / 4 or not model_decreased or np.isnan(rho):
            Delta = Delta / 4
        elif rho > 3.0 / 4 and stop_inner in (NEGATIVE_CURVATURE, EXCEEDED_TR):
            Delta = min(2 * Delta, Delta_bar)
        accept = 0
        if model_decreased and rho > p["rho_prime"]:
            accept = 1
            x = x_prop
            fx = fx_prop
            fgradx = np.array(_call(terms, x, Z, "accept")[1])
            norm_grad = np.sqrt(_dot(fgradx, fgradx))
            traj["state"].append(getattr(terms, "last_state", None))
            traj["at"].append(kiter)
        kiter += 1
        if rec:
            traj["gradnorm_after"].append(norm_grad); traj["accept"].append(accept); traj["x"].append(x.copy())
        if kiter >= maxiter:
            stop = 1
            break
        if norm_grad < p["mingradnorm"]:
            stop = 0
            break
    out = {k: np.array(traj[k], dtype=np.float64 if k in ("Delta", "f_before", "gradnorm_after") else np.int32) for k in TRAJ_KEYS}
    out.update(x=traj["x"], state=traj["state"], at=traj["at"])
    return dict(x=x, f=fx, gradnorm=norm_grad, iterations=kiter, inner_total=inner_total, stop=stop, traj=out)


MUTANTS = ("trial_state", "trial_cost", "grad_scale")


class HingeTerms:
    """terms(Y, W) of one goal of a host-only AnchoredProblem: parity_util.anchored_numpy (free-free, pinned and node-sphere
    terms) plus whichever of link_hinge_terms_host, self_hinge_terms_host and halfspace_terms_host the problem carries.
    reverse: the shares are added in the other order (a second rendering of the same sum).  last_state: the hinge state
    of the last point evaluated -- half: the active (node, half-space) set, links: {(link, sphere): t} and self:
    {pair: (s, t)} of the active hinges.  last_hinge_f: the hinge shares' part of that point's f.

    mutant plants one fault of a solve kernel (None: the true twin):
      "trial_state"  the Hessian's hinge shares use the frozen state of the last TRIAL point, accepted or not
      "trial_cost"   the hinge shares are left out of the trial point's cost
      "grad_scale"   the hinge shares of G are scaled by 1 + 1e-6"""
    takes_role = True

    def __init__(self, ap, goal_anchor, reverse=False, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.ap, self.ga, self.reverse, self.mutant = ap, np.asarray(goal_anchor, dtype=np.float64), reverse, mutant
        self.Nf = len(ap.free)
        self.families = [name for name, on in (("links", ap.link_hinges), ("self", ap.self_hinges), ("half", ap.halfspaces is not None)) if on]
        self.last_state, self.last_hinge_f, self._trial = None, 0.0, None

    def _share(self, name, Y, W, frozen):
        ap = self.ap
        if name == "links":
            out = ap.link_hinge_terms_host(Y, W, self.ga, frozen_t=None if frozen is None else frozen["links"])
            return out, dict(ap.last_link_t)
        if name == "self":
            out = ap.self_hinge_terms_host(Y, W, self.ga, frozen_st=None if frozen is None else frozen["self"])
            return out, dict(ap.last_self_st)
        out = ap.halfspace_terms_host(Y, W, frozen_active=None if frozen is None else frozen["half"])
        return out, frozenset(ap.last_half_active)

    def __call__(self, Y, W, role=None):
        frozen = self._trial if (self.mutant == "trial_state" and role == "hess") else None
        shares = [anchored_numpy(self.ap, self.Nf, Y, W, self.ga)]
        state, fh = {}, 0.0
        for name in self.families:
            (f, G, H), st = self._share(name, Y, W, frozen)
            if self.mutant == "grad_scale":
                G = G * (1.0 + 1e-6)
            if self.mutant == "trial_cost" and role == "trial":
                f = 0.0
            shares.append((f, G, H))
            state[name] = st
            fh += f
        if self.reverse:
            shares = shares[::-1]
        f, G, H = shares[0]
        G, H = np.array(G), np.array(H)
        for f2, G2, H2 in shares[1:]:
            f, G, H = f + f2, G + G2, H + H2
        if frozen is None:      # (a frozen evaluation reports the frozen state back, not the point's own)
            self.last_state, self.last_hinge_f = state, fh
        if role == "trial":
            self._trial = state
        return f, G, H


class FastTerms:
    """The same sum as HingeTerms, every family evaluated over all of its terms at once (numpy arrays; the closest-point
    functions are the module's own _link_foot and _segment_feet): a rendering of the twin that differs from the mirrors'
    in rounding and summation order only, and costs a tenth.  It carries no state and plants no fault; the host file holds
    it to HingeTerms at 1e-12 and uses it for the many renderings a stable prefix is measured over."""

    def __init__(self, ap, goal_anchor, reverse=False):
        from graphik_amd.solvers import riemannian_solver as rs
        self.rs, self.ap, self.reverse = rs, ap, reverse
        self.N = ap.base.N
        self.free = np.asarray(ap.free)
        self.apos = np.array(ap.anchor_pos, dtype=np.float64)
        if ap.n_goal_anchor:
            self.apos[len(self.apos) - ap.n_goal_anchor:] = np.asarray(goal_anchor, dtype=np.float64).reshape(-1, 3)
        self.ti, self.tj, self.tk, self.tt = (np.asarray(a) for a in ap.free_terms)
        self.an, self.ap_, self.at_, self.ak = anchored_terms(ap, goal_anchor)
        self.is_free = np.zeros(self.N, dtype=bool)
        self.is_free[self.free] = True

    @staticmethod
    def _pair(y, w, tgt, kind):
        d = (y * y).sum(axis=1)
        u = tgt - d
        act = (kind == 1) | ((kind == 2) & (u > 0)) | ((kind == 3) & (u < 0))
        c = np.where(act, d - tgt, 0.0)
        yw = np.where(act, (y * w).sum(axis=1), 0.0)
        return float((np.where(act, u, 0.0) ** 2).sum()), 2 * c[:, None] * y, 2 * (2 * yw[:, None] * y + c[:, None] * w)

    def _full(self, Y, W):
        P, V = np.zeros((self.N, 3)), np.zeros((self.N, 3))
        P[self.free], V[self.free] = Y, W
        P[np.asarray(self.ap.anchors)] = self.apos
        return P, V

    def _anchored(self, Y, W):
        G, H = np.zeros_like(Y), np.zeros_like(Y)
        f1, g, h = self._pair(Y[self.ti] - Y[self.tj], W[self.ti] - W[self.tj], self.tt, self.tk)
        np.add.at(G, self.ti, g); np.add.at(G, self.tj, -g); np.add.at(H, self.ti, h); np.add.at(H, self.tj, -h)
        f2, g, h = self._pair(Y[self.an] - self.ap_, W[self.an], self.at_, self.ak)
        np.add.at(G, self.an, g); np.add.at(H, self.an, h)
        return f1 + f2, G, H

    def _links(self, Y, W):
        ap = self.ap
        P, V = self._full(Y, W)
        ra, rb = ap.link_rows[:, 0], ap.link_rows[:, 1]
        A, B, C = P[ra][:, None], P[rb][:, None], ap.obstacles[None, :, :3]
        t = self.rs._link_foot(A, B, C)[3]
        m = ((1.0 - t)[..., None] * A + t[..., None] * B) - C
        R = np.sqrt(ap.obstacles[None, :, 3] ** 2) + ap.link_radius[:, None]
        res = R * R - (m * m).sum(axis=-1)
        act = (res > 0.0) & (self.is_free[ra] | self.is_free[rb])[:, None]
        c = np.where(act, -res, 0.0)
        om = (1.0 - t)[..., None] * V[ra][:, None] + t[..., None] * V[rb][:, None]
        mo = np.where(act, (m * om).sum(axis=-1), 0.0)
        g = 2.0 * c[..., None] * m
        hv = 2.0 * (2.0 * mo[..., None] * m + c[..., None] * om)
        G, H = np.zeros((self.N, 3)), np.zeros((self.N, 3))
        np.add.at(G, ra, ((1.0 - t)[..., None] * g).sum(axis=1)); np.add.at(G, rb, (t[..., None] * g).sum(axis=1))
        np.add.at(H, ra, ((1.0 - t)[..., None] * hv).sum(axis=1)); np.add.at(H, rb, (t[..., None] * hv).sum(axis=1))
        return float((np.where(act, res, 0.0) ** 2).sum()), G[self.free], H[self.free]

    def _self(self, Y, W):
        ap = self.ap
        P, V = self._full(Y, W)
        l, m_ = ap.self_pairs[:, 0], ap.self_pairs[:, 1]
        ends = [ap.link_rows[l, 0], ap.link_rows[l, 1], ap.link_rows[m_, 0], ap.link_rows[m_, 1]]
        s, t, v, d = self.rs._segment_feet(*(P[e] for e in ends))
        R = ap.link_radius[l] + ap.link_radius[m_]
        res = R * R - d
        act = res > 0.0
        c = np.where(act, -res, 0.0)
        w = (1.0 - s, s, -(1.0 - t), -t)
        om = sum(wq[:, None] * V[e] for wq, e in zip(w, ends))
        vo = np.where(act, (v * om).sum(axis=-1), 0.0)
        g = 2.0 * c[:, None] * v
        hv = 2.0 * (2.0 * vo[:, None] * v + c[:, None] * om)
        G, H = np.zeros((self.N, 3)), np.zeros((self.N, 3))
        for wq, e in zip(w, ends):
            np.add.at(G, e, wq[:, None] * g); np.add.at(H, e, wq[:, None] * hv)
        return float((np.where(act, res, 0.0) ** 2).sum()), G[self.free], H[self.free]

    def _half(self, Y, W):
        ap = self.ap
        n, d0 = ap.halfspaces[:, :3], ap.halfspaces[:, 3]
        res = ap.halfspace_margin[:, None] - (Y @ n.T - d0[None])
        act = (res > 0.0) & (ap.obs_mask == 1)[:, None]
        r = np.where(act, res, 0.0)
        return float((r * r).sum()), -(r @ n), (np.where(act, W @ n.T, 0.0)) @ n

    def __call__(self, Y, W):
        ap = self.ap
        shares = [self._anchored(Y, W)]
        if ap.link_hinges:
            shares.append(self._links(Y, W))
        if ap.self_hinges:
            shares.append(self._self(Y, W))
        if ap.halfspaces is not None:
            shares.append(self._half(Y, W))
        if self.reverse:
            shares = shares[::-1]
        f, G, H = shares[0]
        for f2, G2, H2 in shares[1:]:
            f, G, H = f + f2, G + G2, H + H2
        return f, G, H


def state_changes(a, b):
    """(active set differs, a hinge active in both moved its foot parameter) between the hinge states of two points."""
    active = lambda s: {(fam, key) for fam, v in s.items() for key in v}      # noqa: E731
    moved = any(a[fam][key] != b[fam][key] for fam in ("links", "self") if fam in a for key in a[fam] if key in b[fam])
    return active(a) != active(b), moved
