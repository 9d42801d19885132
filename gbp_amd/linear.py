"""Linear pairwise GBP on the MI355X (include/gbp_lin.h): the reference's generic FactorGraph path
(gbp/gbp.py with nonlinear_factors=False, ndim_posegraph.py) for two-variable factors over d <= 6 dofs.

`LinearEngine.from_factor_graph(graph)` takes a host graph built with the drop-in `gbp.gbp` classes
(after `compute_all_factors()`, ndim_posegraph.py:91) and runs its sweeps on the device; the host
graph is left untouched.  Factors that carry `loss='huber'` / `'constant'` keep it: `iterate(n, robustify=True)`.  No CPU fallback: without a GPU `gbp_lin_create` fails with GBP_ENODEV.
"""
from __future__ import annotations

import ctypes as ct

import numpy as np

from . import _capi
from ._capi import check, dptr, iptr, f64, i32


def _host_factors(factors, index):
    """(var_a, var_b, eta, lam, const, loss, threshold, noise_var) of host Factors (gbp.py:201-294) in the order given; `index` maps
    a variableID to its position in graph.var_nodes."""
    va, vb, fe, fl, fc, loss, thr, nvar = [], [], [], [], [], [], [], []
    for fac in factors:
        if len(fac.adj_vIDs) != 2:
            raise ValueError("only two-variable factors")
        if fac.adaptive_gauss_noise_var != fac.gauss_noise_var:
            raise ValueError(f"factor {fac.factorID} arrives already rescaled by robustify_loss (adaptive_gauss_noise_var != "
                             "gauss_noise_var): the device stores nominal factors and makes the weights itself")
        loss.append(fac.loss); thr.append(float(fac.mahalanobis_threshold)); nvar.append(float(fac.gauss_noise_var))
        va.append(index[fac.adj_vIDs[0]]); vb.append(index[fac.adj_vIDs[1]])
        fe.append(np.asarray(fac.factor.eta, dtype=float)); fl.append(np.asarray(fac.factor.lam, dtype=float))
        x0 = np.asarray(fac.linpoint, dtype=float)
        J = np.atleast_2d(fac.jac_fn(fac.linpoint, *fac.args))
        r = J @ x0 + fac.measurement - fac.meas_fn(fac.linpoint, *fac.args)        # = z - h(0) for a linear h
        fc.append(0.5 * float(np.dot(np.atleast_1d(r), np.atleast_1d(r))) / fac.adaptive_gauss_noise_var)
    return va, vb, fe, fl, fc, loss, thr, nvar


def _new_priors(prior_eta, prior_lam, D):
    """(dN, prior_eta (dN, D), prior_lam (dN, D, D)) of an extend; None: no new variables."""
    dN = 0 if prior_eta is None else f64(prior_eta).reshape(-1, D).shape[0]
    pe = f64(np.zeros((0, D)) if prior_eta is None else prior_eta, (dN, D))
    pl = f64(np.zeros((0, D, D)) if prior_lam is None else prior_lam, (dN, D, D))
    return dN, pe, pl


def _loss_arrays(loss, threshold, noise_var, count):
    """(codes int32, thresholds, noise variances or None) of `count` factors from one loss name or `count` of them and scalars or
    `count` values; at least one entry long, so that an empty list still is a non-NULL pointer."""
    names = [loss] * count if isinstance(loss, str) else list(loss)
    if len(names) != count:
        raise ValueError(f"expected {count} losses, got {len(names)}")
    bad = [l for l in names if l not in _capi.LIN_LOSS]
    if bad:
        raise ValueError(f"unknown loss {bad[0]!r}: None, 'huber' or 'constant'")
    n = max(count, 1)
    codes = np.zeros(n, dtype=np.int32)
    codes[:count] = [_capi.LIN_LOSS[l] for l in names]
    thr = np.ones(n)
    thr[:count] = np.broadcast_to(np.asarray(threshold, dtype=np.float64), (count,))
    nv = None
    if noise_var is not None:
        nv = np.ones(n)
        nv[:count] = np.broadcast_to(np.asarray(noise_var, dtype=np.float64), (count,))
    return codes, thr, nv


class UntilResult:
    """What LinearEngine.iterate_until returns: iters (the deciding sweep, or max_iters), converged, reason (GBP_LIN_STOP_*:
    _capi.LIN_STOP_STEP, LIN_STOP_MAP, or LIN_STOP_NONE when max_iters ran out), and one value per sweep run: step, energy,
    map_distance (the last two None when not asked for).  From iterate_until_nonlinear also relin_counts, and with robustify
    robust_counts: the factors relinearised / flagged in each sweep run, int32 (None otherwise)."""
    __slots__ = ('iters', 'converged', 'reason', 'step', 'energy', 'map_distance', 'relin_counts', 'robust_counts')

    def __init__(self, iters, converged, reason, step, energy, map_distance, relin_counts=None, robust_counts=None):
        self.iters, self.converged, self.reason = iters, converged, reason
        self.step, self.energy, self.map_distance = step, energy, map_distance
        self.relin_counts, self.robust_counts = relin_counts, robust_counts

    def __repr__(self):
        return f"UntilResult(iters={self.iters}, converged={self.converged}, reason={self.reason})"


class NonlinearMapResult:
    """What LinearEngine.solve_map_nonlinear returns: outer (LM iterations run = accepted + rejected), cg_iters (summed over the inner
    solves), converged, reason (_capi.LIN_NLMAP_STEP / GRAD / STALL, or NONE when max_outer ran out), energy0 / energy (the factor
    energy at x0 and at the final x), grad_norm, lambda_ (what the next iteration would use), and one value per iteration run: energy_trace
    (at x before the step), lambdas, steps (max |dx|), dphi, taken (bool).  The final x: LinearEngine.map_mean()."""
    __slots__ = ('outer', 'accepted', 'rejected', 'cg_iters', 'converged', 'reason', 'energy0', 'energy', 'grad_norm', 'lambda_',
                 'energy_trace', 'lambdas', 'steps', 'dphi', 'taken')

    def __init__(self, info, trace):
        for k in ('outer', 'accepted', 'rejected', 'cg_iters', 'reason', 'energy0', 'energy', 'grad_norm', 'lambda_'):
            setattr(self, k, getattr(info, k))
        self.converged = bool(info.converged)
        rows = trace[:info.outer]
        self.energy_trace, self.lambdas, self.steps, self.dphi = (rows[:, k].copy() for k in range(4))
        self.taken = rows[:, 4] != 0.0

    def __repr__(self):
        return f"NonlinearMapResult(outer={self.outer}, accepted={self.accepted}, converged={self.converged}, reason={self.reason}, energy={self.energy:.6g})"


class RobustNonlinearMapResult:
    """What LinearEngine.solve_map_nonlinear_robust returns: rounds (LM runs), outer / accepted / rejected / cg_iters (summed over the
    rounds), converged, reason (_capi.LIN_IRLS_WEIGHTS / MOVE, or NONE when max_rounds ran out), flagged, energy0 / energy (the
    weighted factor energy at the first and the last reweight), weight_change, move, grad_norm; round_trace (rounds + 1, 6): weighted
    energy, flagged count, weight_change, the previous round's move, the LM iterations of the round and its LM reason; lm_trace
    (outer, 5): the rounds' rows of solve_map_nonlinear one after the other; weights (F,) and robust_flag (F,) bool at the final x --
    robust_flag is the outlier report.  The final x: LinearEngine.map_mean()."""
    __slots__ = ('rounds', 'outer', 'accepted', 'rejected', 'cg_iters', 'converged', 'reason', 'flagged', 'energy0', 'energy', 'weight_change', 'move',
                 'grad_norm', 'round_trace', 'lm_trace', 'weights', 'robust_flag')

    def __init__(self, info, round_trace, lm_trace, weights, flag):
        for k in ('rounds', 'outer', 'accepted', 'rejected', 'cg_iters', 'reason', 'flagged', 'energy0', 'energy', 'weight_change', 'move', 'grad_norm'):
            setattr(self, k, getattr(info, k))
        self.converged = bool(info.converged)
        self.round_trace = round_trace[:info.rounds + 1].copy()
        self.lm_trace = lm_trace[:info.outer].copy()
        self.weights, self.robust_flag = weights, flag != 0

    def __repr__(self):
        return (f"RobustNonlinearMapResult(rounds={self.rounds}, outer={self.outer}, converged={self.converged}, reason={self.reason}, "
                f"flagged={self.flagged}, energy={self.energy:.6g})")


class LinearEngine:
    def __init__(self, var_a, var_b, factor_eta, factor_lam, prior_eta, prior_lam, factor_const=None, eta_damping=0.0, device=0):
        self._lib = _capi.load()
        prior_eta = f64(prior_eta)
        self.N, self.D = prior_eta.shape
        prior_lam = f64(prior_lam, (self.N, self.D, self.D))
        var_a, var_b = i32(var_a).reshape(-1), i32(var_b).reshape(-1)
        self.F = var_a.shape[0]
        factor_eta = f64(factor_eta, (self.F, 2 * self.D))
        factor_lam = f64(factor_lam, (self.F, 2 * self.D, 2 * self.D))
        fc = None if factor_const is None else f64(factor_const, (self.F,))
        if var_b.shape[0] != self.F:
            raise ValueError("var_a / var_b length mismatch")
        d = _capi.LinDesc()
        d.n_vars, d.dofs, d.n_factors, d.device = self.N, self.D, self.F, int(device)
        d.var_a, d.var_b = iptr(var_a), iptr(var_b)
        d.factor_eta, d.factor_lam, d.factor_const = dptr(factor_eta), dptr(factor_lam), dptr(fc)
        d.prior_eta, d.prior_lam = dptr(prior_eta), dptr(prior_lam)
        d.eta_damping = float(eta_damping)
        self._h = ct.c_void_p()
        self._nonlinear = False                              # set_nonlinear was called: the handle grows by extend_se2 / extend_se3, shrinks by gbp_lin_shrink_nonlinear
        self._model = None                                   # its model then (_capi.LIN_MODEL_*)
        check(self._lib.gbp_lin_create(ct.byref(self._h), ct.byref(d)))

    @classmethod
    def from_factor_graph(cls, graph, device=0):
        """A host FactorGraph(nonlinear_factors=False) of pairwise equal-size factors (gbp/gbp.py:11-153) -> device."""
        if getattr(graph, 'nonlinear_factors', True):
            raise ValueError("only linear graphs (nonlinear_factors=False) have a device path here; BA graphs use gbp.gbp_ba")
        index = {v.variableID: i for i, v in enumerate(graph.var_nodes)}
        dofs = {v.dofs for v in graph.var_nodes}
        if len(dofs) != 1:
            raise ValueError("all variables must have the same number of dofs")
        D = dofs.pop()
        va, vb, fe, fl, fc, loss, thr, nvar = _host_factors(graph.factors, index)
        for v in graph.var_nodes:                                                       # adjacency order the device assumes
            ids = [f.factorID for f in v.adj_factors]
            if ids != sorted(ids):
                raise ValueError("adj_factors must be in ascending factor id (ndim_posegraph.py:86-88)")
        eng = cls(va, vb, np.array(fe).reshape(-1, 2 * D), np.array(fl).reshape(-1, 2 * D, 2 * D),
                  np.array([v.prior.eta for v in graph.var_nodes]).reshape(-1, D),
                  np.array([v.prior.lam for v in graph.var_nodes]).reshape(-1, D, D),
                  factor_const=fc, eta_damping=graph.eta_damping, device=device)
        if any(l is not None for l in loss):                                           # Factor(loss=, mahalanobis_threshold=) gbp.py:209-210
            eng.set_robust(loss, thr, nvar)
        return eng

    # growing a live graph (var_nodes.append / factors.append / adj_factors.append ndim_posegraph.py:67-88 + update_all_beliefs gbp.py:56-58)
    def extend(self, var_a, var_b, factor_eta, factor_lam, prior_eta=None, prior_lam=None, factor_const=None, loss=None, threshold=2.0,
               noise_var=None):
        """Append dN variables (their priors: ids N .. N + dN - 1) and dF factors (ids F .. F + dF - 1, joining any variables old or
        new) on the device; the messages of the old factors are kept, the new ones start at zero.  loss: None, or one name or dF of
        None / 'huber' / 'constant' for the new factors (rules of set_robust).  Beliefs, where the handle had them, are re-made for
        the grown graph; solve_map / marginals results are dropped until the next solve."""
        var_a, var_b = i32(var_a).reshape(-1), i32(var_b).reshape(-1)
        dF = var_a.shape[0]
        if var_b.shape[0] != dF:
            raise ValueError("var_a / var_b length mismatch")
        dN, pe, pl = _new_priors(prior_eta, prior_lam, self.D)
        fe = f64(np.asarray(factor_eta, dtype=np.float64).reshape(dF, 2 * self.D))
        fl = f64(np.asarray(factor_lam, dtype=np.float64).reshape(dF, 2 * self.D, 2 * self.D))
        fc = None if factor_const is None else f64(factor_const, (dF,))
        d = _capi.LinExt()
        d.n_new_vars, d.n_new_factors = dN, dF
        d.var_a, d.var_b = iptr(var_a), iptr(var_b)
        d.factor_eta, d.factor_lam, d.factor_const = dptr(fe), dptr(fl), dptr(fc)
        d.prior_eta, d.prior_lam = dptr(pe), dptr(pl)
        keep = None
        if loss is not None and dF:
            keep = codes, thr, nv = _loss_arrays(loss, threshold, noise_var, dF)
            d.loss, d.threshold, d.noise_var = iptr(codes), dptr(thr), dptr(nv)
        check(self._lib.gbp_lin_extend(self._h, ct.byref(d)))
        del keep
        self.N, self.F = self.N + dN, self.F + dF

    def sizes(self):
        """(N, F) as the handle holds them."""
        n, f = ct.c_int32(), ct.c_int32()
        check(self._lib.gbp_lin_get_sizes(self._h, ct.byref(n), ct.byref(f)))
        return n.value, f.value

    # shrinking a live graph: retired variables and dropped factors leave, their last messages folded into the survivors' priors
    def shrink(self, retire_vars=(), drop_factors=(), fold=True):
        """Retire variables and drop factors on the device.  A factor leaves if it is listed or has a retired end; with fold=True a
        leaving factor that is not listed and has one surviving end adds its stored message to that end's prior (GBP's own
        marginalisation), otherwise its messages are dropped.  Survivors are renumbered monotonically and keep their messages; beliefs,
        where the handle had them, are re-made; solve_map / marginals results are dropped until the next solve.  On an engine of
        se2_pose_graph every survivor also keeps its linearisation point, iters_since_relin and damping, nothing relinearises, and a
        folded message is the one its factor computed at its last linearisation point, frozen in the prior from then on.
        Returns (var_map, factor_map): int32 arrays over the ids of before the call, the new id or -1."""
        rv, df = i32(np.asarray(retire_vars, dtype=np.int64).reshape(-1)), i32(np.asarray(drop_factors, dtype=np.int64).reshape(-1))
        vmap, fmap = np.empty(max(self.N, 1), dtype=np.int32), np.empty(max(self.F, 1), dtype=np.int32)
        d = _capi.LinShrink()
        d.n_retire_vars, d.retire_vars = rv.shape[0], iptr(rv)
        d.n_drop_factors, d.drop_factors = df.shape[0], iptr(df)
        d.fold = int(fold)
        d.var_map, d.factor_map = iptr(vmap), iptr(fmap)
        check((self._lib.gbp_lin_shrink_nonlinear if self._nonlinear else self._lib.gbp_lin_shrink)(self._h, ct.byref(d)))
        vmap, fmap = vmap[:self.N], fmap[:self.F]
        self.N, self.F = self.sizes()
        return vmap, fmap

    def retire(self, ids, fold=True):
        return self.shrink(retire_vars=ids, fold=fold)

    def cull(self, factor_ids):
        return self.shrink(drop_factors=factor_ids)

    def extend_from_factor_graph(self, graph):
        """Append graph.var_nodes[self.N:] and graph.factors[self.F:] of a host graph that was grown (with compute_factor() on the new
        factors) after from_factor_graph; the same checks.  Returns (dN, dF)."""
        if len(graph.var_nodes) < self.N or len(graph.factors) < self.F:
            raise ValueError(f"the graph holds {len(graph.var_nodes)} variables and {len(graph.factors)} factors, the handle {self.N} and {self.F}: "
                             "a device graph only grows")
        new_vars, new_facs = graph.var_nodes[self.N:], graph.factors[self.F:]
        for i, fac in enumerate(new_facs, start=self.F):                               # the device numbers factors by position
            if fac.factorID != i:
                raise ValueError(f"graph.factors[{i}] has factorID {fac.factorID}: new factors must continue the append order "
                                 "(factorID == position, ndim_posegraph.py:76-88)")
        if any(v.dofs != self.D for v in new_vars):
            raise ValueError("all variables must have the same number of dofs")
        index = {v.variableID: i for i, v in enumerate(graph.var_nodes)}
        D = self.D
        args = _host_factors(new_facs, index)
        for v in graph.var_nodes:
            ids = [f.factorID for f in v.adj_factors]
            if ids != sorted(ids):
                raise ValueError("adj_factors must be in ascending factor id (ndim_posegraph.py:86-88)")
        va, vb, fe, fl, fc, loss, thr, nvar = args
        robust = any(l is not None for l in loss)
        self.extend(va, vb, np.array(fe).reshape(-1, 2 * D), np.array(fl).reshape(-1, 2 * D, 2 * D),
                    np.array([v.prior.eta for v in new_vars]).reshape(-1, D), np.array([v.prior.lam for v in new_vars]).reshape(-1, D, D),
                    factor_const=fc, loss=loss if robust else None, threshold=thr if robust else 2.0, noise_var=nvar if robust else None)
        return len(new_vars), len(new_facs)

    def close(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            self._lib.gbp_lin_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # FactorGraph surface (gbp.py:36-58, 86-92, 146-153)
    def update_all_beliefs(self):
        check(self._lib.gbp_lin_update_beliefs(self._h))

    def synchronous_iteration(self, robustify=False, relinearise=False):
        self.iterate(1, robustify, relinearise)

    def iterate(self, n, robustify=False, relinearise=False):
        """n sweeps; robustify=True: every sweep re-makes the weights first (synchronous_iteration(robustify=True) gbp.py:86-92).
        relinearise=True (a handle of se2_pose_graph): n x synchronous_iteration(local_relin=True) -- every sweep relinearises the
        factors whose belief means left their linearisation point by more than beta, and every factor has its own damping
        (gbp.py:46-54, 64-80); returns the number of factors relinearised in each sweep, (n,) int32, counted on the device.
        Both (losses from set_robust on such a handle): n x synchronous_iteration(local_relin=True, robustify=True) -- every sweep
        first re-makes the weights at the linearisation points as they stand, then relinearises; returns (relin_counts,
        robust_counts), the second the number of factors flagged in each sweep."""
        if relinearise:
            if robustify:
                counts, flagged = np.zeros(max(int(n), 1), dtype=np.int32), np.zeros(max(int(n), 1), dtype=np.int32)
                check(self._lib.gbp_lin_iterate_nonlinear_robust(self._h, int(n), iptr(counts), iptr(flagged)))
                return counts[:max(int(n), 0)], flagged[:max(int(n), 0)]
            counts = np.zeros(max(int(n), 1), dtype=np.int32)
            check(self._lib.gbp_lin_iterate_nonlinear(self._h, int(n), iptr(counts)))
            return counts[:max(int(n), 0)]
        check((self._lib.gbp_lin_iterate_robust if robustify else self._lib.gbp_lin_iterate)(self._h, int(n)))

    # nonlinear pose graphs: FactorGraph(nonlinear_factors=True) (gbp.py:30-34) for the SE(2) relative-pose factor
    @classmethod
    def se2_pose_graph(cls, var_a, var_b, measurement, sqrt_info, prior_eta, prior_lam, beta, num_undamped_iters, min_linear_iters,
                       eta_damping=0.0, device=0):
        """A planar pose graph on variables (tx, ty, theta): factor f joins var_a[f] and var_b[f] with measurement[f] (the pose of b
        in the frame of a) and sqrt_info[f] > 0 per component.  The factors are linearised on the device at the prior means
        (compute_all_factors gbp.py:60-62); iterate(n, relinearise=True) then relinearises them by the reference's local schedule
        (beta, min_linear_iters gbp.py:64-80; num_undamped_iters and eta_damping gbp.py:46-54).  Angles are never wrapped: keep
        theta continuous along the trajectory."""
        var_a = i32(var_a).reshape(-1)
        F = var_a.shape[0]
        eng = cls(var_a, var_b, np.zeros((F, 6)), np.zeros((F, 6, 6)), prior_eta, prior_lam, eta_damping=eta_damping, device=device)
        if eng.D != 3:
            raise ValueError("an SE(2) pose has 3 dofs")
        eng.set_nonlinear(measurement, sqrt_info, beta, num_undamped_iters, min_linear_iters)
        return eng

    @classmethod
    def se3_pose_graph(cls, var_a, var_b, measurement, sqrt_info, prior_eta, prior_lam, beta, num_undamped_iters, min_linear_iters,
                       eta_damping=0.0, device=0):
        """A spatial pose graph on variables (t, w) in R^6, translation then rotation vector (R = Exp(w)): factor f joins var_a[f] and
        var_b[f] with measurement[f] = (z_t, z_w), the pose of b in the frame of a with the relative rotation as a rotation vector, and
        sqrt_info[f] > 0 per component.  Everything else is se2_pose_graph's: linearised on the device at the prior means, relinearised
        by iterate(n, relinearise=True) on the reference's local schedule; losses, extend_se3, retire / cull and
        iterate_until_nonlinear work as on a planar graph, linearisation() returns (F, 12) points.
        The domain: w is never wrapped -- keep it continuous along the trajectory; |w| > pi is legal -- while relative rotations and
        z_w stay below pi in norm (a z_w at or past pi is refused).  Jr(w) loses rank at |w| = 2 pi k."""
        var_a = i32(var_a).reshape(-1)
        F = var_a.shape[0]
        eng = cls(var_a, var_b, np.zeros((F, 12)), np.zeros((F, 12, 12)), prior_eta, prior_lam, eta_damping=eta_damping, device=device)
        if eng.D != 6:
            raise ValueError("an SE(3) pose has 6 dofs")
        eng.set_nonlinear(measurement, sqrt_info, beta, num_undamped_iters, min_linear_iters, model=_capi.LIN_MODEL_SE3_BETWEEN)
        return eng

    def set_nonlinear(self, measurement, sqrt_info, beta, num_undamped_iters, min_linear_iters, model=_capi.LIN_MODEL_SE2_BETWEEN):
        """gbp_lin_set_nonlinear: measurement and sqrt_info are F x M for the model's M (3 for LIN_MODEL_SE2_BETWEEN, 6 for
        LIN_MODEL_SE3_BETWEEN, whose domain rule se3_pose_graph states); a model the library does not know is sent as it is, with
        the arrays it was given, and refused there."""
        M = _capi.LIN_MODEL_DOFS.get(int(model))
        z = np.asarray(measurement, dtype=np.float64)
        z = f64(z.reshape(self.F, M) if M else np.atleast_2d(z))
        s = f64(np.ascontiguousarray(np.broadcast_to(np.asarray(sqrt_info, dtype=np.float64), z.shape)))
        d = _capi.LinNonlinear(int(model), int(num_undamped_iters), int(min_linear_iters), 0, float(beta), dptr(z), dptr(s))
        check(self._lib.gbp_lin_set_nonlinear(self._h, ct.byref(d)))
        self._nonlinear, self._model = True, int(model)

    def extend_se2(self, var_a, var_b, measurement, sqrt_info, prior_eta=None, prior_lam=None):
        """Append dN poses (their priors: ids N .. N + dN - 1; put the odometry prediction there) and dF relative-pose factors (ids
        F .. F + dF - 1, joining any poses old or new) to an engine of se2_pose_graph, on the device.  Every old factor keeps its
        messages, linearisation point, iters_since_relin and damping; nothing relinearises.  The new factors are linearised at their
        adjacent belief means as they are after the belief update of the grown graph (a new pose's belief is its prior), with zero
        messages, iters_since_relin 1 and damping 0 (compute_factor gbp.py:267-294, 248-249).  solve_map / marginals results are dropped
        until the next solve.  `extend` stays refused on such an engine: it takes eta_f, Lambda_f, which the engine owns."""
        self._extend_nonlinear(_capi.LIN_MODEL_SE2_BETWEEN, var_a, var_b, measurement, sqrt_info, prior_eta, prior_lam)

    def extend_se3(self, var_a, var_b, measurement, sqrt_info, prior_eta=None, prior_lam=None):
        """extend_se2 for an engine of se3_pose_graph: measurement and sqrt_info are dF x 6, the priors dN x 6 and dN x 6 x 6; the
        domain rule of se3_pose_graph holds for the new measurements too."""
        self._extend_nonlinear(_capi.LIN_MODEL_SE3_BETWEEN, var_a, var_b, measurement, sqrt_info, prior_eta, prior_lam)

    def _extend_nonlinear(self, model, var_a, var_b, measurement, sqrt_info, prior_eta, prior_lam):
        if self._nonlinear and self._model != model:
            raise ValueError("extend_se2 is for an engine of se2_pose_graph, extend_se3 for one of se3_pose_graph")
        M = _capi.LIN_MODEL_DOFS[model]
        var_a, var_b = i32(var_a).reshape(-1), i32(var_b).reshape(-1)
        dF = var_a.shape[0]
        if var_b.shape[0] != dF:
            raise ValueError("var_a / var_b length mismatch")
        z = f64(np.asarray(measurement, dtype=np.float64).reshape(dF, M))
        s = f64(np.ascontiguousarray(np.broadcast_to(np.asarray(sqrt_info, dtype=np.float64), (dF, M))))
        dN, pe, pl = _new_priors(prior_eta, prior_lam, self.D)
        d = _capi.LinExtNonlinear(dN, dF, iptr(var_a), iptr(var_b), dptr(z), dptr(s), dptr(pe), dptr(pl))
        check(self._lib.gbp_lin_extend_nonlinear(self._h, ct.byref(d)))
        self.N, self.F = self.N + dN, self.F + dF

    def relinearise(self):
        """relinearise_factors (gbp.py:64-80) alone; returns the number of factors relinearised."""
        n = ct.c_int32()
        check(self._lib.gbp_lin_relinearise(self._h, ct.byref(n)))
        return n.value

    def linearisation(self):
        """(linpoint (F, 2 D) = [xa; xb] -- (F, 6), on an engine of se3_pose_graph (F, 12) --, iters_since_relin (F,) int32,
        eta_damping (F,)) of every factor (gbp.py:231, 248-249)."""
        lp, it, dm = np.zeros((max(self.F, 1), 2 * self.D)), np.zeros(max(self.F, 1), dtype=np.int32), np.zeros(max(self.F, 1))
        check(self._lib.gbp_lin_get_linearisation(self._h, dptr(lp), iptr(it), dptr(dm)))
        return lp[:self.F], it[:self.F], dm[:self.F]

    def iterate_until(self, max_iters, tol_step=0.0, tol_map=0.0, energy=False, map_distance=False, robustify=False, check_every=8):
        """Up to max_iters sweeps in one call, the loop of ndim_posegraph.py:104-108 with the decision to stop taken on the device:
        stop after the first sweep whose step max |mu_new - mu_old| <= tol_step, or whose distance from the last solve_map() <=
        tol_map (0: off; tol_map needs map_distance=True).  energy / map_distance add what energy() / map_distance() would return
        after every sweep.  The state afterwards is bit for bit that of iterate(result.iters, robustify), whatever check_every (how
        often the host looks at the device's stop word) is.  Returns an UntilResult."""
        want = (_capi.LIN_TRACE_ENERGY if energy else 0) | (_capi.LIN_TRACE_MAP if map_distance else 0)
        o = _capi.LinUntilOpts(int(max_iters), int(check_every), int(bool(robustify)), want, float(tol_step), float(tol_map))
        i = _capi.LinUntilInfo()
        trace = np.full((max(int(max_iters), 1), 3), np.nan)
        check(self._lib.gbp_lin_iterate_until(self._h, ct.byref(o), dptr(trace), ct.byref(i)))
        rows = trace[:i.iters]
        return UntilResult(i.iters, bool(i.converged), i.reason, rows[:, 0].copy(),
                           rows[:, 1].copy() if energy else None, rows[:, 2].copy() if map_distance else None)

    def iterate_until_nonlinear(self, max_iters, tol_step=0.0, tol_map=0.0, energy=False, map_distance=False, robustify=False, settled=False,
                                check_every=8):
        """iterate_until for an engine of se2_pose_graph: up to max_iters sweeps of iterate(1, relinearise=True) (robustify=True: of
        iterate(1, robustify=True, relinearise=True)) in one call, the stop decided on the device by the rule of iterate_until.
        energy / map_distance add what energy() / map_distance() would return after every sweep -- the distance is from the last
        solve_map(), one Gauss-Newton step, wherever the linearisation has moved since.  settled=True: a sweep in which any factor
        relinearised decides nothing, so a graph that relinearises in every sweep runs out max_iters.  The state afterwards is bit for
        bit that of iterate(result.iters, robustify, relinearise=True), whatever check_every is.  Returns an UntilResult with
        relin_counts (and, with robustify, robust_counts) per sweep run."""
        want = (_capi.LIN_TRACE_ENERGY if energy else 0) | (_capi.LIN_TRACE_MAP if map_distance else 0) | (_capi.LIN_UNTIL_SETTLED if settled else 0)
        o = _capi.LinUntilOpts(int(max_iters), int(check_every), int(bool(robustify)), want, float(tol_step), float(tol_map))
        i = _capi.LinUntilInfo()
        n = max(int(max_iters), 1)
        trace, counts, flagged = np.full((n, 3), np.nan), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        check(self._lib.gbp_lin_iterate_until_nonlinear(self._h, ct.byref(o), dptr(trace), iptr(counts), iptr(flagged) if robustify else None, ct.byref(i)))
        rows = trace[:i.iters]
        return UntilResult(i.iters, bool(i.converged), i.reason, rows[:, 0].copy(), rows[:, 1].copy() if energy else None,
                           rows[:, 2].copy() if map_distance else None, relin_counts=counts[:i.iters].copy(),
                           robust_counts=flagged[:i.iters].copy() if robustify else None)

    def alloc_count(self):
        """The number of device allocations the handle owns (graph arrays and workspaces)."""
        n = ct.c_int32()
        check(self._lib.gbp_lin_get_alloc_count(self._h, ct.byref(n)))
        return n.value

    # robust losses (Factor(loss=, mahalanobis_threshold=), Factor.robustify_loss gbp.py:296-332): one weight per factor
    def set_robust(self, loss, threshold=2.0, noise_var=None, first=0):
        """Per-factor losses: None, 'huber' or 'constant' (a scalar or F of them), Mahalanobis threshold(s), and -- for the constant
        loss -- the factors' noise variance(s).  loss=None clears every loss: the handle is back on the plain path.  Resets the weights
        to 1; they are re-made from the current belief means by robustify_all_factors() / iterate(n, robustify=True).
        On an engine of se2_pose_graph the losses are those of factors first, first + 1, ... (a list: that many; one name: every
        factor from `first` on), whose weights are reset while every other factor keeps loss, threshold and weight; the weights are
        re-made at the LINEARISATION POINTS (gbp.py:309) by robustify_all_factors() / iterate(n, robustify=True, relinearise=True);
        the whitened model needs no noise_var."""
        if self._nonlinear:
            if loss is None:
                check(self._lib.gbp_lin_set_robust_nonlinear(self._h, 0, self.F, None, None))
                return
            count = self.F - int(first) if isinstance(loss, str) else len(list(loss))
            codes, thr, _ = _loss_arrays(loss, threshold, None, max(count, 0))
            check(self._lib.gbp_lin_set_robust_nonlinear(self._h, int(first), count, iptr(codes), dptr(thr)))
            return
        if first:
            raise ValueError("a range of losses (first != 0) is for an engine of se2_pose_graph")
        if loss is None:
            check(self._lib.gbp_lin_set_robust(self._h, None, None, None))
            return
        codes, thr, nv = _loss_arrays(loss, threshold, noise_var, self.F)   # F = 0: still a non-NULL `loss`, which NULL would read as "clear"
        check(self._lib.gbp_lin_set_robust(self._h, iptr(codes), dptr(thr), dptr(nv)))

    def robustify_all_factors(self):
        check((self._lib.gbp_lin_robustify_nonlinear if self._nonlinear else self._lib.gbp_lin_robustify)(self._h))

    def weights(self):
        """(w (F,), robust_flag (F,) bool): sigma^2 / adaptive_gauss_noise_var and Factor.robust_flag of every factor."""
        w, flag = np.ones(max(self.F, 1)), np.zeros(max(self.F, 1), dtype=np.int32)
        check(self._lib.gbp_lin_get_weights(self._h, dptr(w), iptr(flag)))
        return w[:self.F], flag[:self.F].astype(bool)

    def energy(self):
        out = ct.c_double()
        check(self._lib.gbp_lin_energy(self._h, ct.byref(out)))
        return out.value

    def get_means(self):
        mu = np.empty((self.N, self.D))
        check(self._lib.gbp_lin_get_means(self._h, dptr(mu)))
        return mu.reshape(-1)

    def beliefs(self):
        eta, lam = np.empty((self.N, self.D)), np.empty((self.N, self.D, self.D))
        check(self._lib.gbp_lin_get_beliefs(self._h, dptr(eta), dptr(lam)))
        return eta, lam

    def messages(self):
        ea, la = np.empty((self.F, self.D)), np.empty((self.F, self.D, self.D))
        eb, lb = np.empty((self.F, self.D)), np.empty((self.F, self.D, self.D))
        check(self._lib.gbp_lin_get_messages(self._h, dptr(ea), dptr(la), dptr(eb), dptr(lb)))
        return ea, la, eb, lb

    # the batch MAP (FactorGraph.joint_distribution_inf / _cov gbp.py:94-144), by block-Jacobi conjugate gradients on the device
    def joint_matvec(self, x):
        """Lambda_joint @ x for x of N x d (any shape of that size); returns (N, d)."""
        x = f64(np.asarray(x, dtype=np.float64).reshape(self.N, self.D))
        y = np.empty((self.N, self.D))
        check(self._lib.gbp_lin_joint_matvec(self._h, dptr(x), dptr(y)))
        return y

    def joint_eta(self):
        eta = np.empty((self.N, self.D))
        check(self._lib.gbp_lin_joint_eta(self._h, dptr(eta)))
        return eta

    def solve_map(self, rel_tol=1e-12, max_iters=10000, check_every=8, warm_start=False):
        """The batch MAP Lambda_joint^-1 eta_joint: (mu (N, d), info).  info: iters, converged, rel_residual (of the true residual),
        eta_norm.  warm_start: from the current belief means instead of 0.  Running out of max_iters is not an error."""
        o = _capi.LinMapOpts(float(rel_tol), int(max_iters), int(check_every), int(bool(warm_start)))
        i = _capi.LinMapInfo()
        check(self._lib.gbp_lin_solve_map(self._h, ct.byref(o), ct.byref(i)))
        return self.map_mean(), {'iters': i.iters, 'converged': bool(i.converged), 'rel_residual': i.rel_residual, 'eta_norm': i.eta_norm}

    def solve_map_nonlinear(self, max_outer=50, init='means', lambda0=1e-4, lambda_up=10.0, lambda_down=0.1, lambda_min=1e-12, lambda_max=1e8,
                            tol_step=1e-10, tol_grad=1e-8, rel_tol=1e-12, max_iters=10000, check_every=8):
        """The nonlinear batch MAP of an engine of se2_pose_graph / se3_pose_graph by Levenberg-Marquardt on the device
        (gbp_lin_solve_map_nonlinear): the minimiser of sum_f w_f 0.5 |h_f(x) - diag(s_f) z_f|^2 + the priors, at the weights as
        they stand, started at the belief means (init='means') or at the iterate of the last solve_map() / solve_map_nonlinear()
        (init='map').  rel_tol, max_iters, check_every are those of the inner conjugate-gradient solves.  The sweep's state is left
        bit for bit as it was; the result lands where solve_map() leaves its own, so map_mean(), map_distance() and
        iterate_until_nonlinear(map_distance=True) then measure against the nonlinear MAP.  Returns a NonlinearMapResult."""
        if init not in ('means', 'map'):
            raise ValueError("init is 'means' or 'map'")
        o = _capi.LinNlmapOpts(int(max_outer), _capi.LIN_NLMAP_FROM_MAP if init == 'map' else _capi.LIN_NLMAP_FROM_MEANS, float(lambda0), float(lambda_up),
                               float(lambda_down), float(lambda_min), float(lambda_max), float(tol_step), float(tol_grad),
                               _capi.LinMapOpts(float(rel_tol), int(max_iters), int(check_every), 0))
        i = _capi.LinNlmapInfo()
        trace = np.full((max(int(max_outer), 1), 5), np.nan)
        check(self._lib.gbp_lin_solve_map_nonlinear(self._h, ct.byref(o), dptr(trace), ct.byref(i)))
        return NonlinearMapResult(i, trace)

    def solve_map_nonlinear_robust(self, max_rounds=20, tol_weight=1e-9, tol_move=1e-10, max_outer=50, init='means', lambda0=1e-4, lambda_up=10.0,
                                   lambda_down=0.1, lambda_min=1e-12, lambda_max=1e8, tol_step=1e-10, tol_grad=1e-8, rel_tol=1e-12, max_iters=10000,
                                   check_every=8):
        """The robust nonlinear batch MAP (gbp_lin_solve_map_nonlinear_robust): rounds of "make the weights of set_robust()'s losses at
        x, minimise at those weights by solve_map_nonlinear's Levenberg-Marquardt loop" until the weights (tol_weight) or x (tol_move)
        stop changing -- the fixed point robust relinearising GBP converges to, independent of any sweep.  The options after tol_move
        are solve_map_nonlinear's, used by every round; init names the start of the first.  Neither the sweep's state nor the engine's
        own weights() are written.  Returns a RobustNonlinearMapResult; the final x is map_mean()."""
        if init not in ('means', 'map'):
            raise ValueError("init is 'means' or 'map'")
        lm = _capi.LinNlmapOpts(int(max_outer), _capi.LIN_NLMAP_FROM_MAP if init == 'map' else _capi.LIN_NLMAP_FROM_MEANS, float(lambda0), float(lambda_up),
                                float(lambda_down), float(lambda_min), float(lambda_max), float(tol_step), float(tol_grad),
                                _capi.LinMapOpts(float(rel_tol), int(max_iters), int(check_every), 0))
        o = _capi.LinIrlsOpts(int(max_rounds), 0, float(tol_weight), float(tol_move), lm)
        i = _capi.LinIrlsInfo()
        rounds, outer = max(int(max_rounds), 0), max(int(max_outer), 0)
        rt, lt = np.full((rounds + 1, 6), np.nan), np.full((max(rounds * outer, 1), 5), np.nan)
        w, flag = np.ones(self.F), np.zeros(self.F, dtype=np.int32)
        check(self._lib.gbp_lin_solve_map_nonlinear_robust(self._h, ct.byref(o), dptr(rt), dptr(lt), dptr(w), iptr(flag), ct.byref(i)))
        return RobustNonlinearMapResult(i, rt, lt, w, flag)

    def map_mean(self):
        mu = np.empty((self.N, self.D))
        check(self._lib.gbp_lin_get_map(self._h, dptr(mu)))
        return mu

    def map_distance(self):
        """|get_means() - map_mean()|_2 computed on the device: the 'Av distance of means from MAP' of ndim_posegraph.py:108."""
        out = ct.c_double()
        check(self._lib.gbp_lin_map_distance(self._h, ct.byref(out)))
        return out.value

    # exact marginal covariances (the sigma of joint_distribution_cov gbp.py:128-144), by the same iteration on 8 columns at a time
    def marginals(self, ids=None, rel_tol=1e-12, max_iters=10000, check_every=8, joint=False):
        """Blocks of Lambda_joint^-1: (sigma (M, d, d), info), sigma[i] the marginal covariance of variable ids[i] (None: all
        variables); with joint=True (sigma, sigma_joint (M d, M d), info), sigma_joint the inverse restricted to ids x ids.  Neither is
        symmetrised.  info: iters (summed over the batches of 8 columns), converged, batches, rel_residual (the worst column's true
        residual).  max_iters is per batch; running out of it is not an error."""
        if ids is None:
            ids = np.arange(self.N, dtype=np.int32)
        else:
            wide = np.asarray(ids, dtype=np.int64).reshape(-1)
            if wide.size and (wide.min() < -2 ** 31 or wide.max() >= 2 ** 31):
                raise ValueError("variable ids must fit int32")   # before the cast below can wrap them into range
            ids = i32(wide)
        M = ids.shape[0]
        sigma = np.zeros((M, self.D, self.D))
        sj = np.zeros((M * self.D, M * self.D)) if joint else None
        o = _capi.LinMapOpts(float(rel_tol), int(max_iters), int(check_every), 0)
        i = _capi.LinMargInfo()
        check(self._lib.gbp_lin_solve_marginals(self._h, iptr(ids), M, ct.byref(o), dptr(sigma), dptr(sj), ct.byref(i)))
        info = {'iters': i.iters, 'converged': bool(i.converged), 'batches': i.batches, 'rel_residual': i.rel_residual}
        return (sigma, sj, info) if joint else (sigma, info)

    def belief_covariances(self):
        """(N, d, d): the inverses of the belief Lambdas of beliefs(), taken on the host -- what GBP holds for marginals()."""
        _, lam = self.beliefs()
        return np.linalg.inv(lam) if self.N else lam

    def sync(self):
        check(self._lib.gbp_lin_sync(self._h))
