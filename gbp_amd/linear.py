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
        va, vb, fe, fl, fc, loss, thr, nvar = [], [], [], [], [], [], [], []
        for fac in graph.factors:
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

    def synchronous_iteration(self, robustify=False):
        self.iterate(1, robustify)

    def iterate(self, n, robustify=False):
        """n sweeps; robustify=True: every sweep re-makes the weights first (synchronous_iteration(robustify=True) gbp.py:86-92)."""
        check((self._lib.gbp_lin_iterate_robust if robustify else self._lib.gbp_lin_iterate)(self._h, int(n)))

    # robust losses (Factor(loss=, mahalanobis_threshold=), Factor.robustify_loss gbp.py:296-332): one weight per factor
    def set_robust(self, loss, threshold=2.0, noise_var=None):
        """Per-factor losses: None, 'huber' or 'constant' (a scalar or F of them), Mahalanobis threshold(s), and -- for the constant
        loss -- the factors' noise variance(s).  loss=None clears every loss: the handle is back on the plain path.  Resets the weights
        to 1; they are re-made from the current belief means by robustify_all_factors() / iterate(n, robustify=True)."""
        if loss is None:
            check(self._lib.gbp_lin_set_robust(self._h, None, None, None))
            return
        names = [loss] * self.F if isinstance(loss, str) else list(loss)
        if len(names) != self.F:
            raise ValueError(f"expected {self.F} losses, got {len(names)}")
        bad = [l for l in names if l not in _capi.LIN_LOSS]
        if bad:
            raise ValueError(f"unknown loss {bad[0]!r}: None, 'huber' or 'constant'")
        n = max(self.F, 1)                                   # F = 0: still a non-NULL `loss`, which NULL would read as "clear"
        codes = np.zeros(n, dtype=np.int32)
        codes[:self.F] = [_capi.LIN_LOSS[l] for l in names]
        thr = np.ones(n)
        thr[:self.F] = np.broadcast_to(np.asarray(threshold, dtype=np.float64), (self.F,))
        nv = None
        if noise_var is not None:
            nv = np.ones(n)
            nv[:self.F] = np.broadcast_to(np.asarray(noise_var, dtype=np.float64), (self.F,))
        check(self._lib.gbp_lin_set_robust(self._h, iptr(codes), dptr(thr), dptr(nv)))

    def robustify_all_factors(self):
        check(self._lib.gbp_lin_robustify(self._h))

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
