"""CPU oracle of the LINEAR pairwise GBP path (TEST INFRASTRUCTURE ONLY -- imported by tests/, never by gbp_amd/).

Dense numpy restatement of what joeaortiz/gbp does for a FactorGraph(nonlinear_factors=False) of two-variable
factors (ndim_posegraph.py): no packing, no elimination tricks, np.linalg.inv exactly where the reference has it.
Pinned by tests/test_linear_oracle.py against fixture G8 (the reference's own ndim_posegraph.py run).

  compute_messages   gbp/gbp.py:334-373     update_belief   gbp/gbp.py:176-198     energy   gbp/gbp.py:36-44, 251-265
  synchronous_iteration (linear graph: no robustify, no relinearisation, graph damping)   gbp/gbp.py:46-58, 86-92
"""
import numpy as np


class LinearOracle:
    def __init__(self, var_a, var_b, factor_eta, factor_lam, prior_eta, prior_lam, factor_const=None, eta_damping=0.0):
        self.va, self.vb = np.asarray(var_a, dtype=int), np.asarray(var_b, dtype=int)
        self.fe, self.fl = np.asarray(factor_eta, dtype=float), np.asarray(factor_lam, dtype=float)
        self.pe, self.pl = np.asarray(prior_eta, dtype=float), np.asarray(prior_lam, dtype=float)
        self.N, self.D = self.pe.shape
        self.F = self.va.shape[0]
        self.fc = np.zeros(self.F) if factor_const is None else np.asarray(factor_const, dtype=float)
        self.damping = float(eta_damping)
        D = self.D
        self.msg_eta = np.zeros((self.F, 2, D))            # Factor.messages[k].eta / .lam, zero at construction (gbp.py:222)
        self.msg_lam = np.zeros((self.F, 2, D, D))
        self.bel_eta, self.bel_lam, self.mu = np.zeros((self.N, D)), np.zeros((self.N, D, D)), np.zeros((self.N, D))
        self.adj = [[] for _ in range(self.N)]             # (factor, side) in ascending factor id = append order
        for f in range(self.F):
            self.adj[self.va[f]].append((f, 0))
            self.adj[self.vb[f]].append((f, 1))

    def update_all_beliefs(self):                          # gbp.py:56-58 -> 176-198
        for v in range(self.N):
            eta, lam = self.pe[v].copy(), self.pl[v].copy()
            for f, side in self.adj[v]:
                eta = eta + self.msg_eta[f, side]
                lam = lam + self.msg_lam[f, side]
            self.bel_eta[v], self.bel_lam[v] = eta, lam
            self.mu[v] = np.linalg.inv(lam) @ eta

    def compute_all_messages(self):                        # gbp.py:46-54 (graph-level damping), 334-373
        D = self.D
        new_eta, new_lam = np.empty_like(self.msg_eta), np.empty_like(self.msg_lam)
        for f in range(self.F):
            vs = (self.va[f], self.vb[f])
            for out in (0, 1):
                oth = 1 - out
                eta, lam = self.fe[f].copy(), self.fl[f].copy()
                s = slice(oth * D, (oth + 1) * D)
                eta[s] += self.bel_eta[vs[oth]] - self.msg_eta[f, oth]
                lam[s, s] += self.bel_lam[vs[oth]] - self.msg_lam[f, oth]
                o = slice(out * D, (out + 1) * D)
                gain = lam[o, s] @ np.linalg.inv(lam[s, s])
                new_lam[f, out] = lam[o, o] - gain @ lam[s, o]
                new_eta[f, out] = (1 - self.damping) * (eta[o] - gain @ eta[s]) + self.damping * self.msg_eta[f, out]
        self.msg_eta, self.msg_lam = new_eta, new_lam

    def synchronous_iteration(self):                       # gbp.py:86-92
        self.compute_all_messages()
        self.update_all_beliefs()

    def iterate(self, n):
        for _ in range(n):
            self.synchronous_iteration()

    def energy(self):                                      # 0.5 |h(mu) - z|^2 / sigma^2 written through (eta_f, Lambda_f, const)
        e = 0.0
        for f in range(self.F):
            x = np.concatenate([self.mu[self.va[f]], self.mu[self.vb[f]]])
            e += 0.5 * x @ self.fl[f] @ x - self.fe[f] @ x + self.fc[f]
        return e

    def get_means(self):
        return self.mu.reshape(-1).copy()

    def beliefs(self):
        return self.bel_eta.copy(), self.bel_lam.copy()

    def messages(self):
        return self.msg_eta[:, 0].copy(), self.msg_lam[:, 0].copy(), self.msg_eta[:, 1].copy(), self.msg_lam[:, 1].copy()


def toy_posegraph(n=100, dim=3, M=10, std=1.0, seed=0):
    """The graph of ndim_posegraph.py:36-64 as arrays: (var_a, var_b, factor_eta, factor_lam, factor_const, prior_eta, prior_lam).
    Factor = linear_displacement (gbp/factors/linear_displacement.py:8-14): h(x) = x_b - x_a, J = [-I, I]."""
    rs = np.random.RandomState(seed)
    priors_mu = rs.rand(n, dim) * 10
    prior_lam = np.linalg.inv(3 * np.eye(dim))
    pairs, meas = [], []
    for i, mu in enumerate(priors_mu):
        d = np.array([np.linalg.norm(mu - m1) for m1 in priors_mu])
        for j in d.argsort()[1:M + 1]:
            if [j, i] not in pairs:
                meas.append(mu - priors_mu[j] + rs.normal(0., std, dim))
                pairs.append([i, j])
    J = np.hstack([-np.eye(dim), np.eye(dim)])
    fe = np.array([J.T @ z / std ** 2 for z in meas])
    fl = np.array([J.T @ J / std ** 2 for _ in meas])
    fc = np.array([0.5 * z @ z / std ** 2 for z in meas])
    pairs = np.array(pairs)
    return (pairs[:, 0], pairs[:, 1], fe, fl, fc, priors_mu @ prior_lam.T, np.tile(prior_lam, (n, 1, 1)))


class LinearOracleBatched(LinearOracle):
    """`LinearOracle` vectorised over factors, for graphs of a million factors (tests/test_linear_edges_gpu.py).

    The same float64 operations on the same operands: the Schur step takes a stacked np.linalg.inv of the eliminated
    block and forms gain = Lambda_os inv(Lambda_ss) exactly as compute_all_messages does, and a belief adds the prior
    first, then its messages in ascending factor id, one adjacency slot at a time over the variables that have a k-th
    neighbour (not np.add.at, whose order is unspecified).  Pinned to LinearOracle by tests/test_linear_oracle.py."""

    def __init__(self, var_a, var_b, factor_eta, factor_lam, prior_eta, prior_lam, factor_const=None, eta_damping=0.0):
        self.va, self.vb = np.asarray(var_a, dtype=np.int64).reshape(-1), np.asarray(var_b, dtype=np.int64).reshape(-1)
        self.pe, self.pl = np.asarray(prior_eta, dtype=float), np.asarray(prior_lam, dtype=float)
        self.N, self.D = self.pe.shape
        self.F = self.va.shape[0]
        D = self.D
        self.fe = np.asarray(factor_eta, dtype=float).reshape(self.F, 2 * D)
        self.fl = np.asarray(factor_lam, dtype=float).reshape(self.F, 2 * D, 2 * D)
        self.fc = np.zeros(self.F) if factor_const is None else np.asarray(factor_const, dtype=float).reshape(self.F)
        self.damping = float(eta_damping)
        self.msg_eta = np.zeros((self.F, 2, D))
        self.msg_lam = np.zeros((self.F, 2, D, D))
        self.bel_eta, self.bel_lam, self.mu = np.zeros((self.N, D)), np.zeros((self.N, D, D)), np.zeros((self.N, D))
        # adjacency as CSR over (factor, side) edges, ascending factor id per variable
        var = np.concatenate([self.va, self.vb])
        fac = np.concatenate([np.arange(self.F), np.arange(self.F)])
        side = np.concatenate([np.zeros(self.F, dtype=np.int64), np.ones(self.F, dtype=np.int64)])
        order = np.lexsort((fac, var))
        self.adj_f, self.adj_s = fac[order], side[order]
        self.deg = np.bincount(var, minlength=self.N)
        self.vptr = np.concatenate([[0], np.cumsum(self.deg)])
        # slot k: the variables with a k-th neighbour and the CSR index of that neighbour
        self.slots = []
        for k in range(int(self.deg.max()) if self.N else 0):
            vs = np.nonzero(self.deg > k)[0]
            self.slots.append((vs, self.vptr[vs] + k))

    def update_all_beliefs(self):
        eta, lam = self.pe.copy(), self.pl.copy()
        for vs, e in self.slots:
            eta[vs] = eta[vs] + self.msg_eta[self.adj_f[e], self.adj_s[e]]
            lam[vs] = lam[vs] + self.msg_lam[self.adj_f[e], self.adj_s[e]]
        self.bel_eta, self.bel_lam = eta, lam
        self.mu = (np.linalg.inv(lam) @ eta[..., None])[..., 0] if self.N else np.zeros((0, self.D))

    def compute_all_messages(self):
        D = self.D
        new_eta, new_lam = np.empty_like(self.msg_eta), np.empty_like(self.msg_lam)
        vs = (self.va, self.vb)
        for out in (0, 1):
            oth = 1 - out
            s = slice(oth * D, (oth + 1) * D)
            o = slice(out * D, (out + 1) * D)
            eta_s = self.fe[:, s] + (self.bel_eta[vs[oth]] - self.msg_eta[:, oth])
            lam_ss = self.fl[:, s, s] + (self.bel_lam[vs[oth]] - self.msg_lam[:, oth])
            gain = self.fl[:, o, s] @ np.linalg.inv(lam_ss)
            new_lam[:, out] = self.fl[:, o, o] - gain @ self.fl[:, s, o]
            new_eta[:, out] = ((1 - self.damping) * (self.fe[:, o] - (gain @ eta_s[..., None])[..., 0])
                               + self.damping * self.msg_eta[:, out])
        self.msg_eta, self.msg_lam = new_eta, new_lam

    def energy(self):
        x = np.concatenate([self.mu[self.va], self.mu[self.vb]], axis=1)
        return float(np.sum(0.5 * np.einsum('fi,fij,fj->f', x, self.fl, x) - np.einsum('fi,fi->f', self.fe, x) + self.fc))


def residual_energy(mu, var_a, var_b, J, z, sigma):
    """The reference's energy sum_f 0.5 |J_f [mu_a; mu_b] - z_f|^2 / sigma_f^2 (gbp.py:251-265), evaluated EXACTLY
    (fractions.Fraction) from the float64 means and the float64 (J, z, sigma) the graph was built from; rounded once.
    J: (m, 2d) shared or (F, m, 2d); z: (F, m); sigma: scalar or (F,)."""
    from fractions import Fraction
    va, vb = np.asarray(var_a, dtype=np.int64).reshape(-1), np.asarray(var_b, dtype=np.int64).reshape(-1)
    F = va.shape[0]
    z = np.asarray(z, dtype=float).reshape(F, -1)
    J = np.asarray(J, dtype=float)
    J = np.broadcast_to(J, (F,) + J.shape[-2:])
    d = J.shape[-1] // 2
    mu = np.asarray(mu, dtype=float).reshape(-1, d)
    sig = np.broadcast_to(np.asarray(sigma, dtype=float), (F,))
    total = Fraction(0)
    for f in range(F):
        x = [Fraction(float(v)) for v in np.concatenate([mu[va[f]], mu[vb[f]]])]
        r2 = Fraction(0)
        for i in range(J.shape[1]):
            r = -Fraction(float(z[f, i]))
            for j in range(2 * d):
                if J[f, i, j] != 0.0:
                    r += Fraction(float(J[f, i, j])) * x[j]
            r2 += r * r
        total += r2 / (2 * Fraction(float(sig[f])) ** 2)
    return float(total)


def displacement_graph(va, vb, x_true, sigma, rs, prior_sigma=3.0):
    """linear_displacement factors (h = x_b - x_a, J = [-I, I]) measured from `x_true` with noise `sigma`, and the
    priors of ndim_posegraph.py (prior_sigma around the true positions).  Returns (J, z, factor_eta, factor_lam,
    factor_const, prior_eta, prior_lam) in the layout LinearEngine / LinearOracle take."""
    va, vb = np.asarray(va), np.asarray(vb)
    N, D = x_true.shape
    z = x_true[vb] - x_true[va] + rs.normal(0.0, sigma, (va.shape[0], D))
    J = np.hstack([-np.eye(D), np.eye(D)])
    fe = (z @ J) / sigma ** 2
    fl = np.ascontiguousarray(np.broadcast_to(J.T @ J / sigma ** 2, (va.shape[0], 2 * D, 2 * D)))
    fc = 0.5 * np.einsum('fd,fd->f', z, z) / sigma ** 2
    pl = np.eye(D) / prior_sigma ** 2
    return J, z, fe, fl, fc, x_true @ pl.T, np.ascontiguousarray(np.broadcast_to(pl, (N, D, D)))
