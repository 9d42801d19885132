"""Shared by tests/test_linear_robust_cpu.py and tests/test_linear_robust_gpu.py: a numpy oracle of the linear engine's robust losses
(Factor.robustify_loss gbp.py:296-332 taken at the current belief means, include/gbp_lin.h), the graphs it is checked on, the G22
graphs rebuilt from the stored measurements, and the engine's device layout for the host shim."""
import numpy as np

from lin_map_cases import pack, random_pairs, random_priors, star
from oracle.linear_oracle import LinearOracleBatched, toy_posegraph

TOL = 1e-9
LOSSES = (None, 'huber', 'constant')
LOSS_CODE = {None: 0, 'huber': 1, 'constant': 2}


def robust_weight(loss, t, sigma2, M):
    """(w, flag) of one factor from its Mahalanobis distance: w = sigma^2 / adaptive_gauss_noise_var (gbp.py:311-328)."""
    if loss is None or not M > t:
        return 1.0, False
    if loss == 'huber':
        return sigma2 / (sigma2 * M ** 2 / (2 * (t * M - 0.5 * t ** 2))), True
    return sigma2 / M ** 2, True


class RobustOracle(LinearOracleBatched):
    """LinearOracle(Batched) with per-factor losses.  M comes from (J, z, sigma) directly -- |J x - z| / sigma at the current belief
    means, never through (eta_f, Lambda_f) -- and the nominal factor (fe0, fl0) is scaled by w_f before every sweep that robustifies.
    J: (F, m, 2d); z: (F, m); sigma: (F,); loss: F names; threshold: (F,)."""

    def __init__(self, va, vb, J, z, sigma, prior_eta, prior_lam, loss, threshold, eta_damping=0.0):
        self.J, self.z = np.asarray(J, dtype=float), np.asarray(z, dtype=float)
        F = self.J.shape[0]
        self.sigma = np.broadcast_to(np.asarray(sigma, dtype=float), (F,)).copy()
        s2 = self.sigma ** 2
        self.fe0 = np.einsum('fmi,fm->fi', self.J, self.z) / s2[:, None]
        self.fl0 = np.einsum('fmi,fmj->fij', self.J, self.J) / s2[:, None, None]
        self.fc0 = 0.5 * np.einsum('fm,fm->f', self.z, self.z) / s2
        super().__init__(va, vb, self.fe0, self.fl0, prior_eta, prior_lam, factor_const=self.fc0, eta_damping=eta_damping)
        self.loss = [loss] * F if (loss is None or isinstance(loss, str)) else list(loss)
        self.thr = np.broadcast_to(np.asarray(threshold, dtype=float), (F,)).copy()
        self.w, self.flag = np.ones(F), np.zeros(F, dtype=bool)

    def mahalanobis(self):
        x = np.concatenate([self.mu[self.va], self.mu[self.vb]], axis=1)
        r = np.einsum('fmi,fi->fm', self.J, x) - self.z
        return np.sqrt(np.einsum('fm,fm->f', r, r)) / self.sigma

    def robustify_all_factors(self):
        M = self.mahalanobis()
        for f in range(self.F):
            self.w[f], self.flag[f] = robust_weight(self.loss[f], self.thr[f], self.sigma[f] ** 2, M[f])
        self.fe, self.fl = self.fe0 * self.w[:, None], self.fl0 * self.w[:, None, None]

    def synchronous_iteration(self, robustify=False):
        if robustify:
            self.robustify_all_factors()
        super().synchronous_iteration()

    def iterate(self, n, robustify=False):
        for _ in range(n):
            self.synchronous_iteration(robustify)

    def energy(self):                                      # sum_f w_f 0.5 |J x - z|^2 / sigma^2 (gbp.py:43)
        return float(np.sum(self.w * 0.5 * self.mahalanobis() ** 2))


def generic_jz(rs, D, F, rows=None, outliers=0.3):
    """Random J (rows x 2d, d + 1 rows by default: rank-deficient Lambda_f for d > 1), z, sigma; a share of the z far out, so that
    factors land on both sides of the threshold."""
    rows = D + 1 if rows is None else rows
    J = rs.randn(F, rows, 2 * D)
    z = rs.randn(F, rows)
    far = rs.rand(F) < outliers
    z[far] += 8.0 * rs.randn(int(far.sum()), rows)
    return J, z, 0.5 + rs.rand(F)


def mixed_losses(rs, F):
    return [LOSSES[i] for i in rs.randint(0, 3, F)]


def shapes(D):
    """(name, N, va, vb, J, z, sigma, prior_eta, prior_lam, loss, threshold) for every shape the robust sweep is checked on."""
    rs = np.random.RandomState(2200 + D)
    out = []

    def add(name, N, va, vb, rows=None, loss=None):
        va, vb = np.asarray(va, dtype=np.int64), np.asarray(vb, dtype=np.int64)
        F = va.shape[0]
        J, z, sigma = generic_jz(rs, D, F, rows)
        pe, pl = random_priors(rs, N, D)
        out.append((name, N, va, vb, J, z, sigma, pe, pl, mixed_losses(rs, F) if loss is None else loss, 1.0 + 2.0 * rs.rand(F)))
    for F in (1, 63, 64, 65, 129):                          # wave tails of the factor stage, one and several blocks
        N = 2 + F // 3
        add(f'f{F}', N, *random_pairs(rs, N, F))
    N, va, vb = star(rs)                                    # a hub of degree 203 beside an isolated variable
    add('star', N, va, vb)
    add('twice', 3, [0, 0, 1], [1, 1, 2], loss=['huber', 'constant', None])   # one pair joined twice with different losses
    add('rank1', 20, *random_pairs(rs, 20, 45), rows=1)     # J with one row, under SPD priors
    return out


def g22_graph(golden, tag, loss):
    """The G22 graph of (tag, loss) as RobustOracle arguments, from toy_posegraph's structure and the stored measurements."""
    n, dim = (100, 3) if tag == 'n100d3' else (50, 6)
    va, vb, _, _, _, pe, pl = toy_posegraph(n, dim, 10, 1.0, seed=0)
    z = golden[f'{tag}_{loss}_meas']
    assert z.shape == (len(va), dim)
    J = np.broadcast_to(np.hstack([-np.eye(dim), np.eye(dim)]), (len(va), dim, 2 * dim)).copy()
    return va, vb, J, z, 1.0, pe, pl


def engine_args(o):
    """LinearEngine's constructor arguments and set_robust's, from a RobustOracle."""
    return (o.va, o.vb, o.fe0, o.fl0, o.pe, o.pl), dict(factor_const=o.fc0, eta_damping=o.damping), (o.loss, o.thr, o.sigma ** 2)


def dense_weighted_joint(o, w):
    from lin_map_cases import dense_joint
    return dense_joint(o.va, o.vb, o.fe0 * w[:, None], o.fl0 * w[:, None, None], o.pe, o.pl)


def pack_robust(o):
    """lin_map_cases.pack plus what the robust shim reads: constants, belief records [N][d + P + d] with the oracle's means, losses."""
    d = pack(o.va, o.vb, o.fe0, o.fl0, o.pe, o.pl)
    D, N = o.D, o.N
    P = D * (D + 1) // 2
    bel = np.zeros((N, D + P + D))
    bel[:, D + P:] = o.mu
    d.update(fconst=np.ascontiguousarray(o.fc0), bel=bel, loss=np.array([LOSS_CODE[l] for l in o.loss], dtype=np.int32),
             thr=np.ascontiguousarray(o.thr), nvar=np.ascontiguousarray(o.sigma ** 2))
    return d
