"""What the nonlinear tests of the linear engine share (test_linear_nonlinear_cpu.py, test_linear_nonlinear_gpu.py): a vectorised numpy
twin, in fp64 and the formulas of include/gbp_lin.h, of the three stages of gbp_lin_iterate_nonlinear -- relinearise (gbp.py:64-80),
factor with per-factor damping (gbp.py:46-54, 334-373), belief (gbp.py:176-198) -- for the SE(2) relative-pose factor; the graph
builders; and the seeded cases the GPU tests run, whose distance from the relinearisation threshold the CPU test checks.
The twin is pinned to the reference's own run by fixture G25 (tests/golden/make_g25.py) in test_linear_nonlinear_cpu.py."""
import numpy as np

TOL = 1e-9                      # GPU against the twin: as tests/test_linear_gpu.py against oracle/linear_oracle.py
PARITY = 1e-4                   # the project's parity contract against the reference (README)
SQRT_INFO = np.array([10.0, 10.0, 20.0])


def se2_h(x, s):
    """x (F, 6) = [xa; xb], s (F, 3) -> diag(s) h (F, 3)."""
    c, sn = np.cos(x[:, 2]), np.sin(x[:, 2])
    dx, dy = x[:, 3] - x[:, 0], x[:, 4] - x[:, 1]
    return s * np.stack([c * dx + sn * dy, -sn * dx + c * dy, x[:, 5] - x[:, 2]], 1)


def se2_jac(x, s):
    c, sn = np.cos(x[:, 2]), np.sin(x[:, 2])
    dx, dy = x[:, 3] - x[:, 0], x[:, 4] - x[:, 1]
    o, l = np.zeros_like(c), np.ones_like(c)
    J = np.stack([np.stack([-c, -sn, -sn * dx + c * dy, c, sn, o], 1),
                  np.stack([sn, -c, -c * dx - sn * dy, -sn, c, o], 1),
                  np.stack([o, o, -l, o, o, l], 1)], 1)
    return s[:, :, None] * J


def se2_b(J, x0, z, s):
    """J x0 + diag(s) z - h(x0) with what cancels cancelled, as nonlin_factor (gbp_lin_nonlin.hpp) forms it: the translation columns of J
    times x0 are h's first two rows and theta_b - theta_a its third, so only the theta_a column is left.  Summed term by term it loses
    eps |x0| s, which unwrapped angles make as large as one likes (fixture G31, the SE(2) block).  The twin below keeps the
    reference's term-by-term sum (gbp.py:287): at the sizes of its graphs the two differ by rounding."""
    b = s * z
    b[:, 0:2] += J[:, 0:2, 2] * x0[:, 2:3]
    return b


class NonlinTwin:
    """FactorGraph(nonlinear_factors=True) for SE(2) relative-pose factors, vectorised over the factors."""

    def __init__(self, va, vb, z, s, prior_eta, prior_lam, beta, num_undamped_iters, min_linear_iters, eta_damping=0.0):
        self.va, self.vb = np.asarray(va, dtype=np.int64), np.asarray(vb, dtype=np.int64)
        self.F, self.N = self.va.shape[0], prior_eta.shape[0]
        self.z, self.s = np.asarray(z, dtype=float).reshape(self.F, 3), np.broadcast_to(np.asarray(s, dtype=float), (self.F, 3)).copy()
        self.pe, self.pl = np.array(prior_eta, dtype=float), np.array(prior_lam, dtype=float)
        self.beta, self.und, self.minlin, self.damping = float(beta), int(num_undamped_iters), int(min_linear_iters), float(eta_damping)
        self.me = [np.zeros((self.F, 3)), np.zeros((self.F, 3))]            # messages to a, to b (gbp.py:222)
        self.ml = [np.zeros((self.F, 3, 3)), np.zeros((self.F, 3, 3))]
        # belief sums in adj_factors order: ascending factor id (a factor meets a variable once)
        self._idx = np.stack([self.va, self.vb], 1).reshape(-1)
        self.update_all_beliefs()
        self.linpoint = self.adj_means()                                    # compute_all_factors gbp.py:60-62
        self.feta, self.flam = self.compute_factor(self.linpoint)
        self.iters = np.ones(self.F, dtype=np.int32)                        # gbp.py:248-249
        self.fdamp = np.zeros(self.F)

    def update_all_beliefs(self):
        self.be, self.bl = self.pe.copy(), self.pl.copy()
        if self.F:
            np.add.at(self.be, self._idx, np.stack(self.me, 1).reshape(-1, 3))
            np.add.at(self.bl, self._idx, np.stack(self.ml, 1).reshape(-1, 3, 3))
        self.mu = np.linalg.solve(self.bl, self.be[:, :, None])[:, :, 0] if self.N else self.be.copy()

    def adj_means(self):
        return np.concatenate([self.mu[self.va], self.mu[self.vb]], 1)

    def compute_factor(self, x0):
        """eta_f (F, 6), Lambda_f (F, 6, 6) at x0 (gbp.py:280-289, noise variance 1)."""
        J = se2_jac(x0, self.s)
        b = np.einsum('fki,fi->fk', J, x0) + self.s * self.z - se2_h(x0, self.s)
        return np.einsum('fki,fk->fi', J, b), np.einsum('fki,fkj->fij', J, J)

    def distance(self):
        return np.linalg.norm(self.linpoint - self.adj_means(), axis=1)

    def margin(self):
        """min | dist - beta | over the factors whose test can go either way: those allowed to relinearise (iters >= min_linear_iters)
        and whose dist is not EXACTLY 0 (the linpoint is a copy of the means, on the device as here: 0 > beta is false for any beta)."""
        d = self.distance()
        live = (self.iters >= self.minlin) & (d != 0.0)
        return float(np.min(np.abs(d[live] - self.beta), initial=np.inf))

    def relinearise_factors(self):
        """gbp.py:64-80; returns the mask."""
        x = self.adj_means()
        relin = (np.linalg.norm(self.linpoint - x, axis=1) > self.beta) & (self.iters >= self.minlin)
        if relin.any():
            e, l = self.compute_factor(x)
            self.feta[relin], self.flam[relin], self.linpoint[relin] = e[relin], l[relin], x[relin]
        self.iters = np.where(relin, 0, self.iters + 1).astype(np.int32)
        self.fdamp[relin] = 0.0
        return relin

    def compute_all_messages(self, local_relin=True):
        if local_relin:
            self.fdamp[self.iters == self.und] = self.damping              # gbp.py:50-51
            damp = self.fdamp
        else:
            damp = np.full(self.F, self.damping)
        if not self.F:
            return
        ends = (self.va, self.vb)
        new_e, new_l = [], []
        for v in (0, 1):                                                    # message to end v: eliminate the other end
            o = 1 - v
            ef, lf = self.feta.copy(), self.flam.copy()
            ef[:, 3 * o:3 * o + 3] += self.be[ends[o]] - self.me[o]         # gbp.py:348-349
            lf[:, 3 * o:3 * o + 3, 3 * o:3 * o + 3] += self.bl[ends[o]] - self.ml[o]
            K, E = slice(3 * v, 3 * v + 3), slice(3 * o, 3 * o + 3)
            sol = np.linalg.solve(lf[:, E, E], np.concatenate([lf[:, E, K], ef[:, E, None]], 2))
            new_l.append(lf[:, K, K] - lf[:, K, E] @ sol[:, :, :3])
            eta = ef[:, K] - (lf[:, K, E] @ sol[:, :, 3:])[:, :, 0]
            new_e.append((1 - damp)[:, None] * eta + damp[:, None] * self.me[v])   # gbp.py:368
        self.me, self.ml = new_e, new_l

    def synchronous_iteration(self, local_relin=True):
        relin = self.relinearise_factors() if local_relin else np.zeros(self.F, dtype=bool)
        self.compute_all_messages(local_relin)
        self.update_all_beliefs()
        return relin

    def iterate(self, n, relinearise=False):
        masks = [self.synchronous_iteration(relinearise) for _ in range(n)]
        return np.array([m.sum() for m in masks], dtype=np.int32) if relinearise else None

    def energy(self):
        """sum_f 0.5 |h(mu) - diag(s) z|^2 through the nonlinear h (gbp.py:36-44)."""
        r = se2_h(self.adj_means(), self.s) - self.s * self.z
        return 0.5 * float(np.sum(r * r))

    def linearised_energy(self):
        """The same sum through the factors as linearised: 0.5 |J (x - x0) + h(x0) - diag(s) z|^2."""
        J = se2_jac(self.linpoint, self.s)
        r = np.einsum('fki,fi->fk', J, self.adj_means() - self.linpoint) + se2_h(self.linpoint, self.s) - self.s * self.z
        return 0.5 * float(np.sum(r * r))

    def get_means(self):
        return self.mu.reshape(-1)

    def messages(self):
        return self.me[0], self.ml[0], self.me[1], self.ml[1]

    def beliefs(self):
        return self.be, self.bl

    def joint(self):
        """Dense joint at the current linearisation point (gbp.py:94-134): (eta (3N,), Lambda (3N, 3N))."""
        n = 3 * self.N
        eta, lam = self.pe.reshape(-1).copy(), np.zeros((n, n))
        for v in range(self.N):
            lam[3 * v:3 * v + 3, 3 * v:3 * v + 3] = self.pl[v]
        for f in range(self.F):
            ix = np.concatenate([np.arange(3) + 3 * self.va[f], np.arange(3) + 3 * self.vb[f]])
            eta[ix] += self.feta[f]
            lam[np.ix_(ix, ix)] += self.flam[f]
        return eta, lam


# ---- graphs ---------------------------------------------------------------------------------------------------------------------------

def _pose_graph(truth, edges, seed, theta0=0.0):
    rs = np.random.RandomState(seed)
    truth = truth + np.array([0.0, 0.0, theta0])
    N = truth.shape[0]
    va, vb = np.array([e[0] for e in edges], dtype=np.int32), np.array([e[1] for e in edges], dtype=np.int32)
    s = np.tile(SQRT_INFO, (len(edges), 1))
    z = se2_h(np.concatenate([truth[va], truth[vb]], 1), np.ones_like(s)) + rs.normal(0, 1, (len(edges), 3)) / s
    init = truth + rs.normal(0, 1, (N, 3)) * np.array([0.3, 0.3, 0.1])
    pe, pl = np.zeros((N, 3)), np.zeros((N, 3, 3))
    for i in range(N):
        sig = np.full(3, 1e-3) if i == 0 else np.array([1.0, 1.0, 0.5])
        pl[i] = np.diag(1 / sig ** 2)
        pe[i] = pl[i] @ (truth[0] if i == 0 else init[i])
    return dict(N=N, va=va, vb=vb, z=z, s=s, prior_eta=pe, prior_lam=pl, truth=truth)


def _circle(n, turns):
    th = np.arange(n) * 2 * np.pi * turns / max(n, 1)
    return np.stack([5.0 * np.cos(th), 5.0 * np.sin(th), th + np.pi / 2], 1)


def chain(n, seed=1, theta0=0.0):
    """n poses along 1.5 unwrapped turns of a circle, n - 1 odometry factors."""
    return _pose_graph(_circle(n, 1.5), [(i, i + 1) for i in range(n - 1)], seed, theta0)


def ring(n, closures, seed):
    """n poses on one turn, n factors around the ring (the last one back to pose 0: its heading difference is minus a turn, unwrapped)
    and `closures` random chords: F = n + closures."""
    rs = np.random.RandomState(1000 + seed)
    edges = [(i, (i + 1) % n) for i in range(n)]
    while len(edges) < n + closures:
        a, b = sorted(int(q) for q in rs.choice(n, 2, replace=False))
        if b - a > 3 and (a, b) not in edges:
            edges.append((a, b))
    return _pose_graph(_circle(n, 1.0), edges, seed)


def hub(seed=1):
    """A chain of 12 poses whose pose 5 also sees poses 0, 1, 2, 8, 9, 10, 11: 9 factors at one variable (the belief stage adds
    messages four at a time and then one by one)."""
    edges = [(i, i + 1) for i in range(11)] + [(0, 5), (1, 5), (2, 5), (5, 8), (5, 9), (5, 10), (5, 11)]
    return _pose_graph(_circle(12, 0.5), edges, seed)


SCHEDULE = dict(beta=0.05, num_undamped_iters=4, min_linear_iters=2, eta_damping=0.4)
SWEEPS = 12


def _shape_cases():
    out = [('F1', lambda: chain(2), SCHEDULE), ('hub9', lambda: hub(), SCHEDULE),
           ('turns40', lambda: chain(20, seed=2, theta0=40 * 2 * np.pi + 1e-3), SCHEDULE)]
    for F in (63, 64, 65, 129):
        out.append((f'chain{F}', lambda F=F: chain(F + 1, seed=F), SCHEDULE))
        out.append((f'ring{F}', lambda F=F: ring(F - 6, 6, seed=F), SCHEDULE))
    for und in (0, 1, 4):
        out.append((f'undamped{und}', lambda: ring(24, 4, seed=5), dict(SCHEDULE, num_undamped_iters=und)))
    out.append(('minlin5', lambda: ring(24, 4, seed=5), dict(SCHEDULE, min_linear_iters=5, beta=0.01)))
    out.append(('beta0', lambda: ring(24, 4, seed=5), dict(SCHEDULE, beta=0.0, min_linear_iters=0)))
    return out


CASES = _shape_cases()          # (name, graph builder, schedule): every seeded case the GPU tests run for SWEEPS sweeps


def twin_of(g, schedule):
    return NonlinTwin(g['va'], g['vb'], g['z'], g['s'], g['prior_eta'], g['prior_lam'], schedule['beta'], schedule['num_undamped_iters'],
                      schedule['min_linear_iters'], schedule['eta_damping'])


def run_margin(g, schedule, sweeps=SWEEPS):
    """min over the sweeps of the twin's margin before each of them."""
    t = twin_of(g, schedule)
    m = np.inf
    for _ in range(sweeps):
        m = min(m, t.margin())
        t.synchronous_iteration()
    return m


def g25_graph(g):
    return dict(N=g['prior_eta'].shape[0], va=g['edges'][:, 0].copy(), vb=g['edges'][:, 1].copy(), z=g['z'], s=g['s'],
                prior_eta=g['prior_eta'], prior_lam=g['prior_lam'])


def g25_schedule(g, tag):
    beta, damping, und, minlin, sweeps = g[tag + '_cfg']
    return dict(beta=float(beta), num_undamped_iters=int(und), min_linear_iters=int(minlin), eta_damping=float(damping)), int(sweeps)
