"""What the tests of the SE(3) relative-pose factor of the linear engine share (test_linear_se3_cpu.py, test_linear_se3_gpu.py): the model
in vectorised numpy, in fp64 and the formulas of include/gbp_lin.h (GBP_LIN_MODEL_SE3_BETWEEN); a numpy twin of the whole nonlinear
path -- relinearise, factor with per-factor damping, belief, losses at the linpoints, extend and shrink -- built on the SE(2) twin of
lin_nonlin_cases.py / lin_nonlin_live_cases.py / lin_nonlin_robust_cases.py with every 3 replaced by the model's D; the graph builders;
and the seeded cases the GPU tests run, whose distance from the relinearisation and loss thresholds the CPU test checks.
The twin is pinned to the reference's own run by fixture G28 (tests/golden/make_g28.py)."""
import numpy as np

from lin_nonlin_cases import PARITY, SCHEDULE, TOL                              # noqa: F401  (the GPU tests take them from here)
from lin_nonlin_robust_cases import HUBER, NONE, NonlinRobustTwin

D = 6
SQRT_INFO = np.array([10.0, 10.0, 10.0, 20.0, 20.0, 20.0])
AXIS = np.array([1.0, 2.0, 2.0]) / 3.0
SERIES_BELOW = 0.04             # th^2 below which the coefficients come from their series (gbp_lin_nonlin.hpp: th < 0.2)
NEAR_PI_T, NEAR_PI_COS = 6.76, -0.875       # th^2 / cos th past which Jr^-1's coefficient / Log take their forms for the neighbourhood of pi


# ---- the model ------------------------------------------------------------------------------------------------------------------------

def hat(w):
    o = np.zeros(w.shape[0])
    return np.stack([np.stack([o, -w[:, 2], w[:, 1]], 1), np.stack([w[:, 2], o, -w[:, 0]], 1), np.stack([-w[:, 1], w[:, 0], o], 1)], 1)


def _poly(t, c):
    out = np.zeros_like(t)
    for k in reversed(c):
        out = out * t + k
    return out


def coeffs(t):
    """sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3 from t = th^2 (F,)."""
    small = t < SERIES_BELOW
    th = np.sqrt(np.where(small, 1.0, t))
    tt = np.where(small, 1.0, t)
    sn, cs = np.sin(th), np.cos(th)
    A = np.where(small, _poly(t, [1.0, -1.0 / 6, 1.0 / 120, -1.0 / 5040, 1.0 / 362880, -1.0 / 39916800]), sn / th)
    B = np.where(small, _poly(t, [0.5, -1.0 / 24, 1.0 / 720, -1.0 / 40320, 1.0 / 3628800, -1.0 / 479001600]), (1.0 - cs) / tt)
    C = np.where(small, _poly(t, [1.0 / 6, -1.0 / 120, 1.0 / 5040, -1.0 / 362880, 1.0 / 39916800, -1.0 / 6227020800.0]), (th - sn) / (tt * th))
    return A, B, C


def jrinv_coeff(t):
    """1/th^2 - (1 + cos th) / (2 th sin th) from t = th^2; past th = 2.6 in the half-angle form 1/th^2 - cot(th / 2) / (2 th)."""
    small, near = t < SERIES_BELOW, t > NEAR_PI_T
    th = np.sqrt(np.where(small, 1.0, t))
    tt = np.where(small, 1.0, t)
    half = np.where(near, 0.5 * th, 1.0)
    return np.where(small, _poly(t, [1.0 / 12, 1.0 / 720, 1.0 / 30240, 1.0 / 1209600, 1.0 / 47900160, 691.0 / 1307674368000.0]),
                    np.where(near, 1.0 / tt - np.cos(half) / (2.0 * th * np.sin(half)), 1.0 / tt - (1.0 + np.cos(th)) / (2.0 * th * np.sin(th))))


def ik(w, a, b):
    """I + a [w]x + b [w]x^2, (F, 3, 3)."""
    K = hat(w)
    return np.eye(3)[None] + a[:, None, None] * K + b[:, None, None] * (K @ K)


def so3_log(E):
    """The principal Log: axis from the skew part, angle from atan2(|skew part|, trace part); past cos th = NEAR_PI_COS the axis from the
    symmetric part cos th I + (1 - cos th) a a^T -- its largest diagonal entry by a square root, the other two components by division
    of the off-diagonal entries, the sign from the skew part (gbp_lin_nonlin.hpp, se3_log)."""
    v = 0.5 * np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], 1)
    nv = np.linalg.norm(v, axis=1)
    cs = 0.5 * (np.trace(E, axis1=1, axis2=2) - 1.0)
    th = np.arctan2(nv, cs)
    out = np.where(nv > 0, th / np.where(nv > 0, nv, 1.0), 1.0)[:, None] * v
    near = cs < NEAR_PI_COS
    if near.any():
        En, vn, c, r = E[near], v[near], cs[near], np.arange(int(near.sum()))
        k = np.argmax(np.stack([En[:, 0, 0], En[:, 1, 1], En[:, 2, 2]], 1), axis=1)      # the first of equal entries, as the engine's selects
        oc = 1.0 - c
        ak = np.copysign(np.sqrt((En[r, k, k] - c) / oc), vn[r, k])
        a = 0.5 * (En[r, k, :] + En[r, :, k]) / (oc * ak)[:, None]
        a[r, k] = ak
        out[near] = th[near, None] * a
    return out


def se3_parts(x):
    """Q = R_a^T, E = Q R_b, u, phi, Jr(w_a), Jr(w_b) of x (F, 12)."""
    wa, wb = x[:, 3:6], x[:, 9:12]
    A, B, C = coeffs(np.sum(wa * wa, 1))
    Q, Jra = ik(wa, -A, B), ik(wa, -B, C)
    A, B, C = coeffs(np.sum(wb * wb, 1))
    Rb, Jrb = ik(wb, A, B), ik(wb, -B, C)
    E = Q @ Rb
    u = np.einsum('fij,fj->fi', Q, x[:, 6:9] - x[:, 0:3])
    return Q, E, u, so3_log(E), Jra, Jrb


def se3_h(x, s):
    """x (F, 12) = [xa; xb], s (F, 6) -> diag(s) h (F, 6)."""
    _, _, u, phi, _, _ = se3_parts(x)
    return s * np.concatenate([u, phi], 1)


def se3_jac(x, s):
    """(F, 6, 12), whitened."""
    Q, E, u, phi, Jra, Jrb = se3_parts(x)
    Ji = ik(phi, np.full(x.shape[0], 0.5), jrinv_coeff(np.sum(phi * phi, 1)))
    J = np.zeros((x.shape[0], 6, 12))
    J[:, 0:3, 0:3], J[:, 0:3, 3:6], J[:, 0:3, 6:9] = -Q, hat(u) @ Jra, Q
    J[:, 3:6, 3:6], J[:, 3:6, 9:12] = -Ji @ np.swapaxes(E, 1, 2) @ Jra, Ji @ Jrb
    return s[:, :, None] * J


# ---- the twin -------------------------------------------------------------------------------------------------------------------------

class Se3Twin(NonlinRobustTwin):
    """FactorGraph(nonlinear_factors=True) for SE(3) relative-pose factors, vectorised over the factors: NonlinTwin with D = 6 and the
    model above, with the extend / shrink of LiveTwin and the losses of NonlinRobustTwin (shrink, the loss bookkeeping, the relinearise
    stage and the damping switch are inherited as they are: they do not know D)."""

    def __init__(self, va, vb, z, s, prior_eta, prior_lam, beta, num_undamped_iters, min_linear_iters, eta_damping=0.0):
        self.va, self.vb = np.asarray(va, dtype=np.int64).reshape(-1), np.asarray(vb, dtype=np.int64).reshape(-1)
        self.F, self.N = self.va.shape[0], np.asarray(prior_eta).reshape(-1, D).shape[0]
        self.z, self.s = np.asarray(z, dtype=float).reshape(self.F, D), np.broadcast_to(np.asarray(s, dtype=float), (self.F, D)).copy()
        self.pe, self.pl = np.array(prior_eta, dtype=float).reshape(self.N, D), np.array(prior_lam, dtype=float).reshape(self.N, D, D)
        self.beta, self.und, self.minlin, self.damping = float(beta), int(num_undamped_iters), int(min_linear_iters), float(eta_damping)
        self.me = [np.zeros((self.F, D)), np.zeros((self.F, D))]
        self.ml = [np.zeros((self.F, D, D)), np.zeros((self.F, D, D))]
        self._idx = np.stack([self.va, self.vb], 1).reshape(-1)
        self.update_all_beliefs()
        self.linpoint = self.adj_means()
        self.feta, self.flam = self.compute_factor(self.linpoint)
        self.iters = np.ones(self.F, dtype=np.int32)
        self.fdamp = np.zeros(self.F)
        self.robust = False
        self._fresh(0)

    def update_all_beliefs(self):
        self.be, self.bl = self.pe.copy(), self.pl.copy()
        if self.F:
            np.add.at(self.be, self._idx, np.stack(self.me, 1).reshape(-1, D))
            np.add.at(self.bl, self._idx, np.stack(self.ml, 1).reshape(-1, D, D))
        self.mu = np.linalg.solve(self.bl, self.be[:, :, None])[:, :, 0] if self.N else self.be.copy()

    def _factor_at(self, x0, z, s):
        J = se3_jac(x0, s)
        b = np.einsum('fki,fi->fk', J, x0) + s * z - se3_h(x0, s)
        return np.einsum('fki,fk->fi', J, b), np.einsum('fki,fkj->fij', J, J)

    def compute_factor(self, x0):
        return self._factor_at(x0, self.z, self.s)

    def _messages(self, local_relin):
        if local_relin:
            self.fdamp[self.iters == self.und] = self.damping
            damp = self.fdamp
        else:
            damp = np.full(self.F, self.damping)
        if not self.F:
            return
        ends = (self.va, self.vb)
        new_e, new_l = [], []
        for v in (0, 1):
            o = 1 - v
            ef, lf = self.feta.copy(), self.flam.copy()
            ef[:, D * o:D * o + D] += self.be[ends[o]] - self.me[o]
            lf[:, D * o:D * o + D, D * o:D * o + D] += self.bl[ends[o]] - self.ml[o]
            K, E = slice(D * v, D * v + D), slice(D * o, D * o + D)
            sol = np.linalg.solve(lf[:, E, E], np.concatenate([lf[:, E, K], ef[:, E, None]], 2))
            new_l.append(lf[:, K, K] - lf[:, K, E] @ sol[:, :, :D])
            eta = ef[:, K] - (lf[:, K, E] @ sol[:, :, D:])[:, :, 0]
            new_e.append((1 - damp)[:, None] * eta + damp[:, None] * self.me[v])
        self.me, self.ml = new_e, new_l

    def compute_all_messages(self, local_relin=True):
        return self._weighted(self._messages, local_relin)

    def _joint(self):
        n = D * self.N
        eta, lam = self.pe.reshape(-1).copy(), np.zeros((n, n))
        for v in range(self.N):
            lam[D * v:D * v + D, D * v:D * v + D] = self.pl[v]
        for f in range(self.F):
            ix = np.concatenate([np.arange(D) + D * self.va[f], np.arange(D) + D * self.vb[f]])
            eta[ix] += self.feta[f]
            lam[np.ix_(ix, ix)] += self.flam[f]
        return eta, lam

    def joint(self):
        return self._weighted(self._joint)

    def mahalanobis(self):
        return np.linalg.norm(self.s * self.z - se3_h(self.linpoint, self.s), axis=1)

    def energy(self):
        r = se3_h(self.adj_means(), self.s) - self.s * self.z
        return 0.5 * float(np.sum(self.w * np.sum(r * r, 1)))

    def extend(self, va, vb, z, s, prior_eta=None, prior_lam=None):
        va, vb = np.asarray(va, dtype=np.int64).reshape(-1), np.asarray(vb, dtype=np.int64).reshape(-1)
        dF, F0 = va.shape[0], self.F
        z, s = np.asarray(z, dtype=float).reshape(dF, D), np.broadcast_to(np.asarray(s, dtype=float), (dF, D)).copy()
        if prior_eta is not None:
            self.pe = np.concatenate([self.pe, np.asarray(prior_eta, dtype=float).reshape(-1, D)])
            self.pl = np.concatenate([self.pl, np.asarray(prior_lam, dtype=float).reshape(-1, D, D)])
        self.va, self.vb = np.concatenate([self.va, va]), np.concatenate([self.vb, vb])
        self.z, self.s = np.concatenate([self.z, z]), np.concatenate([self.s, s])
        self.me = [np.concatenate([m, np.zeros((dF, D))]) for m in self.me]
        self.ml = [np.concatenate([m, np.zeros((dF, D, D))]) for m in self.ml]
        self._reindex()
        self.update_all_beliefs()
        x0 = self.adj_means()[F0:]
        e, l = self._factor_at(x0, z, s)
        self.feta, self.flam, self.linpoint = np.concatenate([self.feta, e]), np.concatenate([self.flam, l]), np.concatenate([self.linpoint, x0])
        self.iters = np.concatenate([self.iters, np.ones(dF, dtype=np.int32)])
        self.fdamp = np.concatenate([self.fdamp, np.zeros(dF)])
        self._fresh(F0)


def twin_of(g, schedule, losses=True):
    t = Se3Twin(g['va'], g['vb'], g['z'], g['s'], g['prior_eta'], g['prior_lam'], schedule['beta'], schedule['num_undamped_iters'],
                schedule['min_linear_iters'], schedule['eta_damping'])
    if losses and 'loss' in g:
        t.set_robust(g['loss'], g['thr'])
    return t


# ---- graphs ---------------------------------------------------------------------------------------------------------------------------

def pose_graph(truth, edges, seed, rot_noise=1.0, prior_noise=1.0):
    """Measurements h(truth) + N(0, 1 / s) (rotation part times rot_noise), pose 0 anchored at its truth, the others with loose priors
    at truth + N(0, (0.3, 0.3, 0.3, 0.1, 0.1, 0.1)) (rotation part times rot_noise, all of it times prior_noise)."""
    rs = np.random.RandomState(seed)
    N = truth.shape[0]
    va, vb = np.array([e[0] for e in edges], dtype=np.int32), np.array([e[1] for e in edges], dtype=np.int32)
    s = np.tile(SQRT_INFO, (len(edges), 1))
    scale = np.array([1.0, 1.0, 1.0, rot_noise, rot_noise, rot_noise])
    z = se3_h(np.concatenate([truth[va], truth[vb]], 1), np.ones_like(s)) + rs.normal(0, 1, (len(edges), D)) / s * scale
    init = truth + rs.normal(0, 1, (N, D)) * np.array([0.3, 0.3, 0.3, 0.1, 0.1, 0.1]) * scale * prior_noise
    pe, pl = np.zeros((N, D)), np.zeros((N, D, D))
    for i in range(N):
        sig = np.full(D, 1e-3) if i == 0 else np.array([1.0, 1.0, 1.0, 0.5, 0.5, 0.5])
        pl[i] = np.diag(1 / sig ** 2)
        pe[i] = pl[i] @ (truth[0] if i == 0 else init[i])
    return dict(N=N, va=va, vb=vb, z=z, s=s, prior_eta=pe, prior_lam=pl, truth=truth)


def _helix(ang, step=0.25):
    e1 = np.cross(AXIS, [1.0, 0.0, 0.0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(AXIS, e1)
    pos = 5.0 * (np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2) + step * np.arange(len(ang))[:, None] * AXIS
    return np.concatenate([pos, ang[:, None] * AXIS], 1)


def helix(n, seed=1, angle=4.5):
    """n poses whose rotation vector runs continuously from 0 to `angle` rad about AXIS -- past pi --, n - 1 odometry factors and
    n // 5 closures (b - a > 3, relative rotation below 2.5)."""
    ang = np.arange(n) * angle / max(n - 1, 1)
    rs = np.random.RandomState(2000 + seed)
    edges = [(i, i + 1) for i in range(n - 1)]
    while n > 8 and len(edges) < n - 1 + n // 5:
        a, b = sorted(int(q) for q in rs.choice(n, 2, replace=False))
        if b - a > 3 and ang[b] - ang[a] < 2.5 and (a, b) not in edges:
            edges.append((a, b))
    return pose_graph(_helix(ang), edges, seed)


def ring2(n, seed):
    """n poses on a closed loop, each joined to its next and its next but one around the ring: 2 n factors.  The rotation angle rises
    to 4.5 rad half way round and falls back, so w stays continuous and every relative rotation small."""
    ang = 4.5 * (1.0 - np.abs(2.0 * np.arange(n) / n - 1.0))
    loop = 2 * np.pi * np.arange(n) / n
    truth = _helix(ang, 0.0)
    truth[:, 0:3] = 5.0 * np.stack([np.cos(loop), np.sin(loop), 0.3 * np.sin(2 * loop)], 1)
    edges = [(i, (i + 1) % n) for i in range(n)] + [(i, (i + 2) % n) for i in range(n)]
    return pose_graph(truth, edges, seed)


def star(leaves, seed):
    """Pose 0 joined to `leaves` others: its adjacency list holds that many factors."""
    ang = np.concatenate([[0.7], 0.7 + np.linspace(-1.2, 1.2, leaves)])
    return pose_graph(_helix(ang), [(0, i) for i in range(1, leaves + 1)], seed)


def flat_chain(n, seed, rot):
    """A chain along a line whose true rotation vectors all are `rot` * AXIS and whose measured and prior rotations are exact: with
    rot = 0 every w the device first sees is exactly 0 (th = 0 in every coefficient, |skew part| = 0 in Log); with rot = 1e-7 it
    sits deep in the series."""
    truth = np.concatenate([np.arange(n)[:, None] * np.array([1.0, 0.5, -0.25]), np.tile(rot * AXIS, (n, 1))], 1)
    g = pose_graph(truth, [(i, i + 1) for i in range(n - 1)], seed, rot_noise=0.0)
    if rot == 0.0:
        assert not g['z'][:, 3:].any() and not g['prior_eta'][:, 3:].any()
    return g


SWEEPS = 10
CASES = [('F1', lambda: helix(2, seed=3, angle=0.4), SCHEDULE),
         ('ring258', lambda: ring2(129, seed=4), SCHEDULE),
         ('star70', lambda: star(70, seed=5), SCHEDULE),
         ('zero', lambda: flat_chain(9, 6, 0.0), SCHEDULE),
         ('tiny', lambda: flat_chain(9, 7, 1e-7), SCHEDULE),
         ('helix', lambda: helix(24, seed=8), SCHEDULE),
         ('beta_inf', lambda: helix(12, seed=9), dict(SCHEDULE, beta=np.inf)),
         ('beta0', lambda: helix(12, seed=9), dict(SCHEDULE, beta=0.0, min_linear_iters=0)),
         ('undamped0', lambda: helix(12, seed=9), dict(SCHEDULE, num_undamped_iters=0)),
         ('undamped1', lambda: helix(12, seed=9), dict(SCHEDULE, num_undamped_iters=1))]
OFFSET = np.array([1.5, -1.0, 0.8, 0.3, -0.2, 0.25])


def case(name):
    _, build, sched = next(c for c in CASES if c[0] == name)
    return build(), sched


def robust_case():
    """helix(24) with every closure under Huber at threshold 4 and every other closure corrupted."""
    g = helix(24, seed=8)
    F = len(g['va'])
    loss, z = np.zeros(F, dtype=np.int32), g['z'].copy()
    loss[23:] = HUBER
    z[23::2] += OFFSET
    return dict(g, z=z, loss=loss, thr=np.where(loss == HUBER, 4.0, 1.0)), SCHEDULE


def live_case():
    """(head, tail, schedule) of the live-handle test: robust_case()'s first 16 poses and 15 odometry factors, the last two under Huber,
    and the extend that appends the rest (the closures among them, without a loss)."""
    g, sched = robust_case()
    N0, F0 = 16, 15
    head = dict(N=N0, va=g['va'][:F0], vb=g['vb'][:F0], z=g['z'][:F0], s=g['s'][:F0], prior_eta=g['prior_eta'][:N0], prior_lam=g['prior_lam'][:N0],
                loss=np.array([NONE] * 13 + [HUBER, HUBER], dtype=np.int32), thr=np.array([1.0] * 13 + [4.0, 4.0]))
    tail = dict(va=g['va'][F0:], vb=g['vb'][F0:], z=g['z'][F0:], s=g['s'][F0:], prior_eta=g['prior_eta'][N0:], prior_lam=g['prior_lam'][N0:])
    return head, tail, sched


def live_margins():
    """The live-handle test played on the twin alone: (distance margin, loss margin) before every sweep of it."""
    h, k, sched = live_case()
    t = twin_of(h, sched)
    dm = rm = np.inf

    def sweeps(n):
        nonlocal dm, rm
        for _ in range(n):
            dm, rm = min(dm, t.margin()), min(rm, t.robust_margin())
            t.synchronous_iteration(True, True)

    sweeps(5)
    t.extend(k['va'], k['vb'], k['z'], k['s'], k['prior_eta'], k['prior_lam'])
    sweeps(3)
    t.shrink(retire=[0, 1])
    t.shrink(drop=[t.F - 1])
    sweeps(2)
    return dm, rm


def run_margins(g, schedule, sweeps=SWEEPS, robustify=False):
    """(distance margin, loss margin): the minima over the sweeps of the twin's margins before each of them."""
    t = twin_of(g, schedule)
    dm = rm = np.inf
    for _ in range(sweeps):
        dm = min(dm, t.margin())
        if robustify:
            rm = min(rm, t.robust_margin())
        t.synchronous_iteration(True, robustify)
    return dm, rm


def g28_graph(g, tag):
    out = dict(N=g['prior_eta'].shape[0], va=g['edges'][:, 0].copy(), vb=g['edges'][:, 1].copy(), z=g['robust_z'] if tag == 'robust' else g['z'], s=g['s'],
               prior_eta=g['prior_eta'], prior_lam=g['prior_lam'])
    if tag == 'robust':
        out.update(loss=g['loss'], thr=np.where(g['loss'] != NONE, g['threshold'], 1.0))
    return out


def g28_schedule(g, tag):
    beta, damping, und, minlin, sweeps = g[tag + '_cfg']
    return dict(beta=float(beta), num_undamped_iters=int(und), min_linear_iters=int(minlin), eta_damping=float(damping)), int(sweeps)


def dense_joint(graph, feta, flam):
    N = graph['N']
    eta, lam = graph['prior_eta'].reshape(-1).copy(), np.zeros((D * N, D * N))
    for v in range(N):
        lam[D * v:D * v + D, D * v:D * v + D] = graph['prior_lam'][v]
    for f, (a, b) in enumerate(zip(graph['va'], graph['vb'])):
        ix = np.concatenate([np.arange(D) + D * a, np.arange(D) + D * b])
        eta[ix] += feta[f]
        lam[np.ix_(ix, ix)] += flam[f]
    return eta, lam
