"""What the tests of robust losses on a nonlinear handle share (test_linear_nonlinear_robust_cpu.py, test_linear_nonlinear_robust_gpu.py):
the numpy twin of lin_nonlin_cases.py / lin_nonlin_live_cases.py with loss, threshold, weight and flag per factor, in the words of
include/gbp_lin.h -- robustify_all_factors at the LINPOINTS (gbp.py:309), the weighted factor in the messages, the joint and the
energy, synchronous_iteration(robustify=True) in the order of gbp.py:86-92 -- and the seeded cases the GPU tests run.  Both tests of a
sweep are discontinuous (`M > t`, `dist > beta`); the CPU test shows every case stays >= MARGIN clear of both before every sweep.
The twin is pinned to the reference's own run by fixture G27 (tests/golden/make_g27.py)."""
import numpy as np

from lin_nonlin_cases import SCHEDULE, SWEEPS, chain, hub, ring, se2_h
from lin_nonlin_live_cases import LiveTwin

MARGIN = 1e-7                   # every case stays this clear of `M > t` and of `dist > beta` before every sweep
NONE, HUBER, CONSTANT = 0, 1, 2
LOSS_NAME = {NONE: None, HUBER: 'huber', CONSTANT: 'constant'}
NEW_THR = 1.0                   # what the handle holds as the threshold of a factor without a loss (never read)


class NonlinRobustTwin(LiveTwin):
    """NonlinTwin (through LiveTwin, which adds extend and shrink) with Factor(loss=, mahalanobis_threshold=) on every factor."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.robust = False                                  # losses are set
        self._fresh(0)

    def _fresh(self, keep):
        """Factors from `keep` on are new ones: no loss, weight 1, not flagged."""
        n = self.F - keep
        cat = lambda name, fill, dt: np.concatenate([getattr(self, name)[:keep] if keep else np.zeros(0, dt), np.full(n, fill, dt)])
        self.loss, self.flag = cat('loss', NONE, np.int32), cat('flag', False, bool)
        self.thr, self.w = cat('thr', NEW_THR, float), cat('w', 1.0, float)

    def set_robust(self, loss, threshold=2.0, first=0):
        """gbp_lin_set_robust_nonlinear: loss None clears; else codes (or one code) for factors first, first + 1, ..."""
        if loss is None:
            self.robust = False
            self._fresh(0)
            return
        if not self.robust:
            self._fresh(0)
        loss = np.full(self.F - first, loss, np.int32) if np.isscalar(loss) else np.asarray(loss, dtype=np.int32)
        r = slice(first, first + loss.shape[0])
        thr = np.broadcast_to(np.asarray(threshold, dtype=float), loss.shape)
        self.loss[r], self.thr[r] = loss, np.where(loss != NONE, thr, NEW_THR)
        self.w[r], self.flag[r] = 1.0, False
        self.robust = True

    def mahalanobis(self):
        """M_f = |diag(s) z - h(linpoint)|_2 (gbp.py:309, 312)."""
        return np.linalg.norm(self.s * self.z - se2_h(self.linpoint, self.s), axis=1)

    def robust_margin(self):
        lossy = self.loss != NONE
        return float(np.min(np.abs(self.mahalanobis() - self.thr)[lossy], initial=np.inf))

    def robustify_all_factors(self):
        """gbp.py:82-84, 296-332 with noise variance 1."""
        m, t = self.mahalanobis(), self.thr
        self.flag = (self.loss != NONE) & (m > t)
        safe = np.where(self.flag, m, 1.0)
        w = np.where(self.loss == HUBER, (2 * t * safe - t * t) / safe ** 2, 1.0 / safe ** 2)
        self.w = np.where(self.flag, w, 1.0)
        return self.flag

    def _weighted(self, fn, *a):
        """Runs fn with (eta_f, Lambda_f) times w_f in place of the nominal factor (gbp.py:331-332)."""
        e, l = self.feta, self.flam
        self.feta, self.flam = e * self.w[:, None], l * self.w[:, None, None]
        try:
            return fn(*a)
        finally:
            self.feta, self.flam = e, l

    def compute_all_messages(self, local_relin=True):
        return self._weighted(super().compute_all_messages, local_relin)

    def joint(self):
        return self._weighted(super().joint)

    def energy(self):
        """sum_f w_f 0.5 |h(mu) - diag(s) z|^2 (gbp.py:43)."""
        r = se2_h(self.adj_means(), self.s) - self.s * self.z
        return 0.5 * float(np.sum(self.w * np.sum(r * r, 1)))

    def synchronous_iteration(self, local_relin=True, robustify=False):
        """gbp.py:86-92: robustify at the linpoints as they stand, relinearise, messages, beliefs.  Returns (relin mask, flags) with
        robustify, else the mask."""
        if robustify:
            self.robustify_all_factors()
        relin = super().synchronous_iteration(local_relin)
        return (relin, self.flag.copy()) if robustify else relin

    def iterate(self, n, relinearise=False, robustify=False):
        if not robustify:
            return super().iterate(n, relinearise)
        out = [self.synchronous_iteration(relinearise, True) for _ in range(n)]
        return (np.array([m.sum() for m, _ in out], dtype=np.int32), np.array([f.sum() for _, f in out], dtype=np.int32))

    def extend(self, *a, **k):
        F0 = self.F
        super().extend(*a, **k)
        self._fresh(F0)

    def shrink(self, retire=(), drop=(), fold=True):
        vmap, fmap = super().shrink(retire, drop, fold)
        keep = fmap >= 0
        for name in ('loss', 'thr', 'w', 'flag'):
            setattr(self, name, getattr(self, name)[keep])
        return vmap, fmap


def robust_twin(g, schedule=SCHEDULE, losses=True):
    t = NonlinRobustTwin(g['va'], g['vb'], g['z'], g['s'], g['prior_eta'], g['prior_lam'], schedule['beta'], schedule['num_undamped_iters'],
                         schedule['min_linear_iters'], schedule['eta_damping'])
    if losses and 'loss' in g:
        t.set_robust(g['loss'], g['thr'])
    return t


# ---- graphs: those of lin_nonlin_cases.py with corrupted measurements and losses ------------------------------------------------------

OFFSET = np.array([1.5, -1.0, 0.4])


def with_losses(g, pattern, thr_huber=2.0, thr_constant=3.0, every=3):
    """Corrupts the measurement of every `every`-th factor counted from the LAST one (the closures of a ring are its last factors; at
    least one factor) and gives factor f the loss pattern[f % len(pattern)], counted from the last one too."""
    F = len(g['va'])
    back = F - 1 - np.arange(F)
    z = g['z'].copy()
    z[back % every == 0] += OFFSET
    loss = np.array([pattern[b % len(pattern)] for b in back], dtype=np.int32)
    thr = np.where(loss == HUBER, thr_huber, np.where(loss == CONSTANT, thr_constant, NEW_THR))
    return dict(g, z=z, loss=loss, thr=thr)


MIXED = (HUBER, CONSTANT, NONE)


def _cases():
    out = [('F1', lambda: with_losses(chain(2), (HUBER,)), SCHEDULE), ('hub9', lambda: with_losses(hub(), MIXED), SCHEDULE)]
    for F in (63, 64, 65, 129):
        out.append((f'chain{F}', lambda F=F: with_losses(chain(F + 1, seed=F), MIXED), SCHEDULE))
        out.append((f'ring{F}', lambda F=F: with_losses(ring(F - 6, 6, seed=F), MIXED), SCHEDULE))
    base = lambda: ring(24, 4, seed=5)
    out.append(('all_huber', lambda: with_losses(base(), (HUBER,)), SCHEDULE))
    out.append(('all_constant', lambda: with_losses(base(), (CONSTANT,)), SCHEDULE))
    out.append(('mixed_none', lambda: with_losses(base(), (NONE, HUBER, NONE, CONSTANT)), SCHEDULE))
    out.append(('never_flagged', lambda: with_losses(base(), (HUBER, CONSTANT), 1e6, 1e6), SCHEDULE))
    # Huber only: the constant loss below M = 1 is w = 1 / M^2 > 1, up to 1e3 here, on factors whose residual s z - h has cancelled to
    # M ~ 1e-2 -- twelve sweeps of such a stiff graph amplify the rounding of M (eps |s z| / M, doubled by the square) past what two fp64
    # evaluations of the same formulas can be held to; the Huber weight 2 t / M stays below 1 and is as well conditioned as M itself
    out.append(('all_flagged', lambda: with_losses(base(), (HUBER,), 1e-3), SCHEDULE))
    out.append(('beta0', lambda: with_losses(base(), MIXED), dict(SCHEDULE, beta=0.0, min_linear_iters=0)))
    return out


CASES = _cases()                # (name, graph builder, schedule): every seeded case the GPU tests run for SWEEPS robust sweeps
EXTREME = ('never_flagged', 'all_flagged')


def case(name):
    _, build, sched = next(c for c in CASES if c[0] == name)
    return build(), sched


def run_margins(g, schedule, sweeps=SWEEPS):
    """(robust margin, distance margin, flags (sweeps, F)): the minima over the sweeps of the twin's margins before each of them."""
    t = robust_twin(g, schedule)
    rm = dm = np.inf
    flags = []
    for _ in range(sweeps):
        rm, dm = min(rm, t.robust_margin()), min(dm, t.margin())
        flags.append(t.synchronous_iteration(True, True)[1])
    return rm, dm, np.array(flags)


def g27_graph(g):
    return dict(N=g['prior_eta'].shape[0], va=g['edges'][:, 0].copy(), vb=g['edges'][:, 1].copy(), z=g['z'], s=g['s'], prior_eta=g['prior_eta'],
                prior_lam=g['prior_lam'], loss=g['loss'], thr=g['threshold'])


def g27_schedule(g):
    beta, damping, und, minlin, sweeps = g['cfg']
    return dict(beta=float(beta), num_undamped_iters=int(und), min_linear_iters=int(minlin), eta_damping=float(damping)), int(sweeps)


# ---- a live smoother with closures that get a loss when they are appended ------------------------------------------------------------

def live_schedule(rounds=10, seed=21, hold=10):
    """(starting graph, rounds): each round appends one pose with its odometry factor and one closure onto a held pose -- every other
    closure corrupted --, gives the closure a loss by range, runs two robust sweeps and retires the oldest pose with fold once more
    than `hold` are held.  A round is (extend kwargs, (first - F of before the extend, codes, thresholds), sweeps, shrink kwargs or None)."""
    from lin_nonlin_live_cases import compose, pose_prior
    from lin_nonlin_cases import SQRT_INFO
    rs = np.random.RandomState(seed)
    n0 = 8
    g0 = chain(n0, seed=seed)
    th = np.arange(n0 + rounds) * 2 * np.pi * 1.5 / n0
    truth = np.concatenate([g0['truth'], np.stack([5.0 * np.cos(th), 5.0 * np.sin(th), th + np.pi / 2], 1)[n0:]])
    held, out = list(range(n0)), []
    for k in range(n0, n0 + rounds):
        def meas(i, j):
            return se2_h(np.concatenate([truth[i], truth[j]])[None], np.ones((1, 3)))[0] + rs.normal(0, 1, 3) / SQRT_INFO
        z = [meas(k - 1, k)]
        pe, pl = pose_prior(compose(truth[k - 1], z[0]) + rs.normal(0, 1, 3) * np.array([0.05, 0.05, 0.02]))
        j = int(rs.randint(0, len(held) - 3))
        z.append(meas(held[j], k) + (OFFSET if (k - n0) % 2 == 0 else 0.0))
        ext = dict(va=np.array([len(held) - 1, j]), vb=np.array([len(held), len(held)]), z=np.array(z), s=np.tile(SQRT_INFO, (2, 1)), prior_eta=pe[None],
                   prior_lam=pl[None])
        held.append(k)
        code = HUBER if (k - n0) % 4 < 2 else CONSTANT
        rng = (1, np.array([code], dtype=np.int32), np.array([2.0 if code == HUBER else 3.0]))   # first: counted from the F of before the extend
        shr = None
        if len(held) > hold:
            held.pop(0)
            shr = dict(retire=[0], drop=[], fold=True)
        out.append((ext, rng, 2, shr))
    return g0, out
