"""What the tests of gbp_lin_extend_nonlinear / gbp_lin_shrink_nonlinear share (test_linear_nonlinear_live_cpu.py,
test_linear_nonlinear_live_gpu.py): the numpy twin of lin_nonlin_cases.py with the two calls added, in the words of include/gbp_lin.h --
extend: append, update_all_beliefs(), compute_factor() on the new factors only, iters 1 and damping 0 there, everything older kept;
shrink: the plan and the fold of lin_shrink_cases.py, every per-factor array gathered through the survivors -- and the seeded schedules
the GPU tests run, as lists of steps that a driver plays on an engine and on the twin alike.  The CPU test plays every schedule on the
twin alone and checks its distance from the relinearisation threshold before every sweep.
The twin with both calls is pinned to the reference's own grown run by fixture G26 (tests/golden/make_g26.py)."""
import numpy as np

from lin_nonlin_cases import NonlinTwin, SCHEDULE, SQRT_INFO, SWEEPS, chain, hub, ring, se2_h, se2_jac, twin_of
from lin_shrink_cases import fold_sides, plan

MARGIN = 1e-9                   # every schedule stays this clear of `dist > beta` before every sweep


class LiveTwin(NonlinTwin):
    def _reindex(self):
        self.F, self.N = self.va.shape[0], self.pe.shape[0]
        self._idx = np.stack([self.va, self.vb], 1).reshape(-1)

    def extend(self, va, vb, z, s, prior_eta=None, prior_lam=None):
        va, vb = np.asarray(va, dtype=np.int64).reshape(-1), np.asarray(vb, dtype=np.int64).reshape(-1)
        dF = va.shape[0]
        z, s = np.asarray(z, dtype=float).reshape(dF, 3), np.broadcast_to(np.asarray(s, dtype=float), (dF, 3)).copy()
        if prior_eta is not None:
            self.pe = np.concatenate([self.pe, np.asarray(prior_eta, dtype=float).reshape(-1, 3)])
            self.pl = np.concatenate([self.pl, np.asarray(prior_lam, dtype=float).reshape(-1, 3, 3)])
        F0 = self.F
        self.va, self.vb = np.concatenate([self.va, va]), np.concatenate([self.vb, vb])
        self.z, self.s = np.concatenate([self.z, z]), np.concatenate([self.s, s])
        self.me = [np.concatenate([m, np.zeros((dF, 3))]) for m in self.me]                 # gbp.py:222
        self.ml = [np.concatenate([m, np.zeros((dF, 3, 3))]) for m in self.ml]
        self._reindex()
        self.update_all_beliefs()                                                           # gbp.py:56-58
        x0 = self.adj_means()[F0:]                                                          # compute_factor on the new ones, gbp.py:267-294
        J = se2_jac(x0, s)
        b = np.einsum('fki,fi->fk', J, x0) + s * z - se2_h(x0, s)
        self.feta = np.concatenate([self.feta, np.einsum('fki,fk->fi', J, b)])
        self.flam = np.concatenate([self.flam, np.einsum('fki,fkj->fij', J, J)])
        self.linpoint = np.concatenate([self.linpoint, x0])
        self.iters = np.concatenate([self.iters, np.ones(dF, dtype=np.int32)])              # gbp.py:248-249
        self.fdamp = np.concatenate([self.fdamp, np.zeros(dF)])

    def shrink(self, retire=(), drop=(), fold=True):
        """(var_map, factor_map).  The folded message is the stored one: computed at the leaving factor's last linearisation point."""
        vkeep, fkeep, _, vmap, fmap = plan(self.N, self.va, self.vb, retire, drop)
        side = fold_sides(self.N, self.va, self.vb, retire, drop, fold)
        for f in np.flatnonzero(side):                       # ascending factor id = adjacency order of every variable
            k = side[f] - 1
            v = (self.va, self.vb)[k][f]
            self.pe[v] = self.pe[v] + self.me[k][f]
            self.pl[v] = self.pl[v] + self.ml[k][f]
        self.pe, self.pl = self.pe[vkeep], self.pl[vkeep]
        self.va, self.vb = vmap[self.va[fkeep]].astype(np.int64), vmap[self.vb[fkeep]].astype(np.int64)
        for name in ('z', 's', 'feta', 'flam', 'linpoint', 'iters', 'fdamp'):
            setattr(self, name, getattr(self, name)[fkeep])
        self.me, self.ml = [m[fkeep] for m in self.me], [m[fkeep] for m in self.ml]
        self._reindex()
        self.update_all_beliefs()
        return vmap, fmap


def live_twin(g, schedule=SCHEDULE):
    return LiveTwin(g['va'], g['vb'], g['z'], g['s'], g['prior_eta'], g['prior_lam'], schedule['beta'], schedule['num_undamped_iters'],
                    schedule['min_linear_iters'], schedule['eta_damping'])


def head(g, N0, F0):
    """The graph of g's first N0 poses and first F0 factors (which must join those poses)."""
    assert F0 == 0 or max(g['va'][:F0].max(), g['vb'][:F0].max()) < N0
    return dict(N=N0, va=g['va'][:F0], vb=g['vb'][:F0], z=g['z'][:F0], s=g['s'][:F0], prior_eta=g['prior_eta'][:N0], prior_lam=g['prior_lam'][:N0])


def tail(g, N0, F0, N1=None, F1=None):
    """The extend step that brings head(g, N0, F0) to head(g, N1, F1)."""
    N1, F1 = g['N'] if N1 is None else N1, len(g['va']) if F1 is None else F1
    return ('extend', dict(va=g['va'][F0:F1], vb=g['vb'][F0:F1], z=g['z'][F0:F1], s=g['s'][F0:F1],
                           prior_eta=g['prior_eta'][N0:N1] if N1 > N0 else None, prior_lam=g['prior_lam'][N0:N1] if N1 > N0 else None))


def pose_prior(mean, sigma=(1.0, 1.0, 0.5)):
    lam = np.diag(1.0 / np.asarray(sigma) ** 2)
    return lam @ mean, lam


def compose(x, z):
    """The pose z away from x in x's frame: the odometry prediction."""
    c, sn = np.cos(x[2]), np.sin(x[2])
    return np.array([x[0] + c * z[0] - sn * z[1], x[1] + sn * z[0] + c * z[1], x[2] + z[2]])


def _noisy_z(truth, a, b, rs):
    n = len(a)
    return se2_h(np.concatenate([truth[a], truth[b]], 1).reshape(n, 6), np.ones((n, 3))) + rs.normal(0, 1, (n, 3)) / SQRT_INFO


def hub_plus():
    """hub() -- pose 5 holds 9 factors -- with one more factor, (3, 5), behind its 18: the tenth entry of pose 5's adjacency list."""
    g = hub()
    assert len(g['va']) == 18 and np.bincount(np.concatenate([g['va'], g['vb']]))[5] == 9
    a, b = np.array([3]), np.array([5])
    z = _noisy_z(g['truth'], a, b, np.random.RandomState(77))
    return dict(g, va=np.concatenate([g['va'], a]).astype(np.int32), vb=np.concatenate([g['vb'], b]).astype(np.int32), z=np.concatenate([g['z'], z]),
                s=np.concatenate([g['s'], np.tile(SQRT_INFO, (1, 1))]))


def turns40_plus3():
    """chain(20, seed=2, theta0 = 40 turns + 1e-3), the graph of the `turns40` case, unchanged in its first 20 poses and 19 factors, and
    three more poses along the same circle (the same step in angle) with their odometry factors and priors made as chain() makes them."""
    theta0 = 40 * 2 * np.pi + 1e-3
    g = chain(20, seed=2, theta0=theta0)
    rs = np.random.RandomState(78)
    th = np.arange(20, 23) * 2 * np.pi * 1.5 / 20
    truth = np.concatenate([g['truth'], np.stack([5.0 * np.cos(th), 5.0 * np.sin(th), th + np.pi / 2 + theta0], 1)])
    a, b = np.arange(19, 22), np.arange(20, 23)
    z = _noisy_z(truth, a, b, rs)
    pr = [pose_prior(truth[v] + rs.normal(0, 1, 3) * np.array([0.3, 0.3, 0.1])) for v in b]
    return dict(N=23, va=np.concatenate([g['va'], a]).astype(np.int32), vb=np.concatenate([g['vb'], b]).astype(np.int32), z=np.concatenate([g['z'], z]),
                s=np.concatenate([g['s'], np.tile(SQRT_INFO, (3, 1))]), prior_eta=np.concatenate([g['prior_eta'], np.array([q[0] for q in pr])]),
                prior_lam=np.concatenate([g['prior_lam'], np.array([q[1] for q in pr])]), truth=truth)


def sweep(n=SWEEPS):
    return ('iterate', n)


# ---- the seeded schedules: name -> (starting graph, steps).  A step is ('extend', kwargs of LiveTwin.extend), ('shrink', dict(retire=,
# drop=, fold=)), ('iterate', n) (relinearising sweeps), ('plain', n), ('relin',), ('energy',), ('map',) --------------------------------

def _edge_cases():
    out = {}
    for F0, F1 in ((63, 65), (255, 257)):                    # the wave and block edges of the per-factor kernels
        g = chain(F1 + 1, seed=F1)
        out[f'f{F0}_{F1}'] = (head(g, F0 + 1, F0), [sweep(3), tail(g, F0 + 1, F0), sweep()])
    g = chain(20, seed=3)
    out['dF1'] = (head(g, 19, 18), [sweep(3), tail(g, 19, 18), sweep()])
    out['pose_only'] = (head(g, 19, 18), [sweep(3), tail(g, 19, 18, 20, 18), sweep(4), tail(g, 20, 18, 20, 19), sweep()])   # dN > 0, dF = 0
    g = ring(24, 4, seed=5)
    out['closure_only'] = (head(g, 24, 26), [sweep(3), tail(g, 24, 26), sweep()])                                              # dF > 0, dN = 0
    g = chain(10, seed=4)
    steps = []
    for i in range(1, 10):                                   # from one pose and F = 0, pose by pose
        steps += [tail(g, i, i - 1, i + 1, i), sweep(2)]
    out['from_one_pose'] = (head(g, 1, 0), steps + [sweep()])
    g = hub_plus()                                           # the whole hub(), pose 5 with its 9 factors, and a tenth onto it
    out['onto_hub'] = (head(g, 12, 18), [sweep(3), tail(g, 12, 18), sweep()])
    g = turns40_plus3()                                      # the turns40 case of lin_nonlin_cases.py itself, continued by three poses
    out['turns40_plus3'] = (head(g, 20, 19), [sweep(3), tail(g, 20, 19), sweep()])
    return out


def _shrink_cases():
    out = {}
    g = chain(12, seed=7)
    out['retire_fold'] = (g, [sweep(6), ('shrink', dict(retire=[0], drop=[], fold=True)), sweep()])
    out['retire_nofold'] = (g, [sweep(6), ('shrink', dict(retire=[0], drop=[], fold=False)), sweep()])
    g = ring(24, 4, seed=5)
    out['drop_closure'] = (g, [sweep(6), ('shrink', dict(retire=[], drop=[25], fold=True)), sweep()])
    g = chain(6, seed=8)
    steps = [sweep(4), ('shrink', dict(retire=list(range(6)), drop=[], fold=True))]
    steps += [tail(g, 0, 0, 1, 0)] + [s for i in range(1, 6) for s in (tail(g, i, i - 1, i + 1, i), sweep(2))]
    out['emptied_and_regrown'] = (g, steps + [sweep()])
    g = chain(66, seed=65)
    out['f65_63'] = (g, [sweep(4), ('shrink', dict(retire=[0, 1], drop=[], fold=True)), sweep()])
    # F 257 -> 255 with the energy asked for before and after: the partials of the energy are one per block of 256 factors, and the
    # handle keeps the buffer of the larger F
    g = chain(258, seed=257)
    out['f257_255_energy'] = (g, [sweep(4), ('energy',), ('shrink', dict(retire=[0, 1], drop=[], fold=True)), ('energy',), sweep(), ('energy',)])
    g = chain(600, seed=600)                                  # three blocks of partials down to one
    out['f599_199_energy'] = (g, [sweep(3), ('energy',), ('shrink', dict(retire=list(range(400)), drop=[], fold=True)), ('energy',), sweep(4), ('energy',)])
    return out


EDGE_CASES, SHRINK_CASES = _edge_cases(), _shrink_cases()


def window_schedule(seed=11, steps=40, hold=12, closure_every=7):
    """A fixed-lag smoother: each step appends one pose (prior at the odometry prediction from the truth of the pose before, which the
    caller of a real front-end would take from its estimate) and its odometry factor, every 7th step a closure onto a held pose, retires
    the oldest pose once more than `hold` are held, and sweeps twice.  Ids are those the handle holds at that step."""
    rs = np.random.RandomState(seed)
    th = np.arange(steps + 1) * 2 * np.pi * 1.5 / 30
    truth = np.stack([5.0 * np.cos(th), 5.0 * np.sin(th), th + np.pi / 2], 1)
    pl0 = np.diag(1 / np.full(3, 1e-3) ** 2)
    g0 = dict(N=1, va=np.zeros(0, dtype=np.int32), vb=np.zeros(0, dtype=np.int32), z=np.zeros((0, 3)), s=np.zeros((0, 3)),
              prior_eta=(pl0 @ truth[0])[None], prior_lam=pl0[None])
    out, held = [], [0]                                      # held: the truth index of every pose the handle holds, in id order
    for k in range(1, steps + 1):
        def meas(i, j):
            return se2_h(np.concatenate([truth[i], truth[j]])[None], np.ones((1, 3)))[0] + rs.normal(0, 1, 3) / SQRT_INFO
        z = [meas(k - 1, k)]
        va, vb = [len(held) - 1], [len(held)]
        pe, pl = pose_prior(compose(truth[k - 1], z[0]) + rs.normal(0, 1, 3) * np.array([0.05, 0.05, 0.02]))
        if k % closure_every == 0 and len(held) > 4:
            j = int(rs.randint(0, len(held) - 3))
            z.append(meas(held[j], k)); va.append(j); vb.append(len(held))
        held.append(k)
        out.append([('extend', dict(va=np.array(va), vb=np.array(vb), z=np.array(z), s=np.tile(SQRT_INFO, (len(z), 1)), prior_eta=pe[None], prior_lam=pl[None]))])
        if len(held) > hold:
            held.pop(0)
            out[-1].append(('shrink', dict(retire=[0], drop=[], fold=True)))
        out[-1].append(sweep(2))
    return g0, out


FUZZ_SEEDS = (0, 1, 2, 3, 4, 5)
FUZZ_CALLS = 25


def fuzz_schedule(seed):
    """(starting graph, 25 steps) drawn from extend_se2, shrink, iterate(n, relinearise=True), iterate(n), relinearise(), energy(),
    solve_map().  The structure is tracked here so that every id is legal when its step runs."""
    rs = np.random.RandomState(7000 + seed)
    g = ring(14, 2, seed=40 + seed)
    N, va, vb = g['N'], list(g['va']), list(g['vb'])
    steps = [sweep(2)]
    while len(steps) < FUZZ_CALLS:
        kind = rs.choice(['extend', 'shrink', 'iterate', 'plain', 'relin', 'energy', 'map'], p=[0.25, 0.2, 0.25, 0.08, 0.08, 0.07, 0.07])
        if kind == 'extend':
            dN, dF = int(rs.randint(0, 3)), int(rs.randint(0, 4))
            if N + dN < 2:
                dN, dF = 2, 1
            a, b = [], []
            for _ in range(dF):
                i, j = rs.choice(N + dN, 2, replace=False)
                a.append(int(i)); b.append(int(j))
            for v in range(N, N + dN):                       # a new pose hangs on something where it can
                if v not in a + b and v > 0:
                    a.append(int(rs.randint(0, v))); b.append(v)
            x = rs.normal(0, 3, (N + dN, 3)) * np.array([1, 1, 0.3])
            z = se2_h(np.concatenate([x[a], x[b]], 1).reshape(-1, 6), np.ones((len(a), 3))).reshape(-1, 3) + rs.normal(0, 0.05, (len(a), 3))
            pr = [pose_prior(x[v] + rs.normal(0, 0.1, 3)) for v in range(N, N + dN)]
            steps.append(('extend', dict(va=np.array(a, dtype=np.int64), vb=np.array(b, dtype=np.int64), z=z, s=np.tile(SQRT_INFO, (len(a), 1)),
                                         prior_eta=np.array([p[0] for p in pr]) if dN else None, prior_lam=np.array([p[1] for p in pr]) if dN else None)))
            N += dN; va += a; vb += b
        elif kind == 'shrink':
            if N < 4:
                continue
            retire = sorted(int(v) for v in rs.choice(N, int(rs.randint(0, 3)), replace=False))
            drop = sorted(int(f) for f in rs.choice(len(va), int(rs.randint(0, min(3, len(va) + 1))), replace=False)) if va else []
            fold = bool(rs.randint(0, 2))
            steps.append(('shrink', dict(retire=retire, drop=drop, fold=fold)))
            vkeep, fkeep, _, vmap, _ = plan(N, va, vb, retire, drop)
            va, vb = [int(vmap[v]) for v, k in zip(va, fkeep) if k], [int(vmap[v]) for v, k in zip(vb, fkeep) if k]
            N = int(vkeep.sum())
        elif kind in ('iterate', 'plain'):
            steps.append((kind, int(rs.randint(1, 4))))
        else:
            steps.append((kind,))
    return g, steps


def play_on_twin(t, step):
    """Runs one step on the twin; returns what the same step on the engine must return (counts, maps, a float) or None."""
    kind = step[0]
    if kind == 'extend':
        return t.extend(**step[1])
    if kind == 'shrink':
        return t.shrink(**step[1])
    if kind == 'iterate':
        return t.iterate(step[1], relinearise=True)
    if kind == 'plain':
        return t.iterate(step[1])
    if kind == 'relin':
        return int(t.relinearise_factors().sum())
    if kind == 'energy':
        return t.energy()
    if kind == 'map':
        eta, lam = t.joint()
        return np.linalg.solve(lam, eta).reshape(-1, 3) if t.N else np.zeros((0, 3))
    raise ValueError(kind)


def schedule_margin(g, steps, schedule=SCHEDULE):
    """min over every relinearising call (sweep by sweep) of the twin's margin before it."""
    t, m = live_twin(g, schedule), np.inf
    for step in steps:
        if step[0] == 'iterate':
            for _ in range(step[1]):
                m = min(m, t.margin())
                t.synchronous_iteration()
        else:
            if step[0] == 'relin':
                m = min(m, t.margin())
            play_on_twin(t, step)
    return m


def all_schedules():
    """(name, graph, flat steps, schedule) of every seeded GPU case and fuzz seed."""
    out = [(k, g, s, SCHEDULE) for k, (g, s) in {**EDGE_CASES, **SHRINK_CASES}.items()]
    g, groups = window_schedule()
    out.append(('window', g, [s for grp in groups for s in grp], SCHEDULE))
    out += [(f'fuzz{seed}', *fuzz_schedule(seed), SCHEDULE) for seed in FUZZ_SEEDS]
    out.append(('kept_state', *kept_state_case(), SCHEDULE))
    out.append(('converged_chain', converged_chain(), [sweep(60)], dict(SCHEDULE, beta=np.inf)))
    return out


def kept_state_case():
    g = ring(30, 5, seed=9)
    return head(g, 30, 31), [sweep(5), tail(g, 30, 31)]


def converged_chain():
    return chain(10, seed=6)


def g26_graph(g):
    """The starting graph of fixture G26 and the per-step appends, as steps."""
    N0, F0 = int(g['n0']), int(g['f0'])
    full = dict(N=g['prior_eta'].shape[0], va=g['edges'][:, 0].copy(), vb=g['edges'][:, 1].copy(), z=g['z'], s=g['s'], prior_eta=g['prior_eta'],
                prior_lam=g['prior_lam'])
    return full, head(full, N0, F0)


__all__ = ['LiveTwin', 'live_twin', 'MARGIN', 'EDGE_CASES', 'SHRINK_CASES', 'FUZZ_SEEDS', 'window_schedule', 'fuzz_schedule', 'play_on_twin',
           'schedule_margin', 'all_schedules', 'head', 'tail', 'sweep', 'kept_state_case', 'converged_chain', 'g26_graph', 'twin_of', 'hub_plus', 'turns40_plus3']
