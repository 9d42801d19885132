"""Random call schedules for a live linear handle (include/gbp_lin.h): the shared generator and host model of
tests/test_linear_fuzz_cpu.py and tests/test_linear_fuzz_gpu.py.

random_schedule(seed, D) draws a base graph and N_STEPS steps from np.random.RandomState; a step is 2 to 5 calls -- sweeps with and
without robustify, robustify alone, set_robust (mixed, all NONE, NULL), solve_map (cold / warm) with map_mean and map_distance,
marginals, joint_matvec / joint_eta, update_all_beliefs -- closed by one extend.  A call is legal only for the handle the calls before it
left, so the generator follows the handle's sizes and the header's state (losses set, a solve behind it) itself; LinModel follows them a
second time, on a RobustOracle grown by lin_extend_cases.grow(), and predicts the solvers' results from the dense joint at its own
weights.  healthy() and threshold_margin() are the two conditions under which an engine and the oracle must agree; tally() says which of
the orders nobody chose by hand a run has met.  Host-only: numpy, nothing of the device."""
import collections

import numpy as np

from lin_extend_cases import grow, robust_parts
from lin_map_cases import random_priors
from lin_robust_cases import RobustOracle, dense_weighted_joint, mixed_losses

N_STEPS = 6
SEEDS = tuple(range(16))
DIMS = (1, 3, 6)
EMPTY_SEED = 0                                               # this seed starts from N = F = 0
MARGIN = 1e-6                                                # 1000 x the comparison tolerance: see threshold_margin()
GBP_EINVAL, GBP_ESTATE = -1, -5
SHAPES = ('starts_empty', 'extend_losses_after_clear', 'extend_losses_never_had', 'extend_none_list_with_losses',
          'set_robust_on_arrays_of_an_extend', 'extend_after_solve', 'extend_after_marginals', 'warm_solve_first_after_extend',
          'marginals_2_batches_first_after_extend', 'joint_first_after_extend', 'robustify_alone_then_solve', 'F_across_64_with_losses',
          'F_across_256_with_losses', 'N_across_32', 'extend_dN0', 'extend_dF0', 'extend_empty', 'hub_gains_8')
REFUSALS = ('extend: id out of range', 'extend: a == b', 'extend: loss with threshold 0', 'marginals: repeated id',
            'robustify without losses', 'map_mean without a solve')
REFUSAL_CODE = dict(zip(REFUSALS, (GBP_EINVAL, GBP_EINVAL, GBP_EINVAL, GBP_EINVAL, GBP_ESTATE, GBP_ESTATE)))

Op = collections.namedtuple('Op', 'kind args')
Schedule = collections.namedtuple('Schedule', 'seed D base steps refuse')   # steps: lists of Op, each ending with an 'extend'


def _piece(rs, D, dF, losses):
    """dF factors as the engine takes them (fe, fl, fc) and as the oracle does (J, z, sigma); loss: a list of dF names or None."""
    J, z, sigma, loss, thr = robust_parts(rs, D, dF)
    s2 = sigma ** 2
    return dict(J=J, z=z, sigma=sigma, thr=thr, fe=np.einsum('fmi,fm->fi', J, z) / s2[:, None],
                fl=np.einsum('fmi,fmj->fij', J, J) / s2[:, None, None], fc=0.5 * np.einsum('fm,fm->f', z, z) / s2,
                loss=loss if losses == 'mixed' else [None] * dF if losses == 'none' else None)


def _pairs(rs, N, F, hub):
    """random_pairs; with `hub`, half of the factors (alternating sides) join one variable."""
    if not F:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    a = rs.randint(0, N, F)
    b = (a + 1 + rs.randint(0, N - 1, F)) % N
    if hub:
        h = int(rs.randint(0, N))
        for f in range(0, F, 2):
            other = a[f] if a[f] != h else b[f]
            a[f], b[f] = (h, other) if f % 4 else (other, h)
    return a.astype(np.int64), b.astype(np.int64)


def random_schedule(seed, D):
    """The schedule of (seed, D): deterministic.  base: dict(N, va, vb, pe, pl, damping, set_losses, + _piece); steps: N_STEPS lists of
    Op; refuse: (step, name) -- before that step's first call the refusal `name` of REFUSALS applies to the handle."""
    rs = np.random.RandomState(7000 + 100 * seed + D)
    N = 0 if seed == EMPTY_SEED else int(rs.randint(0, 31))
    F = 0 if N < 2 else int(rs.randint(0, 70))
    on = bool(rs.randint(0, 2))
    base = _piece(rs, D, F, 'mixed' if on else 'none')
    pe, pl = random_priors(rs, N, D)
    va, vb = _pairs(rs, N, F, False)
    base.update(N=N, va=va, vb=vb, pe=pe, pl=pl, damping=float(rs.choice([0.0, 0.4])), set_losses=on)
    steps, start = [], []                                    # start[k]: (N, losses on, solved) before step k
    solved = False
    for k in range(N_STEPS):
        start.append((N, on, solved))
        ops = []
        for _ in range(int(rs.randint(2, 6))):
            kind = ('iterate', 'iterate', 'robustify', 'set_robust', 'solve_map', 'marginals', 'joint', 'update_beliefs')[rs.randint(0, 8)]
            if kind == 'iterate':
                n, want = int(rs.randint(1, 5)), bool(rs.randint(0, 2))
                if want and not on and rs.rand() >= 0.15:    # mostly legal; sometimes the refused call
                    want = False
                ops.append(Op('iterate', dict(n=n, robustify=want, refused=want and not on)))
            elif kind == 'robustify':
                if on:
                    ops.append(Op('robustify', {}))
                else:
                    ops.append(Op('iterate', dict(n=int(rs.randint(1, 5)), robustify=False, refused=False)))
            elif kind == 'set_robust':
                how = ('mixed', 'mixed', 'none', 'clear')[rs.randint(0, 4)]
                loss = mixed_losses(rs, F) if how == 'mixed' else [None] * F if how == 'none' else None
                ops.append(Op('set_robust', dict(loss=loss, thr=1.0 + 2.0 * rs.rand(F))))
                on = loss is not None
            elif kind == 'solve_map':
                ops.append(Op('solve_map', dict(warm=bool(rs.randint(0, 2)))))
                solved = True
            elif kind == 'marginals' and N > 0:
                ids = rs.permutation(N)[:int(rs.randint(1, min(N, 5) + 1))]
                ops.append(Op('marginals', dict(ids=[int(v) for v in ids], joint=bool(rs.randint(0, 2)))))
            elif kind == 'joint':
                ops.append(Op('joint', dict(x=rs.randn(N, D))))
            else:
                ops.append(Op('update_beliefs', {}))
        # the extend that closes the step
        u = rs.rand()
        dN = int(rs.randint(0, 5))
        dF = int(rs.randint(0, 70))
        if u < 0.08:
            dN = dF = 0
        elif u < 0.16:
            dF = 0
        elif u < 0.24:
            dN = 0
        if seed == EMPTY_SEED and k == 0:                    # the empty handle's first step grows it
            dN, dF = max(dN, 2), max(dF, 1)
        if N + dN < 2:
            dF = 0
        how = ('absent', 'mixed', 'mixed', 'none')[rs.randint(0, 4)]
        piece = _piece(rs, D, dF, how)
        ppe, ppl = random_priors(rs, dN, D)
        a, b = _pairs(rs, N + dN, dF, hub=dF >= 16 and rs.rand() < 0.3)
        piece.update(va=a, vb=b, pe=ppe, pl=ppl)
        ops.append(Op('extend', piece))
        if dN + dF:
            solved = False
        if piece['loss'] is not None and dF:
            on = True
        N, F = N + dN, F + dF
        steps.append(ops)
    # one refusal per schedule: the kind this (seed, D) prefers, at the first step before which it applies
    refuse = None
    for j in range(len(REFUSALS)):
        name = REFUSALS[(3 * seed + DIMS.index(D) + j) % len(REFUSALS)]
        for k, (n0, on0, solved0) in enumerate(start):
            ok = {'marginals: repeated id': n0 > 0, 'robustify without losses': not on0, 'map_mean without a solve': not solved0}.get(name, True)
            if ok:
                refuse = (k, name)
                break
        if refuse:
            break
    return Schedule(seed, D, base, steps, refuse)


class LinModel:
    """The handle on the host: a RobustOracle (a handle without losses is one whose losses are all None) plus the three booleans of
    include/gbp_lin.h -- losses_on (gbp_lin_set_robust / gbp_lin_extend), has_beliefs, solved (gbp_lin_solve_map .. the next growing
    extend).  apply(op) returns the GBP_E* code the header gives the call, or None where it is accepted.  `given` keeps the arrays as the
    engine received them piece by piece; `events` what tally() counts; `margins` the threshold margin before every robustify."""

    def __init__(self, s):
        b = s.base
        self.D = s.D
        self.o = RobustOracle(b['va'], b['vb'], b['J'], b['z'], b['sigma'], b['pe'], b['pl'], b['loss'] if b['set_losses'] else None,
                              b['thr'], eta_damping=b['damping'])
        self.o.update_all_beliefs()
        self.losses_on, self.has_beliefs, self.solved = bool(b['set_losses']), True, False
        self.given = {k: b[k] for k in ('va', 'vb', 'fe', 'fl', 'fc', 'pe', 'pl')}
        self.events, self.margins = [], []
        # where the handle's loss arrays come from (None: it has none), whether they are stale (cleared, still allocated)
        self.arrays, self.stale, self.ever = ('set_robust' if b['set_losses'] else None), False, bool(b['set_losses'])
        self.first_solver_pending, self.robustified_alone, self.last, self.grown = False, False, None, False

    N = property(lambda self: self.o.N)
    F = property(lambda self: self.o.F)

    # ---- the header's rules ----
    def _robustify(self):
        self.margins.append(threshold_margin(self))
        self.o.robustify_all_factors()

    def _note_solver(self, what):
        if self.first_solver_pending:
            self.events.append('first:' + what)
        self.first_solver_pending = False

    def apply(self, op):
        o, a = self.o, op.args
        code = None
        if op.kind == 'iterate':
            if a['robustify'] and not self.losses_on:
                code = GBP_ESTATE
            else:
                for _ in range(a['n']):
                    if a['robustify']:
                        self._robustify()
                    o.synchronous_iteration(False)
                self.robustified_alone = False
        elif op.kind == 'robustify':
            if not self.losses_on:
                code = GBP_ESTATE
            else:
                self._robustify()
                self.robustified_alone = self.grown
        elif op.kind == 'set_robust':
            if a['loss'] is not None and self.arrays == 'extend':
                self.events.append('set_robust_on_arrays_of_an_extend')
            o.loss = [None] * o.F if a['loss'] is None else list(a['loss'])
            if a['loss'] is not None:
                o.thr = np.array(a['thr'], dtype=float)
                self.arrays, self.stale, self.ever = self.arrays or 'set_robust', False, True
            else:
                self.stale = self.arrays is not None
            o.w, o.flag = np.ones(o.F), np.zeros(o.F, dtype=bool)
            o.fe, o.fl = o.fe0.copy(), o.fl0.copy()
            self.losses_on = a['loss'] is not None
            self.robustified_alone = False
        elif op.kind == 'solve_map':
            self._note_solver('warm_solve' if a['warm'] else 'cold_solve')
            if self.robustified_alone:
                self.events.append('robustify_alone_then_solve')
            self.solved = True
        elif op.kind == 'marginals':
            self._note_solver('marginals_2_batches' if -(-len(a['ids']) * self.D // 8) >= 2 else 'marginals')
        elif op.kind == 'joint':
            self._note_solver('joint')
        elif op.kind == 'update_beliefs':
            o.update_all_beliefs()
        elif op.kind == 'extend':
            self._extend(a)
        else:
            raise ValueError(op.kind)
        self.last = op.kind if code is None else None
        return code

    def _extend(self, a):
        o = self.o
        dN, dF = len(a['pe']), len(a['va'])
        brings = a['loss'] is not None and dF > 0
        if not dN and not dF:
            self.events.append('extend_empty')
            return
        ev = self.events
        if not dN:
            ev.append('extend_dN0')
        if not dF:
            ev.append('extend_dF0')
        if self.last in ('solve_map', 'marginals'):
            ev.append('extend_after_solve' if self.last == 'solve_map' else 'extend_after_marginals')
        if brings and not self.losses_on:
            if self.stale:
                ev.append('extend_losses_after_clear')
            if not self.ever:
                ev.append('extend_losses_never_had')
        if brings and self.losses_on and all(l is None for l in a['loss']):
            ev.append('extend_none_list_with_losses')
        on_after = self.losses_on or brings
        if on_after and o.F // 64 != (o.F + dF) // 64:
            ev.append('F_across_64_with_losses')
        if on_after and o.F // 256 != (o.F + dF) // 256:
            ev.append('F_across_256_with_losses')
        if o.N < 32 <= o.N + dN:
            ev.append('N_across_32')
        if dF and np.bincount(np.concatenate([a['va'], a['vb']])).max() >= 8:
            ev.append('hub_gains_8')
        # gbp_lin_extend: the old factors keep their losses while losses are set and are at NONE otherwise (the model cleared them
        # already); the new ones get `loss`, or NONE
        self.o = grow(o, a['va'], a['vb'], pe=a['pe'], pl=a['pl'], J=a['J'], z=a['z'], sigma=a['sigma'],
                      loss=a['loss'] if brings else None, threshold=a['thr'])
        for k in ('va', 'vb', 'fe', 'fl', 'fc', 'pe', 'pl'):
            self.given[k] = np.concatenate([self.given[k], a[k]])
        self.losses_on = on_after
        self.arrays, self.stale = ('extend' if on_after else None), False      # every array of the handle is replaced
        self.ever = self.ever or on_after
        self.solved, self.first_solver_pending, self.robustified_alone, self.grown = False, True, False, True

    # ---- what the solvers must return: the dense joint at the model's weights ----
    def joint(self):
        return dense_weighted_joint(self.o, self.o.w)

    def map_mean(self):
        eta, lam = self.joint()
        return np.linalg.solve(lam, eta).reshape(self.N, self.D) if self.N else np.zeros((0, self.D))

    def marginals(self, ids):
        """(sigma (M, d, d), sigma_joint (M d, M d)) of Lambda_joint^-1."""
        D = self.D
        S = np.linalg.inv(self.joint()[1])
        idx = np.concatenate([np.arange(v * D, (v + 1) * D) for v in ids])
        return np.array([S[v * D:(v + 1) * D, v * D:(v + 1) * D] for v in ids]), S[np.ix_(idx, idx)]


def healthy(model):
    """Every belief Lambda positive definite and every |mean| <= 1e6: the oracle's own arithmetic is then far from breaking down."""
    o = model.o
    if not o.N:
        return True
    return bool(np.all(np.isfinite(o.mu)) and np.abs(o.mu).max() <= 1e6 and np.linalg.eigvalsh(o.bel_lam).min() > 0.0)


def threshold_margin(model):
    """min over the factors with a loss of |M - t| / t at the current means: a constant-loss weight jumps at M = t, so engine and
    oracle may legitimately disagree on a factor whose M is within rounding of t."""
    o = model.o
    has = np.array([l is not None for l in o.loss], dtype=bool)
    if not has.any():
        return np.inf
    return float(np.min(np.abs(o.mahalanobis()[has] - o.thr[has]) / o.thr[has]))


def is_legal(model, op):
    """The header's rules for one call on the handle as `model` describes it: None, or the rule broken."""
    a, N, F = op.args, model.N, model.F
    if op.kind == 'iterate':
        return 'robustify without losses' if a['robustify'] and not model.losses_on else None if a['n'] >= 0 else 'negative count'
    if op.kind == 'robustify':
        return None if model.losses_on else 'robustify without losses'
    if op.kind == 'set_robust':
        if a['loss'] is None:
            return None
        if len(a['loss']) != F or len(a['thr']) != F:
            return 'set_robust: F each'
        return None if all(l is None or t > 0 for l, t in zip(a['loss'], a['thr'])) else 'set_robust: threshold'
    if op.kind == 'marginals':
        ids = np.asarray(a['ids'], dtype=np.int64)
        if not ids.size or ids.min() < 0 or ids.max() >= N:
            return 'marginals: id out of range'
        return None if np.unique(ids).size == ids.size else 'marginals: repeated id'
    if op.kind == 'joint':
        return None if a['x'].shape == (N, model.D) else 'joint: x is not N x d'
    if op.kind == 'map_mean':
        return None if model.solved else 'map_mean without a solve'
    if op.kind == 'extend':
        dN, dF, D = len(a['pe']), len(a['va']), model.D
        if len(a['vb']) != dF or a['fe'].shape != (dF, 2 * D) or a['fl'].shape != (dF, 2 * D, 2 * D) or a['fc'].shape != (dF,):
            return 'extend: dF each'
        if dF and (min(a['va'].min(), a['vb'].min()) < 0 or max(a['va'].max(), a['vb'].max()) >= N + dN):
            return 'extend: id out of range'
        if np.any(a['va'] == a['vb']):
            return 'extend: a == b'
        if a['loss'] is not None and any(l is not None and not t > 0 for l, t in zip(a['loss'], a['thr'])):
            return 'extend: loss with threshold 0'
    return None


def refused_variant(rs, model, name=None):
    """One call the header refuses on the handle as it stands: (name, Op, code).  name None: drawn among those that apply."""
    D, N = model.D, model.N
    applies = [r for r in REFUSALS if {'marginals: repeated id': N > 0, 'robustify without losses': not model.losses_on,
                                       'map_mean without a solve': not model.solved}.get(r, True)]
    if name is None:
        name = applies[rs.randint(0, len(applies))]
    assert name in applies, name
    if name.startswith('extend'):                            # a legal small step -- two variables and a factor between them -- spoilt
        piece = _piece(rs, D, 1, 'mixed')
        piece['loss'] = ['huber']
        pe, pl = random_priors(rs, 2, D)
        piece.update(va=np.array([N]), vb=np.array([N + 1]), pe=pe, pl=pl)
        if name == 'extend: id out of range':
            piece['vb'] = np.array([N + 2])
        elif name == 'extend: a == b':
            piece['vb'] = np.array([N])
        else:
            piece['thr'] = np.zeros(1)
        op = Op('extend', piece)
    elif name == 'marginals: repeated id':
        v = int(rs.randint(0, N))
        op = Op('marginals', dict(ids=[v, v], joint=False))
    elif name == 'robustify without losses':
        op = Op('robustify', {})
    else:
        op = Op('map_mean', {})
    return name, op, REFUSAL_CODE[name]


def tally(schedule, model):
    """How often a run -- `model` after it followed `schedule` -- met each shape of SHAPES and each refusal of REFUSALS."""
    out = dict.fromkeys(SHAPES + REFUSALS, 0)
    out['starts_empty'] = int(schedule.base['N'] == 0 and len(schedule.base['va']) == 0)
    first = {'first:warm_solve': 'warm_solve_first_after_extend', 'first:marginals_2_batches': 'marginals_2_batches_first_after_extend',
             'first:joint': 'joint_first_after_extend'}
    for ev in model.events:
        ev = first.get(ev, ev)
        if ev in out:
            out[ev] += 1
    if schedule.refuse is not None:
        out[schedule.refuse[1]] += 1
    return out
