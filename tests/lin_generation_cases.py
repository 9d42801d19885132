"""Shared by tests/test_linear_generation_gpu.py and tools/lin_generation_digest.py: one fixed schedule per kind of live linear handle
-- create, 3 sweeps, extend, 3 sweeps, shrink (retire with fold, and drop), 3 sweeps, extend, shrink -- at the smallest shapes that reach
every branch of a rebuild (gbp_amd/csrc/gbp_lin_generation.hpp): every per-factor array of every group is re-strided and gathered, a
handle whose losses were cleared drops its stale arrays and later gets fresh ones, one extend has dN = 0 and one dF = 0, and one schedule
takes F over 256 and back (the energy's partials grow once and stay).  A `Player` plays a schedule on an engine and on the numpy model of
its kind alike (RobustOracle / grow / shrink of lin_robust_cases.py, lin_extend_cases.py, lin_shrink_cases.py; LiveTwin of
lin_nonlin_live_cases.py).  Host-only: nothing here touches the device until a Player is given an engine."""
import numpy as np

from lin_extend_cases import generic_fc, grow, random_priors, robust_parts
from lin_map_cases import random_pairs
from lin_nonlin_cases import SCHEDULE, chain
from lin_nonlin_live_cases import head, live_twin, pose_prior, tail
from lin_robust_cases import RobustOracle
from lin_shrink_cases import robust_oracle, shrink
from oracle.linear_oracle import LinearOracleBatched

KINDS = ('plain', 'robust', 'cleared', 'plain_f256', 'se2')
DOFS = dict(plain=6, robust=3, cleared=1, plain_f256=1, se2=3)
SWEEPS = 3


def _factors(rs, kind, D, va, vb, losses):
    """The extend step of a linear kind: plain factors with their constants, or (J, z, sigma, loss, threshold)."""
    dF = len(va)
    if kind.startswith('plain'):
        fe, fl, fc = generic_fc(rs, D, dF)
        return dict(va=va, vb=vb, fe=fe, fl=fl, fc=fc)
    J, z, sigma, loss, thr = robust_parts(rs, D, dF, losses)
    return dict(va=va, vb=vb, J=J, z=z, sigma=sigma, loss=loss if losses else None, threshold=thr)


def schedule(kind):
    """(start, steps): `start` makes the model of the kind; a step is ('sweep', n), ('extend', kwargs), ('shrink', dict(retire=, drop=,
    fold=)) or ('clear',).  Ids are those the handle holds at that step."""
    none = np.zeros(0, dtype=np.int64)
    if kind == 'se2':
        g = chain(12, seed=21)
        one = pose_prior(np.array([0.5, -0.25, 0.1]))
        steps = [('sweep', SWEEPS), tail(g, 8, 7, 10, 9), ('sweep', SWEEPS), ('shrink', dict(retire=[0], drop=[4], fold=True)), ('sweep', SWEEPS),
                 ('extend', dict(va=none, vb=none, z=np.zeros((0, 3)), s=np.zeros((0, 3)), prior_eta=one[0][None], prior_lam=one[1][None])),   # dF = 0
                 ('shrink', dict(retire=[2], drop=[0], fold=False))]
        return (lambda: live_twin(head(g, 8, 7), SCHEDULE)), steps
    D = DOFS[kind]
    rs = np.random.RandomState(2700 + D + 10 * KINDS.index(kind))
    N0, F0, dF1 = (12, 250, 12) if kind == 'plain_f256' else (8, 14, 5)      # plain_f256: F 250 -> 262 -> under 256 again
    va, vb = random_pairs(rs, N0, F0)
    if kind.startswith('plain'):
        fe, fl, fc = generic_fc(rs, D, F0)
        pe, pl = random_priors(rs, N0, D)
        start = lambda: LinearOracleBatched(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=0.4)
    else:
        o0 = robust_oracle(rs, D, N0, va, vb, 0.4, 'on')
        start = lambda: RobustOracle(o0.va, o0.vb, o0.J, o0.z, o0.sigma, o0.pe, o0.pl, o0.loss, o0.thr, eta_damping=0.4)
    dN1 = 0 if kind == 'plain_f256' else 2                                  # plain_f256: the extend with dN = 0
    ext1 = _factors(rs, kind, D, *random_pairs(rs, N0 + dN1, dF1), losses=kind == 'robust')
    ext1['pe'], ext1['pl'] = random_priors(rs, dN1, D) if dN1 else (None, None)
    N1 = N0 + dN1 - 1
    if kind == 'robust':                                                    # the extend with dF = 0
        ext2 = _factors(rs, kind, D, none, none, losses=True)
        ext2['pe'], ext2['pl'] = random_priors(rs, 2, D)
    else:                                                                   # plain: dN = 0 again; cleared: new factors bring losses back
        dN2 = 0 if kind == 'plain' else 1
        ext2 = _factors(rs, kind, D, *random_pairs(rs, N1 + dN2, 3), losses=True)
        ext2['pe'], ext2['pl'] = random_priors(rs, dN2, D) if dN2 else (None, None)
    steps = [('sweep', SWEEPS)] + ([('clear',)] if kind == 'cleared' else [])
    steps += [('extend', ext1), ('sweep', SWEEPS), ('shrink', dict(retire=[1], drop=[0, 5], fold=True)), ('sweep', SWEEPS), ('extend', ext2),
              ('shrink', dict(retire=[0], drop=[2], fold=False))]
    return start, steps


def engine_of(model, kind):
    """The engine that holds what `model` holds, before any sweep."""
    from gbp_amd.linear import LinearEngine
    if kind == 'se2':
        m = model
        return LinearEngine.se2_pose_graph(m.va, m.vb, m.z, m.s, m.pe, m.pl, SCHEDULE['beta'], SCHEDULE['num_undamped_iters'],
                                           SCHEDULE['min_linear_iters'], eta_damping=SCHEDULE['eta_damping'])
    if kind.startswith('plain'):
        return LinearEngine(model.va, model.vb, model.fe, model.fl, model.pe, model.pl, factor_const=model.fc, eta_damping=model.damping)
    e = LinearEngine(model.va, model.vb, model.fe0, model.fl0, model.pe, model.pl, factor_const=model.fc0, eta_damping=model.damping)
    e.set_robust(model.loss, model.thr, model.sigma ** 2)
    return e


class Player:
    """Plays steps on an engine and, where one is given, on the model of the kind: after play() both hold the same graph."""

    def __init__(self, kind, engine, model=None):
        self.kind, self.e, self.m = kind, engine, model
        self.live = kind in ('robust', 'cleared')                           # losses are set: sweeps robustify, weights() is an observable
        if kind != 'se2':
            engine.update_all_beliefs()
            if model is not None:
                model.update_all_beliefs()

    def play(self, step):
        what, e, m = step[0], self.e, self.m
        if what == 'sweep':
            if self.kind == 'se2':
                e.iterate(step[1], relinearise=True)
                return m.iterate(step[1], relinearise=True) if m is not None else None
            e.iterate(step[1], robustify=self.live)
            return m.iterate(step[1], **(dict(robustify=True) if self.live else {})) if m is not None else None
        if what == 'clear':
            e.set_robust(None)
            self.live = False
            if m is not None:
                m.loss, m.w, m.flag = [None] * m.F, np.ones(m.F), np.zeros(m.F, dtype=bool)
                m.fe, m.fl = m.fe0.copy(), m.fl0.copy()
            return None
        if what == 'shrink':
            k = step[1]
            maps = e.shrink(k['retire'], k['drop'], fold=k['fold'])
            if m is not None:
                if self.kind == 'se2':
                    m.shrink(**k)
                else:
                    self.m = shrink(m, k['retire'], k['drop'], k['fold'])[0]
            return maps
        k = step[1]                                                         # extend
        if self.kind == 'se2':
            e.extend_se2(k['va'], k['vb'], k['z'], k['s'], k['prior_eta'], k['prior_lam'])
            return m.extend(**k) if m is not None else None
        if 'fe' in k:
            e.extend(k['va'], k['vb'], k['fe'], k['fl'], k['pe'], k['pl'], factor_const=k['fc'])
        else:
            s2 = k['sigma'] ** 2
            e.extend(k['va'], k['vb'], np.einsum('fmi,fm->fi', k['J'], k['z']) / s2[:, None], np.einsum('fmi,fmj->fij', k['J'], k['J']) / s2[:, None, None],
                     k['pe'], k['pl'], factor_const=0.5 * np.einsum('fm,fm->f', k['z'], k['z']) / s2, loss=k['loss'], threshold=k['threshold'],
                     noise_var=s2)
            self.live = self.live or (k['loss'] is not None and len(k['va']) > 0)
        if m is not None:
            self.m = grow(m, **k)
        return None

    def cycle(self):
        """One extend and one shrink that bring the engine back to the sizes it has: a new variable with two factors onto it, retired."""
        e, D = self.e, self.e.D
        N, rs = e.N, np.random.RandomState(5)
        a, b = np.array([0, N]), np.array([N, 1])
        if self.kind == 'se2':
            pr = pose_prior(np.array([0.1, 0.2, 0.05]))
            e.extend_se2(a, b, 0.1 * rs.randn(2, 3), np.ones((2, 3)), pr[0][None], pr[1][None])
        else:
            fe, fl, fc = generic_fc(rs, D, 2)
            e.extend(a, b, fe, fl, *random_priors(rs, 1, D), factor_const=fc)
        e.shrink([N], [], fold=False)

    def observables(self):
        """Every getter of the handle's kind, in a fixed order."""
        e = self.e
        out = list(e.messages()) + list(e.beliefs()) + [e.get_means(), np.array([e.energy()])]
        if self.live:
            out += list(e.weights())
        if self.kind == 'se2':
            out += list(e.linearisation())
        return out
