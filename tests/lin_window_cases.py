"""Random sliding-window schedules for a live linear handle (include/gbp_lin.h): the generator and host model shared by
tests/test_linear_window_fuzz_cpu.py and tests/test_linear_window_fuzz_gpu.py.

window_schedule(seed, D) draws a base graph and N_STEPS steps; a step is 2 to 4 calls drawn as lin_fuzz_cases.random_schedule draws
them (its helpers are imported, nothing of it is changed), then one extend, then one shrink with a random retire list, a random drop list
and either fold.  A shrink renumbers, so the generator follows the graph itself (lin_shrink_cases.plan) and every later call is drawn for
the handle the calls before it left.  WindowModel is lin_fuzz_cases.LinModel with the one further call, on lin_shrink_cases.shrink().
SEEDS are the seeds on which tests/test_linear_window_fuzz_cpu.py proves the model alone healthy and clear of the loss thresholds at
every step for every d.  Host-only: numpy, nothing of the device."""
import numpy as np

from lin_fuzz_cases import LinModel, Op, Schedule, _pairs, _piece
from lin_map_cases import random_priors
from lin_robust_cases import mixed_losses
from lin_shrink_cases import plan, shrink

N_STEPS = 6
DIMS = (1, 3, 6)
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7)


def window_schedule(seed, D):
    """Schedule(seed, D, base, steps, None): steps are lists of Op, each ending with an 'extend' and a 'shrink'."""
    rs = np.random.RandomState(8000 + 100 * seed + D)
    N = int(rs.randint(2, 31))
    F = int(rs.randint(0, 70))
    on = bool(rs.randint(0, 2))
    base = _piece(rs, D, F, 'mixed' if on else 'none')
    pe, pl = random_priors(rs, N, D)
    va, vb = _pairs(rs, N, F, False)
    base.update(N=N, va=va, vb=vb, pe=pe, pl=pl, damping=float(rs.choice([0.0, 0.4])), set_losses=on)
    steps = []
    for k in range(N_STEPS):
        ops = []
        for _ in range(int(rs.randint(2, 5))):
            kind = ('iterate', 'iterate', 'robustify', 'set_robust', 'solve_map', 'marginals', 'joint', 'update_beliefs')[rs.randint(0, 8)]
            if kind == 'iterate' or (kind == 'robustify' and not on) or (kind == 'marginals' and N == 0):
                ops.append(Op('iterate', dict(n=int(rs.randint(1, 5)), robustify=bool(rs.randint(0, 2)) and on, refused=False)))
            elif kind == 'robustify':
                ops.append(Op('robustify', {}))
            elif kind == 'set_robust':
                how = ('mixed', 'mixed', 'none', 'clear')[rs.randint(0, 4)]
                loss = mixed_losses(rs, F) if how == 'mixed' else [None] * F if how == 'none' else None
                ops.append(Op('set_robust', dict(loss=loss, thr=1.0 + 2.0 * rs.rand(F))))
                on = loss is not None
            elif kind == 'solve_map':
                ops.append(Op('solve_map', dict(warm=bool(rs.randint(0, 2)))))
            elif kind == 'marginals':
                ids = rs.permutation(N)[:int(rs.randint(1, min(N, 5) + 1))]
                ops.append(Op('marginals', dict(ids=[int(v) for v in ids], joint=bool(rs.randint(0, 2)))))
            elif kind == 'joint':
                ops.append(Op('joint', dict(x=rs.randn(N, D))))
            else:
                ops.append(Op('update_beliefs', {}))
        # the extend: the window's new poses and their factors
        dN, dF = int(rs.randint(0, 5)), int(rs.randint(0, 70))
        if N + dN < 2:
            dF = 0
        piece = _piece(rs, D, dF, ('absent', 'mixed', 'mixed', 'none')[rs.randint(0, 4)])
        ppe, ppl = random_priors(rs, dN, D)
        a, b = _pairs(rs, N + dN, dF, hub=dF >= 16 and rs.rand() < 0.3)
        piece.update(va=a, vb=b, pe=ppe, pl=ppl)
        ops.append(Op('extend', piece))
        if piece['loss'] is not None and dF:
            on = True
        N, va, vb = N + dN, np.concatenate([va, a]), np.concatenate([vb, b])
        F = len(va)
        # the shrink: anything from nothing to a few variables and factors, either fold
        u = rs.rand()
        retire = rs.permutation(N)[:int(rs.randint(0, 5))] if u >= 0.1 else np.zeros(0, dtype=np.int64)
        drop = rs.permutation(F)[:int(rs.randint(0, 9))] if u < 0.1 or u >= 0.2 else np.zeros(0, dtype=np.int64)
        ops.append(Op('shrink', dict(retire=retire.astype(np.int64), drop=drop.astype(np.int64), fold=bool(rs.randint(0, 2)))))
        vkeep, fkeep, _, vmap, _ = plan(N, va, vb, retire, drop)
        N, va, vb = int(vkeep.sum()), vmap[va[fkeep]].astype(np.int64), vmap[vb[fkeep]].astype(np.int64)
        F = len(va)
        steps.append(ops)
    return Schedule(seed, D, base, steps, None)


class WindowModel(LinModel):
    """LinModel plus gbp_lin_shrink: the oracle shrunk by lin_shrink_cases.shrink(); the header's state as after an extend (every array
    of the handle is replaced, a solve is forgotten); `maps` holds what the call returns."""

    def apply(self, op):
        if op.kind != 'shrink':
            return super().apply(op)
        a = op.args
        if len(a['retire']) or len(a['drop']):
            self.o, vmap, fmap = shrink(self.o, a['retire'], a['drop'], a['fold'])
            self.arrays, self.stale = ('extend' if self.losses_on else None), False
            self.solved, self.first_solver_pending, self.robustified_alone, self.grown = False, True, False, True
        else:
            vmap, fmap = np.arange(self.o.N, dtype=np.int32), np.arange(self.o.F, dtype=np.int32)
        self.maps = (vmap, fmap)
        self.last = 'shrink'
        return None
