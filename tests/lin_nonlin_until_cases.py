"""Shared by tests/test_linear_nonlinear_until_cpu.py and tests/test_linear_nonlinear_until_gpu.py: a numpy model of
gbp_lin_iterate_until_nonlinear (include/gbp_lin.h) over the twins of lin_nonlin_cases.py / lin_nonlin_robust_cases.py -- rows (step,
energy, MAP distance), both counts per sweep, the deciding sweep and the reason for a tolerance, with and without SETTLED -- and the
cases the GPU tests run: the existing builders at the sizes where a kernel can go wrong, one ring with F = 257 (an edge of the
256-thread relinearise and energy blocks), and a pose graph without factors."""
import numpy as np

from lin_nonlin_cases import CASES as PLAIN_CASES, SCHEDULE, hub, ring
from lin_nonlin_robust_cases import HUBER, MARGIN, MIXED, robust_twin, with_losses
from lin_until_cases import STOP_MAP, STOP_NONE, STOP_STEP, TOL, TRACE_ENERGY, TRACE_MAP, decide, step_of, usable_sweep  # noqa: F401 (re-exported)

UNTIL_SETTLED = 4
MAX_S = 40                      # sweeps of a model run that looks for a deciding sweep (lin_until_cases.usable_sweep looks no further)

NAMES = ['F1', 'hub9', 'turns40', 'chain63', 'chain64', 'chain65', 'ring63', 'ring64', 'ring65', 'ring129', 'ring257', 'undamped0', 'undamped1',
         'undamped4', 'minlin5', 'beta0', 'nofactors']
FREEZE = ['hub9', 'ring65', 'ring257', 'undamped4']          # the cases the freeze tests use
# (case, the sweep whose step is the tolerance, where the call stops without SETTLED, where with it)
BETA0_TOL = 0.3                 # generous for `beta0`: met from sweep 4 on, not by sweeps 1 to 3 (only the first sweep relinearises nothing)
SETTLED_PAIRS = [('hub9', 12, 12, 14), ('undamped4', 22, 22, 23), ('minlin5', 56, 56, 59)]


def no_factors():
    g = hub()
    return dict(g, va=np.zeros(0, dtype=np.int32), vb=np.zeros(0, dtype=np.int32), z=np.zeros((0, 3)), s=np.zeros((0, 3)))


def case(name, robust=False):
    """(graph, schedule) of a case; robust: with the mixed losses of with_losses (one Huber factor for F1; none without factors)."""
    if name == 'nofactors':
        return no_factors(), SCHEDULE
    if name == 'ring257':
        g, sched = ring(251, 6, seed=257), SCHEDULE
    else:
        _, build, sched = next(c for c in PLAIN_CASES if c[0] == name)
        g = build()
    if robust:
        g = with_losses(g, (HUBER,) if name == 'F1' else MIXED)
    return g, sched


def twin(g, sched):
    """The robust twin serves both: without losses its weights stay 1."""
    return robust_twin(g, sched)


def settled_decide(step, dist, tol_step, tol_map, relin_count, settled):
    """The rule of the call: lin_until_cases.decide, except that under SETTLED a sweep that relinearised anything decides nothing."""
    if settled and relin_count != 0:
        return STOP_NONE
    return decide(step, dist, tol_step, tol_map)


def run_model(t, max_iters, tol_step=0.0, tol_map=0.0, x_map=None, robustify=False, settled=False, margins=None):
    """The call on a twin: (rows (iters, 3), relin counts, robust counts, iters, reason).  The twin is left after the deciding sweep.
    margins: a list that receives (robust margin, distance margin) of the twin BEFORE every sweep run."""
    rows, rc, fc, reason = [], [], [], STOP_NONE
    for _ in range(max_iters):
        if margins is not None:
            margins.append((t.robust_margin(), t.margin()))
        old = t.mu.copy()
        out = t.synchronous_iteration(True, robustify)
        relin, flags = out if robustify else (out, np.zeros(t.F, dtype=bool))
        step = step_of(t.mu, old)
        dist = None if x_map is None else float(np.linalg.norm(t.mu - x_map))
        rows.append((step, t.energy(), np.nan if dist is None else dist))
        rc.append(int(relin.sum())); fc.append(int(flags.sum()))
        reason = settled_decide(step, dist, tol_step, tol_map, rc[-1], settled)
        if reason != STOP_NONE:
            break
    return np.array(rows).reshape(-1, 3), np.array(rc, dtype=np.int32), np.array(fc, dtype=np.int32), len(rows), reason


def freeze_sweep(name, robust):
    """(s, tol_step, rows, relin counts, robust counts, worst robust margin, worst distance margin up to s) of a freeze case: s the
    first usable sweep of the step column (lin_until_cases.usable_sweep: no multiple of 3 or 8, strictly below every earlier step)."""
    g, sched = case(name, robust)
    margins = []
    rows, rc, fc, _, _ = run_model(twin(g, sched), MAX_S, robustify=robust, margins=margins)
    s = usable_sweep(rows[:, 0])
    if s is None:
        return None, None, rows, rc, fc, None, None
    m = np.array(margins[:s])
    return s, float(rows[s - 1, 0]), rows, rc, fc, float(m[:, 0].min()), float(m[:, 1].min())
