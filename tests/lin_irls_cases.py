"""What the tests of gbp_lin_solve_map_nonlinear_robust share (test_linear_irls_cpu.py, test_linear_irls_gpu.py): a numpy twin of the call
-- the reweight / Levenberg-Marquardt rounds of include/gbp_lin.h with DENSE solves, built on the twin of lin_gn_cases.py (its `solve`
is the round) --, and the seeded cases the GPU tests run, whose M_f the CPU test shows to stay clear of every threshold at every
reweight and whose accept decisions it shows to stay clear of dPhi = 0.
The twin's fixed point is pinned to the reference's by fixture G30 (tests/golden/make_g30.py)."""
import numpy as np

import lin_gn_cases as gn
import lin_nonlin_cases as se2
import lin_se3_cases as se3
from lin_gn_cases import _adj, _model
from lin_nonlin_robust_cases import CONSTANT, HUBER, NEW_THR, NONE

IRLS_NONE, IRLS_WEIGHTS, IRLS_MOVE = 0, 1, 2                # GBP_LIN_IRLS_*
CLEAR = 1e-7                                                # every M_f of a GPU case stays this clear of its threshold, every accept decision of dPhi = 0
GRAD_CLEAR = 1e-6                                           # ... and every tested gradient norm this clear of tol_grad (the device forms it to ~1e-8)
# Measured over every case below (test_linear_irls_cpu.py prints them and holds the constant to them): the twin's final x moves by at
# most 1.24e-7 (max-norm, relative to max(1, |x|)) between runs whose dense solves are each moved by a random vector of residual
# 1e-12 |eta| and 1e-14 |eta|.  The bound on the device's final x is 10 x that.
X_TOL = 1.3e-6


def mahalanobis(t, x):
    """M_f = |diag(s) z - h(x)| at the point x (N, D)."""
    if not t.F:
        return np.zeros(0)
    _, h, _ = _model(t)
    return np.linalg.norm(t.s * t.z - h(_adj(t, x), t.s), axis=1)


def losses_of(t):
    """(loss codes, thresholds) the handle holds: all NONE while no losses are set."""
    if getattr(t, 'robust', False):
        return t.loss, t.thr
    return np.zeros(t.F, np.int32), np.full(t.F, NEW_THR)


def weights_at(t, x):
    """(w, flag, M): Factor.robustify_loss (gbp.py:296-332) with every linpoint at x and noise variance 1."""
    loss, thr = losses_of(t)
    m = mahalanobis(t, x)
    flag = (loss != NONE) & (m > thr)
    safe = np.where(flag, m, 1.0)
    w = np.where(loss == HUBER, (2 * thr * safe - thr * thr) / safe ** 2, 1.0 / safe ** 2)
    return np.where(flag, w, 1.0), flag, m


def solve_robust(t, x0, max_rounds=20, tol_weight=1e-9, tol_move=1e-10, perturb=0.0, **lm):
    """The loop of gbp_lin_solve_map_nonlinear_robust from x0 (N, D); lm: the options of lin_gn_cases.solve, used by every round.
    Returns a dict: x, rounds, outer, accepted, rejected, converged, reason, flagged, energy0, energy, weight_change, move, rows
    (rounds + 1, 6), lm_rows (outer, 5), weights, flag, and per reweight: ws, flags, xs, margins (min |M - t| over the lossy factors),
    and per round: grads (every gradient norm a round tested)."""
    D = t.pe.shape[1]
    x = np.array(x0, dtype=float).reshape(t.N, D)
    out = dict(rounds=0, outer=0, accepted=0, rejected=0, converged=False, reason=IRLS_NONE, grad_norm=0.0, ws=[], flags=[], xs=[], margins=[], grads=[])
    rows, lm_rows = [], [np.zeros((0, 5))]
    if not t.N:
        out.update(converged=True, reason=IRLS_WEIGHTS, x=x, rows=np.zeros((1, 6)), lm_rows=lm_rows[0], weights=np.zeros(0), flag=np.zeros(0, bool), flagged=0,
                   energy0=0.0, energy=0.0, weight_change=0.0, move=0.0)
        return out
    loss, thr = losses_of(t)
    kept = getattr(t, 'w', None)
    w_old, move = None, 0.0
    try:
        for r in range(max_rounds + 1):
            w, flag, m = weights_at(t, x)
            E = 0.5 * float(np.sum(w * m * m))
            change = 0.0 if r == 0 else float(np.abs(w - w_old).max(initial=0.0))
            rows.append([E, float(flag.sum()), change, move, 0.0, 0.0])
            out['ws'].append(w); out['flags'].append(flag); out['xs'].append(x.copy())
            out['margins'].append(float(np.min(np.abs(m - thr)[loss != NONE], initial=np.inf)))
            if r >= 1:
                if tol_weight > 0 and change <= tol_weight:
                    out.update(converged=True, reason=IRLS_WEIGHTS)
                    break
                if tol_move > 0 and move <= tol_move:
                    out.update(converged=True, reason=IRLS_MOVE)
                    break
            if r == max_rounds:
                break
            t.w = w
            one = gn.solve(t, x, perturb=perturb, **lm)
            rows[-1][4:] = [float(one['outer']), float(one['reason'])]
            lm_rows.append(one['rows'])
            for k in ('outer', 'accepted', 'rejected'):
                out[k] += one[k]
            out['grad_norm'] = one['grad_norm']
            out['grads'].append(one['grads'])
            out['rounds'] += 1
            move = float(np.abs(one['x'] - x).max())
            x, w_old = one['x'], w
    finally:
        if kept is None:
            if hasattr(t, 'w'):
                del t.w
        else:
            t.w = kept
    rows = np.array(rows)
    out.update(x=x, rows=rows, lm_rows=np.concatenate(lm_rows), weights=w, flag=flag, flagged=int(flag.sum()), energy0=rows[0, 0], energy=rows[-1, 0],
               weight_change=rows[-1, 2], move=rows[-1, 3])
    return out


# ---- the seeded cases ---------------------------------------------------------------------------------------------------------------------

SIZES = (0, 1, 63, 64, 65, 255, 256, 257)                  # F: the wave edges of the flagged count and the block edges of the partials
MIXED = (HUBER, CONSTANT, NONE)


def _edges(F, closures, seed, reach):
    """A chain of F + 1 - closures poses and `closures` chords a < b with 3 < b - a <= reach."""
    n = F + 1 - closures
    rs = np.random.RandomState(3000 + seed)
    edges = [(i, i + 1) for i in range(n - 1)]
    while len(edges) < F:
        a, b = sorted(int(q) for q in rs.choice(n, 2, replace=False))
        if 3 < b - a <= reach and (a, b) not in edges:
            edges.append((a, b))
    return n, edges


def graph(model, F, seed, closures=0):
    """A chain (closures = 0) or a chain closed by chords, F factors in all; F = 0: five poses with priors only."""
    if F == 0:
        return gn._no_factors(3 if model == 1 else 6)
    n, edges = _edges(F, closures, seed, max(4, (F + 1 - closures) // 3))
    if model == 1:
        return se2._pose_graph(se2._circle(n, 1.5), edges, seed)
    return se3.pose_graph(se3._helix(np.arange(n) * 4.5 / max(n - 1, 1)), edges, seed)


def with_losses(g, model, pattern, thr_huber=2.0, thr_constant=3.0, every=3, scale=1.0):
    """Corrupts the measurement of every `every`-th factor counted from the LAST one by the offset the robust sweep tests use (times
    `scale`) and gives factor f the loss pattern[f % len(pattern)], counted from the last one too."""
    F = len(g['va'])
    if not F:
        return dict(g, loss=np.zeros(0, np.int32), thr=np.zeros(0))
    back = F - 1 - np.arange(F)
    z = g['z'].copy()
    z[back % every == 0] += scale * (np.array([1.5, -1.0, 0.4]) if model == 1 else se3.OFFSET)
    loss = np.array([pattern[b % len(pattern)] for b in back], dtype=np.int32)
    thr = np.where(loss == HUBER, thr_huber, np.where(loss == CONSTANT, thr_constant, NEW_THR))
    return dict(g, z=z, loss=loss, thr=thr)


# The options of the compared runs: as lin_gn_cases.RUN every round stops on the gradient, at a tolerance loose enough that no step with
# |dPhi| < CLEAR is judged, with tol_step off and the device's inner solves at 1e-14; four rounds at the most keep a case to seconds
# (the dense twin pays for them too) -- a run that ends with reason NONE is compared row for row like any other.
RUN = dict(gn.RUN, max_rounds=4, tol_weight=1e-9, tol_move=1e-10)


def _cases():
    out = {}
    for model, tag in ((1, 'se2'), (2, 'se3')):
        for F in SIZES:
            out[f'{tag}_chain{F}'] = (model, lambda model=model, F=F: with_losses(graph(model, F, seed=F + 1), model, MIXED), RUN)
        for F in (65, 257):
            out[f'{tag}_ring{F}'] = (model, lambda model=model, F=F: with_losses(graph(model, F, seed=F + 2, closures=6), model, MIXED), RUN)
        ring = lambda model=model: graph(model, 70, seed=9, closures=6)
        # every lossy factor flagged (Huber only, as the sweep tests: the constant weight 1 / M^2 above 1 amplifies M's rounding);
        # none flagged; and losses on a third of the factors only
        out[f'{tag}_all_flagged'] = (model, lambda ring=ring, model=model: with_losses(ring(), model, (HUBER,), 1e-3), RUN)
        out[f'{tag}_none_flagged'] = (model, lambda ring=ring, model=model: with_losses(ring(), model, (HUBER, CONSTANT), 1e6, 1e6), RUN)
        out[f'{tag}_some_lossy'] = (model, lambda ring=ring, model=model: with_losses(ring(), model, (NONE, HUBER, NONE, NONE, CONSTANT, NONE)), RUN)
    # rounds whose Levenberg-Marquardt runs reject steps (a small lambda0 from a turned start), and rounds that END IN STALL (lambda_max
    # below the lambda a rejection asks for): the loop goes on to the next reweight all the same
    rej = dict(gn.REJECT, max_rounds=3, tol_weight=1e-9, tol_move=1e-10)
    out['se3_reject'] = (2, lambda: with_losses(gn._turned(se3.helix(24, seed=8), 6, -2.0), 2, MIXED), rej)
    out['se3_stall'] = (2, lambda: with_losses(gn._turned(se3.helix(24, seed=8), 6, -2.0), 2, MIXED), dict(rej, lambda_max=1e-6))
    return out


CASES = _cases()                # name: (model, graph builder, options)


def graph_of(name):
    model, build, opts = CASES[name]
    return model, build(), dict(opts)


def split(opts):
    """(the round options, the Levenberg-Marquardt options the TWIN takes) of a case's options."""
    rounds = {k: opts[k] for k in ('max_rounds', 'tol_weight', 'tol_move') if k in opts}
    lm = {k: v for k, v in opts.items() if k not in rounds and k not in ('rel_tol', 'max_iters', 'check_every')}
    return rounds, lm


def twin_run(t, x0, opts, perturb=0.0):
    rounds, lm = split(opts)
    return solve_robust(t, x0, perturb=perturb, **rounds, **lm)


# ---- fixture G30 ----------------------------------------------------------------------------------------------------------------------------

def g30_graph(golden, tag):
    """(model, graph with losses) of fixture G30's tag: the G27 ring / the G28 helix with the losses the generator used."""
    g30 = golden('G30_nonlinear_map_robust')
    if tag == 'se2':
        g = golden('G27_se2_posegraph_robust')
        base = dict(N=g['prior_eta'].shape[0], va=g['edges'][:, 0].copy(), vb=g['edges'][:, 1].copy(), z=g['z'], s=g['s'], prior_eta=g['prior_eta'],
                    prior_lam=g['prior_lam'])
        return 1, dict(base, loss=g30['se2_loss'], thr=g30['se2_threshold'])
    g = se3.g28_graph(golden('G28_se3_posegraph'), 'main')
    return 2, dict(g, z=g30['se3_z'], loss=g30['se3_loss'], thr=g30['se3_threshold'])
