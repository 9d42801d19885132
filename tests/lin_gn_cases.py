"""What the tests of gbp_lin_solve_map_nonlinear share (test_linear_gn_cpu.py, test_linear_gn_gpu.py): a numpy twin of the call -- the
Levenberg-Marquardt loop of include/gbp_lin.h with DENSE solves in place of the conjugate gradients --, built on NonlinTwin / Se3Twin
(their compute_factor, h and weights); the gradient of Phi formed from se2_jac / se3_jac and not from the solver's own arrays; and the
seeded cases the GPU tests run, whose accept decisions the CPU test shows to stay clear of dPhi = 0.
The twin's optimum is pinned to the reference's Gauss-Newton fixed point by fixture G29 (tests/golden/make_g29.py)."""
import numpy as np

import lin_nonlin_cases as se2
import lin_se3_cases as se3
from lin_nonlin_cases import se2_h, se2_jac
from lin_nonlin_robust_cases import HUBER, robust_twin
from lin_se3_cases import se3_h, se3_jac

NONE, STEP, GRAD, STALL = 0, 1, 2, 3                        # GBP_LIN_NLMAP_*
DIAG_FLOOR = 1e-12                                          # GN_DIAG_FLOOR (gbp_lin_gn.hpp)
DEFAULTS = dict(max_outer=50, lambda0=1e-4, lambda_up=10.0, lambda_down=0.1, lambda_min=1e-12, lambda_max=1e8, tol_step=1e-10, tol_grad=1e-8)
CLEAR = 1e-7                                                # every accept decision of a GPU case stays this clear of dPhi = 0
# Measured over every case below (test_linear_gn_cpu.py prints them and holds the constant to them): the twin's final x moves by at
# most 5.21e-8 (max-norm, relative to max(1, |x|)) between dense solves each moved by a random vector whose residual is 1e-12 |eta| and
# 1e-14 |eta| -- what inner solves stopped at cg.rel_tol 1e-12 and 1e-14 may leave; |eta| holds the anchor's 1e6 prior, so 1e-12 |eta| is
# 5e-6 against curvatures of order 1 to 100.  The bound on the device's final x is 10 x that.
X_TOL = 5.3e-7


def _model(t):
    D = t.pe.shape[1]
    return (D, se2_h, se2_jac) if D == 3 else (D, se3_h, se3_jac)


def _adj(t, x):
    return np.concatenate([x[t.va], x[t.vb]], 1)


def _weights(t):
    return getattr(t, 'w', np.ones(t.F))


def factor_energy(t, x):
    """sum_f w_f 0.5 |h(x) - diag(s) z|^2."""
    if not t.F:
        return 0.0
    _, h, _ = _model(t)
    r = h(_adj(t, x), t.s) - t.s * t.z
    return 0.5 * float(np.sum(_weights(t) * np.sum(r * r, 1)))


def gradient(t, x):
    """grad Phi(x) (N, D) from the model's Jacobian: sum_f w_f J^T (h - diag(s) z) + Lambda0 x - eta0."""
    D, h, jac = _model(t)
    g = np.einsum('vij,vj->vi', t.pl, x) - t.pe
    if t.F:
        xx = _adj(t, x)
        gf = _weights(t)[:, None] * np.einsum('fki,fk->fi', jac(xx, t.s), h(xx, t.s) - t.s * t.z)
        np.add.at(g, t.va, gf[:, :D])
        np.add.at(g, t.vb, gf[:, D:])
    return g


def joint_at(t, x):
    """Dense (eta (N D,), Lambda (N D, N D)) of the joint linearised at x, at the weights as they stand."""
    D, _, _ = _model(t)
    n = D * t.N
    eta, lam = t.pe.reshape(-1).copy(), np.zeros((n, n))
    for v in range(t.N):
        lam[D * v:D * v + D, D * v:D * v + D] = t.pl[v]
    if t.F:
        fe, fl = t.compute_factor(_adj(t, x))
        w = _weights(t)
        for f in range(t.F):
            ix = np.concatenate([np.arange(D) + D * t.va[f], np.arange(D) + D * t.vb[f]])
            eta[ix] += w[f] * fe[f]
            lam[np.ix_(ix, ix)] += w[f] * fl[f]
    return eta, lam


def solve(t, x0, perturb=0.0, **opts):
    """The loop of gbp_lin_solve_map_nonlinear from x0 (N, D).  perturb: each dense solution is moved by a vector whose residual is
    `perturb` |eta| (what an inner solve stopped at that rel_tol may leave).  Returns a dict: x, rows (outer, 5), outer, accepted,
    rejected, converged, reason, energy0, energy, grad_norm, lambda_."""
    o = dict(DEFAULTS, **opts)
    D, _, _ = _model(t)
    x = np.array(x0, dtype=float).reshape(t.N, D)
    out = dict(rows=[], grads=[], outer=0, accepted=0, rejected=0, converged=False, reason=NONE, grad_norm=0.0, grad_scale=0.0)
    lam, E = o['lambda0'], factor_energy(t, x)
    out['energy0'] = E
    if not t.N:
        out.update(converged=True, reason=GRAD)
    linear, fresh = t.F == 0, True
    rs = np.random.RandomState(5)
    for _ in range(o['max_outer'] if t.N else 0):
        if fresh:
            eta, L = joint_at(t, x)
            d = np.maximum(np.diag(L), DIAG_FLOOR)
            E = factor_energy(t, x)
            out['grad_norm'] = float(np.linalg.norm(eta - L @ x.reshape(-1)))
            out['grads'].append(out['grad_norm'])
            # what the device's residual is formed from: entries of eta + lambda D x, each rounded at its own size
            out['grad_scale'] = float(np.linalg.norm(np.abs(eta) + (0.0 if linear else lam) * d * np.abs(x.reshape(-1))))
            if o['tol_grad'] > 0 and out['grad_norm'] <= o['tol_grad']:
                out.update(converged=True, reason=GRAD)
                break
        fresh = False
        used = 0.0 if linear else lam
        A, b = L + used * np.diag(d), eta + used * d * x.reshape(-1)
        xc = np.linalg.solve(A, b)
        if perturb:
            r = rs.normal(0, 1, b.shape)
            xc = xc + np.linalg.solve(A, r * (perturb * np.linalg.norm(b) / np.linalg.norm(r)))
        xc = xc.reshape(t.N, D)
        with np.errstate(all='ignore'):
            Ec = factor_energy(t, xc)
        dx = xc - x
        dphi = (Ec - E) + float(np.sum(dx * (np.einsum('vij,vj->vi', t.pl, 0.5 * (xc + x)) - t.pe)))
        step = float(np.abs(dx).max())
        stop = o['tol_step'] > 0 and step <= o['tol_step']
        take = bool(dphi <= 0) if (stop or linear) else bool(dphi < 0)
        out['rows'].append([E, used, step, dphi, float(take)])
        out['outer'] += 1
        if take:
            x, E, fresh = xc, Ec, True
            out['accepted'] += 1
        else:
            out['rejected'] += 1
        if stop:
            out.update(converged=True, reason=STEP)
            break
        if linear:
            if take:
                out.update(converged=True, reason=GRAD, grad_norm=float(np.linalg.norm(eta - L @ x.reshape(-1))))
            break
        if take:
            lam = max(lam * o['lambda_down'], o['lambda_min'])
        else:
            if lam > o['lambda_max']:
                out['reason'] = STALL
                break
            lam *= o['lambda_up']
    out.update(x=x, energy=E, lambda_=lam, rows=np.array(out['rows']).reshape(-1, 5))
    return out


# ---- the seeded cases ---------------------------------------------------------------------------------------------------------------------

def _se2_star(leaves, seed):
    """Pose 0 joined to `leaves` others on an arc: its adjacency run holds that many factors."""
    th = np.concatenate([[0.0], np.linspace(-1.2, 1.2, leaves)])
    truth = np.stack([5.0 * np.cos(th), 5.0 * np.sin(th), th + np.pi / 2], 1)
    truth[0, :2] = 0.0
    return se2._pose_graph(truth, [(0, i) for i in range(1, leaves + 1)], seed)


def _turned(g, D, angle):
    """The graph with the loose priors' means turned: every heading (SE(2)) / every rotation vector's length along AXIS (SE(3)) but the
    anchor's is off by `angle`, so the belief means the solve starts from are rotated far from where the factors want them."""
    pe = g['prior_eta'].copy()
    for v in range(1, g['N']):
        mean = np.linalg.solve(g['prior_lam'][v], pe[v])
        if D == 3:
            mean[2] += angle
        else:
            mean[3:] += angle * se3.AXIS
        pe[v] = g['prior_lam'][v] @ mean
    return dict(g, prior_eta=pe)


def _no_factors(D, n=5, seed=3):
    rs = np.random.RandomState(seed)
    pl = np.array([np.diag(rs.uniform(0.5, 4.0, D)) + 0.1 for _ in range(n)])
    return dict(N=n, va=np.zeros(0, np.int32), vb=np.zeros(0, np.int32), z=np.zeros((0, D)), s=np.ones((0, D)), prior_eta=rs.normal(0, 2, (n, D)),
                prior_lam=pl)


def _empty(D):
    return dict(N=0, va=np.zeros(0, np.int32), vb=np.zeros(0, np.int32), z=np.zeros((0, D)), s=np.ones((0, D)), prior_eta=np.zeros((0, D)),
                prior_lam=np.zeros((0, D, D)))


# The options of the GPU comparison runs.  Every accept decision has to stay CLEAR of dPhi = 0, and close to the optimum dPhi itself goes
# to 0 (it is about -|grad|^2 / curvature): the runs therefore stop on the gradient, at a tolerance loose enough that no step with
# |dPhi| < CLEAR is ever judged (test_linear_gn_cpu.py checks it), and tol_step is off.  rel_tol / max_iters are the device's inner
# solves (the twin solves densely and ignores them): against a joint eta that holds the anchor's 1e6 prior, 1e-12 |eta| leaves the
# iterates of a long run with rejections 1e-8 from the twin's, so the compared runs solve to 1e-14.
RUN = dict(tol_grad=1e-2, tol_step=0.0, rel_tol=1e-14, max_iters=2000)
REJECT = dict(RUN, tol_grad=1e-3, lambda0=1e-9)            # a small lambda0 from a turned start: the undamped steps overshoot
CASES = {
    # name: (model, graph builder, options)
    'se2_F1': (1, lambda: se2.chain(2), RUN),
    'se2_ring258': (1, lambda: se2.ring(129, 129, seed=4), RUN),
    'se2_hub70': (1, lambda: _se2_star(70, seed=5), RUN),
    'se2_F0': (1, lambda: _no_factors(3), RUN),
    'se2_N0': (1, lambda: _empty(3), RUN),
    'se2_reject': (1, lambda: _turned(se2.chain(20, seed=2), 3, 2.5), REJECT),
    'se2_stall': (1, lambda: _turned(se2.chain(20, seed=2), 3, 2.5), dict(REJECT, lambda_max=1e-6)),
    'se3_F1': (2, lambda: se3.helix(2, seed=3, angle=0.4), RUN),
    'se3_ring258': (2, lambda: se3.ring2(129, seed=4), dict(RUN, tol_grad=2e-2)),
    'se3_star70': (2, lambda: se3.star(70, seed=5), RUN),
    'se3_F0': (2, lambda: _no_factors(6), RUN),
    'se3_N0': (2, lambda: _empty(6), RUN),
    'se3_reject': (2, lambda: _turned(se3.helix(24, seed=8), 6, -2.0), REJECT),
    'se3_stall': (2, lambda: _turned(se3.helix(24, seed=8), 6, -2.0), dict(REJECT, lambda_max=1e-6)),
}
GOLDEN_CASES = ('se2_G25', 'se3_G28')


def graph_of(name, golden=None):
    """(model, graph, options); the two fixture graphs need `golden` (conftest.golden)."""
    if name == 'se2_G25':
        return 1, se2.g25_graph(golden('G25_se2_posegraph')), dict(RUN)
    if name == 'se3_G28':
        return 2, se3.g28_graph(golden('G28_se3_posegraph'), 'main'), dict(RUN)
    model, build, opts = CASES[name]
    return model, build(), dict(opts)


def twin_of(model, g, losses=False):
    """The sweep twin of the graph (SE(2): NonlinRobustTwin, SE(3): Se3Twin) on the schedule the other nonlinear tests use."""
    if model == 1:
        return robust_twin(g, se2.SCHEDULE, losses)
    return se3.twin_of(g, se3.SCHEDULE, losses)


def min_clearance(rows):
    """min |dPhi| over the rows: how far every accept decision of a run stays from dPhi = 0 (rows with a NaN dPhi reject whatever)."""
    d = np.abs(rows[:, 3])
    return float(np.min(d[np.isfinite(d)], initial=np.inf))


def huber_closures(g, first):
    """Losses for the robust GPU cases: Huber at threshold 2 on the factors from `first` on."""
    F = len(g['va'])
    loss = np.zeros(F, dtype=np.int32)
    loss[first:] = HUBER
    return dict(g, loss=loss, thr=np.where(loss == HUBER, 2.0, 1.0))
