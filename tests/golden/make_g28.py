#!/usr/bin/env python3
"""Generate fixture G28 (an SE(3) pose graph relinearised, and in one tag robustified, by the reference's local schedule) from the
reference's own classes.

    python tests/golden/make_g28.py --reference PATH_TO_THE_REFERENCE

The reference's generic path -- gbp.gbp.FactorGraph(nonlinear_factors=True) with relinearise_factors (gbp.py:64-80), the per-factor
damping of compute_all_messages (gbp.py:46-54), Factor.compute_factor (gbp.py:267-294) and, for the tag `robust`, Factor.robustify_loss
(gbp.py:296-332) through synchronous_iteration(robustify=True) -- is run as it is; what is defined here is the measurement model alone,
which the reference does not have: the spatial relative-pose factor on x = (t, w), w a rotation vector, R = Exp(w),
    h(xa, xb) = diag(s) [ R_a^T (t_b - t_a) ; Log(R_a^T R_b) ]
and its Jacobian (include/gbp_lin.h, GBP_LIN_MODEL_SE3_BETWEEN), whitened by the square-root information s so that the reference's
scalar noise std is 1.  It is written here one factor at a time with closed forms and scipy-free numpy, apart from the vectorised twin
of tests/lin_se3_cases.py, which the CPU test then pins to this run.  Nothing of the reference is copied.

Graph: 30 poses on a helix (radius 5, pitch 0.25 per pose) about the tilted axis (1, 2, 2) / 3, the rotation vector w = angle * axis
running CONTINUOUSLY from 0 to 4.5 rad -- past pi; nothing is wrapped --, 29 odometry factors and 6 random loop closures (b - a > 3,
relative rotation below 2.5 rad), s = (10, 10, 10, 20, 20, 20) with measurement noise to match; pose 0 anchored (prior sigma 1e-3), the
others with priors sigma (1, 1, 1, 0.5, 0.5, 0.5) at truth + N(0, (0.3, 0.3, 0.3, 0.1, 0.1, 0.1)).
Tag `main`: FactorGraph(eta_damping=0.4, beta=0.05, num_undamped_iters=4, min_linear_iters=2), update_all_beliefs(),
compute_all_factors(), 60 x synchronous_iteration().  Tag `b0`: beta = 0, min_linear_iters = 0, 15 sweeps.  Tag `robust`: `main` with
the measurements of three closures (factors 29, 31, 33) corrupted by OFFSET and the Huber loss at threshold 4 on all six closures,
60 x synchronous_iteration(robustify=True).
The tests `dist > beta` and `M > t` are discontinuous: before every sweep of `main` and `robust` the generator takes
min_f | |linpoint_f - means_f| - beta | and (robust) min_f | M_f - t_f | at the linpoints as they stand, and moves on to the next seed
(from 28) until every minimum over the runs is >= 1e-7; `seed`, `main_margin`, `robust_margin` (the distance one) and
`robust_loss_margin` record what was used.  `b0` needs no margin: there dist is exactly 0 (first sweep) or far from 0.

Stored: the graph (edges, z, s, prior_eta, prior_lam, truth), for `robust` its own z (`robust_z`), loss (0 none, 1 huber) and threshold
per factor; per tag and sweep the relinearised mask (`_mask`, uint8), iters_since_relin (`_iters`), eta_damping (`_damp`), energy()
(`_energy`), get_means() (`_means`) and for `robust` the weight (`_w`) and robust_flag (`_flag`) of every factor; after the sweeps of
SNAP[tag] (`_s<k>_`) every factor's eta and lam AS THE REFERENCE HOLDS THEM (for `robust`: times the weight) and linpoint, both
messages and the belief eta, lam; at the end of `main` joint_distribution_cov()'s mu and the diagonal 6 x 6 blocks of sigma.  The tests
never read the reference.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

from make_golden import save      # noqa: E402

N, CLOSURES, RADIUS, PITCH, ANGLE = 30, 6, 5.0, 0.25, 4.5
AXIS = np.array([1.0, 2.0, 2.0]) / 3.0
SQRT_INFO = np.array([10.0, 10.0, 10.0, 20.0, 20.0, 20.0])
MARGIN = 1e-7
RUNS = {'main': dict(beta=0.05, damping=0.4, undamped=4, minlin=2, sweeps=60, robust=False),
        'b0': dict(beta=0.0, damping=0.4, undamped=4, minlin=0, sweeps=15, robust=False),
        'robust': dict(beta=0.05, damping=0.4, undamped=4, minlin=2, sweeps=60, robust=True)}
SNAP = {'main': (1, 2, 10, 60), 'b0': (1, 15), 'robust': (1, 2, 10, 60)}
OUTLIERS, OFFSET = (29, 31, 33), np.array([1.5, -1.0, 0.8, 0.3, -0.2, 0.25])
HUBER_THR = 4.0


def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def coeffs(th):
    """sin th / th, (1 - cos th) / th^2 (by the half angle: no cancellation), (th - sin th) / th^3 (series below 0.2, where it cancels)."""
    if th == 0.0:
        return 1.0, 0.5, 1.0 / 6
    a, b = np.sin(th) / th, 0.5 * (np.sin(0.5 * th) / (0.5 * th)) ** 2
    t = th * th
    c = sum((-t) ** k / FACT[2 * k + 3] for k in range(7)) if th < 0.2 else (th - np.sin(th)) / th ** 3
    return a, b, c


FACT = np.cumprod([1.0] + list(range(1, 20)))


def exp_so3(w):
    a, b, _ = coeffs(np.linalg.norm(w))
    K = hat(w)
    return np.eye(3) + a * K + b * K @ K


def log_so3(E):
    v = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    n = np.linalg.norm(v)
    th = np.arctan2(n, 0.5 * (np.trace(E) - 1.0))
    return v if n == 0.0 else th / n * v


def jr(w):
    _, b, c = coeffs(np.linalg.norm(w))
    K = hat(w)
    return np.eye(3) - b * K + c * K @ K


def jr_inv(p):
    th = np.linalg.norm(p)
    K = hat(p)
    t = th * th
    if th < 0.2:                                             # 1/th^2 - cot(th/2) / (2 th) cancels: its series (Bernoulli numbers)
        c = 1.0 / 12 + t * (1.0 / 720 + t * (1.0 / 30240 + t * (1.0 / 1209600 + t * (1.0 / 47900160 + t * 691.0 / 1307674368000.0))))
    else:
        c = 1 / t - 1.0 / (2 * th * np.tan(0.5 * th))
    return np.eye(3) + 0.5 * K + c * K @ K


def meas_fn(x, s):
    x = np.asarray(x, dtype=float)                          # the reference holds a linpoint as a list
    Q = exp_so3(x[3:6]).T
    return s * np.concatenate([Q @ (x[6:9] - x[0:3]), log_so3(Q @ exp_so3(x[9:12]))])


def jac_fn(x, s):
    x = np.asarray(x, dtype=float)
    Q = exp_so3(x[3:6]).T
    E = Q @ exp_so3(x[9:12])
    u, Ji, Ja = Q @ (x[6:9] - x[0:3]), jr_inv(log_so3(E)), jr(x[3:6])
    J = np.zeros((6, 12))
    J[0:3, 0:3], J[0:3, 3:6], J[0:3, 6:9] = -Q, hat(u) @ Ja, Q
    J[3:6, 3:6], J[3:6, 9:12] = -Ji @ E.T @ Ja, Ji @ jr(x[9:12])
    return s[:, None] * J


def problem(seed):
    rs = np.random.RandomState(seed)
    ang = np.arange(N) * ANGLE / (N - 1)
    e1 = np.cross(AXIS, [1.0, 0.0, 0.0]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(AXIS, e1)
    pos = RADIUS * (np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2) + PITCH * np.arange(N)[:, None] * AXIS
    truth = np.concatenate([pos, ang[:, None] * AXIS], 1)
    edges = [(i, i + 1) for i in range(N - 1)]
    while len(edges) < N - 1 + CLOSURES:
        a, b = sorted(rs.choice(N, 2, replace=False))
        if b - a > 3 and ang[b] - ang[a] < 2.5 and (a, b) not in edges:
            edges.append((int(a), int(b)))
    init = truth + rs.normal(0, 1, (N, 6)) * np.array([0.3, 0.3, 0.3, 0.1, 0.1, 0.1])
    pe, pl = np.zeros((N, 6)), np.zeros((N, 6, 6))
    for i in range(N):
        sig = np.full(6, 1e-3) if i == 0 else np.array([1.0, 1.0, 1.0, 0.5, 0.5, 0.5])
        pl[i] = np.diag(1 / sig ** 2)
        pe[i] = pl[i] @ (truth[0] if i == 0 else init[i])
    z = np.zeros((len(edges), 6))
    for f, (a, b) in enumerate(edges):
        z[f] = meas_fn(np.concatenate([truth[a], truth[b]]), np.ones(6)) + rs.normal(0, 1, 6) / SQRT_INFO
    assert np.linalg.norm(z[:, 3:], axis=1).max() < 2.6
    return dict(edges=np.array(edges, dtype=np.int32), z=z, s=np.tile(SQRT_INFO, (len(edges), 1)), prior_eta=pe, prior_lam=pl, truth=truth)


def build(gbp, p, cfg, z):
    g = gbp.FactorGraph(nonlinear_factors=True, eta_damping=cfg['damping'], beta=cfg['beta'], num_undamped_iters=cfg['undamped'],
                        min_linear_iters=cfg['minlin'])
    for i in range(N):
        v = gbp.VariableNode(i, 6)
        v.prior.lam, v.prior.eta = p['prior_lam'][i].copy(), p['prior_eta'][i].copy()
        g.var_nodes.append(v)
    for f, (a, b) in enumerate(p['edges']):
        s = p['s'][f]
        loss = 'huber' if cfg['robust'] and f >= N - 1 else None
        fac = gbp.Factor(f, [g.var_nodes[a], g.var_nodes[b]], s * z[f], 1.0, meas_fn, jac_fn, loss, HUBER_THR, s)
        g.var_nodes[a].adj_factors.append(fac)
        g.var_nodes[b].adj_factors.append(fac)
        g.factors.append(fac)
    g.n_var_nodes, g.n_factor_nodes = N, len(g.factors)
    g.update_all_beliefs()
    g.compute_all_factors()
    return g


def run_one(gbp, p, tag, z):
    """(arrays, distance margin, loss margin): the run's minima over sweeps and factors of | |linpoint - means| - beta | and of
    | M - t | over the factors with a loss."""
    cfg = RUNS[tag]
    g = build(gbp, p, cfg, z)
    F, S = len(g.factors), cfg['sweeps']
    out = dict(mask=np.zeros((S, F), np.uint8), iters=np.zeros((S, F), np.int32), damp=np.zeros((S, F)), energy=np.zeros(S), means=np.zeros((S, N * 6)))
    if cfg['robust']:
        out.update(w=np.zeros((S, F)), flag=np.zeros((S, F), np.uint8))
    margin = lmargin = np.inf
    for it in range(S):
        for fac in g.factors:
            mu = np.concatenate([np.linalg.inv(b.lam) @ b.eta for b in fac.adj_beliefs])
            margin = min(margin, abs(np.linalg.norm(np.array(fac.linpoint) - mu) - cfg['beta']))
            if fac.loss is not None:
                m = np.linalg.norm(fac.measurement - meas_fn(np.asarray(fac.linpoint, dtype=float), *fac.args))
                lmargin = min(lmargin, abs(m - fac.mahalanobis_threshold))
        if cfg['robust']:
            g.synchronous_iteration(local_relin=True, robustify=True)
            out['w'][it] = [fac.gauss_noise_var / fac.adaptive_gauss_noise_var for fac in g.factors]
            out['flag'][it] = [fac.robust_flag for fac in g.factors]
        else:
            g.synchronous_iteration()
        out['iters'][it] = [fac.iters_since_relin for fac in g.factors]
        out['mask'][it] = out['iters'][it] == 0
        out['damp'][it] = [fac.eta_damping for fac in g.factors]
        out['energy'][it] = g.energy()
        out['means'][it] = g.get_means()
        if it + 1 in SNAP[tag]:
            k = f's{it + 1}_'
            out[k + 'feta'] = np.array([fac.factor.eta for fac in g.factors])
            out[k + 'flam'] = np.array([fac.factor.lam for fac in g.factors])
            out[k + 'linpoint'] = np.array([np.asarray(fac.linpoint, dtype=float) for fac in g.factors])
            for side, name in enumerate('ab'):
                out[k + 'msg_eta_' + name] = np.array([fac.messages[side].eta for fac in g.factors])
                out[k + 'msg_lam_' + name] = np.array([fac.messages[side].lam for fac in g.factors])
            out[k + 'bel_eta'] = np.array([v.belief.eta for v in g.var_nodes])
            out[k + 'bel_lam'] = np.array([v.belief.lam for v in g.var_nodes])
    if tag == 'main':
        mu, sigma = g.joint_distribution_cov()
        out['map_mu'] = np.asarray(mu).reshape(N, 6)
        out['map_sigma_diag'] = np.array([sigma[6 * i:6 * i + 6, 6 * i:6 * i + 6] for i in range(N)])
    return out, margin, lmargin


def run():
    from gbp import gbp
    seed = 28
    while True:
        p = problem(seed)
        zr = p['z'].copy()
        zr[list(OUTLIERS)] += OFFSET
        assert np.linalg.norm(zr[:, 3:], axis=1).max() < 3.0
        main, margin, _ = run_one(gbp, p, 'main', p['z'])
        rob, rmargin, lmargin = run_one(gbp, p, 'robust', zr)
        if min(margin, rmargin, lmargin) >= MARGIN:
            break
        print(f"seed {seed}: within {min(margin, rmargin):.2e} of beta, {lmargin:.2e} of a loss threshold; next seed")
        seed += 1
    b0, _, _ = run_one(gbp, p, 'b0', p['z'])
    flags = rob['flag'][:, N - 1:].astype(bool)
    assert flags.any() and (flags[1:] != flags[:-1]).any() and not flags[-1].all(), "no closure is flagged, no flag changes, or all end flagged"
    assert not rob['flag'][:, :N - 1].any() and np.all(rob['w'][:, :N - 1] == 1.0)
    F = len(p['edges'])
    arrays = dict(p, seed=np.array(seed), main_margin=np.array(margin), robust_margin=np.array(rmargin), robust_loss_margin=np.array(lmargin),
                  robust_z=zr, loss=np.array([0] * (N - 1) + [1] * (F - N + 1), dtype=np.int32), threshold=np.full(F, HUBER_THR))
    for tag, out in (('main', main), ('b0', b0), ('robust', rob)):
        cfg = RUNS[tag]
        arrays[tag + '_cfg'] = np.array([cfg['beta'], cfg['damping'], cfg['undamped'], cfg['minlin'], cfg['sweeps']], dtype=float)
        for k, v in out.items():
            arrays[f'{tag}_{k}'] = v
        print(f"{tag}: relinearisations per sweep {out['mask'].sum(1).tolist()}, energy {out['energy'][0]:.4f} -> {out['energy'][-1]:.4f}")
    print(f"robust: flagged per sweep {rob['flag'].sum(1).tolist()}")
    print(f"seed {seed}, margins {margin:.3e} {rmargin:.3e} {lmargin:.3e}, F = {F}, max |w| {np.linalg.norm(p['truth'][:, 3:], axis=1).max():.3f}")
    save('G28_se3_posegraph', **arrays)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import warnings
    warnings.simplefilter('ignore')
    run()
