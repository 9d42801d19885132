#!/usr/bin/env python3
"""Generate fixture G25 (an SE(2) pose graph relinearised by the reference's local schedule) from the reference's own classes.

    python tests/golden/make_g25.py --reference PATH_TO_THE_REFERENCE

The reference's generic path -- gbp.gbp.FactorGraph(nonlinear_factors=True) with relinearise_factors (gbp.py:64-80), the per-factor
damping of compute_all_messages (gbp.py:46-54) and Factor.compute_factor (gbp.py:267-294) -- is run as it is; what is defined here is
the measurement model alone, which the reference does not have: the planar relative-pose factor on x = (tx, ty, theta),
    h(xa, xb) = diag(s) [ c dx + s_ dy ; -s_ dx + c dy ; theta_b - theta_a ],   c, s_ = cos, sin theta_a,  (dx, dy) = xb - xa
and its Jacobian, whitened by the square-root information s so that the reference's scalar noise std is 1.  Nothing of the reference is
copied.

Graph: 30 poses on a circle of radius 5 whose heading runs through 1.5 UNWRAPPED turns (the reference wraps no angle), 29 odometry
factors and 6 random loop closures (b - a > 3), s = (10, 10, 20) with measurement noise to match; pose 0 anchored (prior sigma 1e-3),
the others with priors sigma (1, 1, 0.5) at truth + N(0, (0.3, 0.3, 0.1)).
Tag `main`: FactorGraph(eta_damping=0.4, beta=0.05, num_undamped_iters=4, min_linear_iters=2), update_all_beliefs(),
compute_all_factors(), 60 x synchronous_iteration().  Tag `b0`: beta = 0, min_linear_iters = 0, 15 sweeps, same graph.
The test `dist > beta` is discontinuous: before every sweep of `main` the generator takes min_f | |linpoint_f - means_f| - beta | and
moves on to the next seed (from 25) until the minimum over the run is >= 1e-7; `seed` and `main_margin` record what was used.  `b0`
needs no margin: there dist is either exactly 0 (first sweep: the linpoint IS the means) or far from 0.

Stored: the graph (edges, z, s, prior_eta, prior_lam, truth); per tag and sweep the relinearised mask (`_mask`, uint8), iters_since_relin
(`_iters`) and eta_damping (`_damp`) of every factor, energy() (`_energy`) and get_means() (`_means`); after the sweeps of SNAP[tag]
(`_s<k>_`) every factor's eta, lam and linpoint, both messages and the belief eta, lam; at the end of `main` joint_distribution_cov()'s
mu and the diagonal 3 x 3 blocks of sigma.  The tests never read the reference.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

from make_golden import save      # noqa: E402

N, CLOSURES, RADIUS, TURNS = 30, 6, 5.0, 1.5
SQRT_INFO = np.array([10.0, 10.0, 20.0])
MARGIN = 1e-7
RUNS = {'main': dict(beta=0.05, damping=0.4, undamped=4, minlin=2, sweeps=60),
        'b0': dict(beta=0.0, damping=0.4, undamped=4, minlin=0, sweeps=15)}
SNAP = {'main': (1, 2, 10, 60), 'b0': (1, 15)}


def meas_fn(x, s):
    c, sn = np.cos(x[2]), np.sin(x[2])
    dx, dy = x[3] - x[0], x[4] - x[1]
    return s * np.array([c * dx + sn * dy, -sn * dx + c * dy, x[5] - x[2]])


def jac_fn(x, s):
    c, sn = np.cos(x[2]), np.sin(x[2])
    dx, dy = x[3] - x[0], x[4] - x[1]
    return s[:, None] * np.array([[-c, -sn, -sn * dx + c * dy, c, sn, 0.0],
                                  [sn, -c, -c * dx - sn * dy, -sn, c, 0.0],
                                  [0.0, 0.0, -1.0, 0.0, 0.0, 1.0]])


def problem(seed):
    rs = np.random.RandomState(seed)
    th = np.arange(N) * 2 * np.pi / N * TURNS
    truth = np.stack([RADIUS * np.cos(th), RADIUS * np.sin(th), th + np.pi / 2], 1)
    edges = [(i, i + 1) for i in range(N - 1)]
    while len(edges) < N - 1 + CLOSURES:
        a, b = sorted(rs.choice(N, 2, replace=False))
        if b - a > 3 and (a, b) not in edges:
            edges.append((int(a), int(b)))
    init = truth + rs.normal(0, 1, (N, 3)) * np.array([0.3, 0.3, 0.1])
    pe, pl = np.zeros((N, 3)), np.zeros((N, 3, 3))
    for i in range(N):
        sig = np.full(3, 1e-3) if i == 0 else np.array([1.0, 1.0, 0.5])
        pl[i] = np.diag(1 / sig ** 2)
        pe[i] = pl[i] @ (truth[0] if i == 0 else init[i])
    z = np.zeros((len(edges), 3))
    for f, (a, b) in enumerate(edges):
        z[f] = meas_fn(np.concatenate([truth[a], truth[b]]), np.ones(3)) + rs.normal(0, 1, 3) / SQRT_INFO
    return dict(edges=np.array(edges, dtype=np.int32), z=z, s=np.tile(SQRT_INFO, (len(edges), 1)), prior_eta=pe, prior_lam=pl, truth=truth)


def build(gbp, p, cfg):
    g = gbp.FactorGraph(nonlinear_factors=True, eta_damping=cfg['damping'], beta=cfg['beta'], num_undamped_iters=cfg['undamped'],
                        min_linear_iters=cfg['minlin'])
    for i in range(N):
        v = gbp.VariableNode(i, 3)
        v.prior.lam, v.prior.eta = p['prior_lam'][i].copy(), p['prior_eta'][i].copy()
        g.var_nodes.append(v)
    for f, (a, b) in enumerate(p['edges']):
        s = p['s'][f]
        fac = gbp.Factor(f, [g.var_nodes[a], g.var_nodes[b]], s * p['z'][f], 1.0, meas_fn, jac_fn, None, 2, s)
        g.var_nodes[a].adj_factors.append(fac)
        g.var_nodes[b].adj_factors.append(fac)
        g.factors.append(fac)
    g.n_var_nodes, g.n_factor_nodes = N, len(g.factors)
    g.update_all_beliefs()
    g.compute_all_factors()
    return g


def run_one(gbp, p, tag):
    """(arrays, margin): margin is the run's min over sweeps and factors of | |linpoint - means| - beta |."""
    cfg = RUNS[tag]
    g = build(gbp, p, cfg)
    F, S = len(g.factors), cfg['sweeps']
    out = dict(mask=np.zeros((S, F), np.uint8), iters=np.zeros((S, F), np.int32), damp=np.zeros((S, F)), energy=np.zeros(S), means=np.zeros((S, N * 3)))
    margin = np.inf
    for it in range(S):
        for fac in g.factors:
            mu = np.concatenate([np.linalg.inv(b.lam) @ b.eta for b in fac.adj_beliefs])
            margin = min(margin, abs(np.linalg.norm(np.array(fac.linpoint) - mu) - cfg['beta']))
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
        out['map_mu'] = np.asarray(mu).reshape(N, 3)
        out['map_sigma_diag'] = np.array([sigma[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(N)])
    return out, margin


def run():
    from gbp import gbp
    seed = 25
    while True:
        p = problem(seed)
        main, margin = run_one(gbp, p, 'main')
        if margin >= MARGIN:
            break
        print(f"seed {seed}: a factor comes within {margin:.2e} of beta; next seed")
        seed += 1
    b0, _ = run_one(gbp, p, 'b0')
    arrays = dict(p, seed=np.array(seed), main_margin=np.array(margin))
    for tag, out in (('main', main), ('b0', b0)):
        cfg = RUNS[tag]
        arrays[tag + '_cfg'] = np.array([cfg['beta'], cfg['damping'], cfg['undamped'], cfg['minlin'], cfg['sweeps']], dtype=float)
        for k, v in out.items():
            arrays[f'{tag}_{k}'] = v
        print(f"{tag}: relinearisations per sweep {out['mask'].sum(1).tolist()}, energy {out['energy'][0]:.4f} -> {out['energy'][-1]:.4f}")
    print(f"seed {seed}, margin {margin:.3e}, F = {len(p['edges'])}")
    save('G25_se2_posegraph', **arrays)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import warnings
    warnings.simplefilter('ignore')
    run()
