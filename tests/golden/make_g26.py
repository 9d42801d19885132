#!/usr/bin/env python3
"""Generate fixture G26 (an SE(2) pose graph GROWN while the reference's local schedule relinearises it) from the reference's own classes.

    python tests/golden/make_g26.py --reference PATH_TO_THE_REFERENCE

The graph, the measurement model (meas_fn / jac_fn) and the schedule are G25's (make_g25.py: 30 poses on 1.5 unwrapped turns, s = (10, 10,
20), FactorGraph(eta_damping=0.4, beta=0.05, num_undamped_iters=4, min_linear_iters=2)); nothing of the reference is copied.  What is
new is the order of events.  The run starts from the first 8 poses and their 7 odometry factors (update_all_beliefs(),
compute_all_factors()).  Then, 22 times: two synchronous_iteration()s, then ONE append -- var_nodes.append of the next pose,
factors.append / adj_factors.append of its odometry factor and, for 5 of the poses (CLOSE_AT), of a loop closure from a random pose more
than 3 back -- followed by update_all_beliefs() (gbp.py:56-58) and compute_factor() on the NEW factors only (gbp.py:267-294), which
linearises them at their adjacent belief means; a new pose's belief is its prior.  20 more sweeps follow the last append.
As for G25 the generator takes, before every sweep, min_f | |linpoint_f - means_f| - beta | and moves on to the next seed (from 26) until
the minimum over the run is >= 1e-7; `seed` and `margin` record what was used.

Stored: the whole graph in append order (edges, z, s, prior_eta, prior_lam, truth); n0, f0 (the start) and `appends` (one row per append:
the sweep it follows, N and F after it); per sweep the number of factors (`sweep_f`) and, padded to the final F, the relinearised mask
(`mask`, uint8), iters_since_relin (`iters`) and eta_damping (`damp`), and energy(); at the end get_means(), every factor's eta, lam and
linpoint, both messages, the belief eta, lam, and joint_distribution_cov()'s mu and the diagonal 3 x 3 blocks of its sigma.  The tests
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
from make_g25 import N, SQRT_INFO, RADIUS, TURNS, MARGIN, meas_fn, jac_fn      # noqa: E402

N0 = 8
CLOSE_AT = (12, 16, 20, 24, 28)
CFG = dict(beta=0.05, damping=0.4, undamped=4, minlin=2)
SWEEPS_BETWEEN, SWEEPS_AFTER = 2, 20


def problem(seed):
    """The graph in append order: the N0 - 1 odometry factors of the start, then per pose its odometry factor and, at CLOSE_AT, a closure."""
    rs = np.random.RandomState(seed)
    th = np.arange(N) * 2 * np.pi / N * TURNS
    truth = np.stack([RADIUS * np.cos(th), RADIUS * np.sin(th), th + np.pi / 2], 1)
    edges = [(i, i + 1) for i in range(N0 - 1)]
    appends = []                                             # (pose, number of factors it brings)
    for k in range(N0, N):
        edges.append((k - 1, k))
        if k in CLOSE_AT:
            edges.append((int(rs.randint(0, k - 3)), k))
        appends.append(len(edges))
    init = truth + rs.normal(0, 1, (N, 3)) * np.array([0.3, 0.3, 0.1])
    pe, pl = np.zeros((N, 3)), np.zeros((N, 3, 3))
    for i in range(N):
        sig = np.full(3, 1e-3) if i == 0 else np.array([1.0, 1.0, 0.5])
        pl[i] = np.diag(1 / sig ** 2)
        pe[i] = pl[i] @ (truth[0] if i == 0 else init[i])
    z = np.zeros((len(edges), 3))
    for f, (a, b) in enumerate(edges):
        z[f] = meas_fn(np.concatenate([truth[a], truth[b]]), np.ones(3)) + rs.normal(0, 1, 3) / SQRT_INFO
    return dict(edges=np.array(edges, dtype=np.int32), z=z, s=np.tile(SQRT_INFO, (len(edges), 1)), prior_eta=pe, prior_lam=pl, truth=truth), appends


def add_pose(gbp, g, p, i):
    v = gbp.VariableNode(i, 3)
    v.prior.lam, v.prior.eta = p['prior_lam'][i].copy(), p['prior_eta'][i].copy()
    g.var_nodes.append(v)


def add_factor(gbp, g, p, f):
    a, b = p['edges'][f]
    s = p['s'][f]
    fac = gbp.Factor(f, [g.var_nodes[a], g.var_nodes[b]], s * p['z'][f], 1.0, meas_fn, jac_fn, None, 2, s)
    g.var_nodes[a].adj_factors.append(fac)
    g.var_nodes[b].adj_factors.append(fac)
    g.factors.append(fac)
    return fac


def run_one(gbp, p, f_after):
    g = gbp.FactorGraph(nonlinear_factors=True, eta_damping=CFG['damping'], beta=CFG['beta'], num_undamped_iters=CFG['undamped'],
                        min_linear_iters=CFG['minlin'])
    for i in range(N0):
        add_pose(gbp, g, p, i)
    for f in range(N0 - 1):
        add_factor(gbp, g, p, f)
    g.n_var_nodes, g.n_factor_nodes = len(g.var_nodes), len(g.factors)
    g.update_all_beliefs()
    g.compute_all_factors()
    F, S = len(p['edges']), SWEEPS_BETWEEN * len(f_after) + SWEEPS_AFTER
    out = dict(mask=np.zeros((S, F), np.uint8), iters=np.zeros((S, F), np.int32), damp=np.zeros((S, F)), energy=np.zeros(S), sweep_f=np.zeros(S, np.int32),
               appends=np.zeros((len(f_after), 3), np.int32))
    margin, it = np.inf, 0

    def sweeps(n):
        nonlocal margin, it
        for _ in range(n):
            for fac in g.factors:
                mu = np.concatenate([np.linalg.inv(b.lam) @ b.eta for b in fac.adj_beliefs])
                margin = min(margin, abs(np.linalg.norm(np.array(fac.linpoint) - mu) - CFG['beta']))
            g.synchronous_iteration()
            f = len(g.factors)
            out['sweep_f'][it] = f
            out['iters'][it, :f] = [fac.iters_since_relin for fac in g.factors]
            out['mask'][it, :f] = out['iters'][it, :f] == 0
            out['damp'][it, :f] = [fac.eta_damping for fac in g.factors]
            out['energy'][it] = g.energy()
            it += 1

    for k, f1 in enumerate(f_after):
        sweeps(SWEEPS_BETWEEN)
        add_pose(gbp, g, p, N0 + k)
        new = [add_factor(gbp, g, p, f) for f in range(len(g.factors), f1)]
        g.n_var_nodes, g.n_factor_nodes = len(g.var_nodes), len(g.factors)
        g.update_all_beliefs()
        for fac in new:
            fac.compute_factor()
        out['appends'][k] = (it, len(g.var_nodes), len(g.factors))
    sweeps(SWEEPS_AFTER)
    out['means'] = g.get_means()
    out['feta'] = np.array([fac.factor.eta for fac in g.factors])
    out['flam'] = np.array([fac.factor.lam for fac in g.factors])
    out['linpoint'] = np.array([np.asarray(fac.linpoint, dtype=float) for fac in g.factors])
    for side, name in enumerate('ab'):
        out['msg_eta_' + name] = np.array([fac.messages[side].eta for fac in g.factors])
        out['msg_lam_' + name] = np.array([fac.messages[side].lam for fac in g.factors])
    out['bel_eta'] = np.array([v.belief.eta for v in g.var_nodes])
    out['bel_lam'] = np.array([v.belief.lam for v in g.var_nodes])
    mu, sigma = g.joint_distribution_cov()
    out['map_mu'] = np.asarray(mu).reshape(N, 3)
    out['map_sigma_diag'] = np.array([sigma[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(N)])
    return out, margin


def run():
    from gbp import gbp
    seed = 26
    while True:
        p, f_after = problem(seed)
        out, margin = run_one(gbp, p, f_after)
        if margin >= MARGIN:
            break
        print(f"seed {seed}: a factor comes within {margin:.2e} of beta; next seed")
        seed += 1
    print(f"relinearisations per sweep {out['mask'].sum(1).tolist()}, energy {out['energy'][0]:.4f} -> {out['energy'][-1]:.4f}")
    print(f"seed {seed}, margin {margin:.3e}, F = {len(p['edges'])}")
    cfg = np.array([CFG['beta'], CFG['damping'], CFG['undamped'], CFG['minlin'], len(out['energy'])], dtype=float)
    save('G26_se2_posegraph_grown', **p, **out, seed=np.array(seed), margin=np.array(margin), cfg=cfg, n0=np.array(N0), f0=np.array(N0 - 1))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import warnings
    warnings.simplefilter('ignore')
    run()
