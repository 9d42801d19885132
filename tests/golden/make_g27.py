#!/usr/bin/env python3
"""Generate fixture G27 (the SE(2) pose graph of G25 with outlier loop closures and robust losses, relinearised AND robustified by the
reference's own schedule) from the reference's own classes.

    python tests/golden/make_g27.py --reference PATH_TO_THE_REFERENCE

The reference's generic path -- gbp.gbp.FactorGraph(nonlinear_factors=True) run through synchronous_iteration(local_relin=True,
robustify=True) (gbp.py:86-92): robustify_all_factors (Factor.robustify_loss gbp.py:296-332, which evaluates meas_fn at Factor.linpoint,
gbp.py:309), relinearise_factors (gbp.py:64-80), compute_all_messages with the per-factor damping (gbp.py:46-54), update_all_beliefs --
is run as it is; what is defined here is the measurement model alone, as in make_g25.py.  Nothing of the reference is copied.

Graph: the G25 graph (make_g25.problem: 30 poses, 29 odometry factors, 6 loop closures, s = (10, 10, 20)); the measurements of three
closures (factors 29, 31, 33) are corrupted by (1.5, -1.0, 0.4), so they are outliers.  Losses: huber at threshold 2 on closures 29, 30,
31; constant at threshold 3 on 32, 33 and at threshold 60 on 34; none on the odometry.
FactorGraph(eta_damping=0.4, beta=0.05, num_undamped_iters=4, min_linear_iters=2), update_all_beliefs(), compute_all_factors(),
SWEEPS x synchronous_iteration(local_relin=True, robustify=True).
Both tests of a sweep are discontinuous -- `M > t` of robustify_loss and `dist > beta` of relinearise_factors -- so before every sweep
the generator takes min_f | M_f - t_f | over the factors with a loss (M at the linpoint as it stands) and min_f | dist_f - beta |, and
moves on to the next seed (from 27) until both minima over the run are >= 1e-7; `seed`, `robust_margin` and `dist_margin` record what
was used.  Asserted: some factor is flagged at some sweep, some factor with a loss is never flagged, and some flag changes during the run.

Stored: the graph (edges, z, s, prior_eta, prior_lam, truth), loss (0 none, 1 huber, 2 constant) and threshold per factor, cfg; per
sweep the weight gauss_noise_var / adaptive_gauss_noise_var (`w`) and robust_flag (`flag`) of every factor, the relinearised mask
(`mask`), iters_since_relin (`iters`), eta_damping (`damp`), energy() (`energy`) and get_means() (`means`); after the sweeps of SNAP
(`s<k>_`) every factor's eta and lam AS THE REFERENCE HOLDS THEM (the nominal factor times its weight) and linpoint, both messages and
the belief eta, lam.  The tests never read the reference.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

from make_golden import save      # noqa: E402
from make_g25 import N, problem   # noqa: E402

MARGIN = 1e-7
CFG = dict(beta=0.05, damping=0.4, undamped=4, minlin=2, sweeps=30)
SNAP = (1, 2, 10, 30)
OUTLIERS, OFFSET = (29, 31, 33), np.array([1.5, -1.0, 0.4])
LOSSES = {29: ('huber', 2.0), 30: ('huber', 2.0), 31: ('huber', 2.0), 32: ('constant', 3.0), 33: ('constant', 3.0), 34: ('constant', 60.0)}
CODE = {None: 0, 'huber': 1, 'constant': 2}


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


def build(gbp, p):
    g = gbp.FactorGraph(nonlinear_factors=True, eta_damping=CFG['damping'], beta=CFG['beta'], num_undamped_iters=CFG['undamped'],
                        min_linear_iters=CFG['minlin'])
    for i in range(N):
        v = gbp.VariableNode(i, 3)
        v.prior.lam, v.prior.eta = p['prior_lam'][i].copy(), p['prior_eta'][i].copy()
        g.var_nodes.append(v)
    for f, (a, b) in enumerate(p['edges']):
        s = p['s'][f]
        loss, thr = LOSSES.get(f, (None, 2.0))
        fac = gbp.Factor(f, [g.var_nodes[a], g.var_nodes[b]], s * p['z'][f], 1.0, meas_fn, jac_fn, loss, thr, s)
        g.var_nodes[a].adj_factors.append(fac)
        g.var_nodes[b].adj_factors.append(fac)
        g.factors.append(fac)
    g.n_var_nodes, g.n_factor_nodes = N, len(g.factors)
    g.update_all_beliefs()
    g.compute_all_factors()
    return g


def run_one(gbp, p):
    """(arrays, robust margin, distance margin) of one run."""
    g = build(gbp, p)
    F, S = len(g.factors), CFG['sweeps']
    out = dict(w=np.zeros((S, F)), flag=np.zeros((S, F), np.uint8), mask=np.zeros((S, F), np.uint8), iters=np.zeros((S, F), np.int32), damp=np.zeros((S, F)),
               energy=np.zeros(S), means=np.zeros((S, N * 3)))
    rmargin = dmargin = np.inf
    for it in range(S):
        for fac in g.factors:
            mu = np.concatenate([np.linalg.inv(b.lam) @ b.eta for b in fac.adj_beliefs])
            dmargin = min(dmargin, abs(np.linalg.norm(np.array(fac.linpoint) - mu) - CFG['beta']))
            if fac.loss is not None:
                m = np.linalg.norm(fac.measurement - meas_fn(np.asarray(fac.linpoint, dtype=float), *fac.args))
                rmargin = min(rmargin, abs(m - fac.mahalanobis_threshold))
        g.synchronous_iteration(local_relin=True, robustify=True)
        out['w'][it] = [fac.gauss_noise_var / fac.adaptive_gauss_noise_var for fac in g.factors]
        out['flag'][it] = [fac.robust_flag for fac in g.factors]
        out['iters'][it] = [fac.iters_since_relin for fac in g.factors]
        out['mask'][it] = out['iters'][it] == 0
        out['damp'][it] = [fac.eta_damping for fac in g.factors]
        out['energy'][it] = g.energy()
        out['means'][it] = g.get_means()
        if it + 1 in SNAP:
            k = f's{it + 1}_'
            out[k + 'feta'] = np.array([fac.factor.eta for fac in g.factors])
            out[k + 'flam'] = np.array([fac.factor.lam for fac in g.factors])
            out[k + 'linpoint'] = np.array([np.asarray(fac.linpoint, dtype=float) for fac in g.factors])
            for side, name in enumerate('ab'):
                out[k + 'msg_eta_' + name] = np.array([fac.messages[side].eta for fac in g.factors])
                out[k + 'msg_lam_' + name] = np.array([fac.messages[side].lam for fac in g.factors])
            out[k + 'bel_eta'] = np.array([v.belief.eta for v in g.var_nodes])
            out[k + 'bel_lam'] = np.array([v.belief.lam for v in g.var_nodes])
    return out, rmargin, dmargin


def run():
    from gbp import gbp
    seed = 27
    while True:
        p = problem(seed)
        assert len(p['edges']) == 35
        p['z'] = p['z'].copy()
        p['z'][list(OUTLIERS)] += OFFSET
        out, rmargin, dmargin = run_one(gbp, p)
        if min(rmargin, dmargin) >= MARGIN:
            break
        print(f"seed {seed}: within {rmargin:.2e} of a threshold, {dmargin:.2e} of beta; next seed")
        seed += 1
    lossy = np.array(sorted(LOSSES))
    flags = out['flag'][:, lossy].astype(bool)
    assert flags.any(), "no factor is ever flagged"
    assert (~flags.any(0)).any(), "every factor with a loss is flagged at some sweep"
    assert (flags[1:] != flags[:-1]).any(), "no flag changes during the run"
    assert not out['flag'][:, :29].any() and np.all(out['w'][:, :29] == 1.0)
    F = len(p['edges'])
    arrays = dict(p, seed=np.array(seed), robust_margin=np.array(rmargin), dist_margin=np.array(dmargin),
                  loss=np.array([CODE[LOSSES.get(f, (None, 0))[0]] for f in range(F)], dtype=np.int32),
                  threshold=np.array([LOSSES.get(f, (None, 2.0))[1] for f in range(F)]),
                  cfg=np.array([CFG['beta'], CFG['damping'], CFG['undamped'], CFG['minlin'], CFG['sweeps']], dtype=float))
    arrays.update(out)
    print(f"relinearisations per sweep {out['mask'].sum(1).tolist()}\nflagged per sweep {out['flag'].sum(1).tolist()}\n"
          f"flags of the closures, first and last sweep: {out['flag'][0, 29:].tolist()} {out['flag'][-1, 29:].tolist()}\n"
          f"energy {out['energy'][0]:.4f} -> {out['energy'][-1]:.4f}")
    print(f"seed {seed}, robust margin {rmargin:.3e}, distance margin {dmargin:.3e}, F = {F}")
    save('G27_se2_posegraph_robust', **arrays)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import warnings
    warnings.simplefilter('ignore')
    run()
