#!/usr/bin/env python3
"""Generate fixture G30 (the ROBUST nonlinear batch MAP of two pose graphs: the fixed point of robustify + relinearise + solve, by the
reference's own classes driven as iteratively reweighted Gauss-Newton).

    python tests/golden/make_g30.py --reference PATH_TO_THE_REFERENCE

The graphs are those of fixture G27 (the SE(2) ring with three corrupted closures; Huber at 2 on closures 29-31, constant at 3 on 32, 33
and at 60 on 34) and of fixture G28's tag `robust` (the SE(3) helix with closures 29, 31, 33 corrupted), read back from the committed
fixtures; the reference's gbp.gbp.FactorGraph(nonlinear_factors=True) is built from them by make_g27.build / make_g28.build.  On the
helix make_g28.build gives all six closures Huber at 4; here closures 32 and 33 are changed to the constant loss at 5 and closure 34 to
the constant loss at 60 (SE3_LOSSES), so that both losses are exercised and one lossy factor is never flagged.
The reference is driven as the loop it has every piece of but no driver for:
    repeat:  every factor: Factor.linpoint = the current mu's two parts; Factor.robustify_loss()   (gbp.py:296-332: the weight from
             M at the linpoint, gbp.py:309)
             Gauss-Newton at those weights, as make_g29.py: every factor Factor.compute_factor(linpoint = x) (gbp.py:267-294, which
             divides by adaptive_gauss_noise_var: the weighted factor), x = joint_distribution_cov()[0] (gbp.py:128-144), until
             max |x_new - x| <= 1e-11
from mu_0 = the prior means, until max |mu_new - mu| <= 1e-10.  Asserted: the reference converges within 30 rounds, at least one factor
is flagged at the fixed point and at least one factor with a loss is not.

Stored per tag (`se2_`, `se3_`): `x0` (N, D); per round r: `mu` (R, N, D) -- the point the round's weights were made at, the last one
being the fixed point --, `w` (R, F) = gauss_noise_var / adaptive_gauss_noise_var and `flag` (R, F) at that point, `moves` (R - 1,)
max |mu_{r+1} - mu_r|, `gn_iters` (R - 1,); the losses and thresholds used (`loss`, `threshold`) and, for the helix, `z` (the
measurements with the corrupted closures).  The tests never read the reference.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_g27                   # noqa: E402
import make_g28                   # noqa: E402
from make_golden import save      # noqa: E402

MAX_ROUNDS, TOL_MOVE, MAX_GN, TOL_GN = 30, 1e-10, 40, 1e-11
SE3_LOSSES = {32: ('constant', 5.0), 33: ('constant', 5.0), 34: ('constant', 60.0)}
CODE = {None: 0, 'huber': 1, 'constant': 2}


def adjacent(fac, mu, D):
    return np.concatenate([mu[D * v.variableID:D * v.variableID + D] for v in fac.adj_var_nodes])


def reweighted_gauss_newton(g, D):
    N = len(g.var_nodes)
    mu = np.concatenate([np.linalg.solve(v.prior.lam, v.prior.eta) for v in g.var_nodes])
    x0 = mu.reshape(N, D).copy()
    mus, ws, flags, moves, gn_iters = [], [], [], [], []
    for _ in range(MAX_ROUNDS + 1):
        for fac in g.factors:
            fac.linpoint = list(adjacent(fac, mu, D))
            fac.robustify_loss()
        mus.append(mu.reshape(N, D).copy())
        ws.append([fac.gauss_noise_var / fac.adaptive_gauss_noise_var for fac in g.factors])
        flags.append([bool(fac.robust_flag) and fac.loss is not None for fac in g.factors])
        if moves and moves[-1] <= TOL_MOVE:
            break
        x = mu
        for it in range(MAX_GN):
            for fac in g.factors:
                fac.compute_factor(linpoint=list(adjacent(fac, x, D)))
            new = np.asarray(g.joint_distribution_cov()[0], dtype=float).reshape(-1)
            step = float(np.abs(new - x).max())
            x = new
            if step <= TOL_GN:
                break
        assert step <= TOL_GN, f"Gauss-Newton did not settle at the weights of round {len(moves)}"
        gn_iters.append(it + 1)
        moves.append(float(np.abs(x - mu).max()))
        mu = x
    assert moves[-1] <= TOL_MOVE, f"the reference did not converge within {MAX_ROUNDS} rounds: moves {moves}"
    flag = np.array(flags)
    lossy = np.array([fac.loss is not None for fac in g.factors])
    assert flag[-1].any(), "no factor is flagged at the fixed point"
    assert (lossy & ~flag[-1]).any(), "every factor with a loss is flagged at the fixed point"
    return dict(x0=x0, mu=np.array(mus), w=np.array(ws), flag=flag.astype(np.uint8), moves=np.array(moves), gn_iters=np.array(gn_iters, dtype=np.int32),
                loss=np.array([CODE[fac.loss] for fac in g.factors], dtype=np.int32),
                threshold=np.array([fac.mahalanobis_threshold if fac.loss is not None else 1.0 for fac in g.factors]))


def run():
    from gbp import gbp
    arrays = {}
    p = dict(np.load(os.path.join(HERE, 'G27_se2_posegraph_robust.npz')))
    out = reweighted_gauss_newton(make_g27.build(gbp, p), 3)
    arrays.update({'se2_' + k: v for k, v in out.items()})
    print(f"se2: {len(out['moves'])} rounds, moves {out['moves']}, GN iterations {out['gn_iters'].tolist()}, flagged per round {out['flag'].sum(1).tolist()}")
    p = dict(np.load(os.path.join(HERE, 'G28_se3_posegraph.npz')))
    g = make_g28.build(gbp, p, make_g28.RUNS['robust'], p['robust_z'])
    for f, (loss, thr) in SE3_LOSSES.items():
        g.factors[f].loss, g.factors[f].mahalanobis_threshold = loss, thr
    out = reweighted_gauss_newton(g, 6)
    arrays.update({'se3_' + k: v for k, v in out.items()})
    arrays['se3_z'] = p['robust_z']
    print(f"se3: {len(out['moves'])} rounds, moves {out['moves']}, GN iterations {out['gn_iters'].tolist()}, flagged per round {out['flag'].sum(1).tolist()}")
    save('G30_nonlinear_map_robust', **arrays)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import warnings
    warnings.simplefilter('ignore')
    run()
