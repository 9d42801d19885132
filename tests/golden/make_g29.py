#!/usr/bin/env python3
"""Generate fixture G29 (the nonlinear batch MAP of two pose graphs, by the reference's own classes driven as Gauss-Newton).

    python tests/golden/make_g29.py --reference PATH_TO_THE_REFERENCE

The graphs are those of fixtures G25 (the SE(2) ring of make_g25.py) and G28 (the SE(3) helix of make_g28.py, tag `main`), read back
from the committed fixtures; the reference's gbp.gbp.FactorGraph(nonlinear_factors=True) is built from them by make_g25.build /
make_g28.build, with the measurement models those generators define.  It is then driven as Gauss-Newton, which the reference has every
piece of but no loop for:
    repeat:  every factor: Factor.compute_factor(linpoint = the current mu, its two variables' parts)  (gbp.py:267-294: what
             compute_all_factors() calls, with the linearisation point given -- without the argument it takes the belief means, which
             this loop never moves);  mu, _ = joint_distribution_cov()  (gbp.py:128-144)
from mu_0 = the prior means (what update_all_beliefs() leaves before any message), until max |mu_new - mu| <= 1e-11 or 40 iterations (the reference's
dense inverse of a joint that holds a 1e6 anchor leaves steps of a few 1e-13 for ever: 1e-11 is the fixed point to its rounding).
Both graphs converge from the prior means (the generator asserts it), so no other start is recorded.

Stored per tag (`se2_`, `se3_`): `x0` (N, D), `iterates` (K, N, D) -- mu after every iteration --, `steps` (K,) max |mu_new - mu|, and
`energy` (K + 1,) -- FactorGraph.energy() is taken at the belief means, which this loop never moves, so the generator sums
0.5 |meas_fn(mu) - measurement|^2 over the factors itself (noise std 1).  The tests never read the reference.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

import make_g25                   # noqa: E402
import make_g28                   # noqa: E402
from make_golden import save      # noqa: E402

MAX_ITERS, TOL = 40, 1e-11


def gauss_newton(g, D):
    N = len(g.var_nodes)
    mu = np.concatenate([np.linalg.solve(v.prior.lam, v.prior.eta) for v in g.var_nodes])
    x0 = mu.reshape(N, D).copy()

    def energy(mu):
        e = 0.0
        for fac in g.factors:
            x = np.concatenate([mu[D * v.variableID:D * v.variableID + D] for v in fac.adj_var_nodes])
            r = fac.meas_fn(x, *fac.args) - fac.measurement
            e += 0.5 * float(r @ r)
        return e

    iterates, steps, energies = [], [], [energy(mu)]
    for _ in range(MAX_ITERS):
        for fac in g.factors:
            fac.compute_factor(linpoint=list(np.concatenate([mu[D * v.variableID:D * v.variableID + D] for v in fac.adj_var_nodes])))
        new, _ = g.joint_distribution_cov()
        new = np.asarray(new, dtype=float).reshape(-1)
        steps.append(float(np.abs(new - mu).max()))
        mu = new
        iterates.append(mu.reshape(N, D).copy())
        energies.append(energy(mu))
        if steps[-1] <= TOL:
            break
    assert steps[-1] <= TOL, f"Gauss-Newton did not settle from the prior means: steps {steps}"
    return dict(x0=x0, iterates=np.array(iterates), steps=np.array(steps), energy=np.array(energies))


def run():
    from gbp import gbp
    arrays = {}
    p = dict(np.load(os.path.join(HERE, 'G25_se2_posegraph.npz')))
    out = gauss_newton(make_g25.build(gbp, p, make_g25.RUNS['main']), 3)
    arrays.update({'se2_' + k: v for k, v in out.items()})
    print(f"se2: {len(out['steps'])} iterations, steps {out['steps']}, energy {out['energy'][0]:.4f} -> {out['energy'][-1]:.6f}")
    p = dict(np.load(os.path.join(HERE, 'G28_se3_posegraph.npz')))
    out = gauss_newton(make_g28.build(gbp, p, make_g28.RUNS['main'], p['z']), 6)
    arrays.update({'se3_' + k: v for k, v in out.items()})
    print(f"se3: {len(out['steps'])} iterations, steps {out['steps']}, energy {out['energy'][0]:.4f} -> {out['energy'][-1]:.6f}")
    save('G29_nonlinear_map', **arrays)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import warnings
    warnings.simplefilter('ignore')
    run()
