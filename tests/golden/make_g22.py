#!/usr/bin/env python3
"""Generate fixture G22 (robust losses on the toy linear pose graphs) from the reference's own program.

    python tests/golden/make_g22.py --reference PATH_TO_THE_REFERENCE

Like make_g21 this runs the reference's ndim_posegraph.py by runpy (with --n_iters 0: the graph as built, no sweep), for
`--n_varnodes 100 --dim 3` and for its defaults, and copies nothing of it.  Per run (tags n100d3 / defaults) and per loss (huber,
constant; threshold 2): about 10 % of the measurements are turned into gross outliers (a fixed seed; + N(0, 15) per coordinate), every
factor gets the loss, compute_all_factors() is called again, and for 30 sweeps every factor.linpoint is set to its adjacent belief
means -- computed as robustify_loss itself computes them, gbp.py:306-308 -- before graph.synchronous_iteration(robustify=True).  That
is the one stated departure of the device engine from the reference: a linear factor never moves its linpoint,
so the reference's robustify_loss (gbp.py:309) would otherwise stay at the prior means for good.  The arithmetic is all the reference's.

Stored per (tag, loss): the measurements used (`_meas`, (F, d)), per sweep the adaptive_gauss_noise_var (`_var`, (30, F)) and
robust_flag (`_flag`, (30, F) uint8) of every factor and the energy after the sweep (`_energy`, (30,)), the final means (`_means`) and
beliefs (`_bel_eta`, `_bel_lam`), and joint_distribution_cov()'s mu at the final weights (`_map_mu`).
The constant loss is discontinuous at M = t, so the generator asserts that no factor in any sweep has |M - t| < 1e-6 and moves to the
next outlier seed until that holds (`_seed` records it); huber is continuous there.
The tests rebuild the graphs with oracle.linear_oracle.toy_posegraph(n, dim, 10, 1.0, seed=0) plus the stored measurements, and never
read the reference.
"""
import argparse
import contextlib
import io
import os
import runpy
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)

from make_golden import save      # noqa: E402

SWEEPS, THRESHOLD, OUTLIER_FRACTION, OUTLIER_STD, MARGIN = 30, 2.0, 0.1, 15.0, 1e-6


def build(ref, argv):
    old_argv = sys.argv
    sys.argv = ['ndim_posegraph.py'] + argv + ['--n_iters', '0']
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            g = runpy.run_path(os.path.join(ref, 'ndim_posegraph.py'), run_name='__main__')
    finally:
        sys.argv = old_argv
    return g['graph']


def belief_means(factor):
    mu = np.array([])
    for belief in factor.adj_beliefs:
        mu = np.concatenate((mu, np.linalg.inv(belief.lam) @ belief.eta))
    return mu


def run_one(ref, argv, loss, seed):
    """None when some factor comes within MARGIN of the threshold (constant loss only)."""
    graph = build(ref, argv)
    rs = np.random.RandomState(seed)
    F, d = len(graph.factors), graph.var_nodes[0].dofs
    bad = rs.rand(F) < OUTLIER_FRACTION
    for f, factor in enumerate(graph.factors):
        if bad[f]:
            factor.measurement = factor.measurement + rs.normal(0.0, OUTLIER_STD, d)
        factor.loss = loss
        factor.mahalanobis_threshold = THRESHOLD
    graph.compute_all_factors()
    var, flag, energy = np.zeros((SWEEPS, F)), np.zeros((SWEEPS, F), dtype=np.uint8), np.zeros(SWEEPS)
    for s in range(SWEEPS):
        for factor in graph.factors:
            factor.linpoint = belief_means(factor)
            m = np.linalg.norm(factor.measurement - factor.meas_fn(factor.linpoint, *factor.args)) / np.sqrt(factor.gauss_noise_var)
            if loss == 'constant' and abs(m - THRESHOLD) < MARGIN:
                return None
        graph.synchronous_iteration(robustify=True)
        var[s] = [factor.adaptive_gauss_noise_var for factor in graph.factors]
        flag[s] = [factor.robust_flag for factor in graph.factors]
        energy[s] = graph.energy()
    mu, _ = graph.joint_distribution_cov()
    return dict(meas=np.array([factor.measurement for factor in graph.factors]), var=var, flag=flag, energy=energy,
                means=graph.get_means(), bel_eta=np.array([v.belief.eta for v in graph.var_nodes]),
                bel_lam=np.array([v.belief.lam for v in graph.var_nodes]), map_mu=np.asarray(mu), seed=np.array(seed), n_outliers=np.array(int(bad.sum())))


def run(ref):
    arrays = {}
    for tag, argv in (('n100d3', ['--n_varnodes', '100', '--dim', '3']), ('defaults', [])):
        for loss in ('huber', 'constant'):
            seed, out = 22, None
            while out is None:
                out = run_one(ref, argv, loss, seed)
                seed += 1
            for k, v in out.items():
                arrays[f'{tag}_{loss}_{k}'] = v
            print(f"{tag} {loss}: seed {int(out['seed'])}, {int(out['n_outliers'])} outliers of {out['meas'].shape[0]} factors, robust in the "
                  f"last sweep {int(out['flag'][-1].sum())}, energy {out['energy'][0]:.4f} -> {out['energy'][-1]:.4f}")
    save('G22_toy_linear_robust', **arrays)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import warnings
    warnings.simplefilter('ignore', SyntaxWarning)
    run(args.reference)
