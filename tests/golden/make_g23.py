#!/usr/bin/env python3
"""Generate fixture G23 (a toy linear pose graph grown in three stages) from the reference's own classes.

    python tests/golden/make_g23.py --reference PATH_TO_THE_REFERENCE

Runs the reference's ndim_posegraph.py by runpy (`--n_varnodes 50 --dim 3 --M 5 --n_iters 0`: the graph as built, no sweep) for its
priors, pairs and noisy measurements, and copies nothing of it.  A second graph is then built with the reference's gbp.FactorGraph /
VariableNode / Factor as a robot would build it:
  stage 0: the first 30 variables and the factors among them (in the order the program made them), update_all_beliefs(),
           compute_all_factors(), 10 x synchronous_iteration();
  stage 1: variables 30..39 and every factor that now has both ends (var_nodes.append, factors.append, adj_factors.append,
           compute_factor() on the new factors), update_all_beliefs(), 10 sweeps;
  stage 2: the last 10 and the remaining factors, update_all_beliefs(), 10 sweeps.
Factors are numbered in append order, so every variable's adj_factors stays ascending in factor id.

Stored: `va`, `vb`, `meas` of every factor in append order, `stage_n` = (30, 40, 50) and `stage_f` (factors after each stage),
`prior_eta`, `prior_lam`, and per stage s: `s{s}_grown_means` / `_grown_bel_eta` / `_grown_bel_lam` right after the growth's
update_all_beliefs(), and `s{s}_means`, `s{s}_bel_eta`, `s{s}_bel_lam`, `s{s}_energy` after its 10 sweeps.
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

STAGES, SWEEPS = (30, 40, 50), 10


def run(ref):
    from gbp import gbp
    from gbp.factors import linear_displacement
    old_argv = sys.argv
    sys.argv = ['ndim_posegraph.py', '--n_varnodes', '50', '--dim', '3', '--M', '5', '--n_iters', '0']
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            g = runpy.run_path(os.path.join(ref, 'ndim_posegraph.py'), run_name='__main__')
    finally:
        sys.argv = old_argv
    pairs, meas, std = g['measurements_nodeIDs'], g['noisy_measurements'], g['args'].gauss_noise_std
    priors_eta, priors_lam, dim = g['priors_eta'], g['priors_lambda'], g['args'].dim
    graph = gbp.FactorGraph(nonlinear_factors=False)
    arrays, va, vb, zz, stage_f = {}, [], [], [], []
    done = [False] * len(pairs)
    n_old = 0
    for s, n in enumerate(STAGES):
        for i in range(n_old, n):
            v = gbp.VariableNode(i, dim)
            v.prior.eta = priors_eta[i]
            v.prior.lam = priors_lam[i]
            graph.var_nodes.append(v)
        new = []
        for k, (i, j) in enumerate(pairs):
            if not done[k] and i < n and j < n:
                done[k] = True
                fac = gbp.Factor(len(graph.factors), [graph.var_nodes[i], graph.var_nodes[j]], meas[k], std, linear_displacement.meas_fn,
                                 linear_displacement.jac_fn, loss=None, mahalanobis_threshold=2)
                graph.var_nodes[i].adj_factors.append(fac)
                graph.var_nodes[j].adj_factors.append(fac)
                graph.factors.append(fac)
                new.append(fac)
                va.append(i); vb.append(j); zz.append(meas[k])
        graph.update_all_beliefs()
        for fac in new:
            fac.compute_factor()
        graph.n_var_nodes = n
        arrays[f's{s}_grown_means'] = graph.get_means()
        arrays[f's{s}_grown_bel_eta'] = np.array([v.belief.eta for v in graph.var_nodes])
        arrays[f's{s}_grown_bel_lam'] = np.array([v.belief.lam for v in graph.var_nodes])
        for _ in range(SWEEPS):
            graph.synchronous_iteration()
        arrays[f's{s}_means'] = graph.get_means()
        arrays[f's{s}_bel_eta'] = np.array([v.belief.eta for v in graph.var_nodes])
        arrays[f's{s}_bel_lam'] = np.array([v.belief.lam for v in graph.var_nodes])
        arrays[f's{s}_energy'] = np.array(graph.energy())
        stage_f.append(len(graph.factors))
        n_old = n
        print(f"stage {s}: {n} variables, {len(graph.factors)} factors, energy {float(arrays[f's{s}_energy']):.4f}")
    assert all(done)
    for v in graph.var_nodes:
        ids = [f.factorID for f in v.adj_factors]
        assert ids == sorted(ids)
    save('G23_toy_linear_grown', va=np.array(va), vb=np.array(vb), meas=np.array(zz), stage_n=np.array(STAGES), stage_f=np.array(stage_f),
         prior_eta=np.array(priors_eta), prior_lam=np.array(priors_lam), **arrays)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import warnings
    warnings.simplefilter('ignore', SyntaxWarning)
    run(args.reference)
