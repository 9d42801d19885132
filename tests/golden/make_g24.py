#!/usr/bin/env python3
"""Generate fixture G24 (a toy linear pose graph shrunk: its ten oldest variables retired into priors) from the reference's own classes.

    python tests/golden/make_g24.py --reference PATH_TO_THE_REFERENCE

Runs the reference's ndim_posegraph.py by runpy (`--n_varnodes 50 --dim 3 --M 5 --n_iters 0`: the graph as built, no sweep) for its
priors, pairs and noisy measurements, and copies nothing of it.  A second graph is then built with the reference's gbp.FactorGraph /
VariableNode / Factor (factors numbered in the order the program made them, so adj_factors is ascending in factor id), swept
10 times, and shrunk by hand the way a fixed-lag smoother would:
  * variables 0..9 are taken out of graph.var_nodes, every factor with such an end out of graph.factors and out of the kept
    variables' adj_factors;
  * before that, for every kept variable in turn and every removed factor in its adj_factors order, the factor's message to that variable
    (Factor.messages[k], k the variable's place in the factor) is added to the variable's prior.eta / prior.lam -- a factor with both ends
    removed adds nothing;
  * update_all_beliefs();
then swept 10 more times.

Stored: `va`, `vb`, `meas` of every factor of the FULL graph in append order, `prior_eta`, `prior_lam` of the full graph, `retire`
(the removed variables), `pre_means` after the first 10 sweeps, `shrunk_means` / `shrunk_bel_eta` / `shrunk_bel_lam` /
`shrunk_prior_eta` / `shrunk_prior_lam` right after the shrink's update_all_beliefs(), and `means`, `bel_eta`, `bel_lam`, `energy` after
the 10 further sweeps (survivors in their old order).
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

RETIRE, SWEEPS = 10, 10


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
    n = len(priors_eta)
    graph = gbp.FactorGraph(nonlinear_factors=False)
    for i in range(n):
        v = gbp.VariableNode(i, dim)
        v.prior.eta = priors_eta[i]
        v.prior.lam = priors_lam[i]
        graph.var_nodes.append(v)
    for k, (i, j) in enumerate(pairs):
        fac = gbp.Factor(k, [graph.var_nodes[i], graph.var_nodes[j]], meas[k], std, linear_displacement.meas_fn, linear_displacement.jac_fn,
                         loss=None, mahalanobis_threshold=2)
        graph.var_nodes[i].adj_factors.append(fac)
        graph.var_nodes[j].adj_factors.append(fac)
        graph.factors.append(fac)
    graph.update_all_beliefs()
    graph.compute_all_factors()
    graph.n_var_nodes = n
    for _ in range(SWEEPS):
        graph.synchronous_iteration()
    arrays = {'pre_means': graph.get_means()}

    gone = set(range(RETIRE))
    leaving = [fac for fac in graph.factors if gone & set(fac.adj_vIDs)]
    for v in graph.var_nodes[RETIRE:]:
        for fac in v.adj_factors:                           # adj_factors order = ascending factor id
            if fac in leaving:
                k = fac.adj_vIDs.index(v.variableID)
                v.prior.eta = v.prior.eta + fac.messages[k].eta
                v.prior.lam = v.prior.lam + fac.messages[k].lam
        v.adj_factors = [fac for fac in v.adj_factors if fac not in leaving]
    graph.factors = [fac for fac in graph.factors if fac not in leaving]
    graph.var_nodes = graph.var_nodes[RETIRE:]
    graph.n_var_nodes = n - RETIRE
    graph.update_all_beliefs()
    arrays['shrunk_means'] = graph.get_means()
    arrays['shrunk_bel_eta'] = np.array([v.belief.eta for v in graph.var_nodes])
    arrays['shrunk_bel_lam'] = np.array([v.belief.lam for v in graph.var_nodes])
    arrays['shrunk_prior_eta'] = np.array([v.prior.eta for v in graph.var_nodes])
    arrays['shrunk_prior_lam'] = np.array([v.prior.lam for v in graph.var_nodes])
    for _ in range(SWEEPS):
        graph.synchronous_iteration()
    arrays['means'] = graph.get_means()
    arrays['bel_eta'] = np.array([v.belief.eta for v in graph.var_nodes])
    arrays['bel_lam'] = np.array([v.belief.lam for v in graph.var_nodes])
    arrays['energy'] = np.array(graph.energy())
    print(f"{n} -> {len(graph.var_nodes)} variables, {len(pairs)} -> {len(graph.factors)} factors, energy {float(arrays['energy']):.4f}")
    save('G24_toy_linear_shrunk', va=np.array([i for i, _ in pairs]), vb=np.array([j for _, j in pairs]), meas=np.array(meas),
         prior_eta=np.array(priors_eta), prior_lam=np.array(priors_lam), retire=np.arange(RETIRE), **arrays)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import warnings
    warnings.simplefilter('ignore', SyntaxWarning)
    run(args.reference)
