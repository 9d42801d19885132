#!/usr/bin/env python3
"""Generate fixture G21 (the covariance half of the batch solution of the toy linear pose graphs) from the reference's own program.

    python tests/golden/make_g21.py --reference PATH_TO_THE_REFERENCE

Like make_golden.g8 this runs the reference's ndim_posegraph.py by runpy, for `--n_varnodes 100 --dim 3` and for its defaults, and
copies nothing of it: the script itself calls FactorGraph.joint_distribution_cov (gbp.py:128-144) and leaves `sigma`, the dense inverse
of the joint Lambda, in its globals.  Stored from that sigma, per run (tags n100d3 / defaults): the d x d diagonal blocks of all
variables (`_sigma_diag`, (N, d, d)), the ids (0, 7, N - 1) (`_joint_ids`) and the joint block over them (`_sigma_joint`, (3d, 3d)).
The tests rebuild the graphs with oracle.linear_oracle.toy_posegraph(n, dim, 10, 1.0, seed=0), as the G8 tests do, and never read
the reference.
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


def run(ref):
    arrays = {}
    for tag, argv in (('n100d3', ['--n_varnodes', '100', '--dim', '3', '--n_iters', '1']), ('defaults', ['--n_iters', '1'])):
        old_argv = sys.argv
        sys.argv = ['ndim_posegraph.py'] + argv
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                g = runpy.run_path(os.path.join(ref, 'ndim_posegraph.py'), run_name='__main__')
        finally:
            sys.argv = old_argv
        sigma = np.asarray(g['sigma'], dtype=np.float64)
        n, d = len(g['graph'].var_nodes), g['graph'].var_nodes[0].dofs
        assert sigma.shape == (n * d, n * d)
        ids = np.array([0, 7, n - 1], dtype=np.int32)
        idx = np.concatenate([np.arange(v * d, (v + 1) * d) for v in ids])
        arrays[f'{tag}_sigma_diag'] = np.array([sigma[v * d:(v + 1) * d, v * d:(v + 1) * d] for v in range(n)])
        arrays[f'{tag}_joint_ids'] = ids
        arrays[f'{tag}_sigma_joint'] = sigma[np.ix_(idx, idx)]
        print(f'{tag}: {n} variables x {d} dofs, max |sigma - sigma^T| {np.abs(sigma - sigma.T).max():.2e}')
    save('G21_toy_linear_sigma', **arrays)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import warnings
    warnings.simplefilter('ignore', SyntaxWarning)
    run(args.reference)
