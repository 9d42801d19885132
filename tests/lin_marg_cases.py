"""Shared by tests/test_linear_marginals_cpu.py and tests/test_linear_marginals_gpu.py: the tree the belief covariances are exact on,
and the blocks of a dense inverse that gbp_lin_solve_marginals returns.  The graphs themselves are lin_map_cases.shapes."""
import numpy as np


def chain(n=12, D=3):
    """A tree: n variables in a chain of displacement factors (sigma 0.5) under priors of sigma 2:
    (va, vb, factor_eta, factor_lam, factor_const, prior_eta, prior_lam)."""
    from oracle.linear_oracle import displacement_graph
    rs = np.random.RandomState(5)
    va, vb = np.arange(n - 1), np.arange(1, n)
    _, _, fe, fl, fc, pe, pl = displacement_graph(va, vb, rs.rand(n, D) * 4, 0.5, rs, prior_sigma=2.0)
    return va, vb, fe, fl, fc, pe, pl


def diag_blocks(S, ids, D):
    """(len(ids), D, D): the diagonal blocks of the variables `ids` of a dense (N D, N D) matrix."""
    return np.array([S[v * D:(v + 1) * D, v * D:(v + 1) * D] for v in ids]).reshape(-1, D, D)


def sub(S, ids, D):
    """S restricted to the coordinates of the variables `ids`, in that order."""
    idx = np.concatenate([np.arange(v * D, (v + 1) * D) for v in ids])
    return S[np.ix_(idx, idx)]
