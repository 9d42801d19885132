"""Culling of observations from the reference's BA graph on the host: the oracle side of BAEngine.cull in tests/test_cull_*.py, the
sibling of tests/retire_host.py.

cull_graph works on any object graph of the reference's shape (a NumpyBA's, or the reference's own BAFactorGraph in
tests/golden/make_g19.py) and performs steps 1-6 of gbp_ba_cull (include/gbp_ba.h):
  1. remove   every listed factor leaves graph.factors, its camera's adj_factors and its landmark's adj_factors; its messages go with
              it and NOTHING is added to any prior (where retire_graph folds, this drops)
  2. drop     every camera and every landmark left without a factor
  3. renumber survivors keep their order, ids become compact; the maps carry -1 for what is gone
  4. / 5.     nothing to do on objects: a surviving factor IS its state, a surviving node keeps its prior
  6.          update_all_beliefs()
"""
import numpy as np

from retire_host import make_numpy_ba, renumbering, _index, U3, U6      # noqa: F401  (make_numpy_ba: re-exported for the tests)


def check_ids(factor_ids, F):
    ids = [int(f) for f in np.asarray(factor_ids).reshape(-1)]
    if any(f < 0 or f >= F for f in ids):
        raise ValueError("factor id out of range")
    if len(set(ids)) != len(ids):
        raise ValueError("factor id repeated")
    if ids and len(ids) >= F:
        raise ValueError("the list leaves no factor")
    return set(ids)


def cull_graph(graph, cams, lmks, factor_ids):
    """Steps 1-6 on the object graph `graph` whose camera / landmark nodes are the lists `cams` / `lmks`.  Returns
    (surviving cameras, surviving landmarks, cam_map, lmk_map, factor_map); the graph is changed in place."""
    gone = check_ids(factor_ids, len(graph.factors))
    if not gone:
        return cams, lmks, renumbering(np.ones(len(cams), bool)), renumbering(np.ones(len(lmks), bool)), renumbering(np.ones(len(graph.factors), bool))
    keep_f = np.array([i not in gone for i in range(len(graph.factors))], bool)
    culled = {id(f) for f, k in zip(graph.factors, keep_f) if not k}
    for v in list(cams) + list(lmks):                           # 1. remove: the messages go with the factor objects
        v.adj_factors[:] = [f for f in v.adj_factors if id(f) not in culled]
    graph.factors[:] = [f for f, k in zip(graph.factors, keep_f) if k]
    keep_c = np.array([len(v.adj_factors) > 0 for v in cams], bool)         # 2. drop
    keep_l = np.array([len(v.adj_factors) > 0 for v in lmks], bool)
    new_cams = [v for v, k in zip(cams, keep_c) if k]
    new_lmks = [v for v, k in zip(lmks, keep_l) if k]
    for i, v in enumerate(new_cams):                            # 3. renumber
        v.variableID = i
        if hasattr(v, 'c_id'):
            v.c_id = i
    for i, v in enumerate(new_lmks):
        v.variableID = len(new_cams) + i
        if hasattr(v, 'l_id'):
            v.l_id = i
    for fid, f in enumerate(graph.factors):
        f.factorID = fid
        f.adj_vIDs = [v.variableID for v in f.adj_var_nodes]
    graph.var_nodes = new_cams + new_lmks
    graph.n_var_nodes, graph.n_factor_nodes, graph.n_edges = len(graph.var_nodes), len(graph.factors), 2 * len(graph.factors)
    graph.update_all_beliefs()                                  # 6.
    return new_cams, new_lmks, renumbering(keep_c), renumbering(keep_l), renumbering(keep_f)


def cull_numpy_ba(nb, factor_ids):
    """Cull factors from NumpyBA `nb` in place.  Returns (cam_map, lmk_map, factor_map)."""
    nb.cams, nb.lmks, cm, lm, fm = cull_graph(nb.graph, nb.cams, nb.lmks, factor_ids)
    nb.C, nb.L = len(nb.cams), len(nb.lmks)
    _index(nb)
    return cm, lm, fm


def residuals_of(graph):
    """Factor.compute_residual of every factor, (F, 2)."""
    return np.array([f.compute_residual() for f in graph.factors], np.float64).reshape(-1, 2)


def largest_residuals(res, candidates, share):
    """The ceil(share * len(candidates)) factor ids among `candidates` with the largest reprojection error, ascending."""
    candidates = np.asarray(candidates, np.int64)
    n = int(np.ceil(share * candidates.size))
    err = np.linalg.norm(res[candidates], axis=1)
    return np.sort(candidates[np.argsort(-err, kind='stable')[:n]]).astype(np.int32)


# ---- fixture G19 (tests/golden/make_g19.py): the reference's own run with two culls, replayed -------------------------------------------
# Tolerances of the sweeps' ARE / energy as in retire_host.g18_replay (the G4 / G14 parity tests' 1e-6 / 1e-5).
G19_MSG_STEP = 6                                                # (make_g19.SAMPLE_MSG)


def g19_problem(g):
    from retire_host import g18_problem
    return g18_problem(g)


class HostGraph:
    """The replay's view of a NumpyBA shrunk by cull_numpy_ba."""

    def __init__(self, base, loss):
        self.nb = make_numpy_ba(base, loss=loss)

    def __getattr__(self, name):
        return getattr(self.nb, name)

    def cull(self, factor_ids):
        return cull_numpy_ba(self.nb, factor_ids)

    def residuals(self):
        return (residuals_of(self.nb.graph),)

    def count_relinearising(self):
        return sum(1 for f in self.nb.graph.factors if f.iters_since_relin == 0)

    def relin(self):
        fs = self.nb.graph.factors
        return (np.array([f.iters_since_relin for f in fs]), np.array([f.eta_damping for f in fs]),
                np.array([f.adaptive_gauss_noise_var for f in fs]))

    def priors(self):
        c, l = self.nb.cams, self.nb.lmks
        return (np.array([v.prior.eta for v in c]), np.array([v.prior.lam for v in c]),
                np.array([v.prior.eta for v in l]), np.array([v.prior.lam for v in l]))

    def messages(self):
        fs = self.nb.graph.factors
        return (np.array([f.messages[0].eta for f in fs]), np.array([f.messages[0].lam for f in fs]),
                np.array([f.messages[1].eta for f in fs]), np.array([f.messages[1].lam for f in fs]))


def g19_replay(g, graph, belief_tol, msg_tol, are_rtol=1e-6, energy_rtol=1e-5, verbose=False):
    """Replay fixture G19 on `graph` (HostGraph or an adapter of BAEngine with the same methods): the STORED lists are culled, never a
    selection made here.  Compares every record; returns the worst relative belief gap seen."""
    from conftest import rel_err_rows
    huber = str(g['loss']) == 'huber'
    graph.generate_priors_var(50.0)
    graph.update_all_beliefs()
    sweeps, n_culls, worst, k = int(g['sweeps']), int(g['n_culls']), 0.0, 0

    def four(arrays, prefix, what, tol):
        nonlocal worst
        ce, cl, le, ll = arrays
        for mine, key in ((ce, 'cam_eta'), (cl[:, U6[0], U6[1]], 'cam_lam'), (le, 'lmk_eta'), (ll[:, U3[0], U3[1]], 'lmk_lam')):
            gap = rel_err_rows(mine, g[f'{prefix}_{key}'])
            if what == 'belief':
                worst = max(worst, gap)
            if verbose:
                print(f'G19 {prefix}_{key}: {gap:.3e}')
            assert gap < tol, (prefix, key, gap)

    for b in range(n_culls + 1):
        if b:
            res = graph.residuals()[0]
            gap = float(np.abs(res - g[f'c{b}_residuals']).max() / np.abs(g[f'c{b}_residuals']).max())
            if verbose:
                print(f'G19 c{b} residuals before the cull: {gap:.3e}')
            assert gap < belief_tol, (b, gap)
            cm, lm, fm = graph.cull(g[f'c{b}_factor_ids'])
            np.testing.assert_array_equal(cm, g[f'c{b}_cam_map'])
            np.testing.assert_array_equal(lm, g[f'c{b}_lmk_map'])
            np.testing.assert_array_equal(fm, g[f'c{b}_factor_map'])
            four(graph.priors(), f'c{b}_prior', 'prior', belief_tol)
            four(graph.beliefs(), f'c{b}_cull', 'belief', belief_tol)
        for i in range(sweeps):
            if b == 0 and i in (3, 8):
                graph.set_iters_since_relin(1)
            graph.iterate(1)
            assert graph.count_relinearising() == int(g['n_relin'][k]), (b, i)
            assert np.isclose(graph.are(), g['are'][k], rtol=are_rtol, atol=0), (b, i, graph.are(), g['are'][k])
            assert np.isclose(graph.energy(), g['energy'][k], rtol=energy_rtol, atol=0), (b, i, graph.energy(), g['energy'][k])
            k += 1
        four(graph.beliefs(), f'c{b}_end', 'belief', belief_tol)
        it, damp, av = graph.relin()
        np.testing.assert_array_equal(it, g[f'c{b}_end_iters_since_relin'])
        np.testing.assert_array_equal(damp, g[f'c{b}_end_eta_damping'])
        if huber:
            np.testing.assert_allclose(av, g[f'c{b}_end_adaptive_var'], rtol=1e-8)
    ce, cl, le, ll = graph.messages()
    step = G19_MSG_STEP
    assert len(ce[::step]) == len(g['msg_cam_eta'])
    for mine, key in ((ce[::step], 'msg_cam_eta'), (cl[::step][:, U6[0], U6[1]], 'msg_cam_lam'), (le[::step], 'msg_lmk_eta'),
                      (ll[::step][:, U3[0], U3[1]], 'msg_lmk_lam')):
        gap = rel_err_rows(mine, g[key])
        if verbose:
            print(f'G19 {key}: {gap:.3e}')
        assert gap < msg_tol, key
    assert k == len(g['are'])
    return worst
