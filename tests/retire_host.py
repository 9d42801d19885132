"""Retirement of cameras from the reference's BA graph on the host: the oracle side of BAEngine.retire in tests/test_retire_*.py, the
counterpart of tests/extend_host.py.

retire_graph works on any object graph of the reference's shape (a NumpyBA's, or the reference's own BAFactorGraph in
tests/golden/make_g18.py) and performs steps 1-6 of gbp_ba_retire (include/gbp_ba.h):
  1. fold     for every factor f of a retired camera, l its landmark: l.prior.eta += f.messages[1].eta, l.prior.lam += f.messages[1].lam,
              in l.adj_factors order; f leaves l.adj_factors and graph.factors
  2. drop     the retired cameras, and every landmark left without a factor
  3. renumber survivors keep their order, ids become compact; the maps carry -1 for what is gone
  4. / 5.     nothing to do on objects: a surviving factor IS its state, a surviving node keeps its prior (plus the folds)
  6.          update_all_beliefs()
"""
import numpy as np

from extend_host import make_numpy_ba, _index, U3, U6      # noqa: F401  (make_numpy_ba: re-exported for the tests)


def renumbering(keep):
    """old id -> new id for a boolean survival mask: old id minus the number of removed ids below it, -1 for what is gone."""
    keep = np.asarray(keep, bool)
    removed_below = np.cumsum(~keep) - (~keep)
    return np.where(keep, np.arange(keep.size) - removed_below, -1).astype(np.int32)


def check_ids(cam_ids, C):
    ids = [int(c) for c in np.asarray(cam_ids).reshape(-1)]
    if any(c < 0 or c >= C for c in ids):
        raise ValueError("camera id out of range")
    if len(set(ids)) != len(ids):
        raise ValueError("camera id repeated")
    return set(ids)


def retire_graph(graph, cams, lmks, cam_ids):
    """Steps 1-6 on the object graph `graph` whose camera / landmark nodes are the lists `cams` / `lmks`.  Returns
    (surviving cameras, surviving landmarks, cam_map, lmk_map, factor_map); the graph is changed in place."""
    gone = check_ids(cam_ids, len(cams))
    if not gone:
        return cams, lmks, renumbering(np.ones(len(cams), bool)), renumbering(np.ones(len(lmks), bool)), renumbering(np.ones(len(graph.factors), bool))
    gone_nodes = {id(cams[c]) for c in gone}
    keep_f = np.array([id(f.adj_var_nodes[0]) not in gone_nodes for f in graph.factors], bool)
    if not keep_f.any():
        raise ValueError("the set leaves no factor")
    retired = {id(f) for f, k in zip(graph.factors, keep_f) if not k}
    for l in lmks:                                              # 1. fold, in adj_factors order
        stay = []
        for f in l.adj_factors:
            if id(f) in retired:
                l.prior.eta = l.prior.eta + f.messages[1].eta
                l.prior.lam = l.prior.lam + f.messages[1].lam
            else:
                stay.append(f)
        l.adj_factors[:] = stay
    graph.factors[:] = [f for f, k in zip(graph.factors, keep_f) if k]
    keep_c = np.array([c not in gone for c in range(len(cams))], bool)      # 2. drop
    keep_l = np.array([len(l.adj_factors) > 0 for l in lmks], bool)
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


def retire_numpy_ba(nb, cam_ids):
    """Retire cameras from NumpyBA `nb` in place.  Returns (cam_map, lmk_map, factor_map)."""
    nb.cams, nb.lmks, cm, lm, fm = retire_graph(nb.graph, nb.cams, nb.lmks, cam_ids)
    nb.C, nb.L = len(nb.cams), len(nb.lmks)
    _index(nb)
    return cm, lm, fm


def survivors_problem(problem_arrays, cm, lm, fm):
    """The survivors' BAProblem from the old one given as reference-order arrays (K, cam_means, lmk_means, meas, cam_idx, lmk_idx) and the maps."""
    from gbp_amd.synthetic import BAProblem
    K, cam_means, lmk_means, meas, cam_idx, lmk_idx = problem_arrays
    kf = fm >= 0
    return BAProblem(K=K, cam_means=np.asarray(cam_means)[cm >= 0], lmk_means=np.asarray(lmk_means)[lm >= 0], meas=np.asarray(meas)[kf],
                     cam_idx=cm[np.asarray(cam_idx)[kf]].astype(np.int32), lmk_idx=lm[np.asarray(lmk_idx)[kf]].astype(np.int32))


def graph_arrays(nb):
    """(cam_means, lmk_means, meas, cam_idx, lmk_idx) of a NumpyBA as it is now: belief means, factors in reference order."""
    lmk_index = {id(v): i for i, v in enumerate(nb.lmks)}
    fs = nb.graph.factors
    return (np.array([v.mu for v in nb.cams]), np.array([v.mu for v in nb.lmks]), np.array([f.measurement for f in fs]),
            np.array([nb._cam_index[id(f.adj_var_nodes[0])] for f in fs], np.int32),
            np.array([lmk_index[id(f.adj_var_nodes[1])] for f in fs], np.int32))


# ---- fixture G18 (tests/golden/make_g18.py): the reference's own fixed-lag run, replayed ------------------------------------------------
# Both G18 runs are followed through every retirement and every sweep (no horizon as extend_host.G17_HOLD: the numpy restatement stays
# within 2e-10 of the reference's ARE on all 30 sweeps of either run, but for the three early sweeps of fr1desk_small in which the energy
# jumps to 1e8 - 1e10 -- points that pass close to a camera plane -- where ARE / energy agree to 4e-9 / 6e-8: the ARE / energy tolerances
# are the G4 / G14 parity tests' 1e-6 / 1e-5, as in g17_replay).
G18_MSG_STEP = 6                                                # (make_g18.SAMPLE_MSG)


def g18_problem(g):
    from gbp_amd.synthetic import BAProblem
    return BAProblem(K=g['base_K'], cam_means=g['base_cam_means'], lmk_means=g['base_lmk_means'], meas=g['base_meas'],
                     cam_idx=g['base_cam_idx'], lmk_idx=g['base_lmk_idx'])


class HostGraph:
    """The replay's view of a NumpyBA shrunk by retire_numpy_ba."""

    def __init__(self, base, loss):
        self.nb = make_numpy_ba(base, loss=loss)

    def __getattr__(self, name):
        return getattr(self.nb, name)

    def retire(self, cam_ids):
        return retire_numpy_ba(self.nb, cam_ids)

    def count_relinearising(self):
        return sum(1 for f in self.nb.graph.factors if f.iters_since_relin == 0)

    def relin(self):
        fs = self.nb.graph.factors
        return (np.array([f.iters_since_relin for f in fs]), np.array([f.eta_damping for f in fs]),
                np.array([f.adaptive_gauss_noise_var for f in fs]))

    def lmk_priors(self):
        return np.array([v.prior.eta for v in self.nb.lmks]), np.array([v.prior.lam for v in self.nb.lmks])

    def messages(self):
        fs = self.nb.graph.factors
        return (np.array([f.messages[0].eta for f in fs]), np.array([f.messages[0].lam for f in fs]),
                np.array([f.messages[1].eta for f in fs]), np.array([f.messages[1].lam for f in fs]))


def g18_replay(g, graph, belief_tol, msg_tol, are_rtol=1e-6, energy_rtol=1e-5, verbose=False):
    """Replay fixture G18 on `graph` (HostGraph or an adapter of BAEngine with the same methods) and compare every record.  Returns the
    worst relative belief gap seen."""
    from conftest import rel_err_rows
    huber = str(g['loss']) == 'huber'
    graph.generate_priors_var(50.0)
    graph.update_all_beliefs()
    sweeps, n_ret, worst, k = int(g['sweeps']), int(g['n_retirements']), 0.0, 0

    def cmp_beliefs(prefix):
        nonlocal worst
        ce, cl, le, ll = graph.beliefs()
        for mine, key in ((ce, 'cam_eta'), (cl[:, U6[0], U6[1]], 'cam_lam'), (le, 'lmk_eta'), (ll[:, U3[0], U3[1]], 'lmk_lam')):
            gap = rel_err_rows(mine, g[f'{prefix}_{key}'])
            worst = max(worst, gap)
            if verbose:
                print(f'G18 {prefix}_{key}: {gap:.3e}')
            assert gap < belief_tol, (prefix, key, gap)

    for b in range(n_ret + 1):
        if b:
            cm, lm, fm = graph.retire(g[f'r{b}_cam_ids'])
            np.testing.assert_array_equal(cm, g[f'r{b}_cam_map'])
            np.testing.assert_array_equal(lm, g[f'r{b}_lmk_map'])
            np.testing.assert_array_equal(fm, g[f'r{b}_factor_map'])
            pe, pl = graph.lmk_priors()
            gap = max(rel_err_rows(pe, g[f'r{b}_lmk_prior_eta']), rel_err_rows(pl[:, U3[0], U3[1]], g[f'r{b}_lmk_prior_lam']))
            if verbose:
                print(f'G18 r{b} landmark priors: {gap:.3e}')
            assert gap < belief_tol, (b, gap)
            cmp_beliefs(f'r{b}_ret')
        for i in range(sweeps):
            if b == 0 and i in (3, 8):
                graph.set_iters_since_relin(1)
            graph.iterate(1)
            assert graph.count_relinearising() == int(g['n_relin'][k]), (b, i)
            assert np.isclose(graph.are(), g['are'][k], rtol=are_rtol, atol=0), (b, i)
            assert np.isclose(graph.energy(), g['energy'][k], rtol=energy_rtol, atol=0), (b, i)
            k += 1
        cmp_beliefs(f'r{b}_end')
        it, damp, av = graph.relin()
        np.testing.assert_array_equal(it, g[f'r{b}_end_iters_since_relin'])
        np.testing.assert_array_equal(damp, g[f'r{b}_end_eta_damping'])
        if huber:
            np.testing.assert_allclose(av, g[f'r{b}_end_adaptive_var'], rtol=1e-8)
    ce, cl, le, ll = graph.messages()
    step = G18_MSG_STEP
    assert len(ce[::step]) == len(g['msg_cam_eta'])
    for mine, key in ((ce[::step], 'msg_cam_eta'), (cl[::step][:, U6[0], U6[1]], 'msg_cam_lam'), (le[::step], 'msg_lmk_eta'),
                      (ll[::step][:, U3[0], U3[1]], 'msg_lmk_lam')):
        gap = rel_err_rows(mine, g[key])
        if verbose:
            print(f'G18 {key}: {gap:.3e}')
        assert gap < msg_tol, key
    assert k == len(g['are'])
    return worst
