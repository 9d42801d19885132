"""Retirement of landmarks from the reference's BA graph on the host: the oracle side of BAEngine.retire_landmarks in
tests/test_retire_lmk_*.py, the mirror image of tests/retire_host.py.

retire_landmarks_graph works on any object graph of the reference's shape (a NumpyBA's, or the reference's own BAFactorGraph in
tests/golden/make_g20.py) and performs steps 1-6 of gbp_ba_retire_landmarks (include/gbp_ba.h):
  1. fold     (fold=True only) for every factor f of a listed landmark, c its camera: c.prior.eta += f.messages[0].eta,
              c.prior.lam += f.messages[0].lam, in c.adj_factors order; f leaves c.adj_factors and graph.factors.  fold=False: the
              factors leave and nothing is added to any prior
  2. drop     the listed landmarks, and every camera and landmark left without a factor (an orphaned camera's folded prior goes with it)
  3. renumber survivors keep their order, ids become compact; the maps carry -1 for what is gone
  4. / 5.     nothing to do on objects: a surviving factor IS its state, a surviving node keeps its prior (plus the folds)
  6.          update_all_beliefs()
"""
import numpy as np

from retire_host import make_numpy_ba, renumbering, _index, g18_problem, U3, U6      # noqa: F401  (re-exported for the tests)


def check_ids(lmk_ids, L):
    ids = [int(l) for l in np.asarray(lmk_ids).reshape(-1)]
    if any(l < 0 or l >= L for l in ids):
        raise ValueError("landmark id out of range")
    if len(set(ids)) != len(ids):
        raise ValueError("landmark id repeated")
    return set(ids)


def retire_landmarks_graph(graph, cams, lmks, lmk_ids, fold=True):
    """Steps 1-6 on the object graph `graph` whose camera / landmark nodes are the lists `cams` / `lmks`.  Returns
    (surviving cameras, surviving landmarks, cam_map, lmk_map, factor_map); the graph is changed in place."""
    gone = check_ids(lmk_ids, len(lmks))
    if not gone:
        return cams, lmks, renumbering(np.ones(len(cams), bool)), renumbering(np.ones(len(lmks), bool)), renumbering(np.ones(len(graph.factors), bool))
    gone_nodes = {id(lmks[l]) for l in gone}
    keep_f = np.array([id(f.adj_var_nodes[1]) not in gone_nodes for f in graph.factors], bool)
    if not keep_f.any():
        raise ValueError("the list leaves no factor")
    retired = {id(f) for f, k in zip(graph.factors, keep_f) if not k}
    for c in cams:                                              # 1. fold, in adj_factors order
        stay = []
        for f in c.adj_factors:
            if id(f) in retired:
                if fold:
                    c.prior.eta = c.prior.eta + f.messages[0].eta
                    c.prior.lam = c.prior.lam + f.messages[0].lam
            else:
                stay.append(f)
        c.adj_factors[:] = stay
    for l in lmks:
        l.adj_factors[:] = [f for f in l.adj_factors if id(f) not in retired]
    graph.factors[:] = [f for f, k in zip(graph.factors, keep_f) if k]
    keep_c = np.array([len(v.adj_factors) > 0 for v in cams], bool)         # 2. drop
    keep_l = np.array([len(v.adj_factors) > 0 for v in lmks], bool)         # (a listed landmark has no factor left)
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


def retire_landmarks_numpy_ba(nb, lmk_ids, fold=True):
    """Retire landmarks from NumpyBA `nb` in place.  Returns (cam_map, lmk_map, factor_map)."""
    nb.cams, nb.lmks, cm, lm, fm = retire_landmarks_graph(nb.graph, nb.cams, nb.lmks, lmk_ids, fold)
    nb.C, nb.L = len(nb.cams), len(nb.lmks)
    _index(nb)
    return cm, lm, fm


def pick_first_list(cam_idx, lmk_idx, n_cams, n_lmks):
    """A list for a first retirement that exercises every rule (make_g20.py; the tests use the stored list): every landmark of one
    camera -- the one with the fewest landmarks among those that are neither the first nor the last camera and do not see landmark 0:
    it is orphaned, so the camera map is not a shift --, the two lowest landmarks of the smallest degree there is (degree 1 where the
    graph has such landmarks) and every 11th landmark from 5 on.  Landmark 0 is not on it: no prefix of the ids.  Returns (ids, camera)."""
    cam_idx, lmk_idx = np.asarray(cam_idx), np.asarray(lmk_idx)
    per_cam = np.bincount(cam_idx, minlength=n_cams)
    ok = [c for c in range(1, n_cams - 1) if per_cam[c] > 0 and 0 not in lmk_idx[cam_idx == c]]
    c = min(ok, key=lambda k: (per_cam[k], k))
    ids = set(int(l) for l in lmk_idx[cam_idx == c])
    deg = np.bincount(lmk_idx, minlength=n_lmks)
    ids |= set(int(l) for l in np.flatnonzero((deg == deg[deg > 0].min()) & (np.arange(n_lmks) > 0))[:2])
    ids |= set(range(5, n_lmks, 11))
    return np.array(sorted(ids), np.int32), c


# ---- fixture G20 (tests/golden/make_g20.py): the reference's own run with two landmark retirements, replayed ----------------------------
# Tolerances of the sweeps' ARE / energy as in retire_host.g18_replay (the G4 / G14 parity tests' 1e-6 / 1e-5).
G20_MSG_STEP = 6                                                # (make_g20.SAMPLE_MSG)


def g20_problem(g):
    return g18_problem(g)


class HostGraph:
    """The replay's view of a NumpyBA shrunk by retire_landmarks_numpy_ba."""

    def __init__(self, base, loss):
        self.nb = make_numpy_ba(base, loss=loss)

    def __getattr__(self, name):
        return getattr(self.nb, name)

    def retire_landmarks(self, lmk_ids, fold=True):
        return retire_landmarks_numpy_ba(self.nb, lmk_ids, fold)

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


def g20_replay(g, graph, belief_tol, msg_tol, are_rtol=1e-6, energy_rtol=1e-5, verbose=False):
    """Replay fixture G20 on `graph` (HostGraph or an adapter of BAEngine with the same methods): the STORED lists are retired.  Compares
    every record; returns the worst relative belief gap seen."""
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
                print(f'G20 {prefix}_{key}: {gap:.3e}')
            assert gap < belief_tol, (prefix, key, gap)

    for b in range(n_ret + 1):
        if b:
            cm, lm, fm = graph.retire_landmarks(g[f'r{b}_lmk_ids'], fold=bool(g[f'r{b}_fold']))
            np.testing.assert_array_equal(cm, g[f'r{b}_cam_map'])
            np.testing.assert_array_equal(lm, g[f'r{b}_lmk_map'])
            np.testing.assert_array_equal(fm, g[f'r{b}_factor_map'])
            pe, pl = graph.priors()[:2]
            gap = max(rel_err_rows(pe, g[f'r{b}_cam_prior_eta']), rel_err_rows(pl[:, U6[0], U6[1]], g[f'r{b}_cam_prior_lam']))
            if verbose:
                print(f'G20 r{b} camera priors: {gap:.3e}')
            assert gap < belief_tol, (b, gap)
            cmp_beliefs(f'r{b}_ret')
        for i in range(sweeps):
            if b == 0 and i in (3, 8):
                graph.set_iters_since_relin(1)
            graph.iterate(1)
            assert graph.count_relinearising() == int(g['n_relin'][k]), (b, i)
            assert np.isclose(graph.are(), g['are'][k], rtol=are_rtol, atol=0), (b, i, graph.are(), g['are'][k])
            assert np.isclose(graph.energy(), g['energy'][k], rtol=energy_rtol, atol=0), (b, i, graph.energy(), g['energy'][k])
            k += 1
        cmp_beliefs(f'r{b}_end')
        it, damp, av = graph.relin()
        np.testing.assert_array_equal(it, g[f'r{b}_end_iters_since_relin'])
        np.testing.assert_array_equal(damp, g[f'r{b}_end_eta_damping'])
        if huber:
            np.testing.assert_allclose(av, g[f'r{b}_end_adaptive_var'], rtol=1e-8)
    ce, cl, le, ll = graph.messages()
    step = G20_MSG_STEP
    assert len(ce[::step]) == len(g['msg_cam_eta'])
    for mine, key in ((ce[::step], 'msg_cam_eta'), (cl[::step][:, U6[0], U6[1]], 'msg_cam_lam'), (le[::step], 'msg_lmk_eta'),
                      (ll[::step][:, U3[0], U3[1]], 'msg_lmk_lam')):
        gap = rel_err_rows(mine, g[key])
        if verbose:
            print(f'G20 {key}: {gap:.3e}')
        assert gap < msg_tol, key
    assert k == len(g['are'])
    return worst
