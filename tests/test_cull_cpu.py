"""CPU side of observation culling (gbp_ba_cull, gbp_ba_get_residuals): the symbols and their bindings, the renumbering formula, and the
host oracle of culling (tests/cull_host.py) against a graph built from the survivors alone and against the reference's own run
(fixture G19)."""
import numpy as np
import pytest

from cull_host import make_numpy_ba, cull_numpy_ba, renumbering
from retire_host import survivors_problem, graph_arrays

W = 50.0


def test_cull_symbols_are_bound():
    from gbp_amd import build, _capi
    build.build()
    for name in ('gbp_ba_cull', 'gbp_ba_get_residuals'):
        assert name in _capi.SIGNATURES
        assert hasattr(_capi.load(), name)
    from gbp_amd.engine import BAEngine
    for name in ('cull', 'residuals', 'cull_outliers'):
        assert callable(getattr(BAEngine, name))


def _problem(**kw):
    from gbp_amd.synthetic import make_synthetic
    return make_synthetic(**dict(dict(n_cams=12, n_lmks=160, obs_per_lmk=4, window=5, seed=2), **kw))


def _host(p, sweeps=4, **kw):
    nb = make_numpy_ba(p, **kw)
    nb.generate_priors_var(W)
    nb.update_all_beliefs()
    nb.iterate(sweeps)
    return nb


def orphaning_list(cam_idx, lmk_idx, cam, lmk, extra):
    """All factors (reference order) of camera `cam` and of landmark `lmk`, plus `extra`: the camera and the landmark become orphans."""
    return np.union1d(np.flatnonzero((cam_idx == cam) | (lmk_idx == lmk)), extra).astype(np.int32)


def test_renumbering_maps_follow_the_stated_formula():
    """new id = old id - number of removed ids below it, -1 for what is gone; factors stay camera-major; a camera and a landmark whose
    factors are all on the list go."""
    p = _problem()
    nb = _host(p, sweeps=1)
    cam0, lmk0 = graph_arrays(nb)[3:]
    F = cam0.size
    ids = orphaning_list(cam0, lmk0, 3, 17, np.arange(5, F, 11))
    cm, lm, fm = cull_numpy_ba(nb, ids)
    keep_f = ~np.isin(np.arange(F), ids)
    keep_c, keep_l = np.zeros(p.n_cams, bool), np.zeros(p.n_lmks, bool)
    keep_c[cam0[keep_f]] = True
    keep_l[lmk0[keep_f]] = True
    assert not keep_c[3] and not keep_l[17] and keep_c.sum() == p.n_cams - 1
    for got, keep in ((cm, keep_c), (lm, keep_l), (fm, keep_f)):
        want = np.array([i - int((~keep[:i]).sum()) if keep[i] else -1 for i in range(keep.size)])
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got, renumbering(keep))
    cam1, lmk1 = graph_arrays(nb)[3:]
    np.testing.assert_array_equal(cam1, cm[cam0[keep_f]])
    np.testing.assert_array_equal(lmk1, lm[lmk0[keep_f]])
    assert (np.diff(cam1) >= 0).all()
    assert [f.factorID for f in nb.graph.factors] == list(range(int(keep_f.sum())))
    assert (nb.C, nb.L) == (int(keep_c.sum()), int(keep_l.sum()))


@pytest.mark.parametrize('loss', [None, 'huber'])
def test_host_cull_equals_a_graph_of_the_survivors_with_the_state_injected(loss):
    """Culling on the object graph and sweeping on equals a NumpyBA built from the survivors' problem alone into which the priors, the
    messages and the factors' state are injected.  Priors do not change by a bit; a variable none of whose factors went keeps its belief
    to 1e-12; a variable that lost factors has belief = prior + the surviving messages."""
    p = _problem()
    nb = _host(p, sweeps=5, loss=loss)
    arrays = graph_arrays(nb)
    F = len(nb.graph.factors)
    ids = orphaning_list(arrays[3], arrays[4], 3, 17, np.arange(5, F, 11))
    bel_before = {id(v): (v.belief.eta.copy(), v.belief.lam.copy()) for v in nb.cams + nb.lmks}
    pri_before = {id(v): (v.prior.eta.copy(), v.prior.lam.copy()) for v in nb.cams + nb.lmks}
    culled = {id(nb.graph.factors[i]) for i in ids}
    touched = {id(v) for v in nb.cams + nb.lmks if any(id(f) in culled for f in v.adj_factors)}
    cm, lm, fm = cull_numpy_ba(nb, ids)
    assert F - len(nb.graph.factors) == int((fm < 0).sum()) == ids.size
    assert (cm < 0).sum() == 1 and (lm < 0).sum() >= 1
    n_touched = 0
    for v in nb.cams + nb.lmks:
        k = 0 if v.dofs == 6 else 1
        assert np.array_equal(v.prior.eta, pri_before[id(v)][0]) and np.array_equal(v.prior.lam, pri_before[id(v)][1])
        if id(v) in touched:                                    # what is left: the prior and the surviving factors' messages
            n_touched += 1
            eta, lam = v.prior.eta.copy(), v.prior.lam.copy()
            for f in v.adj_factors:
                eta, lam = eta + f.messages[k].eta, lam + f.messages[k].lam
            np.testing.assert_allclose(v.belief.eta, eta, rtol=1e-12, atol=1e-12 * np.abs(eta).max())
            np.testing.assert_allclose(v.belief.lam, lam, rtol=1e-12, atol=1e-12 * np.abs(lam).max())
        else:
            np.testing.assert_allclose(v.belief.eta, bel_before[id(v)][0], rtol=1e-12, atol=1e-12 * np.abs(bel_before[id(v)][0]).max())
            np.testing.assert_allclose(v.belief.lam, bel_before[id(v)][1], rtol=1e-12, atol=1e-12 * np.abs(bel_before[id(v)][1]).max())
    assert 0 < n_touched < len(nb.cams + nb.lmks)
    fresh = make_numpy_ba(survivors_problem((p.K,) + arrays, cm, lm, fm), loss=loss)
    assert len(fresh.graph.factors) == len(nb.graph.factors) and (fresh.C, fresh.L) == (nb.C, nb.L)
    for v, w in zip(nb.graph.var_nodes, fresh.graph.var_nodes):
        w.prior.eta, w.prior.lam = v.prior.eta.copy(), v.prior.lam.copy()
    for f, g in zip(nb.graph.factors, fresh.graph.factors):
        assert np.array_equal(f.measurement, g.measurement) and f.adj_vIDs == g.adj_vIDs
        g.compute_factor(linpoint=np.array(f.linpoint))
        g.adaptive_gauss_noise_var, g.robust_flag = f.adaptive_gauss_noise_var, f.robust_flag
        g.factor.eta, g.factor.lam = f.factor.eta.copy(), f.factor.lam.copy()
        g.iters_since_relin, g.eta_damping = f.iters_since_relin, f.eta_damping
        for k in range(2):
            g.messages[k].eta, g.messages[k].lam = f.messages[k].eta.copy(), f.messages[k].lam.copy()
    fresh.update_all_beliefs()
    for s in range(6):
        nb.iterate(1)
        fresh.iterate(1)
        assert [f.iters_since_relin for f in nb.graph.factors] == [f.iters_since_relin for f in fresh.graph.factors], s
    for x, y in zip(nb.beliefs(), fresh.beliefs()):
        np.testing.assert_allclose(x, y, rtol=1e-9, atol=1e-9 * np.abs(y).max())
    assert abs(nb.are() - fresh.are()) <= 1e-10 * fresh.are()


def test_host_cull_rejects_bad_lists_and_accepts_an_empty_one():
    nb = _host(_problem(), sweeps=1)
    F = len(nb.graph.factors)
    for bad in ([F], [-1], [2, 2], list(range(F))):
        with pytest.raises(ValueError):
            cull_numpy_ba(nb, bad)
    cm, lm, fm = cull_numpy_ba(nb, [])
    np.testing.assert_array_equal(cm, np.arange(12))
    np.testing.assert_array_equal(fm, np.arange(F))
    assert len(nb.graph.factors) == F and lm.size == nb.L


@pytest.mark.parametrize('tag', ['small', 'vsmall_huber'])
def test_host_cull_replays_reference_fixture_g19(tag):
    """tests/cull_host.py culls the stored lists from a NumpyBA the way make_g19.py culled them from the reference's own graph: the G19
    trajectory (two culls, the first orphaning a camera and a landmark, ba.py's schedule) is followed through every sweep.  The bound is
    the one the project holds any float64 restatement of the reference to (NumpyBA against fixture G4 in tests/test_oracle_golden.py, the
    GPU against this fixture): beliefs, priors and residuals 1e-6, messages 1e-5.  The restatement sums in another order than the
    reference, and the run without a robust loss relinearises in waves that amplify such rounding differences (extend_host.G17_HOLD),
    so no tighter bound follows from float64 alone; a wrong step of cull_graph shows at order one."""
    from conftest import golden
    from cull_host import HostGraph, g19_problem, g19_replay
    g = golden(f'G19_cull_{tag}')
    ids, cm, lm = g['c1_factor_ids'], g['c1_cam_map'], g['c1_lmk_map']
    assert (cm < 0).any() and (lm < 0).any() and not np.array_equal(cm[cm >= 0], np.flatnonzero(cm >= 0))
    lmk_of = g['base_lmk_idx'][np.argsort(g['base_cam_idx'], kind='stable')]
    lost = np.bincount(lmk_of[ids], minlength=lm.size)
    assert ((lost > 0) & (lm >= 0)).any()                       # a surviving landmark lost some of its factors
    worst = g19_replay(g, HostGraph(g19_problem(g), None if str(g['loss']) == 'None' else str(g['loss'])), belief_tol=1e-6, msg_tol=1e-5)
    assert worst < 1e-6
