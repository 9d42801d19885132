"""CPU side of camera retirement (gbp_ba_retire): the symbol and its binding, the renumbering formula, and the host oracle of retirement
(tests/retire_host.py) against a graph built from the survivors alone and against the reference's own run (fixture G18)."""
import numpy as np
import pytest

from retire_host import make_numpy_ba, retire_numpy_ba, renumbering, survivors_problem, graph_arrays

W = 50.0


def test_retire_symbol_is_bound():
    from gbp_amd import build, _capi
    build.build()
    assert 'gbp_ba_retire' in _capi.SIGNATURES
    assert hasattr(_capi.load(), 'gbp_ba_retire')
    from gbp_amd.engine import BAEngine
    assert callable(getattr(BAEngine, 'retire'))


def _problem(**kw):
    from gbp_amd.synthetic import make_synthetic
    return make_synthetic(**dict(dict(n_cams=12, n_lmks=160, obs_per_lmk=4, window=5, seed=2), **kw))


def _host(p, sweeps=4, **kw):
    nb = make_numpy_ba(p, **kw)
    nb.generate_priors_var(W)
    nb.update_all_beliefs()
    nb.iterate(sweeps)
    return nb


def test_renumbering_maps_follow_the_stated_formula():
    """new id = old id - number of removed ids below it, -1 for what is gone; factors stay camera-major."""
    p = _problem()
    nb = _host(p, sweeps=1)
    cam0, lmk0 = graph_arrays(nb)[3:]
    gone = [2, 0, 1, 3, 7]
    cm, lm, fm = retire_numpy_ba(nb, gone)
    keep_c = ~np.isin(np.arange(p.n_cams), gone)
    keep_f = keep_c[cam0]
    keep_l = np.zeros(p.n_lmks, bool)
    keep_l[lmk0[keep_f]] = True
    for got, keep in ((cm, keep_c), (lm, keep_l), (fm, keep_f)):
        want = np.array([i - int((~keep[:i]).sum()) if keep[i] else -1 for i in range(keep.size)])
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(got, renumbering(keep))
    assert (~keep_l).any()                                      # (this problem has landmarks seen by the retired cameras only)
    cam1, lmk1 = graph_arrays(nb)[3:]
    np.testing.assert_array_equal(cam1, cm[cam0[keep_f]])
    np.testing.assert_array_equal(lmk1, lm[lmk0[keep_f]])
    assert (np.diff(cam1) >= 0).all()
    assert [f.factorID for f in nb.graph.factors] == list(range(int(keep_f.sum())))
    assert (nb.C, nb.L) == (int(keep_c.sum()), int(keep_l.sum()))


@pytest.mark.parametrize('loss', [None, 'huber'])
def test_host_retirement_equals_a_graph_of_the_survivors_with_the_state_injected(loss):
    """Retiring on the object graph and sweeping on equals a NumpyBA built from the survivors' problem alone into which the folded priors,
    the messages and the factors' state are injected: same objects' arithmetic, so the runs agree to rounding."""
    p = _problem()
    nb = _host(p, sweeps=5, loss=loss)
    arrays = graph_arrays(nb)
    before = {id(f): f for f in nb.graph.factors}
    bel_before = {id(v): (v.belief.eta.copy(), v.belief.lam.copy()) for v in nb.cams + nb.lmks}
    pri_before = {id(v): (v.prior.eta.copy(), v.prior.lam.copy()) for v in nb.cams + nb.lmks}
    msgs = {id(v): [(f.messages[1].eta.copy(), f.messages[1].lam.copy(), nb._cam_index[id(f.adj_var_nodes[0])]) for f in v.adj_factors] for v in nb.lmks}
    gone = [3, 0]
    cm, lm, fm = retire_numpy_ba(nb, gone)
    assert len(before) - len(nb.graph.factors) == int((fm < 0).sum()) > 0
    for v in nb.cams:                                           # camera priors never change
        assert np.array_equal(v.prior.eta, pri_before[id(v)][0]) and np.array_equal(v.prior.lam, pri_before[id(v)][1])
    for v in nb.lmks:                                           # landmark priors: + the retired factors' messages, in adj_factors order
        eta, lam = pri_before[id(v)]
        for me, ml, c in msgs[id(v)]:
            if c in gone:
                eta, lam = eta + me, lam + ml
        assert np.array_equal(v.prior.eta, eta) and np.array_equal(v.prior.lam, lam)
    for v in nb.cams + nb.lmks:                                 # beliefs: unchanged up to summation order
        np.testing.assert_allclose(v.belief.eta, bel_before[id(v)][0], rtol=1e-12, atol=1e-12 * np.abs(bel_before[id(v)][0]).max())
        np.testing.assert_allclose(v.belief.lam, bel_before[id(v)][1], rtol=1e-12, atol=1e-12 * np.abs(bel_before[id(v)][1]).max())
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


def test_host_retirement_rejects_bad_lists_and_accepts_an_empty_one():
    nb = _host(_problem(), sweeps=1)
    for bad in ([12], [-1], [2, 2], list(range(12))):
        with pytest.raises(ValueError):
            retire_numpy_ba(nb, bad)
    F = len(nb.graph.factors)
    cm, lm, fm = retire_numpy_ba(nb, [])
    np.testing.assert_array_equal(cm, np.arange(12))
    np.testing.assert_array_equal(fm, np.arange(F))
    assert len(nb.graph.factors) == F and lm.size == nb.L


@pytest.mark.parametrize('tag', ['small', 'vsmall_huber'])
def test_host_retirement_replays_reference_fixture_g18(tag):
    """tests/retire_host.py retires cameras from a NumpyBA the way make_g18.py retired them from the reference's own graph: the G18
    trajectory (two retirements, the first of a non-prefix set, ba.py's schedule) agrees to 1e-8 in every belief and message, through every sweep."""
    from conftest import golden
    from retire_host import HostGraph, g18_problem, g18_replay
    g = golden(f'G18_retire_{tag}')
    worst = g18_replay(g, HostGraph(g18_problem(g), None if str(g['loss']) == 'None' else str(g['loss'])), belief_tol=1e-8, msg_tol=1e-8)
    assert worst < 1e-8
