"""CPU side of landmark retirement (gbp_ba_retire_landmarks): the symbol and its binding, the renumbering formula, and the host oracle
(tests/retire_lmk_host.py) against a graph built from the survivors alone and against the reference's own run (fixture G20)."""
import numpy as np
import pytest

from retire_host import survivors_problem, graph_arrays
from retire_lmk_host import make_numpy_ba, retire_landmarks_numpy_ba, renumbering

W = 50.0


def test_retire_landmarks_symbol_is_bound():
    from gbp_amd import build, _capi
    build.build()
    assert 'gbp_ba_retire_landmarks' in _capi.SIGNATURES
    assert hasattr(_capi.load(), 'gbp_ba_retire_landmarks')
    assert (_capi.RETIRE_FOLD, _capi.RETIRE_DROP) == (0, 1)
    assert _capi.load().gbp_abi_version() == 3
    from gbp_amd.engine import BAEngine
    assert callable(getattr(BAEngine, 'retire_landmarks'))


def _problem(**kw):
    from gbp_amd.synthetic import make_synthetic
    return make_synthetic(**dict(dict(n_cams=12, n_lmks=160, obs_per_lmk=4, window=5, seed=2), **kw))


def _host(p, sweeps=4, **kw):
    nb = make_numpy_ba(p, **kw)
    nb.generate_priors_var(W)
    nb.update_all_beliefs()
    nb.iterate(sweeps)
    return nb


def _list_that_orphans_a_camera(cam0, lmk0, cam):
    """every landmark camera `cam` sees, and a few more"""
    return sorted(set(int(l) for l in lmk0[cam0 == cam]) | {7, 33, 150})


@pytest.mark.parametrize('fold', [True, False])
def test_renumbering_maps_follow_the_stated_formula(fold):
    """new id = old id - number of removed ids below it, -1 for what is gone; factors stay camera-major; a camera all of whose landmarks
    go is an orphan and goes too."""
    p = _problem()
    nb = _host(p, sweeps=1)
    cam0, lmk0 = graph_arrays(nb)[3:]
    gone = _list_that_orphans_a_camera(cam0, lmk0, 8)
    assert 0 not in gone
    cm, lm, fm = retire_landmarks_numpy_ba(nb, gone, fold)
    keep_f = ~np.isin(lmk0, gone)
    keep_l = np.zeros(p.n_lmks, bool)
    keep_l[lmk0[keep_f]] = True
    keep_c = np.zeros(p.n_cams, bool)
    keep_c[cam0[keep_f]] = True
    assert not keep_c[8] and keep_c.sum() == p.n_cams - 1
    assert not keep_l[gone].any()
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
def test_host_retirement_equals_a_graph_of_the_survivors_with_the_state_injected(loss):
    """Retiring on the object graph and sweeping on equals a NumpyBA built from the survivors' problem alone into which the folded camera
    priors (old prior + the departing factors' messages), the messages and the factors' state are injected."""
    p = _problem()
    nb = _host(p, sweeps=5, loss=loss)
    arrays = graph_arrays(nb)
    n_before = len(nb.graph.factors)
    bel_before = {id(v): (v.belief.eta.copy(), v.belief.lam.copy()) for v in nb.cams + nb.lmks}
    pri_before = {id(v): (v.prior.eta.copy(), v.prior.lam.copy()) for v in nb.cams + nb.lmks}
    lmk_index = {id(v): i for i, v in enumerate(nb.lmks)}
    msgs = {id(v): [(f.messages[0].eta.copy(), f.messages[0].lam.copy(), lmk_index[id(f.adj_var_nodes[1])]) for f in v.adj_factors] for v in nb.cams}
    gone = _list_that_orphans_a_camera(arrays[3], arrays[4], 8)
    cm, lm, fm = retire_landmarks_numpy_ba(nb, gone, True)
    assert n_before - len(nb.graph.factors) == int((fm < 0).sum()) > 0 and cm[8] == -1
    for v in nb.lmks:                                           # landmark priors never change
        assert np.array_equal(v.prior.eta, pri_before[id(v)][0]) and np.array_equal(v.prior.lam, pri_before[id(v)][1])
    touched = 0
    for v in nb.cams:                                           # camera priors: + the departing factors' messages, in adj_factors order
        eta, lam = pri_before[id(v)]
        for me, ml, l in msgs[id(v)]:
            if l in gone:
                eta, lam = eta + me, lam + ml
                touched += 1
        assert np.array_equal(v.prior.eta, eta) and np.array_equal(v.prior.lam, lam)
    assert touched
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


def test_host_drop_leaves_every_prior_alone():
    p = _problem()
    nb = _host(p, sweeps=3)
    pri_before = {id(v): (v.prior.eta.copy(), v.prior.lam.copy()) for v in nb.cams + nb.lmks}
    retire_landmarks_numpy_ba(nb, [5, 16, 27, 100], fold=False)
    for v in nb.cams + nb.lmks:
        assert np.array_equal(v.prior.eta, pri_before[id(v)][0]) and np.array_equal(v.prior.lam, pri_before[id(v)][1])


def test_host_retirement_rejects_bad_lists_and_accepts_an_empty_one():
    nb = _host(_problem(), sweeps=1)
    for bad in ([160], [-1], [2, 2], list(range(160))):
        with pytest.raises(ValueError):
            retire_landmarks_numpy_ba(nb, bad)
    F = len(nb.graph.factors)
    cm, lm, fm = retire_landmarks_numpy_ba(nb, [])
    np.testing.assert_array_equal(cm, np.arange(12))
    np.testing.assert_array_equal(lm, np.arange(160))
    np.testing.assert_array_equal(fm, np.arange(F))
    assert len(nb.graph.factors) == F and nb.L == 160


@pytest.mark.parametrize('tag', ['small', 'vsmall_huber'])
def test_host_retirement_replays_reference_fixture_g20(tag):
    """tests/retire_lmk_host.py retires landmarks from a NumpyBA the way make_g20.py retired them from the reference's own graph: the G20
    trajectory (a FOLD of a non-prefix list that orphans a camera, then a DROP, ba.py's schedule) agrees to 1e-8 in every belief, folded
    camera prior and message, through every sweep."""
    from conftest import golden
    from retire_lmk_host import HostGraph, g20_problem, g20_replay
    g = golden(f'G20_retire_lmk_{tag}')
    cm, ids = g['r1_cam_map'], g['r1_lmk_ids']
    assert (cm < 0).sum() == 1 and cm[-1] >= 0 and cm[0] == 0 and 0 not in ids       # neither map of the first call is a shift
    worst = g20_replay(g, HostGraph(g20_problem(g), None if str(g['loss']) == 'None' else str(g['loss'])), belief_tol=1e-8, msg_tol=1e-8)
    assert worst < 1e-8
