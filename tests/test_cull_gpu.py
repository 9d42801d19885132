"""gbp_ba_cull / BAEngine.cull and gbp_ba_get_residuals / BAEngine.residuals on the GPU: single observations leave a live BA graph, their
messages are DROPPED (nothing is folded into any prior), cameras and landmarks left without a factor leave too and everything that
stays keeps its GBP state.  The sibling of tests/test_retire_gpu.py.

Oracles: tests/cull_host.py culls the same factors from the reference's own object graph (NumpyBA), and fixture G19 is the reference's
own run (tests/golden/make_g19.py); the tests cull the STORED lists.  The structural checks pin the shrunk handle to a handle freshly
created from the survivors and the carried state to its value before the call, bit for bit.  Tolerances are those of the retire tests:
1e-9 against the host oracle, beliefs 1e-6 and messages 1e-5 against the reference fixture."""
import numpy as np
import pytest

from conftest import rel_err_rows
from cull_host import make_numpy_ba, cull_numpy_ba
from retire_host import retire_numpy_ba, survivors_problem

pytestmark = pytest.mark.gpu

W = 50.0
HOST_TOL = 1e-9


@pytest.fixture(scope='module')
def lib():
    from gbp_amd import build
    build.build()
    from gbp_amd import _capi
    return _capi


def _problem(n_cams=12, n_lmks=160, obs=4, window=5, seed=2, **kw):
    from gbp_amd.synthetic import make_synthetic
    return make_synthetic(n_cams=n_cams, n_lmks=n_lmks, obs_per_lmk=obs, window=window, seed=seed, **kw)


def _engine(problem, **kw):
    from gbp_amd.engine import BAEngine
    e = BAEngine.from_problem(problem, **kw)
    e.generate_priors_var(W)
    e.update_all_beliefs()
    return e


def _host(problem, **kw):
    nb = make_numpy_ba(problem, **kw)
    nb.generate_priors_var(W)
    nb.update_all_beliefs()
    return nb


def _state(e):
    return dict(bel=e.beliefs(), msg=e.messages(), fac=e.factors(dense=False), rs=e.relin_state(), pri=e.priors())


def _bitwise(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _list(e, cam=3, lmk=17, step=11):
    """All factors of camera `cam` and of landmark `lmk` (both become orphans) and every `step`-th factor from the 5th on."""
    fac = e.factors(dense=False)
    return np.union1d(np.flatnonzero((fac['cam'] == cam) | (fac['lmk'] == lmk)), np.arange(5, e.F, step)).astype(np.int32)


def _gap_to_host(e, nb, where):
    worst = 0.0
    for k, (a, h) in enumerate(zip(e.beliefs(), nb.beliefs())):
        gap = rel_err_rows(a, h)
        print(f'{where}: belief array {k} against the host oracle {gap:.3e}')
        assert gap <= HOST_TOL, (where, k, gap)
        worst = max(worst, gap)
    return worst


def _same_relin(e, nb):
    rs = e.relin_state()
    np.testing.assert_array_equal(rs['iters_since_relin'], [f.iters_since_relin for f in nb.graph.factors])
    np.testing.assert_array_equal(rs['eta_damping'], [f.eta_damping for f in nb.graph.factors])


# ---- 1. the reference's own run ---------------------------------------------------------------------------------------------------
class _EngineGraph:
    """BAEngine behind the methods g19_replay calls (tests/cull_host.py)."""

    def __init__(self, base, loss, fused):
        from gbp_amd.engine import BAEngine
        self.e = BAEngine.from_problem(base, loss=loss, fused=fused)

    def __getattr__(self, name):
        return getattr(self.e, name)

    def relin(self):
        rs = self.e.relin_state()
        return rs['iters_since_relin'], rs['eta_damping'], rs['adaptive_var']


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('tag', ['small', 'vsmall_huber'])
def test_g19_reference_cull_replay(lib, tag, fused):
    """Fixture G19: the reference's own classes ran this schedule (make_g19.py).  Maps equal, relinearisation counts exact every sweep,
    the per-factor residual view before each cull, all priors and beliefs after it and at batch ends < 1e-6, messages < 1e-5, ARE / energy
    at the G18 replay's tolerances, iters_since_relin and eta_damping exact at batch ends -- through both culls and all 30 sweeps."""
    from conftest import golden
    from cull_host import g19_problem, g19_replay
    g = golden(f'G19_cull_{tag}')
    eg = _EngineGraph(g19_problem(g), None if str(g['loss']) == 'None' else str(g['loss']), fused)
    worst = g19_replay(g, eg, belief_tol=1e-6, msg_tol=1e-5, verbose=True)
    print(f'G19 {tag} fused={fused}: worst belief gap {worst:.3e}')
    assert worst < 1e-6
    assert eg.e.check_layout() == 0
    eg.e.close()


# ---- 2. the residual view ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss', [None, 'huber'])
def test_residual_view_sums_ranges_and_host(lib, loss):
    p = _problem()
    e, nb = _engine(p, loss=loss), _host(p, loss=loss)
    e.iterate(4)
    nb.iterate(4)
    r2, m, av = e.residuals()
    assert r2.shape == (e.F, 2) and m.shape == (e.F,) and av.shape == (e.F,)
    host = np.array([f.compute_residual() for f in nb.graph.factors])
    gap = np.abs(r2 - host).max() / np.abs(host).max()
    print(f'residual view against the host oracle: {gap:.3e}')
    assert gap <= HOST_TOL
    nr = np.linalg.norm(r2, axis=1)
    np.testing.assert_allclose(m, nr / 2.0, rtol=1e-14)                       # gauss_noise_std = 2
    assert _bitwise(av, e.relin_state()['adaptive_var'])
    if loss:
        assert (av != 4.0).any()
    sums = e.residual_sums()                                                # the same numbers in another summation order
    np.testing.assert_allclose([nr.sum(), (0.5 * nr * nr / av).sum()], sums, rtol=1e-12)
    assert abs(e.are() - nr.mean()) <= 1e-12 * e.are()
    for f0, n in ((0, 1), (63, 130), (e.F - 7, 7), (5, 0)):                  # a sub-range is the same rows, bit for bit
        s2, sm, sa = e.residuals(f0, n)
        assert _bitwise(s2, r2[f0:f0 + n]) and _bitwise(sm, m[f0:f0 + n]) and _bitwise(sa, av[f0:f0 + n])
    only = np.empty(e.F)
    assert lib.load().gbp_ba_get_residuals(e._h, 0, e.F, None, lib.dptr(only), None) == 0 and _bitwise(only, m)
    for f0, n in ((-1, 2), (0, e.F + 1), (e.F, 1), (0, -1)):
        assert lib.load().gbp_ba_get_residuals(e._h, f0, n, None, lib.dptr(only), None) == -1
    e.close()
    from gbp_amd.engine import BAEngine
    f = BAEngine.from_problem(p)                                            # no beliefs yet
    with pytest.raises(lib.GbpError) as ei:
        f.residuals()
    assert ei.value.code == -5
    f.close()


def test_cull_outliers_is_the_view_plus_a_threshold(lib):
    p = _problem()
    a, b = _engine(p), _engine(p)
    for e in (a, b):
        e.iterate(3)
    m = a.residuals()[1]
    nstds = float(np.sort(m)[-20] + np.sort(m)[-21]) / 2                    # between two values: 20 factors exceed it
    ids, cm, lm, fm = a.cull_outliers(nstds)
    np.testing.assert_array_equal(ids, np.flatnonzero(m > nstds))
    assert ids.size == 20 and (fm < 0).sum() == 20 and a.F == b.F - 20
    for x, y in zip((cm, lm, fm), b.cull(ids)):
        np.testing.assert_array_equal(x, y)
    assert _bitwise(a.save_state(), b.save_state())
    blob = a.save_state()
    ids, cm, lm, fm = a.cull_outliers(1e9)                                  # none exceeds it: nothing happens
    assert ids.size == 0 and np.array_equal(fm, np.arange(a.F)) and _bitwise(a.save_state(), blob)
    a.close()
    b.close()


# ---- 3. carried state is bitwise, nothing is folded --------------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [True, False])
def test_carry_is_bitwise(lib, fused):
    p = _problem()
    e = _engine(p, loss='huber', fused=fused)
    e.iterate(4)
    before = _state(e)
    cam, lmk = before['fac']['cam'], before['fac']['lmk']
    # all factors of camera 3 and of landmark 17 (both become orphans) and every 3rd factor of cameras 6 to 8: other cameras stay untouched
    ids = np.union1d(np.flatnonzero((cam == 3) | (lmk == 17)), np.flatnonzero((cam >= 6) & (cam <= 8))[::3]).astype(np.int32)
    cm, lm, fm = e.cull(ids)
    after = _state(e)
    kc, kl, kf = cm >= 0, lm >= 0, fm >= 0
    assert (~kf).sum() == ids.size and not kc[3] and not kl[17] and kc.sum() == 11 and (e.C, e.L, e.F) == (kc.sum(), kl.sum(), kf.sum())
    np.testing.assert_array_equal(fm[kf], np.arange(kf.sum()))
    for k in range(4):
        assert _bitwise(after['msg'][k], before['msg'][k][kf])
    for key in ('linpoint', 'z'):
        assert _bitwise(after['fac'][key], before['fac'][key][kf])
    np.testing.assert_array_equal(after['fac']['cam'], cm[before['fac']['cam'][kf]])
    np.testing.assert_array_equal(after['fac']['lmk'], lm[before['fac']['lmk'][kf]])
    for key in ('iters_since_relin', 'eta_damping', 'adaptive_var', 'robust_flag'):
        assert _bitwise(after['rs'][key], before['rs'][key][kf])
    for k, keep in zip(range(4), (kc, kc, kl, kl)):                         # EVERY surviving prior, bit for bit: nothing was folded
        assert _bitwise(after['pri'][k], before['pri'][k][keep])
    # beliefs: prior + the surviving messages; a variable none of whose factors went keeps its belief up to summation order
    tc, tl = np.zeros(p.n_cams, bool), np.zeros(p.n_lmks, bool)
    tc[before['fac']['cam'][~kf]] = True
    tl[before['fac']['lmk'][~kf]] = True
    assert (tl & kl).any() and (~tl & kl).any() and (tc & kc).any() and (~tc & kc).any()
    for k, keep, touched in zip(range(4), (kc, kc, kl, kl), (tc, tc, tl, tl)):
        gap = rel_err_rows(after['bel'][k][~touched[keep]], before['bel'][k][keep & ~touched])
        print(f'cull: untouched belief array {k} moved by {gap:.3e}')
        assert gap <= 1e-12
    want = [a.copy() for a in after['pri']]
    for f in range(e.F):
        c, l = after['fac']['cam'][f], after['fac']['lmk'][f]
        for k, v in ((0, c), (1, c), (2, l), (3, l)):
            want[k][v] += after['msg'][k][f]
    for k in range(4):
        gap = rel_err_rows(after['bel'][k], want[k])
        print(f'cull: belief array {k} against prior + surviving messages {gap:.3e}')
        # the landmark view inverts the stored covariance: ~cond(Lambda) * 1e-16 (gbp_view_kernels.hpp).  Lambda >= the prior m / W^2 I with m
        # the largest factor entry, and at most 4 messages of entries ~m on top: cond <~ 4 W^2 = 1e4, with a factor ten to spare 1e-11
        assert gap <= 1e-10
    assert e.check_layout() == 0
    e.close()


# ---- 4. cull = create of the survivors + the carried state ------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [True, False, None])
def test_cull_equals_create_plus_state(lib, fused):
    p = _problem()
    runs = []
    for _ in range(2):
        e = _engine(p, fused=fused)
        e.iterate(3)
        fac = e.factors(dense=False)
        means = e.means()
        maps = e.cull(_list(e))
        runs.append(e)
    a, b2 = runs
    assert _bitwise(a.save_state(), b2.save_state())           # reproducible run to run
    f = _engine(survivors_problem((p.K, means[0], means[1], fac['z'], fac['cam'], fac['lmk']), *maps), fused=fused)
    assert a.plan_info() == f.plan_info() and a.info() == f.info()
    f.load_state(a.save_state())                              # same graph hash, same layout
    a.iterate(5)
    f.iterate(5)
    sa, sf = _state(a), _state(f)
    for k in range(4):
        assert _bitwise(sa['bel'][k], sf['bel'][k]) and _bitwise(sa['msg'][k], sf['msg'][k])
    for key in ('iters_since_relin', 'eta_damping'):
        assert _bitwise(sa['rs'][key], sf['rs'][key])
    assert _bitwise(a.save_state(), f.save_state())
    for e in runs + [f]:
        e.close()


# ---- 5. a reordered handle ---------------------------------------------------------------------------------------------------------
def test_reordered_handle_culls_in_the_callers_numbering(lib):
    """The criterion of tests/test_reorder_gpu.py for a live graph: the maps are the caller's numbering, flag or no flag; user-order
    views agree with a handle without the flag driven the same way (1e-7, relinearisation ages exactly); the survivors are ordered
    afresh by the rule."""
    from reorder_host import shuffle_landmarks, rule_order
    q, _ = shuffle_landmarks(_problem(n_cams=16, n_lmks=300, window=4), seed=7)
    a, plain = _engine(q, reorder_landmarks=True, loss='huber'), _engine(q, loss='huber')
    assert not np.array_equal(a.landmark_order(), np.arange(a.L))
    for e in (a, plain):
        e.iterate(3)
    ids = _list(plain)
    np.testing.assert_array_equal(ids, _list(a))
    for x, y in zip(a.residuals(), plain.residuals()):
        np.testing.assert_allclose(x, y, rtol=1e-7, atol=1e-7 * np.abs(y).max())
    ma, mp = a.cull(ids), plain.cull(ids)
    for x, y in zip(ma, mp):
        np.testing.assert_array_equal(x, y)
    assert ma[1][17] == -1
    for e in (a, plain):
        e.iterate(3)
    fa, fp = a.factors(dense=False), plain.factors(dense=False)
    np.testing.assert_array_equal(fa['cam'], fp['cam'])
    np.testing.assert_array_equal(fa['lmk'], fp['lmk'])
    np.testing.assert_array_equal(a.landmark_order(), rule_order(fa['cam'], fa['lmk'], a.C, a.L))
    assert a.check_layout() == 0
    for name in ('beliefs', 'priors', 'means', 'residuals'):
        for x, y in zip(getattr(a, name)(), getattr(plain, name)()):
            gap = rel_err_rows(x, y)
            assert gap < 1e-7, (name, gap)
    assert np.array_equal(a.iters_since_relin(), plain.iters_since_relin())
    a.close()
    plain.close()


# ---- 6. landmarks above a tile ----------------------------------------------------------------------------------------------------
def test_chunk_tile_landmark_loses_factors_from_the_middle(lib):
    """Landmarks of 70 observations live in chunk tiles (plan pack_mode >= 1).  Landmark 0 loses 4 factors from the middle of its list
    and stays above a tile, landmark 1 loses 8 and falls below it, landmark 2 goes altogether."""
    from gbp_amd.synthetic import make_synthetic, BAProblem
    big = make_synthetic(n_cams=80, n_lmks=6, obs_per_lmk=70, window=80, seed=4)
    few = make_synthetic(n_cams=80, n_lmks=60, obs_per_lmk=2, window=8, seed=5)
    p = BAProblem(K=big.K, cam_means=big.cam_means, lmk_means=np.concatenate([big.lmk_means, few.lmk_means]),
                  meas=np.concatenate([big.meas, few.meas]), cam_idx=np.concatenate([big.cam_idx, few.cam_idx]),
                  lmk_idx=np.concatenate([big.lmk_idx, few.lmk_idx + 6]).astype(np.int32))
    assert np.bincount(p.cam_idx, minlength=p.n_cams).min() > 0
    e, nb = _engine(p, loss='huber'), _host(p, loss='huber')
    assert e.plan_info()['pack_mode'] >= 1, e.plan_info()
    e.iterate(3)
    nb.iterate(3)
    lmk = e.factors(dense=False)['lmk']
    of = [np.flatnonzero(lmk == l) for l in range(3)]
    assert all(o.size == 70 for o in of)
    ids = np.concatenate([of[0][33:37], of[1][20:24], of[1][40:44], of[2]]).astype(np.int32)
    for x, y in zip(e.cull(ids), cull_numpy_ba(nb, ids)):
        np.testing.assert_array_equal(x, y)
    assert e.plan_info()['pack_mode'] >= 1 and e.check_layout() == 0
    deg = np.bincount(e.factors(dense=False)['lmk'], minlength=e.L)
    assert deg[0] == 66 and deg[1] == 62 and e.L == p.n_lmks - 1
    _gap_to_host(e, nb, 'chunk tiles, after the cull')
    e.iterate(4)
    nb.iterate(4)
    _gap_to_host(e, nb, 'chunk tiles, 4 sweeps on')
    _same_relin(e, nb)
    e.close()


# ---- 7. state that must survive ---------------------------------------------------------------------------------------------------
def _tracks_host(setup, step, **kw):
    """Set both up, cull, step both: the engine stays with the host model."""
    p = _problem()
    e, nb = _engine(p, **kw), _host(p, **kw)
    for x in (e, nb):
        setup(x)
    ids = _list(e)
    for a, b in zip(e.cull(ids), cull_numpy_ba(nb, ids)):
        np.testing.assert_array_equal(a, b)
    _gap_to_host(e, nb, 'after the cull')
    for x in (e, nb):
        step(x)
    _gap_to_host(e, nb, 'after the steps')
    _same_relin(e, nb)
    return e


def test_dense_remainder_is_carried(lib):
    e = _tracks_host(lambda x: x.iterate(9), lambda x: x.iterate(9), num_undamped_iters=0)
    e.close()


def test_pending_relinearisation_survives_cull(lib):
    def setup(x):
        x.iterate(9)
        (x.relinearise_factors if hasattr(x, 'relinearise_factors') else x.graph.relinearise_factors)()

    def step(x):
        if hasattr(x, 'compute_all_messages'):
            x.compute_all_messages()
        else:
            x.graph.compute_all_messages()
        x.update_all_beliefs()
        x.iterate(3)
    e = _tracks_host(setup, step)
    e.close()


def test_empty_list_continues_bitwise(lib):
    p = _problem()
    a, twin = _engine(p), _engine(p)
    a.iterate(3)
    twin.iterate(3)
    cm, lm, fm = a.cull([])
    np.testing.assert_array_equal(cm, np.arange(a.C))
    np.testing.assert_array_equal(lm, np.arange(a.L))
    np.testing.assert_array_equal(fm, np.arange(a.F))
    assert lib.load().gbp_ba_cull(a._h, 0, None, None, None, None) == 0
    assert _bitwise(a.save_state(), twin.save_state())
    a.iterate(4)
    twin.iterate(4)
    assert _bitwise(a.save_state(), twin.save_state())
    np.testing.assert_array_equal(a.relin_counts(7), twin.relin_counts(7))
    a.close()
    twin.close()


def test_snapshot_is_dropped_and_means_stream_after_a_cull(lib):
    e = _engine(_problem())
    e.iterate(2)
    e.snapshot_state()
    e.means_snapshot()
    e.cull(_list(e))
    with pytest.raises(lib.GbpError) as ei:
        e.restore_snapshot()
    assert ei.value.code == -5
    e.means_snapshot()
    cm, lm = e.means_fetch(wait=True)
    rc, rl = e.means()
    assert cm.shape == (11, 6) and _bitwise(cm, rc) and _bitwise(lm, rl)
    e.close()


# ---- 8. composition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss', [None, 'huber'])
def test_extend_cull_retire_iterate_tracks_the_host(lib, loss):
    from gbp_amd.synthetic import keyframe_batches
    from extend_host import extend as host_extend
    sp = keyframe_batches(_problem(n_cams=16, n_lmks=200, window=5), [12, 4])
    e, nb = _engine(sp.base, loss=loss), _host(sp.base, loss=loss)
    for x in (e, nb):
        x.iterate(3)
    b = sp.batches[0]
    e.extend(b['cam_means'], b['lmk_means'], b['meas'], b['cam_idx'], b['lmk_idx'], prior_weaker_factor=W)
    host_extend(nb, b, prior_weaker_factor=W)
    for x in (e, nb):
        x.iterate(2)
    ids = _list(e, cam=5, lmk=30, step=9)
    for x, y in zip(e.cull(ids), cull_numpy_ba(nb, ids)):
        np.testing.assert_array_equal(x, y)
    _gap_to_host(e, nb, 'extend, cull')
    for x in (e, nb):
        x.iterate(2)
    for x, y in zip(e.retire([0, 1]), retire_numpy_ba(nb, [0, 1])):
        np.testing.assert_array_equal(x, y)
    _gap_to_host(e, nb, 'extend, cull, retire')
    for s in range(4):
        e.iterate(1)
        nb.iterate(1)
        np.testing.assert_array_equal(e.iters_since_relin() == 0, np.array([f.iters_since_relin == 0 for f in nb.graph.factors]))
    _gap_to_host(e, nb, 'extend, cull, retire, 4 sweeps')
    _same_relin(e, nb)
    assert abs(e.are() - nb.are()) <= HOST_TOL * abs(nb.are())
    assert e.check_layout() == 0
    e.close()


# ---- 9. failures leave the handle as it was ---------------------------------------------------------------------------------------
def _untouched(a, twin, blob):
    assert (a.C, a.L, a.F) == (twin.C, twin.L, twin.F)
    assert _bitwise(a.save_state(), blob)
    for name in ('beliefs', 'priors', 'messages', 'residuals'):
        for x, y in zip(getattr(a, name)(), getattr(twin, name)()):
            assert _bitwise(x, y), name


def test_failures_leave_the_handle_untouched(lib):
    from gbp_amd.engine import BAEngine
    p = _problem()
    a, twin = _engine(p), _engine(p)
    for e in (a, twin):
        e.iterate(3)
    blob = a.save_state()
    F = a.F
    for bad, names in (([2, 7, 2], 'entry 2'), ([F], 'entry 0'), ([4, -1], 'entry 1'), (list(range(F)), None)):
        with pytest.raises(lib.GbpError) as ei:
            a.cull(bad)
        assert ei.value.code == -1, bad
        if names:
            assert names in str(ei.value), str(ei.value)                   # the message names the entry
        _untouched(a, twin, blob)
    ids = np.array([1], np.int32)
    h = a._h
    assert lib.load().gbp_ba_cull(h, -1, lib.iptr(ids), None, None, None) == -1
    assert lib.load().gbp_ba_cull(h, 1, None, None, None, None) == -1
    _untouched(a, twin, blob)
    a.iterate(1)
    twin.iterate(1)
    assert _bitwise(a.save_state(), twin.save_state())
    a.close()
    twin.close()
    # no beliefs yet: the handle then goes on as an untouched one
    f, ft = BAEngine.from_problem(p), BAEngine.from_problem(p)
    with pytest.raises(lib.GbpError) as ei:
        f.cull([0])
    assert ei.value.code == -5
    for x in (f, ft):
        x.generate_priors_var(W)
        x.update_all_beliefs()
        x.iterate(1)
    assert _bitwise(f.save_state(), ft.save_state())
    f.close()
    ft.close()


def test_sharded_handles_refuse_to_cull(lib):
    """A 2-rank peer-store set-up on one GPU and an exchange callback: GBP_ESTATE, the state blob bitwise what it was."""
    p = _problem()

    def pair():
        r = [_engine(p), _engine(p)]
        hs = [e.peer_export(2, same_process=True) for e in r]
        for k, e in enumerate(r):
            e.peer_connect(k, hs, same_process=True, rendezvous=True)
        return r
    shrunk, twin = pair(), pair()
    for e in shrunk:
        with pytest.raises(lib.GbpError) as ei:
            e.cull([0])
        assert ei.value.code == -5
    for x, y in zip(shrunk, twin):
        assert _bitwise(x.save_state(), y.save_state())
        for u, v in zip(x.messages(), y.messages()):
            assert _bitwise(u, v)
    for e in shrunk + twin:
        e.close()
    g, gt = _engine(p), _engine(p)
    for x in (g, gt):
        x.set_exchange(lambda s_, r_, n_, st: 0, 0, 1)
    with pytest.raises(lib.GbpError) as ei:
        g.cull([0])
    assert ei.value.code == -5
    for x in (g, gt):
        x.iterate_sharded(1)
    assert _bitwise(g.save_state(), gt.save_state())
    for u, v in zip(g.beliefs(), gt.beliefs()):
        assert _bitwise(u, v)
    g.close()
    gt.close()


# ---- 10. the drop-in package ------------------------------------------------------------------------------------------------------
def test_compat_graph_culls_and_reports_residuals(lib):
    import sys
    import os
    from conftest import REPO
    sys.path.insert(0, os.path.join(REPO, 'gbp_amd', 'compat'))
    try:
        from gbp.gbp_ba import BAFactorGraph
    finally:
        sys.path.remove(os.path.join(REPO, 'gbp_amd', 'compat'))
    p = _problem()
    cfg = dict(gauss_noise_std=2.0, loss=None, Nstds=3.0, beta=0.01, num_undamped_iters=6, min_linear_iters=8, eta_damping=0.4)
    g = BAFactorGraph(p, cfg)
    g.generate_priors_var(W)
    g.update_all_beliefs()
    g.synchronous_iteration()
    res = g.compute_residuals()
    assert isinstance(res, list) and len(res) == 2 * len(g.factors)
    one_by_one = np.concatenate([f.compute_residual() for f in g.factors])
    np.testing.assert_allclose(res, one_by_one, rtol=1e-12, atol=1e-12 * np.abs(one_by_one).max())
    assert abs(g.factors[7].reprojection_err() - np.hypot(res[14], res[15])) <= 1e-12 * np.hypot(res[14], res[15])
    its = np.array([f.iters_since_relin for f in g.factors])
    cam_of = np.array([f.adj_vIDs[0] for f in g.factors])
    mu5 = np.array(g.cam_nodes[5].mu)
    ids = _list(g._engine)
    cm, lm, fm = g.cull_observations(ids)
    kf = fm >= 0
    assert len(g.cam_nodes) == 11 and len(g.lmk_nodes) == int((lm >= 0).sum()) and len(g.factors) == int(kf.sum()) == its.size - ids.size
    assert len(g.var_nodes) == len(g.cam_nodes) + len(g.lmk_nodes) and g.n_factor_nodes == len(g.factors) and g.n_edges == 2 * len(g.factors)
    assert [f.iters_since_relin for f in g.factors] == list(its[kf])
    fac = g._engine.factors(dense=False)
    for i in range(0, len(g.factors), 37):
        assert list(g.factors[i].adj_vIDs) == [int(fac['cam'][i]), len(g.cam_nodes) + int(fac['lmk'][i])]
    np.testing.assert_array_equal([f.adj_vIDs[0] for f in g.factors], cm[cam_of[kf]])
    assert cm[5] == 4 and np.array_equal(g.cam_nodes[4].mu, g._engine.means()[0][4])                       # the views index the survivors
    assert not np.array_equal(g.cam_nodes[4].mu, mu5)                                                     # (camera 5 lost factors: its belief moved)
    assert len(g.compute_residuals()) == 2 * len(g.factors)
    g.synchronous_iteration()
    assert np.isfinite(g.are())
