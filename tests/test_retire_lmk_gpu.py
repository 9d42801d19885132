"""gbp_ba_retire_landmarks / BAEngine.retire_landmarks on the GPU: landmarks leave a live BA graph by name, what their factors told the
cameras is folded into the cameras' priors (fold=True) or discarded (fold=False), and everything that stays keeps its GBP state.  The
mirror image of tests/test_retire_gpu.py.

Oracle: tests/retire_lmk_host.py retires the same landmarks from the reference's own object graph (NumpyBA) and replays fixture G20
(the reference's own run).  The structural checks pin the shrunk handle to a handle freshly created from the survivors, the carried
state to its value before the call bit for bit, the folded priors to the message view, and the DROP mode to gbp_ba_cull."""
import numpy as np
import pytest

from conftest import rel_err_rows
from retire_host import survivors_problem
from retire_lmk_host import make_numpy_ba, retire_landmarks_numpy_ba, renumbering

pytestmark = pytest.mark.gpu

W = 50.0


@pytest.fixture(scope='module')
def lib():
    from gbp_amd import build
    build.build()
    from gbp_amd import _capi
    return _capi


def _problem(n_cams=16, n_lmks=150, obs=4, window=6, seed=1, **kw):
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


def _orphaning_list(p, cam=9, extra=(7, 33, 140)):
    """every landmark of camera `cam` (the camera is orphaned) and a few more; landmark 0 stays: no prefix"""
    ids = sorted(set(int(l) for l in p.lmk_idx[p.cam_idx == cam]) | set(extra))
    assert 0 not in ids
    return np.array(ids, np.int32)


def _gap_to_host(e, nb, where, tol=1e-7):
    worst = 0.0
    for a, h in zip(e.beliefs(), nb.beliefs()):
        gap = rel_err_rows(a, h)
        assert gap < tol, (where, gap)
        worst = max(worst, gap)
    pe = e.priors()
    ph = (np.array([v.prior.eta for v in nb.cams]), np.array([v.prior.lam for v in nb.cams]),
          np.array([v.prior.eta for v in nb.lmks]), np.array([v.prior.lam for v in nb.lmks]))
    for a, h in zip(pe, ph):
        gap = rel_err_rows(a, h)
        assert gap < tol, (where, 'priors', gap)
    return worst


def _same_relin(e, nb):
    rs = e.relin_state()
    np.testing.assert_array_equal(rs['iters_since_relin'], [f.iters_since_relin for f in nb.graph.factors])
    np.testing.assert_array_equal(rs['eta_damping'], [f.eta_damping for f in nb.graph.factors])


# ---- 1. the reference's own run ---------------------------------------------------------------------------------------------------
class _EngineGraph:
    """BAEngine behind the methods g20_replay calls (tests/retire_lmk_host.py)."""

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
def test_g20_reference_landmark_retirement_replay(lib, tag, fused):
    """Fixture G20: the reference's own classes ran this schedule (make_g20.py): a FOLD of a non-prefix list that orphans a camera, then a
    DROP.  Maps equal, relinearisation counts exact every sweep, beliefs and the folded camera priors < 1e-6, messages < 1e-5, ARE / energy
    1e-6 / 1e-5 relative, iters_since_relin and eta_damping exact at batch ends -- the tolerances gbp_ba_retire is held to against G18."""
    from conftest import golden
    from retire_lmk_host import g20_problem, g20_replay
    g = golden(f'G20_retire_lmk_{tag}')
    eg = _EngineGraph(g20_problem(g), None if str(g['loss']) == 'None' else str(g['loss']), fused)
    worst = g20_replay(g, eg, belief_tol=1e-6, msg_tol=1e-5, verbose=True)
    print(f'G20 {tag} fused={fused}: worst belief gap {worst:.3e}')
    assert worst < 1e-6
    eg.e.close()


# ---- 2. carried state is bitwise ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [True, False])
def test_carry_is_bitwise(lib, fused):
    """Right after a FOLD call the surviving beliefs are what they were: the folded prior holds exactly the messages the belief sum has
    lost, so only the summation order differs.  Bound 1e-7 relative (the one tests/test_retire_gpu.py puts on the same statement about
    gbp_ba_retire); on the reference's own objects make_g20.py printed a gap of 1.0e-15 for both runs, and this test prints its own
    (about 1e-16 to 1e-15 is expected: fp64 sums of a few dozen terms in another order).  Everything else that stays is bitwise: landmark
    priors, the priors of cameras that lost no factor, every surviving factor's linearisation point, messages, adaptive variance and
    relinearisation state."""
    p = _problem()
    e = _engine(p, loss='huber', fused=fused)
    e.iterate(4)
    before = _state(e)
    ids = _orphaning_list(p)
    cm, lm, fm = e.retire_landmarks(ids)
    after = _state(e)
    kc, kl, kf = cm >= 0, lm >= 0, fm >= 0
    np.testing.assert_array_equal(kf, ~np.isin(before['fac']['lmk'], ids))
    np.testing.assert_array_equal(fm, renumbering(kf))
    assert cm[9] == -1 and kc.sum() == 15 and not kl[ids].any() and kl.sum() == p.n_lmks - ids.size
    np.testing.assert_array_equal(cm, renumbering(kc))
    np.testing.assert_array_equal(lm, renumbering(kl))
    for k in range(4):
        assert _bitwise(after['msg'][k], before['msg'][k][kf])
    for key in ('linpoint', 'z'):
        assert _bitwise(after['fac'][key], before['fac'][key][kf])
    np.testing.assert_array_equal(after['fac']['cam'], cm[before['fac']['cam'][kf]])
    np.testing.assert_array_equal(after['fac']['lmk'], lm[before['fac']['lmk'][kf]])
    for key in ('iters_since_relin', 'eta_damping', 'adaptive_var', 'robust_flag'):
        assert _bitwise(after['rs'][key], before['rs'][key][kf])
    for k, keep in zip(range(4), (kc, kc, kl, kl)):
        gap = rel_err_rows(after['bel'][k], before['bel'][k][keep])
        print(f'retire_landmarks fused={fused}: belief array {k} moved by {gap:.3e}')
        assert gap < 1e-7
    assert _bitwise(after['pri'][2], before['pri'][2][kl]) and _bitwise(after['pri'][3], before['pri'][3][kl])
    lost = np.zeros(p.n_cams, bool)
    lost[before['fac']['cam'][~kf]] = True
    assert (kc & ~lost).any() and (kc & lost).any()
    assert _bitwise(after['pri'][0][~lost[kc]], before['pri'][0][kc & ~lost])
    assert _bitwise(after['pri'][1][~lost[kc]], before['pri'][1][kc & ~lost])
    assert not _bitwise(after['pri'][0][lost[kc]], before['pri'][0][kc & lost])
    assert e.check_layout() == 0
    e.close()


# ---- 3. the folded camera priors against the message view ------------------------------------------------------------------------
def _three_chunk_problem():
    """6 cameras x 300 landmarks x 3 observations, every camera with exactly 150 factors: three chunks of the fold, the last one partial.
    Landmarks 0..149 are seen by cameras {0, 1, 2}, landmarks 150..299 by {3, 4, 5}, but for two: landmark 149 by {0, 2, 3} and landmark
    150 by {1, 4, 5}.  (Geometry: all 1 800 observations of the generator's 6 x 300 problem, of which these 900 are kept.)"""
    import dataclasses
    p = _problem(n_cams=6, n_lmks=300, obs=6, window=None, seed=3)
    sees = np.zeros((300, 6), bool)
    sees[:150, :3] = True
    sees[150:, 3:] = True
    sees[149] = [True, False, True, True, False, False]
    sees[150] = [False, True, False, False, True, True]
    keep = sees[p.lmk_idx, p.cam_idx]
    q = dataclasses.replace(p, meas=p.meas[keep], cam_idx=p.cam_idx[keep], lmk_idx=p.lmk_idx[keep])
    assert q.n_factors == 900 and (np.bincount(q.cam_idx) == 150).all()
    return q


def test_folded_priors_are_the_sum_of_the_messages(lib):
    """The list -- landmarks 150..298 -- leaves cameras 0 and 2 without a retiring factor, camera 1 with exactly one (landmark 150),
    camera 3 with all but two and cameras 4 and 5 with all but one (landmark 299).  The new camera prior is the old one plus the numpy
    sum of the departing factors' messages as engine.messages() reported them: < 1e-12 relative of the largest entry (fp64 sums of at
    most 150 terms: 150 x 1.1e-16, the two summation orders together stay a factor of 30 below the bound).  Two runs from the same state
    blob give the same bits."""
    p = _three_chunk_problem()
    a, b = _engine(p, loss='huber'), _engine(p, loss='huber')
    a.iterate(5)
    b.load_state(a.save_state())
    fac, msg, pri0 = a.factors(dense=False), a.messages(), a.priors()
    ids = np.arange(150, 299, dtype=np.int32)
    goes = np.isin(fac['lmk'], ids)
    per_cam = np.bincount(fac['cam'][goes], minlength=6)
    np.testing.assert_array_equal(per_cam, [0, 1, 0, 148, 149, 149])
    maps = a.retire_landmarks(ids)
    maps_b = b.retire_landmarks(ids)
    for x, y in zip(maps, maps_b):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(maps[0], np.arange(6))
    pri1, pri1_b = a.priors(), b.priors()
    for x, y in zip(pri1, pri1_b):
        assert _bitwise(x, y)
    eta, lam = pri0[0].copy(), pri0[1].copy()
    for c in range(6):
        mine = goes & (fac['cam'] == c)
        eta[c] += msg[0][mine].sum(axis=0)
        lam[c] += msg[1][mine].sum(axis=0)
    for c in range(6):
        ge = np.abs(pri1[0][c] - eta[c]).max() / np.abs(eta[c]).max()
        gl = np.abs(pri1[1][c] - lam[c]).max() / np.abs(lam[c]).max()
        print(f'camera {c}: {per_cam[c]} folded, prior eta gap {ge:.2e} lam gap {gl:.2e}')
        assert ge < 1e-12 and gl < 1e-12, c
    for c in (0, 2):                                            # not written at all
        assert _bitwise(pri1[0][c], pri0[0][c]) and _bitwise(pri1[1][c], pri0[1][c])
    assert not _bitwise(pri1[1][1], pri0[1][1])
    a.iterate(3)
    b.iterate(3)
    assert _bitwise(a.save_state(), b.save_state())
    a.close()
    b.close()


# ---- 4. DROP is cull -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [True, False])
def test_drop_equals_cull_of_the_landmarks_factors(lib, fused):
    p = _problem()
    a, b = _engine(p, loss='huber', fused=fused), _engine(p, loss='huber', fused=fused)
    a.iterate(4)
    b.load_state(a.save_state())
    ids = _orphaning_list(p)
    fids = np.flatnonzero(np.isin(a.factors(dense=False)['lmk'], ids)).astype(np.int32)
    pri0 = a.priors()
    ma, mb = a.retire_landmarks(ids, fold=False), b.cull(fids)
    for x, y in zip(ma, mb):
        np.testing.assert_array_equal(x, y)
    assert ma[0][9] == -1
    assert _bitwise(a.save_state(), b.save_state())
    for x, y, keep in zip(a.priors(), pri0, (ma[0] >= 0, ma[0] >= 0, ma[1] >= 0, ma[1] >= 0)):
        assert _bitwise(x, y[keep])                             # nothing is added to any prior
    a.iterate(5)
    b.iterate(5)
    assert _bitwise(a.save_state(), b.save_state())
    a.close()
    b.close()


# ---- 5. retire = create of the survivors + the carried state ---------------------------------------------------------------------
@pytest.mark.parametrize('fused', [True, False, None])
def test_retire_landmarks_equals_create_plus_state(lib, fused):
    p = _problem()
    a = _engine(p, fused=fused)
    a.iterate(3)
    fac, means = a.factors(dense=False), a.means()
    maps = a.retire_landmarks(_orphaning_list(p))
    f = _engine(survivors_problem((p.K, means[0], means[1], fac['z'], fac['cam'], fac['lmk']), *maps), fused=fused)
    assert a.plan_info() == f.plan_info() and a.info() == f.info()
    f.load_state(a.save_state())                              # same graph hash, same layout
    a.iterate(8)
    f.iterate(8)
    sa, sf = _state(a), _state(f)
    for k in range(4):
        assert _bitwise(sa['bel'][k], sf['bel'][k]) and _bitwise(sa['msg'][k], sf['msg'][k]) and _bitwise(sa['pri'][k], sf['pri'][k])
    for key in ('iters_since_relin', 'eta_damping'):
        assert _bitwise(sa['rs'][key], sf['rs'][key])
    a.close()
    f.close()


# ---- 6. edges ----------------------------------------------------------------------------------------------------------------------
def _big_landmark_problem():
    """landmark 0 is seen by all 80 cameras (above a tile: chunk tiles), 60 landmarks by 2 cameras each, 10 by one camera only"""
    from gbp_amd.synthetic import make_synthetic, BAProblem
    big = make_synthetic(n_cams=80, n_lmks=1, obs_per_lmk=80, window=80, seed=4)
    few = make_synthetic(n_cams=80, n_lmks=60, obs_per_lmk=2, window=8, seed=5)
    one = make_synthetic(n_cams=80, n_lmks=10, obs_per_lmk=1, window=8, seed=6)
    parts = (big, few, one)
    off = np.cumsum([0] + [q.n_lmks for q in parts])
    cam = np.concatenate([q.cam_idx for q in parts])
    order = np.argsort(cam, kind='stable')                      # camera-major, as the reference orders a file
    p = BAProblem(K=big.K, cam_means=big.cam_means, lmk_means=np.concatenate([q.lmk_means for q in parts]),
                  meas=np.concatenate([q.meas for q in parts])[order], cam_idx=cam[order].astype(np.int32),
                  lmk_idx=np.concatenate([q.lmk_idx + o for q, o in zip(parts, off)])[order].astype(np.int32))
    deg = np.bincount(p.lmk_idx, minlength=p.n_lmks)
    assert deg[0] == 80 and (deg[1:61] == 2).all() and (deg[61:] == 1).all()
    return p


@pytest.mark.parametrize('which', ['the big one', 'all but the big one', 'degree one'])
def test_landmark_above_a_tile_and_landmarks_of_degree_one(lib, which):
    """A landmark of 80 factors spans chunk tiles (tile packing 1).  Retired alone, every camera folds exactly one message; with everything
    else retired it is the only landmark left (cameras keep one factor each); and a list of degree-1 landmarks with some of degree 2."""
    p = _big_landmark_problem()
    e, nb = _engine(p, loss='huber'), _host(p, loss='huber')
    assert e.plan_info()['pack_mode'] == 1, e.plan_info()
    e.iterate(3)
    nb.iterate(3)
    ids = {'the big one': [0], 'all but the big one': list(range(1, p.n_lmks)), 'degree one': [62, 61, 70, 5, 17]}[which]
    for x, y in zip(e.retire_landmarks(ids), retire_landmarks_numpy_ba(nb, ids)):
        np.testing.assert_array_equal(x, y)
    assert (e.C, e.L, e.F) == (nb.C, nb.L, len(nb.graph.factors)) and e.check_layout() == 0
    if which == 'all but the big one':
        assert (e.C, e.L, e.F) == (80, 1, 80)
    _gap_to_host(e, nb, which)
    e.iterate(4)
    nb.iterate(4)
    _gap_to_host(e, nb, which + ', 4 sweeps on')
    _same_relin(e, nb)
    e.close()


def test_reordered_handle_retires_in_the_callers_numbering(lib):
    """A handle with GBP_FLAG_REORDER_LMKS on a file whose landmark ids are shuffled: ids and maps are the caller's, and the user-order
    views equal those of a handle WITHOUT the flag on the problem relabelled into the internal numbering, driven with the relabelled
    list, to the bound of the carry test (1e-7; relinearisation ages exactly)."""
    from reorder_host import shuffle_landmarks, relabel_landmarks, rule_order
    q, _ = shuffle_landmarks(_problem(n_cams=16, n_lmks=300, window=4), seed=7)
    a = _engine(q, reorder_landmarks=True, loss='huber')
    order = a.landmark_order()                                  # internal id of the caller's landmark
    assert not np.array_equal(order, np.arange(a.L))
    plain = _engine(relabel_landmarks(q, order), loss='huber')
    for e in (a, plain):
        e.iterate(3)
    ids = np.array(sorted(set(int(l) for l in q.lmk_idx[q.cam_idx == 9]) | {int(q.lmk_idx[0])}), np.int32)
    lmk_before = a.factors(dense=False)['lmk']
    np.testing.assert_array_equal(order[lmk_before], plain.factors(dense=False)['lmk'])
    ma, mp = a.retire_landmarks(ids), plain.retire_landmarks(order[ids])
    np.testing.assert_array_equal(ma[0], mp[0])
    np.testing.assert_array_equal(ma[2], mp[2])
    np.testing.assert_array_equal(ma[2], renumbering(~np.isin(lmk_before, ids)))
    keep_l = np.ones(q.n_lmks, bool)
    keep_l[ids] = False
    np.testing.assert_array_equal(ma[1], renumbering(keep_l))   # the caller's numbering
    assert ma[0][9] == -1
    u = np.flatnonzero(keep_l)
    to_plain = np.empty(u.size, np.int64)
    to_plain[ma[1][u]] = mp[1][order[u]]                        # a's new landmark -> the plain handle's new landmark
    for e in (a, plain):
        e.iterate(3)
    fa = a.factors(dense=False)
    np.testing.assert_array_equal(a.landmark_order(), rule_order(fa['cam'], fa['lmk'], a.C, a.L))
    assert a.check_layout() == 0
    for name in ('beliefs', 'priors', 'means'):
        va, vp = getattr(a, name)(), getattr(plain, name)()
        for k, (x, y) in enumerate(zip(va, vp)):
            y = y if (k < 2 and len(va) == 4) or (k < 1 and len(va) == 2) else y[to_plain]
            gap = rel_err_rows(x, y)
            assert gap < 1e-7, (name, k, gap)
    assert np.array_equal(a.iters_since_relin(), plain.iters_since_relin())
    a.close()
    plain.close()


def _tracks_host(setup, step, tol, **kw):
    """Set both up, retire landmarks (FOLD), step both: the engine stays with the host model.  Returns what the engine's message view
    said the fold should add, for the caller's own checks."""
    p = _problem()
    e, nb = _engine(p, **kw), _host(p, **kw)
    for x in (e, nb):
        setup(x)
    ids = _orphaning_list(p)
    fac, msg, pri0 = e.factors(dense=False), e.messages(), e.priors()
    maps = e.retire_landmarks(ids)
    for a, b in zip(maps, retire_landmarks_numpy_ba(nb, ids)):
        np.testing.assert_array_equal(a, b)
    pe = e.priors()
    assert rel_err_rows(pe[0], np.array([v.prior.eta for v in nb.cams])) <= tol
    assert rel_err_rows(pe[1], np.array([v.prior.lam for v in nb.cams])) <= tol
    goes = np.isin(fac['lmk'], ids)
    eta = pri0[0].copy()
    np.add.at(eta, fac['cam'][goes], msg[0][goes])
    assert rel_err_rows(pe[0], eta[maps[0] >= 0]) <= 1e-12       # the FULL message of the view, remainder included
    for x in (e, nb):
        step(x)
    for k, (a, h) in enumerate(zip(e.beliefs(), nb.beliefs())):
        assert rel_err_rows(a, h) <= tol, k
    _same_relin(e, nb)
    e.close()


def test_dense_remainder_is_folded_and_carried(lib):
    """num_undamped_iters = 0: factors are damped in the sweep they relinearise in, the handle carries the dense remainder, and its camera
    part is part of the message that arrives in the camera's prior (the host's messages are dense: they hold it)."""
    _tracks_host(lambda x: x.iterate(9), lambda x: x.iterate(9), tol=1e-9, num_undamped_iters=0)


def test_pending_relinearisation_survives(lib):
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
    _tracks_host(setup, step, tol=1e-9)


# ---- 7. failures leave the handle as it was; what is dropped ----------------------------------------------------------------------
def test_failures_leave_the_handle_untouched(lib):
    from gbp_amd.engine import BAEngine
    p = _problem()
    a, twin = _engine(p), _engine(p)
    for e in (a, twin):
        e.iterate(3)
    blob = a.save_state()
    for bad, word in (([150], 'entry 0'), ([3, -1], 'entry 1'), ([2, 5, 2], 'entry 2'), (list(range(150)), 'no factor')):
        with pytest.raises(lib.GbpError) as ei:
            a.retire_landmarks(bad)
        assert ei.value.code == -1 and word in str(ei.value), (bad, str(ei.value))
        assert (a.C, a.L, a.F) == (twin.C, twin.L, twin.F)
        assert _bitwise(a.save_state(), blob)
    ids = np.array([1], np.int32)
    h, L = a._h, lib.load()
    assert L.gbp_ba_retire_landmarks(h, 1, lib.iptr(ids), 2, None, None, None) == -1          # a bad mode
    assert L.gbp_ba_retire_landmarks(h, 1, lib.iptr(ids), -1, None, None, None) == -1
    assert L.gbp_ba_retire_landmarks(h, 0, None, 7, None, None, None) == -1
    assert L.gbp_ba_retire_landmarks(h, -1, lib.iptr(ids), 0, None, None, None) == -1         # a negative count
    assert L.gbp_ba_retire_landmarks(h, 1, None, 0, None, None, None) == -1                   # a NULL list with n > 0
    assert _bitwise(a.save_state(), blob)
    a.iterate(4)
    twin.iterate(4)
    assert _bitwise(a.save_state(), twin.save_state())
    a.close()
    twin.close()
    # no beliefs yet: the handle then goes on as an untouched one
    f, ft = BAEngine.from_problem(p), BAEngine.from_problem(p)
    with pytest.raises(lib.GbpError) as ei:
        f.retire_landmarks([0])
    assert ei.value.code == -5
    for x in (f, ft):
        x.generate_priors_var(W)
        x.update_all_beliefs()
        x.iterate(3)
    assert _bitwise(f.save_state(), ft.save_state())
    f.close()
    ft.close()


def test_a_list_that_leaves_no_factor_beside_a_landmark_without_factors(lib):
    """Landmark 150 has no factor.  Listing it is no error (it goes as an orphan would); listing every OTHER landmark leaves no factor
    although a landmark is not on the list: GBP_EINVAL from the survivors' count, the handle untouched."""
    import dataclasses
    p = _problem()
    q = dataclasses.replace(p, lmk_means=np.concatenate([p.lmk_means, p.lmk_means[:1] + 0.5]))
    a = _engine(q)
    a.iterate(2)
    blob = a.save_state()
    with pytest.raises(lib.GbpError) as ei:
        a.retire_landmarks(np.arange(150))
    assert ei.value.code == -1 and 'no factor' in str(ei.value)
    assert _bitwise(a.save_state(), blob) and (a.C, a.L, a.F) == (16, 151, 600)
    cm, lm, fm = a.retire_landmarks([150, 3])
    assert lm[150] == -1 and lm[3] == -1 and (lm >= 0).sum() == 149 and (fm < 0).sum() == 4 and (cm >= 0).all()
    a.iterate(2)
    assert np.isfinite(a.are()) and a.check_layout() == 0
    a.close()


def test_sharded_handles_refuse(lib):
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
            e.retire_landmarks([0])
        assert ei.value.code == -5
    for x, y in zip(shrunk, twin):
        assert _bitwise(x.save_state(), y.save_state())
    for e in shrunk + twin:
        e.close()
    g, gt = _engine(p), _engine(p)
    for x in (g, gt):
        x.set_exchange(lambda s_, r_, n_, st: 0, 0, 1)
    with pytest.raises(lib.GbpError) as ei:
        g.retire_landmarks([0], fold=False)
    assert ei.value.code == -5
    for x in (g, gt):
        x.iterate_sharded(3)
    assert _bitwise(g.save_state(), gt.save_state())
    g.close()
    gt.close()


@pytest.mark.parametrize('fold', [True, False])
def test_empty_list_continues_bitwise(lib, fold):
    p = _problem()
    a, twin = _engine(p), _engine(p)
    a.iterate(3)
    twin.iterate(3)
    cm, lm, fm = a.retire_landmarks([], fold=fold)
    np.testing.assert_array_equal(cm, np.arange(a.C))
    np.testing.assert_array_equal(lm, np.arange(a.L))
    np.testing.assert_array_equal(fm, np.arange(a.F))
    assert _bitwise(a.save_state(), twin.save_state())
    a.iterate(4)
    twin.iterate(4)
    assert _bitwise(a.save_state(), twin.save_state())
    np.testing.assert_array_equal(a.relin_counts(7), twin.relin_counts(7))
    a.close()
    twin.close()


def test_snapshot_is_dropped_and_means_stream_afterwards(lib):
    e = _engine(_problem())
    e.iterate(2)
    e.snapshot_state()
    e.means_snapshot()
    e.retire_landmarks([0, 1])
    with pytest.raises(lib.GbpError) as ei:
        e.restore_snapshot()
    assert ei.value.code == -5
    e.means_snapshot()
    cm, lm = e.means_fetch(wait=True)
    rc, rl = e.means()
    assert lm.shape == (148, 3) and _bitwise(cm, rc) and _bitwise(lm, rl)
    e.close()


# ---- 8. the drop-in package ------------------------------------------------------------------------------------------------------
def test_compat_graph_lets_go_of_landmarks(lib):
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
    its = np.array([f.iters_since_relin for f in g.factors])
    ids_of = np.array([list(f.adj_vIDs) for f in g.factors])
    mu5 = np.array(g.lmk_nodes[5].mu)
    ids = _orphaning_list(p)
    cm, lm, fm = g.retire_landmarks(ids)
    kf = fm >= 0
    assert len(g.cam_nodes) == 15 and len(g.lmk_nodes) == p.n_lmks - ids.size and len(g.factors) == int(kf.sum())
    assert len(g.var_nodes) == len(g.cam_nodes) + len(g.lmk_nodes) and g.n_factor_nodes == len(g.factors) and g.n_edges == 2 * len(g.factors)
    assert [f.iters_since_relin for f in g.factors] == list(its[kf])
    fac = g._engine.factors(dense=False)
    for i in range(0, len(g.factors), 37):
        assert list(g.factors[i].adj_vIDs) == [int(fac['cam'][i]), len(g.cam_nodes) + int(fac['lmk'][i])]
    np.testing.assert_array_equal([f.adj_vIDs[0] for f in g.factors], cm[ids_of[kf, 0]])
    np.testing.assert_array_equal([f.adj_vIDs[1] - len(g.cam_nodes) for f in g.factors], lm[ids_of[kf, 1] - 16])
    np.testing.assert_allclose(g.lmk_nodes[int(lm[5])].mu, mu5, rtol=1e-12)
    g.synchronous_iteration()
    assert np.isfinite(g.are())
    cm2, _, fm2 = g.retire_landmarks([0, 2], fold=False)
    assert len(g.factors) == int((fm2 >= 0).sum()) and len(g.cam_nodes) == int((cm2 >= 0).sum())
    g.synchronous_iteration()
    assert np.isfinite(g.are())
