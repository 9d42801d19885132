"""gbp_ba_window_step / BAEngine.window_step on the GPU: append a keyframe, cull observations, retire keyframes and let go of landmarks
in ONE rebuild of a live handle, with every id in the numbering from before the call.

Oracles: the four existing calls on a twin engine started from the same state blob (tests/window_host.py carries the ids through the
maps), the reference's own object graph (NumpyBA) put through the same four steps, and a handle freshly created from the resulting
problem.  Tolerances are those tests/test_retire_lmk_gpu.py holds the single calls to: copies are bitwise, a fold summed in another order
1e-12, beliefs after further sweeps 1e-9, the engine against the host model 1e-7."""
import numpy as np
import pytest

from conftest import rel_err_rows
from window_fuzz_cases import carry_batch, carry_ids
from window_host import (EngineOps, base_case, big_landmark_problem, check_case, filter_batch, four_calls, hold_back, result_problem,
                         three_chunk_problem, window_step_numpy_ba)

pytestmark = pytest.mark.gpu

W = 50.0


@pytest.fixture(scope='module')
def lib():
    from gbp_amd import build
    build.build()
    from gbp_amd import _capi
    return _capi


@pytest.fixture(scope='module')
def case():
    c = base_case()
    check_case(c)
    return c


def _engine(problem, **kw):
    from gbp_amd.engine import BAEngine
    e = BAEngine.from_problem(problem, **kw)
    e.generate_priors_var(W)
    e.update_all_beliefs()
    return e


def _pair(problem, sweeps=6, setup=None, **kw):
    """two engines in one state: b starts from a's blob"""
    a, b = _engine(problem, **kw), _engine(problem, **kw)
    (setup or (lambda x: x.iterate(sweeps)))(a)
    b.load_state(a.save_state())
    return a, b


def _host(problem, **kw):
    from extend_host import make_numpy_ba
    nb = make_numpy_ba(problem, **kw)
    nb.generate_priors_var(W)
    nb.update_all_beliefs()
    return nb


def _bitwise(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _tuple(b):
    return None if b is None else (b['cam_means'], b['lmk_means'], b['meas'], b['cam_idx'], b['lmk_idx'])


def _step(e, batch=None, cull=(), retire=(), lmks=(), fold=True):
    return e.window_step(cull=cull, retire=retire, retire_landmarks=lmks, fold_landmarks=fold, batch=_tuple(batch), prior_weaker_factor=W)


def _same_maps(x, y):
    for name, a, b in zip(x._fields, x, y):
        np.testing.assert_array_equal(a, b, err_msg=name)


def _equal_to_four_calls(a, b, steps, sweeps=5, touched_cams=None):
    """a went through the four calls, b through one window step, both from one state: what must be equal, and how equal.
    touched_cams (ids AFTER the step): the cameras whose prior a fold into cameras touched; None: any may be."""
    assert (a.C, a.L, a.F) == (b.C, b.L, b.F) and a.plan_info() == b.plan_info() and b.check_layout() == 0
    fa, fb = a.factors(dense=False), b.factors(dense=False)
    for key in fa:
        if fa[key] is not None:
            assert _bitwise(fa[key], fb[key]), key
    for x, y in zip(a.messages(), b.messages()):
        assert _bitwise(x, y)
    ra, rb = a.relin_state(), b.relin_state()
    for key in ra:
        assert _bitwise(ra[key], rb[key]), key
    pa, pb = a.priors(), b.priors()
    assert _bitwise(pa[2], pb[2]) and _bitwise(pa[3], pb[3])    # landmark folds run in the same order on both sides
    if touched_cams is not None:
        quiet = np.ones(a.C, bool)
        quiet[touched_cams] = False
        assert _bitwise(pa[0][quiet], pb[0][quiet]) and _bitwise(pa[1][quiet], pb[1][quiet])
    for k, (x, y) in enumerate(zip(pa + a.beliefs(), pb + b.beliefs())):
        gap = rel_err_rows(x, y)
        print(f'window step vs four calls: array {k} gap {gap:.3e}')
        assert gap < 1e-12, k
    for e in (a, b):
        steps(e) if callable(steps) else e.iterate(sweeps)
    for k, (x, y) in enumerate(zip(a.beliefs(), b.beliefs())):
        assert rel_err_rows(x, y) < 1e-9, k
    assert np.array_equal(a.iters_since_relin(), b.iters_since_relin())


# ---- 1. one step equals the four calls ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fold', [True, False])
@pytest.mark.parametrize('fused', [True, False, None])
def test_equals_the_four_calls(lib, case, fused, fold):
    a, b = _pair(case.base, fused=fused, loss='huber')
    fac = a.factors(dense=False)
    ma = four_calls(EngineOps(a, prior_weaker_factor=W), case.batch, case.cull, case.retire, case.lmks, fold)
    mb = _step(b, case.batch, case.cull, case.retire, case.lmks, fold)
    _same_maps(ma, mb)
    assert mb.cam_map[case.orphan] == -1 and mb.cam_map[15] >= 0 and mb.lmk_map[0] >= 0 and mb.lmk_map[case.saved] >= 0
    assert (mb.new_factor_ids >= 0).all() and (mb.new_cam_ids >= 0).all()
    assert not np.array_equal(mb.factor_map[mb.factor_map >= 0], np.arange((mb.factor_map >= 0).sum()))     # old ids moved past late factors
    goes = np.isin(fac['lmk'], case.lmks) & ~np.isin(fac['cam'], case.retire)
    goes[case.cull] = False
    touched = mb.cam_map[np.unique(fac['cam'][goes])]
    _equal_to_four_calls(a, b, None, touched_cams=touched[touched >= 0] if fold else np.zeros(0, np.int64))
    a.close()
    b.close()


# ---- 2. each part alone is the old call -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('part', ['cull', 'retire', 'lmks fold', 'lmks drop', 'batch'])
def test_each_part_alone_is_the_old_call(lib, case, part):
    """gbp_ba_cull, gbp_ba_retire and gbp_ba_retire_landmarks are fronts of the window step's engine: each beside a window step that
    carries only its part compares a front with the engine it calls (and 'batch' compares gbp_ba_extend, a path of its own, with it).
    Maps and the whole state blob byte for byte, after the call and after three more sweeps."""
    a, b = _pair(case.base, loss='huber')
    ident = lambda n: np.arange(n, dtype=np.int32)
    C, L, F = a.C, a.L, a.F
    if part == 'batch':
        bt = case.batch
        o2n = a.extend(*_tuple(bt), prior_weaker_factor=W)
        m = _step(b, batch=bt)
        np.testing.assert_array_equal(m.factor_map, o2n)
        np.testing.assert_array_equal(m.cam_map, ident(C))
        np.testing.assert_array_equal(m.lmk_map, ident(L))
        np.testing.assert_array_equal(m.new_cam_ids, C + ident(2))
        np.testing.assert_array_equal(np.sort(np.concatenate([m.factor_map, m.new_factor_ids])), ident(b.F))
    else:
        old = dict(cull=lambda: a.cull(case.cull), retire=lambda: a.retire(case.retire),
                   **{'lmks fold': lambda: a.retire_landmarks(case.lmks), 'lmks drop': lambda: a.retire_landmarks(case.lmks, fold=False)})[part]()
        m = _step(b, cull=case.cull if part == 'cull' else (), retire=case.retire if part == 'retire' else (),
                  lmks=case.lmks if part.startswith('lmks') else (), fold=part != 'lmks drop')
        for x, y in zip(old, m[:3]):
            np.testing.assert_array_equal(x, y)
        assert m.new_cam_ids.size == m.new_lmk_ids.size == m.new_factor_ids.size == 0
    assert (a.C, a.L, a.F) == (b.C, b.L, b.F)
    assert _bitwise(a.save_state(), b.save_state())
    a.iterate(3)
    b.iterate(3)
    assert _bitwise(a.save_state(), b.save_state())
    a.close()
    b.close()


# ---- 3. the saved landmark --------------------------------------------------------------------------------------------------------------
def test_the_landmark_the_new_keyframe_saves(lib, case):
    a, b = _pair(case.base, loss='huber')
    fac, msg, pri = b.factors(dense=False), b.messages(), b.priors()
    m = _step(b, case.batch, case.cull, case.retire, case.lmks)
    nl = m.lmk_map[case.saved]
    assert nl >= 0
    mine = (fac['lmk'] == case.saved) & np.isin(fac['cam'], case.retire)
    assert mine.any() and mine.sum() == (fac['lmk'] == case.saved).sum()
    eta, lam = pri[2][case.saved] + msg[2][mine].sum(axis=0), pri[3][case.saved] + msg[3][mine].sum(axis=0)
    after = b.priors()
    assert np.abs(after[2][nl] - eta).max() <= 1e-12 * np.abs(eta).max() and np.abs(after[3][nl] - lam).max() <= 1e-12 * np.abs(lam).max()
    # retire first, extend afterwards: the landmark is orphaned, and the batch that observes it cannot be given any more
    cm, lm, fm = a.retire(case.retire)
    assert lm[case.saved] == -1
    bt = case.batch
    with pytest.raises(lib.GbpError):
        lmk_u = np.concatenate([lm, a.L + np.arange(len(bt['lmk_means']), dtype=np.int32)])
        cam_u = np.concatenate([cm, a.C + np.arange(len(bt['cam_means']), dtype=np.int32)])
        a.extend(bt['cam_means'], bt['lmk_means'], bt['meas'], cam_u[bt['cam_idx']], lmk_u[bt['lmk_idx']], prior_weaker_factor=W)
    a.close()
    b.close()


# ---- 4. against the reference's object graph --------------------------------------------------------------------------------------------
def _gap_to_host(e, nb, where, tol=1e-7):
    for a, h in zip(e.beliefs(), nb.beliefs()):
        gap = rel_err_rows(a, h)
        assert gap < tol, (where, gap)
    ph = (np.array([v.prior.eta for v in nb.cams]), np.array([v.prior.lam for v in nb.cams]),
          np.array([v.prior.eta for v in nb.lmks]), np.array([v.prior.lam for v in nb.lmks]))
    for a, h in zip(e.priors(), ph):
        gap = rel_err_rows(a, h)
        assert gap < tol, (where, 'priors', gap)


def _same_relin(e, nb):
    rs = e.relin_state()
    np.testing.assert_array_equal(rs['iters_since_relin'], [f.iters_since_relin for f in nb.graph.factors])
    np.testing.assert_array_equal(rs['eta_damping'], [f.eta_damping for f in nb.graph.factors])


def test_sliding_window_tracks_the_reference_graph(lib):
    """Three consecutive steps of a sliding window (14 cameras, then 2 + 2 + 2), 4 sweeps between them: every step appends a keyframe pair
    with late observations, retires the two oldest cameras, lets go of the landmarks nobody above the fourth-oldest camera sees and culls
    the two factors with the largest residual among those that would stay."""
    from gbp_amd.synthetic import make_synthetic, keyframe_batches
    split = keyframe_batches(make_synthetic(n_cams=20, n_lmks=150, obs_per_lmk=4, window=6, seed=1), [14, 2, 2, 2], defer=0.3)
    e, nb = _engine(split.base, loss='huber'), _host(split.base, loss='huber')
    # ids of the split's batches are in the numbering of the GROWING graph; the window also shrinks, so carry them along
    cam_now, lmk_now = np.arange(split.base.n_cams), np.arange(split.base.n_lmks)       # split id -> current id
    for k, raw in enumerate(split.batches):
        e.iterate(4)
        nb.iterate(4)
        fac = e.factors(dense=False)
        dL = len(raw['lmk_means'])
        bt, cam_u, lmk_u = carry_batch(raw, cam_now, lmk_now, e.C, e.L)
        retire = np.array([0, 1], np.int32)
        top = np.full(e.L + dL, -1)
        np.maximum.at(top, fac['lmk'], fac['cam'])
        np.maximum.at(top, bt['lmk_idx'], bt['cam_idx'])
        lmks = np.flatnonzero((top[:e.L] >= 2) & (top[:e.L] < 4)).astype(np.int32)
        bt = filter_batch(bt, retire, lmks)
        stays = np.flatnonzero(~np.isin(fac['cam'], retire) & ~np.isin(fac['lmk'], lmks))
        cull = stays[np.argsort(e.residuals()[1][stays])[-2:]].astype(np.int32)
        mh = window_step_numpy_ba(nb, bt, cull, retire, lmks, prior_weaker_factor=W)
        me = _step(e, bt, cull, retire, lmks)
        _same_maps(mh, me)
        assert (e.C, e.L, e.F) == (nb.C, nb.L, len(nb.graph.factors)) and e.check_layout() == 0
        _gap_to_host(e, nb, f'step {k}')
        _same_relin(e, nb)
        cam_now, lmk_now = carry_ids(cam_u, lmk_u, me)
    e.iterate(4)
    nb.iterate(4)
    _gap_to_host(e, nb, '4 sweeps after the last step')
    _same_relin(e, nb)
    e.close()


# ---- 5. one rebuild -----------------------------------------------------------------------------------------------------------------------
def test_one_rebuild(lib, case):
    a, b = _pair(case.base)
    assert a.rebuild_count() == 1 and b.rebuild_count() == 1
    four_calls(EngineOps(a, prior_weaker_factor=W), case.batch, case.cull, case.retire, case.lmks)
    _step(b, case.batch, case.cull, case.retire, case.lmks)
    assert a.rebuild_count() == 5 and b.rebuild_count() == 2
    _step(b)
    b.cull([])
    b.retire([])
    b.retire_landmarks([])
    assert b.rebuild_count() == 2
    a.close()
    b.close()


# ---- 6. equals create plus state ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [True, False, None])
def test_equals_create_plus_state(lib, case, fused):
    a = _engine(case.base, fused=fused)
    a.iterate(6)
    fac, means = a.factors(dense=False), a.means()
    m = _step(a, case.batch, case.cull, case.retire, case.lmks)
    f = _engine(result_problem(case.base.K, means[0], means[1], fac, case.batch, m), fused=fused)
    assert a.plan_info() == f.plan_info() and a.info() == f.info()
    f.load_state(a.save_state())                              # same graph hash, same layout
    a.iterate(5)
    f.iterate(5)
    assert _bitwise(a.save_state(), f.save_state())
    a.close()
    f.close()


# ---- 7. edges -------------------------------------------------------------------------------------------------------------------------------
def _late_batch_case(problem, rows, cull, retire, lmks, check=None, **kw):
    """The problem without the observations `rows`, which a batch without new variables brings late (the old cameras' ranges shift in
    the four calls); cull(fac) -> ids in the base graph's factor numbering."""
    base, batch = hold_back(problem, rows)
    assert not np.isin(batch['cam_idx'], retire).any() and not np.isin(batch['lmk_idx'], lmks).any()
    a, b = _pair(base, sweeps=4, **kw)
    fac = a.factors(dense=False)
    if check:
        check(fac)
    ids = cull(fac)
    ma = four_calls(EngineOps(a, prior_weaker_factor=W), batch, ids, retire, lmks)
    mb = _step(b, batch, ids, retire, lmks)
    _same_maps(ma, mb)
    assert (mb.new_factor_ids >= 0).all()
    _equal_to_four_calls(a, b, None)
    a.close()
    b.close()


def _rows(p, pairs):
    return [int(np.flatnonzero((p.cam_idx == c) & (p.lmk_idx == l))[0]) for c, l in pairs]


def test_three_chunks_of_a_camera_fold(lib):
    """Every camera has 150 factors; the listed landmarks take 148 of camera 3's and 149 of camera 4's, camera 5 is retired and a few of
    the departing factors are culled: three chunks of 64 on one side, other chunks on the other.  Four observations of cameras 0, 3 and 4
    arrive late with the batch, so the cameras' ranges have moved when the four calls fold."""
    p = three_chunk_problem()
    lmks = np.arange(150, 299)

    def check(fac):
        goes = np.isin(fac['lmk'], lmks) & (fac['cam'] != 5)
        assert np.bincount(fac['cam'][goes], minlength=6).max() > 128

    def cull(fac):
        pick = lambda c, ls: [int(np.flatnonzero((fac['cam'] == c) & (fac['lmk'] == l))[0]) for l in ls]
        return np.array(pick(3, [160, 170]) + pick(4, [210]) + pick(0, [20]), np.int32)
    _late_batch_case(p, _rows(p, [(3, 149), (4, 299), (0, 5), (0, 6)]), cull, [5], lmks, check=check, loss='huber')


@pytest.mark.parametrize('which', ['the big one', 'degree one'])
def test_landmark_above_a_tile_and_landmarks_of_degree_one(lib, which):
    """A landmark of 80 factors spans chunk tiles; landmarks of degree 1 and 2 beside it.  Late observations: of two degree-2 landmarks,
    and (where the big landmark stays) two of the big one."""
    p = big_landmark_problem()
    lmks = {'the big one': [0], 'degree one': [62, 61, 70, 5, 17]}[which]
    retire = [0, 79]
    busy = np.bincount(p.cam_idx, minlength=p.n_cams) >= 4       # cameras that keep observations when two of theirs come late
    busy[retire] = False
    late = [int(np.flatnonzero((p.lmk_idx == l) & busy[p.cam_idx])[0]) for l in (3, 9)]
    if which == 'degree one':
        big = np.flatnonzero((p.lmk_idx == 0) & busy[p.cam_idx])
        late += [int(big[2]), int(big[5])]

    def cull(fac):
        big = np.flatnonzero(fac['lmk'] == 0)
        return np.array([big[3], big[40]] if which == 'degree one' else [np.flatnonzero(fac['lmk'] == 7)[0]], np.int32)
    a = _engine(hold_back(p, late)[0], loss='huber')
    assert a.plan_info()['pack_mode'] == 1, a.plan_info()
    a.close()
    _late_batch_case(p, late, cull, retire, lmks, loss='huber')


def test_reordered_handle_takes_the_callers_numbering(lib, case):
    """GBP_FLAG_REORDER_LMKS on the base graph with shuffled landmark ids: all lists, the batch and all maps are the caller's."""
    from reorder_host import shuffle_landmarks
    q, to_q = shuffle_landmarks(case.base, seed=7)               # to_q: base landmark -> its id in q
    to_q = to_q.astype(np.int64)
    bl = case.batch['lmk_idx']
    bt = dict(case.batch, lmk_idx=np.where(bl < case.base.n_lmks, to_q[np.minimum(bl, case.base.n_lmks - 1)], bl).astype(np.int32))
    a, b = _pair(q, reorder_landmarks=True, loss='huber')
    assert not np.array_equal(a.landmark_order(), np.arange(a.L))
    ma = four_calls(EngineOps(a, prior_weaker_factor=W), bt, case.cull, case.retire, to_q[case.lmks])
    mb = _step(b, bt, case.cull, case.retire, to_q[case.lmks])
    _same_maps(ma, mb)
    assert mb.lmk_map[to_q[case.saved]] >= 0 and (mb.lmk_map[to_q[case.lmks]] == -1).all()
    np.testing.assert_array_equal(a.landmark_order(), b.landmark_order())
    _equal_to_four_calls(a, b, None)
    a.close()
    b.close()


def test_dense_remainder_is_folded_and_carried(lib, case):
    a, b = _pair(case.base, sweeps=9, num_undamped_iters=0)
    ma = four_calls(EngineOps(a, prior_weaker_factor=W), case.batch, case.cull, case.retire, case.lmks)
    mb = _step(b, case.batch, case.cull, case.retire, case.lmks)
    _same_maps(ma, mb)
    _equal_to_four_calls(a, b, lambda x: x.iterate(9))
    a.close()
    b.close()


def test_pending_relinearisation_survives(lib, case):
    def setup(x):
        x.iterate(9)
        x.relinearise_factors()

    def steps(x):
        x.compute_all_messages()
        x.update_all_beliefs()
        x.iterate(3)
    a, b = _pair(case.base, setup=setup)
    ma = four_calls(EngineOps(a, prior_weaker_factor=W), case.batch, case.cull, case.retire, case.lmks)
    mb = _step(b, case.batch, case.cull, case.retire, case.lmks)
    _same_maps(ma, mb)
    _equal_to_four_calls(a, b, steps)
    a.close()
    b.close()


# ---- 8. failures leave the handle untouched -----------------------------------------------------------------------------------------------
def test_failures_leave_the_handle_untouched(lib, case):
    import ctypes as ct
    from gbp_amd.engine import BAEngine
    a, twin = _pair(case.base, sweeps=3)
    blob, bt = a.save_state(), case.batch
    C, L, F = a.C, a.L, a.F

    def with_entry(j, cam=None, lmk=None):
        ci, li = bt['cam_idx'].copy(), bt['lmk_idx'].copy()
        if cam is not None:
            ci[j] = cam
        if lmk is not None:
            li[j] = lmk
        return dict(bt, cam_idx=ci, lmk_idx=li)
    bad = [(dict(cull=[F]), 'entry 0'), (dict(cull=[3, -1]), 'entry 1'), (dict(cull=[2, 5, 2]), 'entry 2'),
           (dict(retire=[C]), 'entry 0'), (dict(retire=[1, 1]), 'entry 1'), (dict(lmks=[3, L]), 'entry 1'), (dict(lmks=[7, 8, 7]), 'entry 2'),
           (dict(batch=with_entry(5, cam=C + 2)), 'observation 5'), (dict(batch=with_entry(6, lmk=L + 1)), 'observation 6'),
           (dict(batch=with_entry(4, cam=0), retire=[0]), 'observation 4'), (dict(batch=with_entry(9, lmk=3), lmks=[3]), 'observation 9'),
           (dict(retire=list(range(C))), 'no factor'), (dict(cull=list(range(F))), 'no factor')]
    for kw, word in bad:
        with pytest.raises(lib.GbpError) as ei:
            _step(a, **kw)
        assert ei.value.code == -1 and word in str(ei.value), (kw.keys(), str(ei.value))
        assert (a.C, a.L, a.F) == (C, L, F) and a.rebuild_count() == 1
        assert _bitwise(a.save_state(), blob)
    ids = np.array([1], np.int32)
    Lb = lib.load()

    def raw(**kw):
        w = lib.Window()
        for k, v in kw.items():
            setattr(w, k, v)
        return Lb.gbp_ba_window_step(a._h, ct.byref(w), None)
    assert raw(n_retire_lmks=1, retire_lmk_ids=lib.iptr(ids), lmk_mode=2) == -1                  # a bad mode
    assert raw(lmk_mode=-1) == -1
    assert raw(n_cull=-1, cull_ids=lib.iptr(ids)) == -1                                           # negative counts
    assert raw(n_retire_cams=-1) == -1 and raw(n_retire_lmks=-2) == -1
    assert raw(n_cull=1) == -1 and raw(n_retire_cams=1) == -1 and raw(n_retire_lmks=1) == -1      # NULL lists with a count
    e = lib.Ext()
    e.n_new_factors = 1
    assert raw(batch=ct.pointer(e)) == -1                                                         # NULL batch arrays with a count
    assert Lb.gbp_ba_window_step(a._h, None, None) == -1
    assert _bitwise(a.save_state(), blob) and a.rebuild_count() == 1
    a.iterate(1)
    twin.iterate(1)
    assert _bitwise(a.save_state(), twin.save_state())
    a.close()
    twin.close()
    # no beliefs yet: GBP_ESTATE, and the handle goes on as an untouched one
    f, ft = BAEngine.from_problem(case.base), BAEngine.from_problem(case.base)
    with pytest.raises(lib.GbpError) as ei:
        _step(f, retire=[0])
    assert ei.value.code == -5 and f.rebuild_count() == 1
    for x in (f, ft):
        x.generate_priors_var(W)
        x.update_all_beliefs()
        x.iterate(1)
    assert _bitwise(f.save_state(), ft.save_state())
    f.close()
    ft.close()


def test_sharded_handles_refuse(lib, case):
    p = case.base

    def pair():
        r = [_engine(p), _engine(p)]
        hs = [e.peer_export(2, same_process=True) for e in r]
        for k, e in enumerate(r):
            e.peer_connect(k, hs, same_process=True, rendezvous=True)
        return r
    stepped, twin = pair(), pair()
    for e in stepped:
        with pytest.raises(lib.GbpError) as ei:
            _step(e, retire=[0])
        assert ei.value.code == -5
    for x, y in zip(stepped, twin):
        assert _bitwise(x.save_state(), y.save_state())
    for e in stepped + twin:
        e.close()
    g, gt = _engine(p), _engine(p)
    for x in (g, gt):
        x.set_exchange(lambda s_, r_, n_, st: 0, 0, 1)
    with pytest.raises(lib.GbpError) as ei:
        _step(g, cull=[0])
    assert ei.value.code == -5 and g.rebuild_count() == 1
    for x in (g, gt):
        x.iterate_sharded(1)
    assert _bitwise(g.save_state(), gt.save_state())
    g.close()
    gt.close()


# ---- 9. the empty step; what is dropped ---------------------------------------------------------------------------------------------------
def test_empty_step_continues_bitwise(lib, case):
    a, twin = _pair(case.base, sweeps=3)
    m = _step(a)
    np.testing.assert_array_equal(m.cam_map, np.arange(a.C))
    np.testing.assert_array_equal(m.lmk_map, np.arange(a.L))
    np.testing.assert_array_equal(m.factor_map, np.arange(a.F))
    assert m.new_cam_ids.size == 0 and (a.C, a.L, a.F) == (twin.C, twin.L, twin.F)
    assert _bitwise(a.save_state(), twin.save_state())
    a.iterate(4)
    twin.iterate(4)
    assert _bitwise(a.save_state(), twin.save_state())
    a.close()
    twin.close()


def test_snapshot_is_dropped_and_means_stream_afterwards(lib, case):
    e = _engine(case.base)
    e.iterate(2)
    e.snapshot_state()
    e.means_snapshot()
    _step(e, case.batch, case.cull, case.retire, case.lmks)
    with pytest.raises(lib.GbpError) as ei:
        e.restore_snapshot()
    assert ei.value.code == -5
    e.means_snapshot()
    cm, lm = e.means_fetch(wait=True)
    rc, rl = e.means()
    assert cm.shape == (e.C, 6) and _bitwise(cm, rc) and _bitwise(lm, rl)
    e.close()


# ---- 9b. a batch that is on the device already -----------------------------------------------------------------------------------------
def _on_device(bt):
    import torch
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in bt.items()}
    torch.cuda.synchronize()
    ptrs = tuple(t[k].data_ptr() for k in ('cam_means', 'lmk_means', 'meas', 'cam_idx', 'lmk_idx'))
    return t, ptrs, (bt['cam_means'].shape[0], bt['lmk_means'].shape[0], bt['meas'].shape[0])


def test_device_input_batch(lib, case):
    """GBP_FLAG_DEVICE_INPUT: the same step from device pointers gives the host-array step's maps and state blob, byte for byte."""
    a, b = _pair(case.base, loss='huber')
    ma = _step(a, case.batch, case.cull, case.retire, case.lmks)
    keep, ptrs, sizes = _on_device(case.batch)
    mb = b.window_step(cull=case.cull, retire=case.retire, retire_landmarks=case.lmks, batch=ptrs, prior_weaker_factor=W, device_pointers=sizes)
    _same_maps(ma, mb)
    assert (a.C, a.L, a.F) == (b.C, b.L, b.F) and _bitwise(a.save_state(), b.save_state())
    a.close()
    b.close()


@pytest.mark.parametrize('what', ['retired camera', 'listed landmark', 'camera beyond the union', 'landmark beyond the union'])
def test_device_input_batch_with_a_bad_entry(lib, case, what):
    """The ids of a device batch are checked on the device: the message names the LOWEST bad entry, the handle is untouched."""
    a, twin = _pair(case.base, sweeps=3)
    blob = a.save_state()
    ci, li = case.batch['cam_idx'].copy(), case.batch['lmk_idx'].copy()
    if what == 'retired camera':
        ci[7] = ci[90] = case.retire[1]
    elif what == 'listed landmark':
        li[7] = li[90] = case.lmks[0]
    elif what == 'camera beyond the union':
        ci[7], ci[90] = a.C + 2, -1
    else:
        li[7], li[90] = a.L + 1, -3
    keep, ptrs, sizes = _on_device(dict(case.batch, cam_idx=ci, lmk_idx=li))
    with pytest.raises(lib.GbpError) as ei:
        a.window_step(cull=case.cull, retire=case.retire, retire_landmarks=case.lmks, batch=ptrs, prior_weaker_factor=W, device_pointers=sizes)
    assert ei.value.code == -1 and 'observation 7 ' in str(ei.value), str(ei.value)
    assert (a.C, a.L, a.F) == (twin.C, twin.L, twin.F) and a.rebuild_count() == 1 and _bitwise(a.save_state(), blob)
    a.iterate(1)
    twin.iterate(1)
    assert _bitwise(a.save_state(), twin.save_state())
    a.close()
    twin.close()


# ---- 10. the drop-in package --------------------------------------------------------------------------------------------------------------
def test_compat_graph_takes_a_window_step(lib, case):
    import os
    import sys
    from conftest import REPO
    sys.path.insert(0, os.path.join(REPO, 'gbp_amd', 'compat'))
    try:
        from gbp.gbp_ba import BAFactorGraph
    finally:
        sys.path.remove(os.path.join(REPO, 'gbp_amd', 'compat'))
    cfg = dict(gauss_noise_std=2.0, loss=None, Nstds=3.0, beta=0.01, num_undamped_iters=6, min_linear_iters=8, eta_damping=0.4)
    gs = [BAFactorGraph(case.base, cfg), BAFactorGraph(case.base, cfg)]
    for g in gs:
        g.generate_priors_var(W)
        g.update_all_beliefs()
        g.synchronous_iteration()
    a, b = gs
    b._engine.load_state(a._engine.save_state())
    kept = 60
    assert kept not in case.lmks
    mu = np.array(b.lmk_nodes[kept].mu)

    class CompatOps(EngineOps):
        def extend(self, bt):
            return self.e.extend(*_tuple(bt), prior_weaker_factor=W)

        def cull(self, ids):
            return self.e.cull_observations(ids)

        def retire(self, ids):
            return self.e.retire_keyframes(ids)

        def sizes(self):
            return len(self.e.cam_nodes), len(self.e.lmk_nodes), len(self.e.factors)
    ma = four_calls(CompatOps(a), case.batch, case.cull, case.retire, case.lmks)
    mb = b.window_step(cull=case.cull, retire=case.retire, retire_landmarks=case.lmks, batch=_tuple(case.batch), prior_weaker_factor=W)
    _same_maps(ma, mb)
    assert (len(a.cam_nodes), len(a.lmk_nodes), len(a.factors), len(a.var_nodes)) == (len(b.cam_nodes), len(b.lmk_nodes), len(b.factors), len(b.var_nodes))
    assert b.n_factor_nodes == len(b.factors) and b.n_edges == 2 * len(b.factors) and len(b.var_nodes) == len(b.cam_nodes) + len(b.lmk_nodes)
    assert [list(f.adj_vIDs) for f in a.factors] == [list(f.adj_vIDs) for f in b.factors]
    assert [f.iters_since_relin for f in a.factors] == [f.iters_since_relin for f in b.factors]
    fac = b._engine.factors(dense=False)
    for i in range(0, len(b.factors), 37):
        assert list(b.factors[i].adj_vIDs) == [int(fac['cam'][i]), len(b.cam_nodes) + int(fac['lmk'][i])]
    np.testing.assert_allclose(b.lmk_nodes[int(mb.lmk_map[kept])].mu, mu, rtol=1e-12)
    np.testing.assert_allclose(b.lmk_nodes[int(mb.lmk_map[kept])].mu, a.lmk_nodes[int(ma.lmk_map[kept])].mu, rtol=1e-12)
    for g in gs:
        g.synchronous_iteration()
    assert np.isfinite(b.are()) and abs(a.are() - b.are()) <= 1e-9 * abs(a.are())
