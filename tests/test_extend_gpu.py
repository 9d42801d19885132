"""gbp_ba_extend / BAEngine.extend on the GPU: a live BA graph grows by keyframes and keeps every piece of GBP state.

Oracle: tests/extend_host.py grows the reference's own object graph (NumpyBA) by the same appends.  The structural checks pin the
extended handle to a handle freshly created from the union (same plan, same state blob, bitwise the same sweeps after a state load)
and the carried state to its value before the call, bit for bit."""
import ctypes as ct

import numpy as np
import pytest

from conftest import rel_err_rows
from extend_host import make_numpy_ba, extend as host_extend

pytestmark = pytest.mark.gpu

W = 50.0


@pytest.fixture(scope='module')
def lib():
    from gbp_amd import build
    build.build()
    from gbp_amd import _capi
    return _capi


def _split(n_cams=16, n_lmks=150, sizes=(8, 4, 4), defer=0.0, seed=1, window=6, obs=4):
    from gbp_amd.synthetic import make_synthetic, keyframe_batches
    p = make_synthetic(n_cams=n_cams, n_lmks=n_lmks, obs_per_lmk=obs, window=window, seed=seed)
    return keyframe_batches(p, list(sizes), defer=defer, seed=seed)


def _engine(problem, **kw):
    from gbp_amd.engine import BAEngine
    e = BAEngine.from_problem(problem, **kw)
    e.generate_priors_var(W)
    e.update_all_beliefs()
    return e


def _union(base, batches):
    """The union problem in a file order whose reference order is the grown graph's (base camera-major, then the batches)."""
    from gbp_amd.synthetic import BAProblem
    cat = lambda k: np.concatenate([getattr(base, k)] + [b[k] for b in batches])
    return BAProblem(K=base.K, cam_means=cat('cam_means'), lmk_means=cat('lmk_means'), meas=cat('meas'), cam_idx=cat('cam_idx'),
                     lmk_idx=cat('lmk_idx'))


def _ext(e, b, **kw):
    return e.extend(b['cam_means'], b['lmk_means'], b['meas'], b['cam_idx'], b['lmk_idx'], **kw)


def _state(e):
    return dict(bel=e.beliefs(), msg=e.messages(), fac=e.factors(dense=False), rs=e.relin_state(), pri=e.priors())


def _bitwise(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _disconnected(e, n_cams=6, n_lmks=80, seed=7):
    """A batch that sees none of e's variables: its own cameras and landmarks (ids in e's union numbering)."""
    from gbp_amd.synthetic import make_synthetic
    q = make_synthetic(n_cams=n_cams, n_lmks=n_lmks, obs_per_lmk=4, window=4, seed=seed)
    return dict(cam_means=q.cam_means, lmk_means=q.lmk_means, meas=q.meas, cam_idx=q.cam_idx + e.C, lmk_idx=q.lmk_idx + e.L), q


# ---- 1. replay against the host oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [True, False, None])
@pytest.mark.parametrize('loss', [None, 'huber'])
def test_growth_replay_matches_host_oracle(lib, fused, loss):
    sp = _split(defer=0.1)
    kw = dict(loss=loss)
    e = _engine(sp.base, fused=fused, **kw)
    nb = make_numpy_ba(sp.base, **kw)
    nb.generate_priors_var(W)
    nb.update_all_beliefs()
    worst = 0.0
    for k, b in enumerate([None] + sp.batches):
        if b is not None:
            F_old = e.F
            o2n_d = _ext(e, b, prior_weaker_factor=W)
            o2n_h = host_extend(nb, b, prior_weaker_factor=W)
            np.testing.assert_array_equal(o2n_d, o2n_h)
            new = np.setdiff1d(np.arange(e.F), o2n_d)
            assert new.size == e.F - F_old
            fd = e.factors()
            fh = [nb.graph.factors[i] for i in new]
            # (an old variable's mean is its belief's: the gap is the belief gap of the sweeps so far)
            assert rel_err_rows(fd['linpoint'][new], np.array([f.linpoint for f in fh])) < 1e-8
            assert rel_err_rows(fd['eta'][new], np.array([f.factor.eta for f in fh])) < 1e-8
            assert rel_err_rows(fd['lam'][new], np.array([f.factor.lam for f in fh])) < 1e-8
            for a, h in zip(e.beliefs(), nb.beliefs()):
                worst = max(worst, rel_err_rows(a, h))
        for s in range(6):
            e.iterate(1)
            nb.iterate(1)
            assert e.relin_counts(1)[0] == int(sum(f.iters_since_relin == 0 for f in nb.graph.factors)), (k, s)
        rs = e.relin_state()
        np.testing.assert_array_equal(rs['iters_since_relin'], [f.iters_since_relin for f in nb.graph.factors])
        np.testing.assert_array_equal(rs['eta_damping'], [f.eta_damping for f in nb.graph.factors])
        for a, h in zip(e.beliefs(), nb.beliefs()):
            worst = max(worst, rel_err_rows(a, h))
        assert abs(e.are() - nb.are()) <= 1e-8 * abs(nb.are())
    assert worst < 1e-7, worst
    e.close()


class _EngineGraph:
    """BAEngine behind the methods g17_replay calls (tests/extend_host.py)."""

    def __init__(self, base, loss, fused):
        from gbp_amd.engine import BAEngine
        self.e = BAEngine.from_problem(base, loss=loss, fused=fused)

    def __getattr__(self, name):
        return getattr(self.e, name)

    def extend(self, batch):
        return _ext(self.e, batch, prior_weaker_factor=W)

    def relin(self):
        rs = self.e.relin_state()
        return rs['iters_since_relin'], rs['eta_damping'], rs['adaptive_var']

    def new_factors(self, ids):
        f = self.e.factors()
        return f['eta'][ids], f['lam'][ids], f['linpoint'][ids]


@pytest.mark.parametrize('fused', [True, False, None])
@pytest.mark.parametrize('tag', ['small', 'vsmall_huber'])
def test_g17_reference_growth_replay(lib, tag, fused):
    """Fixture G17: the reference's own classes grew these graphs (make_g17.py).  Relinearisation counts exact every sweep, ARE / energy /
    beliefs / messages at the tolerances of the G4 / G14 parity tests, the new factors' eta_f / Lambda_f / linpoint after every extend,
    iters_since_relin and eta_damping exact after every batch (up to G17_HOLD on the non-robust run)."""
    from conftest import golden
    from extend_host import g17_inputs, g17_replay, G17_HOLD
    g = golden(f'G17_grow_{tag}')
    base, _ = g17_inputs(g)
    eg = _EngineGraph(base, None if str(g['loss']) == 'None' else str(g['loss']), fused)
    worst = g17_replay(g, eg, belief_tol=1e-6, msg_tol=1e-5, factor_tol=1e-8, hold=G17_HOLD[tag])
    assert worst < 1e-6
    eg.e.close()


# ---- 2. carried state is bitwise ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('defer', [0.0, 0.15])
def test_carry_is_bitwise(lib, defer):
    sp = _split(defer=defer, sizes=(8, 8))
    e = _engine(sp.base, loss='huber')
    e.iterate(4)
    before = _state(e)
    b = sp.batches[0]
    lone = np.array([[0.3, -0.2, 4.0]])                      # a landmark no observation sees: its belief is its prior
    bb = dict(b, lmk_means=np.concatenate([b['lmk_means'], lone]))
    lmk_lambda = np.ones(bb['lmk_means'].shape[0])          # new landmarks: the scalars; new cameras: the rule
    lmk_lambda[-1] = 3.0
    C0, L0 = e.C, e.L
    o2n = _ext(e, bb, lmk_prior_lambda=lmk_lambda)
    if defer == 0.0:
        np.testing.assert_array_equal(o2n, np.arange(o2n.size))
    else:
        assert (o2n != np.arange(o2n.size)).any()
    after = _state(e)
    for k in range(4):
        assert _bitwise(after['msg'][k][o2n], before['msg'][k])
    for key in ('linpoint', 'z', 'cam', 'lmk'):
        assert _bitwise(after['fac'][key][o2n], before['fac'][key])
    for key in ('iters_since_relin', 'eta_damping', 'adaptive_var', 'robust_flag'):
        assert _bitwise(after['rs'][key][o2n], before['rs'][key])
    for k, n in zip(range(4), (C0, C0, L0, L0)):
        assert _bitwise(after['pri'][k][:n], before['pri'][k])
        assert rel_err_rows(after['bel'][k][:n], before['bel'][k]) <= 1e-12
    new = np.setdiff1d(np.arange(e.F), o2n)
    assert (after['rs']['iters_since_relin'][new] == 1).all() and (after['rs']['eta_damping'][new] == 0).all()
    assert not after['rs']['robust_flag'][new].any()
    assert (after['rs']['adaptive_var'][new] == 4.0).all()
    ce, cl, le, ll = e.priors()
    be = e.beliefs()
    np.testing.assert_allclose(be[2][-1], le[-1], rtol=1e-12, atol=0)
    np.testing.assert_allclose(be[3][-1], ll[-1], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(ll[-1], 3.0 * np.eye(3), rtol=0, atol=0)
    e.close()


# ---- 3. extend = create of the union + the carried state ------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [True, False, None])
def test_extend_equals_create_plus_state(lib, fused):
    sp = _split(sizes=(8, 4, 4))
    runs = []
    for _ in range(2):
        e = _engine(sp.base, fused=fused)
        e.iterate(3)
        for b in sp.batches:
            _ext(e, b, prior_weaker_factor=W)
            e.iterate(2)
        runs.append(e)
    a, b2 = runs
    for x, y in zip(_state(a)['bel'], _state(b2)['bel']):
        assert _bitwise(x, y)
    assert _bitwise(a.save_state(), b2.save_state())
    u = _union(sp.base, sp.batches)
    f = _engine(u, fused=fused)
    assert a.plan_info() == f.plan_info() and a.info() == f.info()
    f.load_state(a.save_state())                              # same graph hash, same layout
    a.iterate(5)
    f.iterate(5)
    sa, sf = _state(a), _state(f)
    for k in range(4):
        assert _bitwise(sa['bel'][k], sf['bel'][k]) and _bitwise(sa['msg'][k], sf['msg'][k])
    for key in ('iters_since_relin', 'eta_damping'):
        assert _bitwise(sa['rs'][key], sf['rs'][key])
    for e in runs + [f]:
        e.close()


# ---- 4. at scale: the headline graph plus a disconnected 100k-factor component ---------------------------------------------------
def test_headline_graph_grows_by_a_disconnected_component(lib):
    from gbp_amd.synthetic import make_synthetic
    from gbp_amd.engine import BAEngine
    p = make_synthetic()
    q = make_synthetic(n_cams=50, n_lmks=10_000, seed=3)
    a, twin = _engine(p), _engine(p)
    a.iterate(3)
    twin.iterate(3)
    cm, lm = a.factor_lambda_max()
    o2n = a.extend(q.cam_means, q.lmk_means, q.meas, q.cam_idx + p.n_cams, q.lmk_idx + p.n_lmks, prior_weaker_factor=W)
    np.testing.assert_array_equal(o2n, np.arange(p.n_factors))
    b = BAEngine.from_problem(q)
    b.generate_priors_var(W)
    b.update_all_beliefs()
    for s in range(12):
        a.iterate(1)
        twin.iterate(1)
        b.iterate(1)
        assert a.relin_counts(1)[0] == twin.relin_counts(1)[0] + b.relin_counts(1)[0], s
    ba, bt, bb = a.beliefs(), twin.beliefs(), b.beliefs()
    for k, (n_old, n_new) in enumerate(((p.n_cams, q.n_cams), (p.n_cams, q.n_cams), (p.n_lmks, q.n_lmks), (p.n_lmks, q.n_lmks))):
        assert rel_err_rows(ba[k][:n_old], bt[k]) < 1e-9
        assert rel_err_rows(ba[k][n_old:], bb[k]) < 1e-9
    for e in (a, twin, b):
        e.close()


# ---- 5. the plan follows the graph as it grows ----------------------------------------------------------------------------------------
def test_plan_changes_under_growth(lib):
    """A sequence grown from 40 cameras (fused sweep) to 300 beyond what one LDS table holds: the plan changes at every extend and ends with
    camera windows or the general sweep, and the run stays with the same growth run on the general sweep."""
    from gbp_amd.synthetic import make_synthetic, keyframe_batches
    lim = lib.load().gbp_ba_fused_max_cams()
    n = lim + 300
    p = make_synthetic(n_cams=n, n_lmks=20 * n, obs_per_lmk=6, window=60, seed=5)
    sp = keyframe_batches(p, [40, (n - 40) // 2, n - 40 - (n - 40) // 2])     # (40 cameras, all inside every workgroup's window)
    plans, bels = [], []
    for fused in (None, False):
        e = _engine(sp.base, fused=fused)
        e.iterate(2)
        pl = [e.plan_info()]
        for b in sp.batches:
            _ext(e, b, prior_weaker_factor=W)
            e.iterate(2)
            pl.append(e.plan_info())
        plans.append(pl)
        bels.append(e.beliefs())
        e.close()
    auto = plans[0]
    assert auto[0]['fused'] and auto[0]['max_window'] <= 40 < lim, auto[0]                # the fused sweep below the LDS camera limit
    assert auto[1] != auto[0] and auto[2] != auto[1], auto                                   # re-planned for each union
    assert not auto[-1]['fused'] or auto[-1]['max_window'] > 0, auto[-1]
    assert all(not x['fused'] for x in plans[1])
    for x, y in zip(*bels):
        assert rel_err_rows(x, y) < 1e-10


# ---- 6. edge cases ------------------------------------------------------------------------------------------------------------
def test_empty_extension_continues_bitwise(lib):
    sp = _split(sizes=(16,))
    a, twin = _engine(sp.base), _engine(sp.base)
    a.iterate(3)
    twin.iterate(3)
    o2n = a.extend(np.zeros((0, 6)), np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0, np.int32), np.zeros(0, np.int32))
    twin.update_all_beliefs()                                 # (what extend ends with)
    np.testing.assert_array_equal(o2n, np.arange(a.F))
    sa, st = _state(a), _state(twin)        # (not the blobs: unused slots of a tile carry the clock of the build that made them)
    for k in range(4):
        assert _bitwise(sa['bel'][k], st['bel'][k]) and _bitwise(sa['msg'][k], st['msg'][k]) and _bitwise(sa['pri'][k], st['pri'][k])
    a.iterate(4)
    twin.iterate(4)
    for x, y in zip(a.beliefs(), twin.beliefs()):
        assert _bitwise(x, y)
    np.testing.assert_array_equal(a.relin_counts(7), twin.relin_counts(7))
    a.close()
    twin.close()


def _old_component_tracks_twin(setup, step, tol=1e-12, **kw):
    sp = _split(sizes=(16,))
    a, twin = _engine(sp.base, **kw), _engine(sp.base, **kw)
    for e in (a, twin):
        setup(e)
    C, L = a.C, a.L
    b, _ = _disconnected(a)
    _ext(a, b, prior_weaker_factor=W)
    for e in (a, twin):
        step(e)
    ba, bt = a.beliefs(), twin.beliefs()
    for k, n in enumerate((C, C, L, L)):
        assert rel_err_rows(ba[k][:n], bt[k]) <= tol, k
    ra, rt = a.relin_state(), twin.relin_state()
    for key in ('iters_since_relin', 'eta_damping'):
        np.testing.assert_array_equal(ra[key][:twin.F], rt[key])
    a.close()
    twin.close()


def test_dense_remainder_is_carried(lib):
    _old_component_tracks_twin(lambda e: e.iterate(9), lambda e: e.iterate(9), tol=1e-9, num_undamped_iters=0)


def test_pending_relinearisation_survives_extend(lib):
    def setup(e):
        e.iterate(9)
        e.relinearise_factors()

    def step(e):
        e.compute_all_messages()
        e.update_all_beliefs()
        e.iterate(3)
    _old_component_tracks_twin(setup, step, tol=1e-9)


def test_snapshot_is_dropped_and_means_stream_after_growth(lib):
    sp = _split(sizes=(8, 8))
    e = _engine(sp.base)
    e.iterate(2)
    e.snapshot_state()
    e.means_snapshot()
    _ext(e, sp.batches[0], prior_weaker_factor=W)
    with pytest.raises(lib.GbpError) as ei:
        e.restore_snapshot()
    assert ei.value.code == -5
    e.means_snapshot()
    cm, lm = e.means_fetch(wait=True)
    rc, rl = e.means()
    assert cm.shape == (16, 6) and _bitwise(cm, rc) and _bitwise(lm, rl)
    e.close()


# ---- 7. failures leave the handle as it was -----------------------------------------------------------------------------------------
def test_failures_leave_the_handle_untouched(lib):
    from gbp_amd.engine import BAEngine
    sp = _split(sizes=(8, 8))
    a, twin = _engine(sp.base), _engine(sp.base)
    for e in (a, twin):
        e.iterate(3)
    b = sp.batches[0]
    bad = dict(b, lmk_idx=b['lmk_idx'].copy())
    bad['lmk_idx'][3] = a.L + b['lmk_means'].shape[0]        # one past the union's landmarks
    with pytest.raises(lib.GbpError) as ei:
        _ext(a, bad)
    assert ei.value.code == -1
    bad = dict(b, cam_idx=b['cam_idx'].copy())
    bad['cam_idx'][0] = -1
    with pytest.raises(lib.GbpError) as ei:
        _ext(a, bad)
    assert ei.value.code == -1
    assert (a.C, a.L, a.F) == (twin.C, twin.L, twin.F)
    a.iterate(4)
    twin.iterate(4)
    assert _bitwise(a.save_state(), twin.save_state())
    for x, y in zip(a.beliefs(), twin.beliefs()):
        assert _bitwise(x, y)
    # a device-input batch with a bad id (checked by the build on the device)
    import torch
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in bad.items()}
    torch.cuda.synchronize()
    with pytest.raises(lib.GbpError) as ei:
        a.extend(t['cam_means'].data_ptr(), t['lmk_means'].data_ptr(), t['meas'].data_ptr(), t['cam_idx'].data_ptr(), t['lmk_idx'].data_ptr(),
                 device_pointers=(8, b['lmk_means'].shape[0], b['meas'].shape[0]))
    assert ei.value.code == -1
    a.iterate(3)
    twin.iterate(3)
    assert _bitwise(a.save_state(), twin.save_state())
    a.close()
    twin.close()
    # no beliefs yet: the handle then goes on as an untouched one
    f, ft = BAEngine.from_problem(sp.base), BAEngine.from_problem(sp.base)
    with pytest.raises(lib.GbpError) as ei:
        _ext(f, b)
    assert ei.value.code == -5
    for x in (f, ft):
        x.generate_priors_var(W)
        x.update_all_beliefs()
        x.iterate(3)
    assert _bitwise(f.save_state(), ft.save_state())
    f.close()
    ft.close()


def test_sharded_handles_refuse_to_grow(lib):
    """A 2-rank peer-store set-up on one GPU (two handles of one process, as test_peer_ipc_gpu's ranks) and an exchange callback: GBP_ESTATE,
    and each rank's handle then runs its sharded sweeps bit-identically to an untouched twin set-up."""
    sp = _split(sizes=(8, 8))
    b = sp.batches[0]

    def pair():
        r = [_engine(sp.base), _engine(sp.base)]
        hs = [e.peer_export(2, same_process=True) for e in r]
        for k, e in enumerate(r):
            e.peer_connect(k, hs, same_process=True, rendezvous=True)
        return r
    grown, twin = pair(), pair()
    for e in grown:
        with pytest.raises(lib.GbpError) as ei:
            _ext(e, b)
        assert ei.value.code == -5
    for x, y in zip(grown, twin):
        assert _bitwise(x.save_state(), y.save_state())
    for e in grown + twin:
        e.close()
    g, gt = _engine(sp.base), _engine(sp.base)
    for x in (g, gt):
        x.set_exchange(lambda s_, r_, n_, st: 0, 0, 1)
    with pytest.raises(lib.GbpError) as ei:
        _ext(g, b)
    assert ei.value.code == -5
    for x in (g, gt):
        x.iterate_sharded(3)
    assert _bitwise(g.save_state(), gt.save_state())
    g.close()
    gt.close()


def test_device_input_batch(lib):
    import torch
    sp = _split(sizes=(8, 8))
    a, b2 = _engine(sp.base), _engine(sp.base)
    b = sp.batches[0]
    o1 = _ext(a, b)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in b.items()}
    torch.cuda.synchronize()
    o2 = b2.extend(t['cam_means'].data_ptr(), t['lmk_means'].data_ptr(), t['meas'].data_ptr(), t['cam_idx'].data_ptr(),
                   t['lmk_idx'].data_ptr(), device_pointers=(8, b['lmk_means'].shape[0], b['meas'].shape[0]))
    np.testing.assert_array_equal(o1, o2)
    assert _bitwise(a.save_state(), b2.save_state())
    a.close()
    b2.close()


# ---- 8. the drop-in package --------------------------------------------------------------------------------------------------------
def test_compat_graph_grows(lib):
    import sys
    import os
    from conftest import REPO
    sys.path.insert(0, os.path.join(REPO, 'gbp_amd', 'compat'))
    try:
        from gbp.gbp_ba import BAFactorGraph
    finally:
        sys.path.remove(os.path.join(REPO, 'gbp_amd', 'compat'))
    sp = _split(sizes=(8, 4), defer=0.1)
    cfg = dict(gauss_noise_std=2.0, loss=None, Nstds=3.0, beta=0.01, num_undamped_iters=6, min_linear_iters=8, eta_damping=0.4)
    g = BAFactorGraph(sp.base, cfg)
    g.generate_priors_var(W)
    g.update_all_beliefs()
    g.synchronous_iteration()
    n_f = len(g.factors)
    its = [f.iters_since_relin for f in g.factors]
    b = sp.batches[0]
    o2n = g.extend(b['cam_means'], b['lmk_means'], b['meas'], b['cam_idx'], b['lmk_idx'])
    assert len(g.cam_nodes) == 12 and len(g.lmk_nodes) == sp.base.n_lmks + b['lmk_means'].shape[0]
    assert len(g.factors) == n_f + b['meas'].shape[0] and len(g.var_nodes) == len(g.cam_nodes) + len(g.lmk_nodes)
    assert [g.factors[int(i)].iters_since_relin for i in o2n] == its
    new = np.setdiff1d(np.arange(len(g.factors)), o2n)
    e = g._engine
    fac = e.factors(dense=False)
    for i in new[:20]:
        f = g.factors[int(i)]
        assert f.iters_since_relin == 1
        assert list(f.adj_vIDs) == [int(fac['cam'][i]), len(g.cam_nodes) + int(fac['lmk'][i])]
    np.testing.assert_array_equal(g.cam_nodes[11].mu, e.means()[0][11])
    g.synchronous_iteration()


# ---- 9. where a rebuild that lets nothing go and one that can let things go could part ---------------------------------------------------
# (window_host.base_case()'s 16-camera base; default and landmark-reordered handles, the sweep forced fused and forced general)
HANDLES = pytest.mark.parametrize('reorder,fused', [(False, True), (False, False), (True, True), (True, False)])
CAM_LAMBDA, LMK_LAMBDA = np.array([2.0, 5.0]), np.array([1.0, 1.5, 3.0])


@pytest.fixture(scope='module')
def case():
    from window_host import base_case
    return base_case()


def _host_messages(nb):
    fs = nb.graph.factors
    return (np.array([f.messages[0].eta for f in fs]), np.array([f.messages[0].lam for f in fs]),
            np.array([f.messages[1].eta for f in fs]), np.array([f.messages[1].lam for f in fs]))


def _host_grown(problem, batch, sweeps, **prior_kw):
    """The reference's object graph after `sweeps` sweeps and one extend: (old_to_new, beliefs, messages)."""
    nb = make_numpy_ba(problem, loss='huber')
    nb.generate_priors_var(W)
    nb.update_all_beliefs()
    nb.iterate(sweeps)
    o2n = host_extend(nb, batch, **prior_kw)
    return o2n, nb.beliefs(), _host_messages(nb)


@pytest.fixture(scope='module')
def host_bare_new(case):
    from extend_cases import bare_new_batch
    b = bare_new_batch(case.base)
    return b, _host_grown(case.base, b, 3, cam_prior_lambda=CAM_LAMBDA, lmk_prior_lambda=LMK_LAMBDA)


@HANDLES
def test_new_variables_without_a_factor_stay(lib, case, host_bare_new, reorder, fused):
    """Two new cameras and three new landmarks, camera C + 1 and landmark L + 2 named by no factor of the batch (scalars for the priors:
    the rule gives such a variable Lambda = 0): both are in the union, with prior lambda I, lambda mu and a belief that is the prior."""
    b, (o2n_h, bel_h, msg_h) = host_bare_new
    e = _engine(case.base, loss='huber', fused=fused, reorder_landmarks=reorder)
    e.iterate(3)
    C, L, F = e.C, e.L, e.F
    o2n = _ext(e, b, cam_prior_lambda=CAM_LAMBDA, lmk_prior_lambda=LMK_LAMBDA)
    np.testing.assert_array_equal(o2n, o2n_h)
    assert (e.C, e.L, e.F) == (C + 2, L + 3, F + b['meas'].shape[0]) and e.check_layout() == 0
    ce, cl, le, ll = e.priors()
    cm, lm = e.means()
    # lambda I is exact, lambda mu one product (1 ulp), the mean one solve with lambda I
    np.testing.assert_array_equal(cl[C + 1], CAM_LAMBDA[1] * np.eye(6))
    np.testing.assert_array_equal(ll[L + 2], LMK_LAMBDA[2] * np.eye(3))
    np.testing.assert_allclose(ce[C + 1], CAM_LAMBDA[1] * b['cam_means'][1], rtol=1e-15, atol=0)
    np.testing.assert_allclose(le[L + 2], LMK_LAMBDA[2] * b['lmk_means'][2], rtol=1e-15, atol=0)
    np.testing.assert_allclose(cm[C + 1], b['cam_means'][1], rtol=1e-12, atol=0)
    np.testing.assert_allclose(lm[L + 2], b['lmk_means'][2], rtol=1e-12, atol=0)
    bel = e.beliefs()
    for k, (pri, v) in enumerate(((ce, C + 1), (cl, C + 1), (le, L + 2), (ll, L + 2))):
        np.testing.assert_allclose(bel[k][v], pri[v], rtol=1e-12, atol=1e-15)
    worst = max([rel_err_rows(a, h) for a, h in zip(bel, bel_h)] + [rel_err_rows(a, h) for a, h in zip(e.messages(), msg_h)])
    print(f'bare new variables (reorder={reorder}, fused={fused}): worst belief / message gap to the host graph {worst:.3e}')
    assert worst < 1e-7, worst
    e.iterate(3)
    assert all(np.isfinite(x).all() for x in e.beliefs())
    e.close()


@HANDLES
@pytest.mark.parametrize('named', [True, False])
def test_an_old_camera_without_a_factor_stays(lib, case, reorder, fused, named):
    """window_host.bare_camera_problem(): camera 8 has no factor (its prior set by hand, as tools/rebuild_digest.py does).  Extend by
    base_case()'s batch -- which brings late observations of camera 8 (named) -- and by that batch without them: the camera keeps its
    id and its prior, and its belief is its prior (a new factor's messages are zero)."""
    from window_host import bare_camera_problem
    from gbp_amd.engine import BAEngine
    p, bare = bare_camera_problem(), 8
    e = BAEngine.from_problem(p, loss='huber', fused=fused, reorder_landmarks=reorder)
    e.generate_priors_var(W)
    pr = e.priors()
    lam = pr[1][:, 0, 0].max()
    pr[1][bare], pr[0][bare] = lam * np.eye(6), lam * p.cam_means[bare]
    e.set_priors(*pr)
    e.update_all_beliefs()
    e.iterate(3)
    b = case.batch
    assert (b['cam_idx'] == bare).any()
    if not named:
        ok = b['cam_idx'] != bare
        b = dict(b, meas=b['meas'][ok], cam_idx=b['cam_idx'][ok], lmk_idx=b['lmk_idx'][ok])
    before, C, L, F = _state(e), e.C, e.L, e.F
    o2n = _ext(e, b, prior_weaker_factor=W)
    assert (e.C, e.L, e.F) == (C + 2, L + b['lmk_means'].shape[0], F + b['meas'].shape[0]) and e.check_layout() == 0
    assert ((e.factors(dense=False)['cam'] == bare).sum() > 0) == named
    after = _state(e)
    for k in range(4):
        assert _bitwise(after['msg'][k][o2n], before['msg'][k])
    for k, n in zip(range(4), (C, C, L, L)):
        assert _bitwise(after['pri'][k][:n], before['pri'][k])
    for k in range(2):
        assert _bitwise(after['pri'][k][bare], pr[k][bare])
        np.testing.assert_allclose(after['bel'][k][bare], pr[k][bare], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(e.means()[0][bare], p.cam_means[bare], rtol=1e-12, atol=0)
    e.iterate(3)
    assert all(np.isfinite(x).all() for x in e.beliefs())
    e.close()


@HANDLES
def test_late_factors_of_old_cameras_move_old_ids(lib, case, reorder, fused):
    """No new variable, new factors between old ones only, one of camera 0's: every old factor behind camera 0's moves up
    (include/gbp_ba.h: old + the new factors of a lower camera), and carries its messages and linearisation point bit for bit."""
    from extend_cases import old_only_batch
    b = old_only_batch(case.base)
    e = _engine(case.base, loss='huber', fused=fused, reorder_landmarks=reorder)
    e.iterate(4)
    before, C, L, F = _state(e), e.C, e.L, e.F
    o2n = _ext(e, b, prior_weaker_factor=W)
    assert (e.C, e.L, e.F) == (C, L, F + b['meas'].shape[0])
    below = np.cumsum(np.bincount(b['cam_idx'], minlength=C))           # new factors of cameras <= c
    cam = before['fac']['cam']
    expect = np.arange(F) + np.where(cam > 0, below[np.maximum(cam, 1) - 1], 0)
    np.testing.assert_array_equal(o2n, expect)
    assert (o2n != np.arange(F)).sum() == (cam > 0).sum() > 0
    after = _state(e)
    for k in range(4):
        assert _bitwise(after['msg'][k][o2n], before['msg'][k])
        assert _bitwise(after['pri'][k], before['pri'][k])
    for key in ('linpoint', 'z', 'cam', 'lmk'):
        assert _bitwise(after['fac'][key][o2n], before['fac'][key])
    for key in ('iters_since_relin', 'eta_damping', 'adaptive_var', 'robust_flag'):
        assert _bitwise(after['rs'][key][o2n], before['rs'][key])
    e.close()


@HANDLES
def test_the_smallest_graphs_grow(lib, reorder, fused):
    """One camera, one landmark, one factor grows by one more of each (the new camera sees the old landmark, the new landmark nothing)."""
    from extend_cases import smallest_case
    base, b, _ = smallest_case()
    lam = np.array([2.0])
    e = _engine(base, fused=fused, reorder_landmarks=reorder)
    e.iterate(2)
    nb = make_numpy_ba(base)
    nb.generate_priors_var(W)
    nb.update_all_beliefs()
    nb.iterate(2)
    n0 = e.rebuild_count()
    o2n = _ext(e, b, prior_weaker_factor=W, lmk_prior_lambda=lam)
    np.testing.assert_array_equal(o2n, host_extend(nb, b, prior_weaker_factor=W, lmk_prior_lambda=lam))
    np.testing.assert_array_equal(o2n, [0])
    assert (e.C, e.L, e.F) == (2, 2, 2) and e.rebuild_count() == n0 + 1 and e.check_layout() == 0
    worst = max([rel_err_rows(a, h) for a, h in zip(e.beliefs(), nb.beliefs())] + [rel_err_rows(a, h) for a, h in zip(e.messages(), _host_messages(nb))])
    assert worst < 1e-7, worst
    np.testing.assert_array_equal(e.priors()[3][1], 2.0 * np.eye(3))
    e.iterate(3)
    assert all(np.isfinite(x).all() for x in e.beliefs())
    e.close()


@pytest.mark.parametrize('fused', [True, False])
def test_bad_id_in_a_device_batch_leaves_a_reordered_handle_untouched(lib, case, fused):
    import torch
    a, twin = (_engine(case.base, loss='huber', fused=fused, reorder_landmarks=True) for _ in range(2))
    for e in (a, twin):
        e.iterate(3)
    b = case.batch
    bad = dict(b, lmk_idx=b['lmk_idx'].copy())
    bad['lmk_idx'][3] = a.L + b['lmk_means'].shape[0]        # one past the union's landmarks
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in bad.items()}
    torch.cuda.synchronize()
    with pytest.raises(lib.GbpError) as ei:
        a.extend(t['cam_means'].data_ptr(), t['lmk_means'].data_ptr(), t['meas'].data_ptr(), t['cam_idx'].data_ptr(), t['lmk_idx'].data_ptr(),
                 device_pointers=(b['cam_means'].shape[0], b['lmk_means'].shape[0], b['meas'].shape[0]))
    assert ei.value.code == -1
    assert (a.C, a.L, a.F) == (twin.C, twin.L, twin.F)
    a.iterate(3)
    twin.iterate(3)
    assert _bitwise(a.save_state(), twin.save_state())
    for x, y in zip(a.beliefs(), twin.beliefs()):
        assert _bitwise(x, y)
    a.close()
    twin.close()


@HANDLES
def test_a_handle_created_without_a_factor_grows(lib, reorder, fused):
    """One camera and one landmark with no observation (priors by hand: the rule has nothing to go by) take smallest_case()'s batch."""
    from extend_cases import smallest_case
    from gbp_amd.engine import BAEngine
    _, b, bare = smallest_case()
    lam = np.array([2.0])
    e = BAEngine.from_problem(bare, fused=fused, reorder_landmarks=reorder)
    assert (e.C, e.L, e.F) == (1, 1, 0)
    e.set_priors(3.0 * bare.cam_means, 3.0 * np.eye(6)[None], 4.0 * bare.lmk_means, 4.0 * np.eye(3)[None])
    e.update_all_beliefs()
    pr = e.priors()
    o2n = _ext(e, b, prior_weaker_factor=W, lmk_prior_lambda=lam)
    assert o2n.size == 0 and (e.C, e.L, e.F) == (2, 2, 1) and e.check_layout() == 0
    fac = e.factors(dense=False)
    assert (int(fac['cam'][0]), int(fac['lmk'][0])) == (1, 0) and _bitwise(fac['z'][0], b['meas'][0])
    after = e.priors()
    for k in range(4):
        assert _bitwise(after[k][0], pr[k][0])
    np.testing.assert_array_equal(after[3][1], 2.0 * np.eye(3))
    e.iterate(3)
    assert all(np.isfinite(x).all() for x in e.beliefs())
    e.close()
