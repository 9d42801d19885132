"""gbp_ba_retire / BAEngine.retire on the GPU: cameras leave a live BA graph, their factors' messages are folded into the landmarks'
priors and everything that stays keeps its GBP state.  The mirror of tests/test_extend_gpu.py.

Oracle: tests/retire_host.py retires the same cameras from the reference's own object graph (NumpyBA).  The structural checks pin the
shrunk handle to a handle freshly created from the survivors (same plan, bitwise the same sweeps after a state load) and the carried
state to its value before the call, bit for bit.  Tolerances are those of the extend tests."""
import numpy as np
import pytest

from conftest import rel_err_rows
from retire_host import make_numpy_ba, retire_numpy_ba, survivors_problem

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


def _state(e):
    return dict(bel=e.beliefs(), msg=e.messages(), fac=e.factors(dense=False), rs=e.relin_state(), pri=e.priors())


def _bitwise(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _survivors(e, K, maps, before):
    """The survivors' problem of engine state `before` (taken before the retirement) under `maps`."""
    fac = before['fac']
    return survivors_problem((K, before['means'][0], before['means'][1], fac['z'], fac['cam'], fac['lmk']), *maps)


def _host(problem, **kw):
    nb = make_numpy_ba(problem, **kw)
    nb.generate_priors_var(W)
    nb.update_all_beliefs()
    return nb


def _same_step(e, nb, where, worst):
    """One sweep on both; the same factors relinearise, ARE within 1e-8, beliefs recorded."""
    e.iterate(1)
    nb.iterate(1)
    np.testing.assert_array_equal(e.iters_since_relin() == 0, np.array([f.iters_since_relin == 0 for f in nb.graph.factors]), str(where))
    assert e.relin_counts(1)[0] == int(sum(f.iters_since_relin == 0 for f in nb.graph.factors)), where
    assert abs(e.are() - nb.are()) <= 1e-8 * abs(nb.are()), where
    return _belief_gap(e, nb, where, worst)


def _belief_gap(e, nb, where, worst):
    for a, h in zip(e.beliefs(), nb.beliefs()):
        gap = rel_err_rows(a, h)
        assert gap < 1e-7, (where, gap)
        worst = max(worst, gap)
    return worst


# ---- 1. fixed-lag replay against the host oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize('fused', [True, False, None])
@pytest.mark.parametrize('loss', [None, 'huber'])
def test_fixed_lag_replay_matches_host_oracle(lib, fused, loss):
    p = _problem()
    e = _engine(p, fused=fused, loss=loss)
    nb = _host(p, loss=loss)
    worst = 0.0
    for k, gone in enumerate([None, [3, 0], [0, 1, 2], [1]]):
        if gone is not None:
            md, mh = e.retire(gone), retire_numpy_ba(nb, gone)
            for a, b in zip(md, mh):
                np.testing.assert_array_equal(a, b)
            assert (e.C, e.L, e.F) == (nb.C, nb.L, len(nb.graph.factors))
            worst = _belief_gap(e, nb, (k, 'retire'), worst)
            pe = e.priors()
            assert rel_err_rows(pe[2], np.array([v.prior.eta for v in nb.lmks])) < 1e-7
            assert rel_err_rows(pe[3], np.array([v.prior.lam for v in nb.lmks])) < 1e-7
        for s in range(6):
            worst = _same_step(e, nb, (k, s), worst)
        rs = e.relin_state()
        np.testing.assert_array_equal(rs['iters_since_relin'], [f.iters_since_relin for f in nb.graph.factors])
        np.testing.assert_array_equal(rs['eta_damping'], [f.eta_damping for f in nb.graph.factors])
    assert worst < 1e-7, worst
    e.close()


class _EngineGraph:
    """BAEngine behind the methods g18_replay calls (tests/retire_host.py)."""

    def __init__(self, base, loss, fused):
        from gbp_amd.engine import BAEngine
        self.e = BAEngine.from_problem(base, loss=loss, fused=fused)

    def __getattr__(self, name):
        return getattr(self.e, name)

    def relin(self):
        rs = self.e.relin_state()
        return rs['iters_since_relin'], rs['eta_damping'], rs['adaptive_var']

    def lmk_priors(self):
        pr = self.e.priors()
        return pr[2], pr[3]


@pytest.mark.parametrize('fused', [True, False, None])
@pytest.mark.parametrize('tag', ['small', 'vsmall_huber'])
def test_g18_reference_retirement_replay(lib, tag, fused):
    """Fixture G18: the reference's own classes ran this fixed-lag schedule (make_g18.py).  Maps equal, relinearisation counts exact every
    sweep, beliefs (and the folded landmark priors) < 1e-6, messages < 1e-5, ARE / energy at the G17 replay's tolerances, iters_since_relin
    and eta_damping exact at batch ends -- through both retirements and all 30 sweeps of either run."""
    from conftest import golden
    from retire_host import g18_problem, g18_replay
    g = golden(f'G18_retire_{tag}')
    eg = _EngineGraph(g18_problem(g), None if str(g['loss']) == 'None' else str(g['loss']), fused)
    worst = g18_replay(g, eg, belief_tol=1e-6, msg_tol=1e-5, verbose=True)
    print(f'G18 {tag} fused={fused}: worst belief gap {worst:.3e}')
    assert worst < 1e-6
    eg.e.close()


# ---- 2. carried state is bitwise, the fold is the messages' sum ------------------------------------------------------------------
@pytest.mark.parametrize('gone', [[3, 0], [0, 1, 2, 3, 4, 5]])
def test_carry_is_bitwise(lib, gone):
    p = _problem()
    e = _engine(p, loss='huber')
    e.iterate(4)
    before = _state(e)
    cm, lm, fm = e.retire(gone)
    after = _state(e)
    kc, kl, kf = cm >= 0, lm >= 0, fm >= 0
    assert kc.sum() == 16 - len(gone) and (~kf).sum() == np.isin(before['fac']['cam'], gone).sum()
    if len(gone) > 2:
        assert (~kl).any()                                    # orphans were dropped
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
        print(f'retire {gone}: belief array {k} moved by {gap:.3e}')
        assert gap <= 1e-12
    assert _bitwise(after['pri'][0], before['pri'][0][kc]) and _bitwise(after['pri'][1], before['pri'][1][kc])
    # landmark priors: old prior + the retired factors' messages in adj_factors (= reference id) order; untouched landmarks bit for bit
    eta, lam = before['pri'][2].copy(), before['pri'][3].copy()
    touched = np.zeros(p.n_lmks, bool)
    for f in np.flatnonzero(~kf):
        l = before['fac']['lmk'][f]
        eta[l] += before['msg'][2][f]
        lam[l] += before['msg'][3][f]
        touched[l] = True
    assert _bitwise(after['pri'][2][~touched[kl]], before['pri'][2][kl & ~touched])
    assert _bitwise(after['pri'][3][~touched[kl]], before['pri'][3][kl & ~touched])
    assert touched[kl].any()
    assert rel_err_rows(after['pri'][2], eta[kl]) <= 1e-12 and rel_err_rows(after['pri'][3], lam[kl]) <= 1e-12
    assert e.check_layout() == 0
    e.close()


# ---- 3. retire = create of the survivors + the carried state ---------------------------------------------------------------------
@pytest.mark.parametrize('fused', [True, False, None])
def test_retire_equals_create_plus_state(lib, fused):
    p = _problem()
    runs = []
    for _ in range(2):
        e = _engine(p, fused=fused)
        e.iterate(3)
        before = dict(_state(e), means=e.means())
        maps = e.retire([3, 0])
        e.iterate(2)
        runs.append(e)
    a, b2 = runs
    for x, y in zip(a.beliefs(), b2.beliefs()):
        assert _bitwise(x, y)
    assert _bitwise(a.save_state(), b2.save_state())           # reproducible run to run
    f = _engine(_survivors(a, p.K, maps, before), fused=fused)
    assert a.plan_info() == f.plan_info() and a.info() == f.info()
    f.load_state(a.save_state())                              # same graph hash, same layout
    a.iterate(10)
    f.iterate(10)
    sa, sf = _state(a), _state(f)
    for k in range(4):
        assert _bitwise(sa['bel'][k], sf['bel'][k]) and _bitwise(sa['msg'][k], sf['msg'][k])
    for key in ('iters_since_relin', 'eta_damping'):
        assert _bitwise(sa['rs'][key], sf['rs'][key])
    for e in runs + [f]:
        e.close()


# ---- 4. the plan follows the graph as it shrinks ---------------------------------------------------------------------------------
def test_plan_changes_under_shrinkage(lib):
    """More random cameras than one LDS table holds (no windows: every workgroup meets most cameras): the general sweep.  Retired down to
    100 cameras the handle is re-planned as gbp_ba_create would plan the survivors: the fused sweep (whole tables or windows); the run
    stays with the same run forced onto the general sweep."""
    lim = lib.load().gbp_ba_fused_max_cams()
    n = lim + 60
    p = _problem(n_cams=n, n_lmks=60_000, obs=10, window=None, seed=5)      # (~930 factors per camera: every workgroup meets nearly all cameras)
    gone = np.arange(100, n)
    plans, bels = [], []
    for fused in (None, False):
        e = _engine(p, fused=fused)
        e.iterate(2)
        pl = [e.plan_info()]
        e.retire(gone)
        e.iterate(2)
        pl.append(e.plan_info())
        plans.append(pl)
        bels.append(e.beliefs())
        assert e.C == 100 and e.check_layout() == 0
        e.close()
    auto = plans[0]
    assert not auto[0]['fused'] and not auto[0]['staged_by_sparseness'], auto[0]       # above the LDS camera limit, no windows
    assert auto[1]['fused'], auto[1]
    assert all(not x['fused'] for x in plans[1])
    for x, y in zip(*bels):
        assert rel_err_rows(x, y) < 1e-10


# ---- 5. a sliding window on the headline family ----------------------------------------------------------------------------------
def _slide(p, base, step, rounds, host=False, **kw):
    """Base of `base` cameras of sequence `p`, then `rounds` times: extend by `step` cameras, 2 sweeps, retire the oldest `step`, 2 sweeps."""
    from gbp_amd.synthetic import keyframe_batches
    from extend_host import extend as host_extend
    sp = keyframe_batches(p, [base] + [step] * rounds)
    e = _engine(sp.base, **kw)
    nb = _host(sp.base, **kw) if host else None
    e.iterate(2)
    if nb:
        nb.iterate(2)
    trace, worst = [(e.C, e.L, e.F, e.plan_info())], 0.0
    cam_now, lmk_now = np.arange(e.C), np.arange(e.L)         # id in the batches' numbering (nothing ever retired) -> id now, -1: gone
    for r, b in enumerate(sp.batches):
        cam_now = np.concatenate([cam_now, e.C + np.arange(b['cam_means'].shape[0])])
        lmk_now = np.concatenate([lmk_now, e.L + np.arange(b['lmk_means'].shape[0])])
        ci, li = cam_now[b['cam_idx']], lmk_now[b['lmk_idx']]
        seen = (ci >= 0) & (li >= 0)                          # (an observation of a landmark that left as an orphan is dropped)
        b = dict(b, meas=b['meas'][seen], cam_idx=ci[seen].astype(np.int32), lmk_idx=li[seen].astype(np.int32))
        e.extend(b['cam_means'], b['lmk_means'], b['meas'], b['cam_idx'], b['lmk_idx'], prior_weaker_factor=W)
        if nb:
            host_extend(nb, b, prior_weaker_factor=W)
            worst = _belief_gap(e, nb, (r, 'extend'), worst)
            for s in range(2):
                worst = _same_step(e, nb, (r, 'e', s), worst)
        else:
            e.iterate(2)
        cm, lm, _ = e.retire(np.arange(step))
        cam_now[cam_now >= 0] = cm[cam_now[cam_now >= 0]]
        lmk_now[lmk_now >= 0] = lm[lmk_now[lmk_now >= 0]]
        if nb:
            mh = retire_numpy_ba(nb, np.arange(step))
            np.testing.assert_array_equal(cm, mh[0])
            np.testing.assert_array_equal(lm, mh[1])
            worst = _belief_gap(e, nb, (r, 'retire'), worst)
            for s in range(2):
                worst = _same_step(e, nb, (r, 'r', s), worst)
        else:
            e.iterate(2)
        trace.append((e.C, e.L, e.F, e.plan_info()))
    ok = e.check_layout() == 0 and np.isfinite(e.are())
    e.close()
    return trace, worst, ok


def test_sliding_window_stays_bounded(lib):
    """A 2 000-camera sequence walked with a 1 000-camera window in steps of 50.  The bounds come from the problem, not from the run: after
    round r the handle holds cameras [50 r, 1000 + 50 r), so its factors are the observations of those cameras (all of them but the few of
    landmarks that left as orphans and came back into view), its landmarks the ones they see, and the fused sweep's tables have at most
    workgroups x window cameras rows -- never the whole sequence's."""
    p = _problem(n_cams=2000, n_lmks=40_000, obs=6, window=60, seed=11)
    trace, _, ok = _slide(p, 1000, 50, 6)
    assert ok
    plan0 = trace[0][3]
    for r, (C, L, F, plan) in enumerate(trace):
        inside = (p.cam_idx >= 50 * r) & (p.cam_idx < 1000 + 50 * r)
        print(f'round {r}: C {C} L {L} F {F} of {int(inside.sum())} in the window; tiles {plan["n_tiles"]} rows {plan["table_rows"]} fused {plan["fused"]}')
        assert C == 1000
        assert 0.95 * inside.sum() <= F <= inside.sum(), (r, F, int(inside.sum()))
        assert L <= np.unique(p.lmk_idx[inside]).size
        assert plan['fused'] == plan0['fused'] and plan['table_rows'] <= plan['n_blocks'] * C, plan
        assert 64 * plan['n_tiles'] >= F and plan['n_tiles'] <= (F + 63) // 64 + L, plan
    assert trace[-1][2] < 0.6 * p.n_factors


@pytest.mark.parametrize('loss', [None, 'huber'])
def test_sliding_window_matches_host_on_a_sampled_subproblem(lib, loss):
    """The same family and the same slide (extend, sweeps, retire the oldest, sweeps) small enough for the object graph: 40 of 64 cameras."""
    p = _problem(n_cams=64, n_lmks=640, obs=6, window=10, seed=11)
    trace, worst, ok = _slide(p, 40, 6, 4, host=True, loss=loss)
    assert ok and worst < 1e-7
    assert all(t[0] == 40 for t in trace)


# ---- 6. edge cases ---------------------------------------------------------------------------------------------------------------
def test_empty_list_continues_bitwise(lib):
    p = _problem()
    a, twin = _engine(p), _engine(p)
    a.iterate(3)
    twin.iterate(3)
    cm, lm, fm = a.retire([])
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


def _tracks_host(setup, step, tol, **kw):
    """Set both up, retire, step both: the engine stays with the host model."""
    p = _problem()
    e, nb = _engine(p, **kw), _host(p, **kw)
    for x in (e, nb):
        setup(x)
    gone = [3, 0, 1]
    for a, b in zip(e.retire(gone), retire_numpy_ba(nb, gone)):
        np.testing.assert_array_equal(a, b)
    pe = e.priors()
    assert rel_err_rows(pe[2], np.array([v.prior.eta for v in nb.lmks])) <= tol
    assert rel_err_rows(pe[3], np.array([v.prior.lam for v in nb.lmks])) <= tol
    for x in (e, nb):
        step(x)
    for k, (a, h) in enumerate(zip(e.beliefs(), nb.beliefs())):
        assert rel_err_rows(a, h) <= tol, k
    rs = e.relin_state()
    np.testing.assert_array_equal(rs['iters_since_relin'], [f.iters_since_relin for f in nb.graph.factors])
    np.testing.assert_array_equal(rs['eta_damping'], [f.eta_damping for f in nb.graph.factors])
    e.close()


def test_dense_remainder_is_folded_and_carried(lib):
    _tracks_host(lambda x: x.iterate(9), lambda x: x.iterate(9), tol=1e-9, num_undamped_iters=0)


def test_pending_relinearisation_survives_retire(lib):
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


def test_snapshot_is_dropped_and_means_stream_after_retirement(lib):
    e = _engine(_problem())
    e.iterate(2)
    e.snapshot_state()
    e.means_snapshot()
    e.retire([0, 1])
    with pytest.raises(lib.GbpError) as ei:
        e.restore_snapshot()
    assert ei.value.code == -5
    e.means_snapshot()
    cm, lm = e.means_fetch(wait=True)
    rc, rl = e.means()
    assert cm.shape == (14, 6) and _bitwise(cm, rc) and _bitwise(lm, rl)
    e.close()


def test_a_camera_without_a_factor_stays_under_retire_and_goes_under_cull(lib):
    """gbp_ba_retire drops the cameras on its list and no other (include/gbp_ba.h step 2; retire_host: keep_c), every other shrinking call
    drops a camera no staying factor names.  window_host.bare_camera_problem: camera 8 of 16 has no factor.  The prior rule gives such a
    camera Lambda = 0 (a singular belief), so it gets the strongest prior the rule gave any camera, on the handle and on the host."""
    from cull_host import cull_numpy_ba
    from window_host import bare_camera_problem
    from gbp_amd.engine import BAEngine
    p, bare = bare_camera_problem(), 8

    def pair():
        e, nb = BAEngine.from_problem(p, loss='huber'), make_numpy_ba(p, loss='huber')
        e.generate_priors_var(W)
        nb.generate_priors_var(W)
        pr = e.priors()
        lam = pr[1][:, 0, 0].max()
        pr[1][bare], pr[0][bare] = lam * np.eye(6), lam * p.cam_means[bare]
        e.set_priors(*pr)
        nb.cams[bare].prior.lam, nb.cams[bare].prior.eta = pr[1][bare].copy(), pr[0][bare].copy()
        for x in (e, nb):
            x.update_all_beliefs()
            x.iterate(3)
        return e, nb
    e, nb = pair()
    md, mh = e.retire([0]), retire_numpy_ba(nb, [0])
    assert md[0][bare] >= 0 and md[0][0] == -1
    for a, b in zip(md, mh):
        np.testing.assert_array_equal(a, b)
    assert (e.C, e.L, e.F) == (nb.C, nb.L, len(nb.graph.factors)) and e.check_layout() == 0
    worst = _belief_gap(e, nb, 'retire', 0.0)
    for s in range(3):
        worst = _same_step(e, nb, s, worst)
    print(f'bare camera, retire: worst belief gap {worst:.3e}')
    e.close()
    e, nb = pair()
    md, mh = e.cull([100]), cull_numpy_ba(nb, [100])
    assert md[0][bare] == -1 and (md[0] >= 0).sum() == 15
    for a, b in zip(md, mh):
        np.testing.assert_array_equal(a, b)
    assert e.check_layout() == 0
    _belief_gap(e, nb, 'cull', 0.0)
    e.close()


# ---- 7. failures leave the handle as it was --------------------------------------------------------------------------------------
def test_failures_leave_the_handle_untouched(lib):
    from gbp_amd.engine import BAEngine
    p = _problem()
    a, twin = _engine(p), _engine(p)
    for e in (a, twin):
        e.iterate(3)
    blob = a.save_state()
    for bad in ([2, 2], [16], [-1], list(range(16))):
        with pytest.raises(lib.GbpError) as ei:
            a.retire(bad)
        assert ei.value.code == -1, bad
        assert (a.C, a.L, a.F) == (twin.C, twin.L, twin.F)
        assert _bitwise(a.save_state(), blob)
    ids = np.array([1], np.int32)
    h = a._h
    assert lib.load().gbp_ba_retire(h, -1, lib.iptr(ids), None, None, None) == -1
    assert lib.load().gbp_ba_retire(h, 1, None, None, None, None) == -1
    assert _bitwise(a.save_state(), blob)
    a.iterate(4)
    twin.iterate(4)
    assert _bitwise(a.save_state(), twin.save_state())
    a.close()
    twin.close()
    # no beliefs yet: the handle then goes on as an untouched one
    f, ft = BAEngine.from_problem(p), BAEngine.from_problem(p)
    with pytest.raises(lib.GbpError) as ei:
        f.retire([0])
    assert ei.value.code == -5
    for x in (f, ft):
        x.generate_priors_var(W)
        x.update_all_beliefs()
        x.iterate(3)
    assert _bitwise(f.save_state(), ft.save_state())
    f.close()
    ft.close()


def test_sharded_handles_refuse_to_retire(lib):
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
            e.retire([0])
        assert ei.value.code == -5
    for x, y in zip(shrunk, twin):
        assert _bitwise(x.save_state(), y.save_state())
    for e in shrunk + twin:
        e.close()
    g, gt = _engine(p), _engine(p)
    for x in (g, gt):
        x.set_exchange(lambda s_, r_, n_, st: 0, 0, 1)
    with pytest.raises(lib.GbpError) as ei:
        g.retire([0])
    assert ei.value.code == -5
    for x in (g, gt):
        x.iterate_sharded(3)
    assert _bitwise(g.save_state(), gt.save_state())
    g.close()
    gt.close()


# ---- 8. the drop-in package ------------------------------------------------------------------------------------------------------
def test_compat_graph_shrinks(lib):
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
    cam_of = np.array([f.adj_vIDs[0] for f in g.factors])
    mu5 = np.array(g.cam_nodes[5].mu)
    cm, lm, fm = g.retire_keyframes([3, 0])
    kf = fm >= 0
    assert len(g.cam_nodes) == 14 and len(g.lmk_nodes) == int((lm >= 0).sum()) and len(g.factors) == int(kf.sum())
    assert len(g.var_nodes) == len(g.cam_nodes) + len(g.lmk_nodes) and g.n_factor_nodes == len(g.factors) and g.n_edges == 2 * len(g.factors)
    assert [f.iters_since_relin for f in g.factors] == list(its[kf])
    e = g._engine
    fac = e.factors(dense=False)
    for i in range(0, len(g.factors), 37):
        assert list(g.factors[i].adj_vIDs) == [int(fac['cam'][i]), len(g.cam_nodes) + int(fac['lmk'][i])]
    np.testing.assert_array_equal([f.adj_vIDs[0] for f in g.factors], cm[cam_of[kf]])
    np.testing.assert_allclose(g.cam_nodes[int(cm[5])].mu, mu5, rtol=1e-12)
    g.synchronous_iteration()
    assert np.isfinite(g.are())
