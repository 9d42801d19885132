"""Robust (Huber / constant) losses on the nonlinear (SE(2) relative-pose) path of the linear engine on the MI355X (include/gbp_lin.h:
gbp_lin_set_robust_nonlinear / robustify_nonlinear / iterate_nonlinear_robust; the fused robustify + relinearise lane of
gbp_amd/csrc/gbp_lin_nonlin.hpp): against the reference's own run (fixture G27) and the numpy twin of tests/lin_nonlin_robust_cases.py
with flags, masks and both counts compared exactly; bit identity with the plain path and of the fused lane with its two steps; the
solvers on the weighted joint; the range set; a live smoother; the refusals.  fp64 throughout.
Every seeded case here is shown by test_linear_nonlinear_robust_cpu.py to stay >= 1e-7 clear of `M > t` and of `dist > beta`."""
import ctypes as ct

import numpy as np
import pytest

from conftest import golden
from lin_map_cases import rel
from lin_nonlin_cases import PARITY, SCHEDULE, SWEEPS, TOL
from lin_nonlin_robust_cases import CASES, CONSTANT, HUBER, LOSS_NAME, NONE, case, g27_graph, g27_schedule, live_schedule, robust_twin

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5


def make_engine(g, sched=SCHEDULE, losses=True):
    from gbp_amd.linear import LinearEngine
    e = LinearEngine.se2_pose_graph(g['va'], g['vb'], g['z'], g['s'], g['prior_eta'], g['prior_lam'], sched['beta'],
                                    sched['num_undamped_iters'], sched['min_linear_iters'], eta_damping=sched['eta_damping'])
    if losses and 'loss' in g:
        e.set_robust([LOSS_NAME[int(l)] for l in g['loss']], g['thr'])
    return e


def state(e):
    """Everything a robust sweep writes, for bit-for-bit comparisons."""
    w, flag = e.weights()
    return list(e.messages()) + list(e.beliefs()) + [e.get_means()] + list(e.linearisation()) + [w, flag, np.array(e.energy())]


def same_bits(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def assert_matches_twin(e, t, what, tol=TOL):
    lp, it, dm = e.linearisation()
    w, flag = e.weights()
    assert np.array_equal(flag, t.flag), f"{what}: flags differ at {np.nonzero(flag != t.flag)[0][:5]}"
    assert np.array_equal(it, t.iters), f"{what}: iters differ at {np.nonzero(it != t.iters)[0][:5]}"
    assert np.array_equal(dm, t.fdamp), f"{what}: damping differs at {np.nonzero(dm != t.fdamp)[0][:5]}"
    assert rel(w, t.w) < tol, f"{what}: weights {rel(w, t.w):.3e}"
    assert rel(lp, t.linpoint) < tol, f"{what}: linpoint {rel(lp, t.linpoint):.3e}"
    for name, a, b in zip(('eta_a', 'lam_a', 'eta_b', 'lam_b'), e.messages(), t.messages()):
        assert rel(a, b) < tol, f"{what}: message {name} {rel(a, b):.3e}"
    for name, a, b in zip(('eta', 'lam'), e.beliefs(), t.beliefs()):
        assert rel(a, b) < tol, f"{what}: belief {name} {rel(a, b):.3e}"
    assert rel(e.get_means(), t.get_means()) < tol, f"{what}: means {rel(e.get_means(), t.get_means()):.3e}"
    ee, et = e.energy(), t.energy()
    assert abs(ee - et) <= tol * max(abs(et), 1.0), f"{what}: energy {ee!r} vs {et!r}"
    # eta_f, Lambda_f times w_f as every user of the factor reads them: the joint's eta, and its product with a fixed vector
    je, jl = t.joint()
    x = np.cos(np.arange(je.size) * 0.37)
    assert rel(e.joint_eta().reshape(-1), je) < tol, f"{what}: eta_f {rel(e.joint_eta().reshape(-1), je):.3e}"
    assert rel(e.joint_matvec(x).reshape(-1), jl @ x) < tol, f"{what}: Lambda_f {rel(e.joint_matvec(x).reshape(-1), jl @ x):.3e}"


# ---- parity -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_case_matches_twin(name):
    """SWEEPS robust relinearising sweeps in one call: both counts exactly, the state within TOL of the twin, flags and iters exactly."""
    g, sched = case(name)
    e, t = make_engine(g, sched), robust_twin(g, sched)
    assert_matches_twin(e, t, f'{name} after set_robust')
    rc, fc = e.iterate(SWEEPS, robustify=True, relinearise=True)
    trc, tfc = t.iterate(SWEEPS, relinearise=True, robustify=True)
    assert rc.tolist() == trc.tolist(), f"{name}: relin_counts {rc.tolist()} vs {trc.tolist()}"
    assert fc.tolist() == tfc.tolist(), f"{name}: robust_counts {fc.tolist()} vs {tfc.tolist()}"
    assert_matches_twin(e, t, f'{name} after {SWEEPS} sweeps')
    e.close()


def test_reference_run_sweep_by_sweep():
    """G27 one sweep per call: flags, masks, iters, damping and both counts exactly; weights, means, energy, linpoints, messages and
    beliefs within the parity contract against the reference's stored run."""
    g = golden('G27_se2_posegraph_robust')
    sched, sweeps = g27_schedule(g)
    graph = g27_graph(g)
    e = make_engine(graph, sched)
    worst = {}

    def gap(name, a, b):
        worst[name] = max(worst.get(name, 0.0), rel(a, b))
        assert rel(a, b) < PARITY, f"{name}: {rel(a, b):.3e}"

    for s in range(sweeps):
        rc, fc = e.iterate(1, robustify=True, relinearise=True)
        lp, it, dm = e.linearisation()
        w, flag = e.weights()
        assert np.array_equal(flag, g['flag'][s].astype(bool)), f"sweep {s}: flags"
        assert np.array_equal(it == 0, g['mask'][s].astype(bool)), f"sweep {s}: mask"
        assert rc.tolist() == [int(g['mask'][s].sum())] and fc.tolist() == [int(g['flag'][s].sum())], f"sweep {s}: counts {rc} {fc}"
        assert np.array_equal(it, g['iters'][s]) and np.array_equal(dm, g['damp'][s]), f"sweep {s}: iters / damping"
        gap('weights', w, g['w'][s]); gap('means', e.get_means(), g['means'][s]); gap('energy', e.energy(), g['energy'][s])
        k = f's{s + 1}_'
        if k + 'linpoint' in g:
            gap('linpoint', lp, g[k + 'linpoint'])
            for name, a in zip(('msg_eta_a', 'msg_lam_a', 'msg_eta_b', 'msg_lam_b'), e.messages()):
                gap('messages', a, g[k + name])
            eta, lam = e.beliefs()
            gap('beliefs', eta, g[k + 'bel_eta']); gap('beliefs', lam, g[k + 'bel_lam'])
    print('worst gaps against the reference', {k: f'{v:.2e}' for k, v in worst.items()})
    e.close()


# ---- bit identity -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('how', ['all_none', 'never_reached'])
def test_without_effective_losses_the_robust_sweep_is_the_plain_one(how):
    g, sched = case('ring129')
    plain, rob = make_engine(g, sched, losses=False), make_engine(g, sched, losses=False)
    if how == 'all_none':
        rob.set_robust([None] * rob.F)
    else:
        rob.set_robust(['huber', 'constant'] * (rob.F // 2) + ['huber'] * (rob.F % 2), 1e9)
    pc = plain.iterate(SWEEPS, relinearise=True)
    rc, fc = rob.iterate(SWEEPS, robustify=True, relinearise=True)
    assert rc.tolist() == pc.tolist() and not fc.any()
    assert same_bits(state(plain), state(rob))
    plain.close(); rob.close()


def test_two_handles_same_calls_same_bits():
    g, sched = case('ring65')
    a, b = make_engine(g, sched), make_engine(g, sched)
    ca, cb = a.iterate(SWEEPS, robustify=True, relinearise=True), b.iterate(SWEEPS, robustify=True, relinearise=True)
    assert ca[0].tolist() == cb[0].tolist() and ca[1].tolist() == cb[1].tolist() and ca[1].any()
    assert same_bits(state(a), state(b))
    a.close(); b.close()


@pytest.mark.parametrize('name', ['ring129', 'beta0'])
def test_fused_lane_equals_separate_steps(name):
    """robustify_nonlinear then iterate_nonlinear(1) == iterate_nonlinear_robust(1), bit for bit, sweep after sweep."""
    g, sched = case(name)
    a, b = make_engine(g, sched), make_engine(g, sched)
    for s in range(6):
        a.robustify_all_factors()
        ca = a.iterate(1, relinearise=True)
        cb, fb = b.iterate(1, robustify=True, relinearise=True)
        assert ca.tolist() == cb.tolist() and fb[0] == a.weights()[1].sum()
        assert same_bits(state(a), state(b)), f"sweep {s}"
    assert a.weights()[1].any() and not a.weights()[1].all()
    a.close(); b.close()


# ---- solvers ------------------------------------------------------------------------------------------------------------------------

def test_solvers_describe_the_weighted_joint():
    g, sched = case('ring65')
    e, t = make_engine(g, sched), robust_twin(g, sched)
    e.iterate(4, robustify=True, relinearise=True); t.iterate(4, relinearise=True, robustify=True)
    assert t.flag.any()
    je, jl = t.joint()
    x = np.sin(np.arange(je.size) * 0.11)
    assert rel(e.joint_eta().reshape(-1), je) < TOL and rel(e.joint_matvec(x).reshape(-1), jl @ x) < TOL
    mu, info = e.solve_map()
    assert info['converged'] and rel(mu.reshape(-1), np.linalg.solve(jl, je)) < 1e-6      # rel_tol 1e-12 on the residual, cond <= 1e6
    # the stale marking: a robustify alone changes the next solve
    e.iterate(3, relinearise=True); t.iterate(3, relinearise=True)                           # the linpoints move, the weights stand
    before, _ = e.solve_map()
    e.robustify_all_factors(); t.robustify_all_factors()
    after, _ = e.solve_map()
    je, jl = t.joint()
    assert rel(after.reshape(-1), np.linalg.solve(jl, je)) < 1e-6
    assert np.max(np.abs(after - before)) > 1e-5, "the solve did not see the new weights"
    sig, minfo = e.marginals(ids=[0, 7, 30])
    dense = np.linalg.inv(jl)
    assert minfo['converged']
    for i, v in enumerate((0, 7, 30)):
        assert rel(sig[i], dense[3 * v:3 * v + 3, 3 * v:3 * v + 3]) < 1e-6
    e.close()


# ---- the range set ------------------------------------------------------------------------------------------------------------------

def test_range_set_and_clear():
    g, sched = case('ring65')
    e = make_engine(g, sched)
    e.joint_eta()                                               # the solver workspace, which the comparisons with the twin use, exists
    base = e.alloc_count()
    e.iterate(3, robustify=True, relinearise=True)
    w0, f0 = e.weights()
    assert f0.any() and (w0 < 1).any()
    lo, hi = 20, 41
    assert (w0[lo:hi] < 1).any() and (w0[:lo] < 1).any()
    e.set_robust(['constant'] * (hi - lo), 2.5, first=lo)
    w1, f1 = e.weights()
    assert np.all(w1[lo:hi] == 1.0) and not f1[lo:hi].any()
    assert w1[:lo].tobytes() == w0[:lo].tobytes() and w1[hi:].tobytes() == w0[hi:].tobytes()
    assert np.array_equal(f1[:lo], f0[:lo]) and np.array_equal(f1[hi:], f0[hi:])
    t = robust_twin(g, sched)
    t.iterate(3, relinearise=True, robustify=True)
    t.set_robust(np.full(hi - lo, CONSTANT), 2.5, first=lo)
    e.iterate(3, robustify=True, relinearise=True); t.iterate(3, relinearise=True, robustify=True)
    assert_matches_twin(e, t, 'after the range set')
    assert e.alloc_count() == base
    # clearing: all weights 1, nothing allocated or freed, the robust calls refused again
    e.set_robust(None)
    w, f = e.weights()
    assert np.all(w == 1.0) and not f.any() and e.alloc_count() == base
    assert e._lib.gbp_lin_iterate_nonlinear_robust(e._h, 1, None, None) == ESTATE and e._lib.gbp_lin_robustify_nonlinear(e._h) == ESTATE
    # ... and the handle is back on the plain path: one whose losses never acted (a threshold never reached) is, from the sweep after
    # the clear on, bit for bit the handle that never had losses
    plain, both = make_engine(g, sched, losses=False), make_engine(g, sched, losses=False)
    both.set_robust('huber', 1e9)
    plain.iterate(3, relinearise=True); both.iterate(3, robustify=True, relinearise=True)
    both.set_robust(None)
    cp, cb = plain.iterate(SWEEPS, relinearise=True), both.iterate(SWEEPS, relinearise=True)
    assert cp.tolist() == cb.tolist() and same_bits(state(plain), state(both))
    for h in (e, plain, both):
        h.close()


# ---- live ---------------------------------------------------------------------------------------------------------------------------

def test_live_smoother_with_losses_on_new_closures():
    g0, rounds = live_schedule()
    e, t = make_engine(g0), robust_twin(g0)
    allocs = []
    for k, (ext, (off, codes, thr), sweeps, shr) in enumerate(rounds):
        F0 = e.F
        w0, f0 = e.weights()
        e.extend_se2(ext['va'], ext['vb'], ext['z'], ext['s'], ext['prior_eta'], ext['prior_lam']); t.extend(**ext)
        w1, f1 = e.weights()
        assert w1[:F0].tobytes() == w0.tobytes() and np.array_equal(f1[:F0], f0) and np.all(w1[F0:] == 1.0) and not f1[F0:].any()
        e.set_robust([LOSS_NAME[int(c)] for c in codes], thr, first=F0 + off); t.set_robust(codes, thr, first=F0 + off)
        w2, _ = e.weights()
        assert w2[:F0].tobytes() == w0.tobytes()
        rc, fc = e.iterate(sweeps, robustify=True, relinearise=True)
        trc, tfc = t.iterate(sweeps, relinearise=True, robustify=True)
        assert rc.tolist() == trc.tolist() and fc.tolist() == tfc.tolist(), f"round {k}: counts"
        if shr:
            w3, f3 = e.weights()
            _, fmap = e.shrink(retire_vars=shr['retire'], drop_factors=shr['drop'], fold=shr['fold'])
            t.shrink(**shr)
            w4, f4 = e.weights()
            assert w4.tobytes() == w3[fmap >= 0].tobytes() and np.array_equal(f4, f3[fmap >= 0]), f"round {k}: survivors' weights"
        assert_matches_twin(e, t, f'round {k}')
        allocs.append(e.alloc_count())
    assert t.flag.any() and len(set(allocs)) == 1, allocs
    # loss and threshold travelled too: one more robustify from the same linpoints gives the twin's flags
    e.robustify_all_factors(); t.robustify_all_factors()
    assert np.array_equal(e.weights()[1], t.flag) and rel(e.weights()[0], t.w) < TOL
    e.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------

def test_refusals_change_nothing():
    from gbp_amd import _capi
    from gbp_amd.linear import LinearEngine
    g, sched = case('ring65')
    a, b = make_engine(g, sched), make_engine(g, sched)
    a.iterate(3, robustify=True, relinearise=True); b.iterate(3, robustify=True, relinearise=True)
    lib, F = a._lib, a.F
    count = a.alloc_count()
    loss, thr = np.full(F, HUBER, dtype=np.int32), np.full(F, 2.0)
    ip, dp = _capi.iptr, _capi.dptr
    bad_loss, bad_thr, nan_thr = loss.copy(), thr.copy(), thr.copy()
    bad_loss[3], bad_thr[5], nan_thr[0] = 7, 0.0, np.nan
    for args in ((-1, 2, ip(loss), dp(thr)), (0, -1, ip(loss), dp(thr)), (F - 1, 2, ip(loss), dp(thr)), (0, F + 1, ip(loss), dp(thr)),
                 (0, F - 1, None, None), (1, F - 1, None, None), (0, F, ip(loss), None), (0, F, ip(bad_loss), dp(thr)),
                 (0, F, ip(loss), dp(bad_thr)), (0, F, ip(loss), dp(nan_thr))):
        assert lib.gbp_lin_set_robust_nonlinear(a._h, *args) == EINVAL, args[:2]
    assert lib.gbp_lin_set_robust_nonlinear(a._h, 5, 0, None, None) == EINVAL          # NULL is for the whole graph only
    assert lib.gbp_lin_set_robust_nonlinear(a._h, 5, 0, ip(loss), dp(thr)) == 0         # count == 0: nothing changes
    assert lib.gbp_lin_iterate_nonlinear_robust(a._h, -1, None, None) == EINVAL
    assert lib.gbp_lin_iterate_nonlinear_robust(a._h, 0, None, None) == 0
    # the six older calls stay refused on a nonlinear handle with losses, with a message that says why
    uo = _capi.LinUntilOpts(4, 1, 0, 0, 0.0, 0.0)
    ext, shr = _capi.LinExt(), _capi.LinShrink()
    ids = np.zeros(1, dtype=np.int32)
    shr.n_retire_vars, shr.retire_vars, shr.fold = 1, ip(ids), 1
    calls = {'set_robust': lambda: lib.gbp_lin_set_robust(a._h, ip(loss), dp(thr), None), 'robustify': lambda: lib.gbp_lin_robustify(a._h),
             'iterate_robust': lambda: lib.gbp_lin_iterate_robust(a._h, 1), 'iterate_until': lambda: lib.gbp_lin_iterate_until(a._h, ct.byref(uo), None, None),
             'extend': lambda: lib.gbp_lin_extend(a._h, ct.byref(ext)), 'shrink': lambda: lib.gbp_lin_shrink(a._h, ct.byref(shr))}
    for name, call in calls.items():
        assert call() == ESTATE, name
        assert 'nonlinear' in lib.gbp_last_error().decode(), name
    assert a.alloc_count() == count
    a.iterate(1, robustify=True, relinearise=True); b.iterate(1, robustify=True, relinearise=True)
    assert same_bits(state(a), state(b))
    # handles in the wrong state
    lin = LinearEngine(g['va'], g['vb'], np.zeros((F, 6)), np.tile(np.eye(6), (F, 1, 1)), g['prior_eta'], g['prior_lam'])
    assert lib.gbp_lin_set_robust_nonlinear(lin._h, 0, F, ip(loss), dp(thr)) == ESTATE
    assert lib.gbp_lin_robustify_nonlinear(lin._h) == ESTATE and lib.gbp_lin_iterate_nonlinear_robust(lin._h, 1, None, None) == ESTATE
    nol = make_engine(g, sched, losses=False)
    assert lib.gbp_lin_robustify_nonlinear(nol._h) == ESTATE and lib.gbp_lin_iterate_nonlinear_robust(nol._h, 1, None, None) == ESTATE
    for h in (a, b, lin, nol):
        h.close()


def test_repeated_calls_allocate_nothing():
    g, sched = case('ring65')
    e = make_engine(g, sched, losses=False)
    base = e.alloc_count()
    e.set_robust('huber', 2.0)
    assert e.alloc_count() == base + 6                          # loss, threshold, noise variance, weight, flag; the flag counts
    for n in (1, 5, 3, 5):
        e.iterate(n, robustify=True, relinearise=True)          # both counts buffers grow by replacement
        e.set_robust(['constant'] * 4, 3.0, first=60)
        e.robustify_all_factors()
        e.energy()
        assert e.alloc_count() == base + 6
    e.set_robust(None); e.set_robust('constant', 3.0)
    assert e.alloc_count() == base + 6
    e.close()
