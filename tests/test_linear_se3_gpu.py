"""The SE(3) relative-pose factor of the linear engine on the MI355X (include/gbp_lin.h, GBP_LIN_MODEL_SE3_BETWEEN; kernels and model
in gbp_amd/csrc/gbp_lin_nonlin.hpp): against the reference's own run (fixture G28) with masks and flags compared exactly, against the
numpy twin of tests/lin_se3_cases.py on the shapes where a kernel can go wrong, determinism, the live handle, sweeps to convergence,
and the refusals.  fp64 throughout.  Every seeded case here is shown by test_linear_se3_cpu.py to stay >= 1e-9 clear of the thresholds."""
import numpy as np
import pytest

from conftest import golden
from lin_map_cases import rel
from lin_se3_cases import (CASES, PARITY, SCHEDULE, SQRT_INFO, SWEEPS, TOL, case, dense_joint, g28_graph, g28_schedule, live_case, robust_case,
                           twin_of)

pytestmark = pytest.mark.gpu

LOSS = {0: None, 1: 'huber', 2: 'constant'}


def make_engine(g, sched, losses=True):
    from gbp_amd.linear import LinearEngine
    e = LinearEngine.se3_pose_graph(g['va'], g['vb'], g['z'], g['s'], g['prior_eta'], g['prior_lam'], sched['beta'],
                                    sched['num_undamped_iters'], sched['min_linear_iters'], eta_damping=sched['eta_damping'])
    if losses and 'loss' in g:
        e.set_robust([LOSS[int(l)] for l in g['loss']], g['thr'])
    return e


def state(e):
    """Everything a sweep writes, for bit-for-bit comparisons."""
    out = list(e.messages()) + list(e.beliefs()) + [e.get_means()] + list(e.linearisation())
    return out + [e.joint_eta(), e.joint_matvec(np.cos(np.arange(e.N * e.D) * 0.37))]       # eta_f, Lambda_f as the solvers read them


def same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def assert_matches_twin(e, t, what, tol=TOL):
    lp, it, dm = e.linearisation()
    assert lp.shape == (e.F, 12)
    assert np.array_equal(it, t.iters), f"{what}: iters differ at {np.nonzero(it != t.iters)[0][:5]}"
    assert np.array_equal(dm, t.fdamp), f"{what}: damping differs at {np.nonzero(dm != t.fdamp)[0][:5]}"
    assert rel(lp, t.linpoint) < tol, f"{what}: linpoint {rel(lp, t.linpoint):.3e}"
    for name, a, b in zip(('eta_a', 'lam_a', 'eta_b', 'lam_b'), e.messages(), t.messages()):
        assert rel(a, b) < tol, f"{what}: message {name} {rel(a, b):.3e}"
    for name, a, b in zip(('eta', 'lam'), e.beliefs(), t.beliefs()):
        assert rel(a, b) < tol, f"{what}: belief {name} {rel(a, b):.3e}"
    assert rel(e.get_means(), t.get_means()) < tol, f"{what}: means {rel(e.get_means(), t.get_means()):.3e}"
    je, jl = t.joint()                                       # eta_f, Lambda_f (times the weights) through the joint
    x = np.cos(np.arange(je.size) * 0.37)
    assert rel(e.joint_eta().reshape(-1), je) < tol and rel(e.joint_matvec(x).reshape(-1), jl @ x) < tol, f"{what}: factors"
    ee, et = e.energy(), t.energy()
    assert abs(ee - et) <= tol * max(abs(et), 1.0), f"{what}: energy {ee!r} vs {et!r}"
    if t.robust:
        w, flag = e.weights()
        assert np.array_equal(flag, t.flag) and rel(w, t.w) < tol, f"{what}: weights"


# ---- the reference's own run --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', ['main', 'b0', 'robust'])
def test_reference_run_sweep_by_sweep(tag):
    """G28 one sweep per call: masks, counts, iters, per-factor damping and robust flags exactly; means, energy, linpoints, messages,
    beliefs and factors within PARITY of the reference; everything within TOL of the twin at the stored sweeps; at the end of `main`
    solve_map and marginals against joint_distribution_cov."""
    g = golden('G28_se3_posegraph')
    sched, sweeps = g28_schedule(g, tag)
    graph = g28_graph(g, tag)
    robust = tag == 'robust'
    e, t = make_engine(graph, sched), twin_of(graph, sched)
    assert_matches_twin(e, t, f'{tag} after set_nonlinear')
    worst = {}

    def gap(name, a, b):
        worst[name] = max(worst.get(name, 0.0), rel(a, b))
        assert rel(a, b) < PARITY, f"{name}: {rel(a, b):.3e}"

    for s in range(sweeps):
        out = e.iterate(1, robustify=robust, relinearise=True)
        t.synchronous_iteration(True, robust)
        counts = out[0] if robust else out
        lp, it, dm = e.linearisation()
        want = g[f'{tag}_mask'][s].astype(bool)
        assert np.array_equal(it == 0, want), f"sweep {s}: mask differs at {np.nonzero((it == 0) != want)[0][:5]}"
        assert counts.tolist() == [int(want.sum())], f"sweep {s}: count {counts} vs {want.sum()}"
        assert np.array_equal(it, g[f'{tag}_iters'][s]) and np.array_equal(dm, g[f'{tag}_damp'][s]), f"sweep {s}: iters / damping"
        w = np.ones(e.F)
        if robust:
            w, flag = e.weights()
            assert np.array_equal(flag, g['robust_flag'][s].astype(bool)) and out[1].tolist() == [int(g['robust_flag'][s].sum())], f"sweep {s}: flags"
            gap('weights', w, g['robust_w'][s])
        gap('means', e.get_means(), g[f'{tag}_means'][s])
        gap('energy', e.energy(), g[f'{tag}_energy'][s])
        k = f'{tag}_s{s + 1}_'
        if k + 'linpoint' in g:
            gap('linpoint', lp, g[k + 'linpoint'])
            for name, a in zip(('msg_eta_a', 'msg_lam_a', 'msg_eta_b', 'msg_lam_b'), e.messages()):
                gap('messages', a, g[k + name])
            eta, lam = e.beliefs()
            gap('beliefs', eta, g[k + 'bel_eta']); gap('beliefs', lam, g[k + 'bel_lam'])
            je, jl = dense_joint(graph, g[k + 'feta'], g[k + 'flam'])          # the fixture's factors carry the weight, as the joint does
            x = np.cos(np.arange(je.size) * 0.37)
            gap('factors', e.joint_eta().reshape(-1), je); gap('factors', e.joint_matvec(x).reshape(-1), jl @ x)
            assert_matches_twin(e, t, f'{tag} sweep {s + 1}')
    if tag == 'main':
        mu, info = e.solve_map()
        assert info['converged']
        gap('map', mu, g['main_map_mu'])
        sigma, minfo = e.marginals()
        assert minfo['converged']
        gap('marginals', sigma, g['main_map_sigma_diag'])
    print(tag, 'worst gaps against the reference', {k: f'{v:.2e}' for k, v in worst.items()})
    e.close()


# ---- against the twin ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_cases_match_the_twin(name):
    """2 poses and 1 factor; a ring of 129 poses with 258 factors (past a 64-lane wave of the factor stage and a 256-lane block of the
    relinearise stage, a ragged tail in both); a hub with 70 factors; rotations exactly zero and of 1e-7; the helix past pi; beta = +inf,
    beta = 0, num_undamped_iters 0 and 1.  After set_nonlinear and after SWEEPS sweeps in one call: counts and the state against the twin;
    SWEEPS calls of one sweep end bit for bit where the one call did."""
    g, sched = case(name)
    e, e1, t = make_engine(g, sched), make_engine(g, sched), twin_of(g, sched)
    assert_matches_twin(e, t, f'{name} after set_nonlinear')
    counts = e.iterate(SWEEPS, relinearise=True)
    want = t.iterate(SWEEPS, relinearise=True)
    assert np.array_equal(counts, want), f"counts {counts} vs {want}"
    assert_matches_twin(e, t, name)
    if name == 'beta_inf':
        assert not counts.any()
    if name == 'beta0':
        assert counts.tolist() == [0] + [e.F] * (SWEEPS - 1)
    single = [int(e1.iterate(1, relinearise=True)[0]) for _ in range(SWEEPS)]
    assert single == counts.tolist()
    assert same_bits(state(e), state(e1)), "n sweeps in one call differ from n calls of one sweep"
    e.close(); e1.close()


def test_robust_sweeps_match_the_twin():
    g, sched = robust_case()
    e, t = make_engine(g, sched), twin_of(g, sched)
    rc, fc = e.iterate(SWEEPS, robustify=True, relinearise=True)
    wr, wf = t.iterate(SWEEPS, relinearise=True, robustify=True)
    assert np.array_equal(rc, wr) and np.array_equal(fc, wf) and fc.max() > 0
    assert_matches_twin(e, t, 'robust')
    e.robustify_all_factors(); t.robustify_all_factors()
    assert_matches_twin(e, t, 'robustify alone')
    n = e.relinearise()
    assert n == int(t.relinearise_factors().sum())
    assert_matches_twin(e, t, 'relinearise alone')
    e.close()


def test_two_handles_are_bit_identical():
    g, sched = robust_case()
    out = []
    for _ in range(2):
        e = make_engine(g, sched)
        c = [e.iterate(3, relinearise=True), *e.iterate(4, robustify=True, relinearise=True), np.array([e.relinearise()])]
        e.iterate(2)
        out.append((state(e) + list(e.weights()) + c, e))
    assert same_bits(out[0][0], out[1][0])
    out[0][1].close(); out[1][1].close()


# ---- the live handle -------------------------------------------------------------------------------------------------------------------

def _head(g, N0, F0):
    assert max(g['va'][:F0].max(), g['vb'][:F0].max()) < N0
    return dict(N=N0, va=g['va'][:F0], vb=g['vb'][:F0], z=g['z'][:F0], s=g['s'][:F0], prior_eta=g['prior_eta'][:N0], prior_lam=g['prior_lam'][:N0])


def _tail(g, N0, F0):
    return dict(va=g['va'][F0:], vb=g['vb'][F0:], z=g['z'][F0:], s=g['s'][F0:], prior_eta=g['prior_eta'][N0:], prior_lam=g['prior_lam'][N0:])


def _extend(e, k):
    e.extend_se3(k['va'], k['vb'], k['z'], k['s'], k['prior_eta'] if len(k['prior_eta']) else None, k['prior_lam'] if len(k['prior_eta']) else None)


def test_grown_before_any_sweep_is_the_handle_created_whole():
    g, sched = case('helix')                                 # 24 poses, 23 odometry factors, then the closures
    whole, part = make_engine(g, sched), make_engine(_head(g, 16, 15), sched)
    _extend(part, _tail(g, 16, 15))
    assert (part.N, part.F) == (whole.N, whole.F) == part.sizes()
    assert same_bits(state(whole), state(part))
    a, b = whole.iterate(4, relinearise=True), part.iterate(4, relinearise=True)
    assert np.array_equal(a, b) and same_bits(state(whole), state(part))
    whole.close(); part.close()


def test_old_factors_keep_their_state_through_extend_and_shrink():
    """After sweeps: through extend_se3, retire (with a fold, against the twin) and cull every old or surviving factor keeps messages,
    linpoint, iters, damping, loss and weight bit for bit."""
    h, k, sched = live_case()
    N0, F0 = h['N'], len(h['va'])
    e, t = make_engine(h, sched), twin_of(h, sched)
    e.iterate(5, robustify=True, relinearise=True); t.iterate(5, relinearise=True, robustify=True)

    def per_factor(e):
        return list(e.messages()) + list(e.linearisation()) + list(e.weights())

    before = per_factor(e)
    _extend(e, k); t.extend(k['va'], k['vb'], k['z'], k['s'], k['prior_eta'], k['prior_lam'])
    assert same_bits(before, [a[:F0] for a in per_factor(e)])
    assert_matches_twin(e, t, 'after extend_se3')
    e.iterate(3, robustify=True, relinearise=True); t.iterate(3, relinearise=True, robustify=True)
    assert_matches_twin(e, t, 'sweeps after extend_se3')
    before = per_factor(e)
    vmap, fmap = e.retire([0, 1])
    tv, tf = t.shrink(retire=[0, 1])
    assert np.array_equal(vmap, tv) and np.array_equal(fmap, tf) and (fmap < 0).sum() >= 2
    assert same_bits([a[fmap >= 0] for a in before], per_factor(e))
    assert_matches_twin(e, t, 'after a folded retire')
    before = per_factor(e)
    _, fmap = e.cull([e.F - 1])
    t.shrink(drop=[t.F - 1])
    assert same_bits([a[fmap >= 0] for a in before], per_factor(e))
    assert_matches_twin(e, t, 'after cull')
    e.iterate(2, robustify=True, relinearise=True); t.iterate(2, relinearise=True, robustify=True)
    assert_matches_twin(e, t, 'sweeps after shrink')
    e.close()


def test_alloc_count_does_not_grow():
    g, sched = case('helix')
    e = make_engine(g, sched)
    rs = np.random.RandomState(3)
    counts = []
    for i in range(20):
        mu = e.get_means().reshape(-1, 6)[-1]
        lam = np.diag(1.0 / np.array([1.0, 1.0, 1.0, 0.5, 0.5, 0.5]) ** 2)
        z = np.concatenate([rs.normal(0, 0.3, 3), rs.normal(0, 0.05, 3)])
        e.extend_se3([e.N - 1], [e.N], z[None], SQRT_INFO[None], (lam @ (mu + z))[None], lam[None])
        e.retire([0])
        e.iterate(1, relinearise=True)
        counts.append(e.alloc_count())
    assert len(set(counts)) == 1, counts
    assert (e.N, e.F) == e.sizes() and e.N == 24
    e.close()


# ---- sweeps to convergence -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('check_every', [1, 3, 8])
def test_iterate_until_is_iterate(check_every):
    g, sched = case('helix')
    a, b, t = make_engine(g, sched), make_engine(g, sched), twin_of(g, sched)
    for e in (a, b):
        e.solve_map()
    r = a.iterate_until_nonlinear(30, tol_step=0.02, energy=True, map_distance=True, check_every=check_every)
    assert r.converged and r.iters == 15                     # the twin's steps: 1.85e-2 after sweep 15, above 3e-2 before
    counts = b.iterate(r.iters, relinearise=True)
    assert np.array_equal(r.relin_counts, counts) and same_bits(state(a), state(b))
    eta, lam = t.joint()
    x = np.linalg.solve(lam, eta)
    for i in range(r.iters):
        old = t.get_means().copy()
        t.synchronous_iteration()
        assert abs(r.step[i] - np.abs(t.get_means() - old).max()) <= TOL * max(1.0, r.step[i])
        assert abs(r.energy[i] - t.energy()) <= TOL * max(1.0, t.energy())
        d = np.linalg.norm(t.get_means() - x)
        assert abs(r.map_distance[i] - d) <= 1e-7 * max(1.0, d)      # the device's MAP iterate is a CG solve at rel_tol 1e-12, cond ~ 1e6
    a.close(); b.close()


def test_settled_does_not_stop_on_a_sweep_that_relinearised():
    g, sched = case('helix')
    plain, settled = make_engine(g, sched), make_engine(g, sched)
    tol = 0.02                                               # first met by sweep 15, in which two factors relinearise; sweep 16: none
    r0 = plain.iterate_until_nonlinear(30, tol_step=tol, check_every=3)
    r1 = settled.iterate_until_nonlinear(30, tol_step=tol, settled=True, check_every=3)
    assert r0.converged and r1.converged and r0.iters == 15 and r1.iters == 16
    assert r0.relin_counts[14] > 0 and r1.step[14] <= tol and r1.relin_counts[14] > 0 and r1.relin_counts[15] == 0
    plain.close(); settled.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def _refused(fn, code):
    from gbp_amd._capi import GbpError
    with pytest.raises(GbpError) as ei:
        fn()
    assert ei.value.code == code, ei.value


def test_refusals_leave_the_handle_as_it_was():
    from gbp_amd import _capi
    from gbp_amd.linear import LinearEngine
    EINVAL, ESTATE = -1, -5
    g, sched = case('helix')
    F = len(g['va'])
    args = (sched['beta'], sched['num_undamped_iters'], sched['min_linear_iters'])

    def fresh(D):
        return LinearEngine(g['va'], g['vb'], np.zeros((F, 2 * D)), np.zeros((F, 2 * D, 2 * D)), np.zeros((g['N'], D)), np.tile(np.eye(D), (g['N'], 1, 1)))

    e3, e6 = fresh(3), fresh(6)
    for e in (e3, e6):
        e.update_all_beliefs()
    def linear_state(e):                                     # of a handle that is not nonlinear: no linearisation to read
        return list(e.messages()) + list(e.beliefs()) + [e.get_means(), e.joint_eta()]

    s3, s6 = linear_state(e3), linear_state(e6)
    _refused(lambda: e3.set_nonlinear(np.zeros((F, 6)), np.ones((F, 6)), *args, model=_capi.LIN_MODEL_SE3_BETWEEN), EINVAL)     # model 2 on dofs 3
    _refused(lambda: e6.set_nonlinear(np.zeros((F, 3)), np.ones((F, 3)), *args, model=_capi.LIN_MODEL_SE2_BETWEEN), EINVAL)     # model 1 on dofs 6
    _refused(lambda: e6.set_nonlinear(np.zeros((F, 6)), np.ones((F, 6)), *args, model=7), EINVAL)                               # unknown
    bad = g['z'].copy(); bad[3, 4] = np.inf
    _refused(lambda: e6.set_nonlinear(bad, g['s'], *args, model=2), EINVAL)
    bad = g['z'].copy(); bad[5, 1] = np.nan
    _refused(lambda: e6.set_nonlinear(bad, g['s'], *args, model=2), EINVAL)
    for v in (0.0, -1.0, np.inf):
        s = g['s'].copy(); s[2, 5] = v
        _refused(lambda: e6.set_nonlinear(g['z'], s, *args, model=2), EINVAL)
    for norm in (np.pi, 3.5):
        bad = g['z'].copy(); bad[7, 3:] = [0.0, norm, 0.0]     # along one axis: the norm is exactly `norm`
        _refused(lambda: e6.set_nonlinear(bad, g['s'], *args, model=2), EINVAL)
    assert same_bits(s3, linear_state(e3)) and same_bits(s6, linear_state(e6))
    assert not e3._nonlinear and not e6._nonlinear
    _refused(lambda: e6.linearisation(), ESTATE)
    e3.close(); e6.close()

    e = make_engine(g, sched)
    e.iterate(3, relinearise=True)
    before = state(e)
    lam = np.eye(6)
    ok = dict(va=[e.N - 1], vb=[e.N], prior_eta=np.zeros((1, 6)), prior_lam=lam[None])
    z = np.zeros((1, 6)); z[0, 3:] = np.pi * np.array([1.0, 0.0, 0.0])
    _refused(lambda: e.extend_se3(ok['va'], ok['vb'], z, SQRT_INFO[None], ok['prior_eta'], ok['prior_lam']), EINVAL)            # |z_w| >= pi
    z = np.zeros((1, 6)); z[0, 0] = np.nan
    _refused(lambda: e.extend_se3(ok['va'], ok['vb'], z, SQRT_INFO[None], ok['prior_eta'], ok['prior_lam']), EINVAL)
    _refused(lambda: e.extend_se3(ok['va'], ok['vb'], np.zeros((1, 6)), -SQRT_INFO[None], ok['prior_eta'], ok['prior_lam']), EINVAL)
    with pytest.raises(ValueError):
        e.extend_se2(ok['va'], ok['vb'], np.zeros((1, 3)), np.ones((1, 3)), np.zeros((1, 3)), np.eye(3)[None])
    # the linear-only calls, as on SE(2)
    _refused(lambda: e.set_nonlinear(g['z'], g['s'], *args, model=2), ESTATE)
    _refused(lambda: e.extend(ok['va'], ok['vb'], np.zeros((1, 12)), np.zeros((1, 12, 12)), ok['prior_eta'], ok['prior_lam']), ESTATE)
    _refused(lambda: e.iterate(1, robustify=True), ESTATE)
    _refused(lambda: e.iterate_until(5, tol_step=1e-3), ESTATE)
    _refused(lambda: e.iterate(1, robustify=True, relinearise=True), ESTATE)            # no losses set
    assert same_bits(before, state(e)) and (e.N, e.F) == e.sizes()
    e.close()

    g2 = __import__('lin_nonlin_cases').chain(6)
    e2 = LinearEngine.se2_pose_graph(g2['va'], g2['vb'], g2['z'], g2['s'], g2['prior_eta'], g2['prior_lam'], *args)
    before = list(e2.messages()) + list(e2.beliefs()) + list(e2.linearisation())
    with pytest.raises(ValueError):
        e2.extend_se3([5], [6], np.zeros((1, 6)), SQRT_INFO[None], np.zeros((1, 6)), np.eye(6)[None])
    assert same_bits(before, list(e2.messages()) + list(e2.beliefs()) + list(e2.linearisation())) and e2.sizes() == (6, 5)
    e2.close()
