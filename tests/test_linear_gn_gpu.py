"""gbp_lin_solve_map_nonlinear on the MI355X (include/gbp_lin.h; kernels in gbp_amd/csrc/gbp_lin_gn.hpp): the nonlinear batch MAP of SE(2)
and SE(3) pose graphs by Levenberg-Marquardt, against the numpy twin of tests/lin_gn_cases.py run with the same options, against the
gradient of Phi formed from the model's Jacobian, and for what the call must leave alone.  fp64 throughout.  Every accept decision of
the compared runs is shown by test_linear_gn_cpu.py to stay >= 1e-7 clear of dPhi = 0."""
import numpy as np
import pytest

from conftest import golden
from lin_gn_cases import CASES, GOLDEN_CASES, GRAD, STALL, X_TOL, gradient, graph_of, huber_closures, solve, twin_of
from lin_nonlin_cases import SCHEDULE

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-9                  # device sums against numpy: the bound of the until-tests
LOSS = {0: None, 1: 'huber', 2: 'constant'}
ALL = list(CASES) + list(GOLDEN_CASES)


def make_engine(model, g, losses=False):
    from gbp_amd.linear import LinearEngine
    make = LinearEngine.se2_pose_graph if model == 1 else LinearEngine.se3_pose_graph
    e = make(g['va'], g['vb'], g['z'], g['s'], g['prior_eta'], g['prior_lam'], SCHEDULE['beta'], SCHEDULE['num_undamped_iters'],
             SCHEDULE['min_linear_iters'], eta_damping=SCHEDULE['eta_damping'])
    if losses and 'loss' in g:
        e.set_robust([LOSS[int(l)] for l in g['loss']], g['thr'])
    return e


def sweep_state(e):
    """Everything the call must leave bit for bit: messages, beliefs, means, linpoint / iters / damping, weights and flags, and the
    handle's eta_f, Lambda_f as the joint reads them."""
    out = list(e.messages()) + list(e.beliefs()) + [e.get_means()] + list(e.linearisation()) + list(e.weights())
    if e.N:
        out += [e.joint_eta(), e.joint_matvec(np.cos(np.arange(e.N * e.D) * 0.37))]
    return out


def same_bits(a, b):
    return len(a) == len(b) and all(np.asarray(x).shape == np.asarray(y).shape and np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def result_bits(r):
    return [np.array([r.outer, r.accepted, r.rejected, r.cg_iters, int(r.converged), r.reason]), np.array([r.energy0, r.energy, r.grad_norm, r.lambda_]),
            r.energy_trace, r.lambdas, r.steps, r.dphi, r.taken]


def close(a, b, tol=SUM_TOL):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))


def assert_matches_twin(r, x, w, what):
    """The device's run `r` with final x against the twin's run `w` of the same options."""
    rows = w['rows']
    print(what, 'outer', r.outer, 'accepted', r.accepted, 'rejected', r.rejected, 'reason', r.reason, 'cg', r.cg_iters)
    if len(rows):
        gaps = [float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)), initial=0.0)) for a, b in
                ((r.energy_trace, rows[:len(r.energy_trace), 0]), (r.dphi, rows[:len(r.dphi), 3]), (r.steps, rows[:len(r.steps), 2]))]
        print(what, 'energy / dPhi / step gaps', gaps, 'x gap', float(np.abs(x - w['x']).max() / max(1.0, np.abs(w['x']).max())))
    assert (r.outer, r.accepted, r.rejected, r.reason, r.converged) == (w['outer'], w['accepted'], w['rejected'], w['reason'], w['converged']), what
    assert np.array_equal(r.taken, rows[:, 4] != 0), what
    assert r.lambdas.tobytes() == rows[:, 1].tobytes() and r.lambda_ == w['lambda_'], f"{what}: lambda is a product of the options"
    assert close(r.energy_trace, rows[:, 0]) and close(r.dphi, rows[:, 3]) and close(r.steps, rows[:, 2]), what
    assert close(r.energy0, w['energy0']) and close(r.energy, w['energy']), what
    # grad_norm is |(eta + lambda D x) - (Lambda + lambda D) x|: every entry is a difference of numbers as large as eta + lambda D x and
    # carries their rounding, a few eps each (the product adds up to ~20 terms per row); 64 eps |eta + lambda D x|_2 bounds the norm of it
    gtol = SUM_TOL * w['grad_norm'] + 64 * np.finfo(float).eps * w['grad_scale']
    print(what, 'grad_norm', r.grad_norm, 'twin', w['grad_norm'], 'bound', gtol)
    assert abs(r.grad_norm - w['grad_norm']) <= gtol, what
    if x.size:
        assert np.abs(x - w['x']).max() <= X_TOL * max(1.0, np.abs(w['x']).max()), what


# ---- against the twin, same options ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ALL)
def test_run_equals_the_twin(name):
    """1 factor, 258 factors on 129 poses, a hub of 70, F = 0, N = 0, G25 / G28, runs with rejections and runs that stall: the
    accept / reject sequence, reason and outer equal, lambda bit-equal, energies and dPhi within 1e-9, the final x within X_TOL; the
    energy comparable with energy() at the start; and the gradient of Phi at the device's x, from the twin's Jacobian, <= tol_grad."""
    model, g, opts = graph_of(name, golden)
    e, t = make_engine(model, g), twin_of(model, g)
    before = sweep_state(e)
    r = e.solve_map_nonlinear(**opts)
    x = e.map_mean()
    assert_matches_twin(r, x, solve(t, t.mu, **opts), name)
    assert same_bits(before, sweep_state(e)), f"{name}: the sweep's state moved"
    if e.N:
        assert close(r.energy0, e.energy())                 # x0 was the means
    if r.reason == GRAD and e.N:
        gn = float(np.linalg.norm(gradient(t, x)))
        print(name, f'|grad| {gn:.3e}')
        assert gn <= opts['tol_grad'] * (1 + 1e-6)
    if name.endswith('stall'):
        assert r.reason == STALL and not r.converged
    if name.endswith('reject'):
        assert r.rejected >= 3


@pytest.mark.parametrize('name', ['se2_F0', 'se3_F0', 'se2_G25', 'se3_G28'])
def test_init_from_a_previous_solve(name):
    """x0 = the iterate of solve_map(): with max_iters = 0 that is x = 0; a graph without factors then reaches the priors' own solution in
    one accepted step.  And x0 = the result of an earlier call goes on from it."""
    model, g, opts = graph_of(name, golden)
    e, t = make_engine(model, g), twin_of(model, g)
    _, info = e.solve_map(max_iters=0)
    assert not info['converged'] and not e.map_mean().any()
    r = e.solve_map_nonlinear(init='map', **opts)
    w = solve(t, np.zeros_like(t.mu), **opts)
    if name.endswith('F0'):
        assert_matches_twin(r, e.map_mean(), w, name)
        assert (r.outer, r.accepted, r.reason) == (1, 1, GRAD) and r.lambdas.tolist() == [0.0]
        assert np.abs(e.map_mean() - t.mu).max() <= 1e-12 * max(1.0, np.abs(t.mu).max())
    else:                                                    # from 0 the poses are far off and the run is long: the start and the first step are the twin's
        assert r.outer >= 1 and r.energy <= r.energy0
        row = np.array([r.energy_trace[0], r.lambdas[0], r.steps[0], r.dphi[0], float(r.taken[0])])
        print(name, 'first row', row, 'twin', w['rows'][0])
        assert close(r.energy0, w['energy0']) and close(row, w['rows'][0]) and r.lambdas[0] == w['rows'][0, 1]
        assert abs(w['rows'][0, 3]) >= 1e-7                  # that decision is clear of dPhi = 0
    x1 = e.map_mean()
    r2 = e.solve_map_nonlinear(init='map', **opts)           # goes on from x1
    assert close(r2.energy0, r.energy) and r2.energy <= r2.energy0 * (1 + 1e-12)
    if r2.outer == 0:
        assert e.map_mean().tobytes() == x1.tobytes()


# ---- independent optimality, plain and with Huber weights ---------------------------------------------------------------------------------

@pytest.mark.parametrize('name,first', [('se2_G25', 29), ('se3_G28', 29)])
def test_optimum_with_huber_weights_left_by_robust_sweeps(name, first):
    """tol_grad = 1e-4.  The decrease test has a floor: E ~ 130 here is known to eps E ~ 3e-14, and a step from a point with gradient g
    lowers Phi by about g^2 / (2 curvature), curvatures being s^2 = 100 .. 400: below g ~ sqrt(2 * 3e-14 * 400) ~ 5e-6 dPhi drowns in the
    rounding of E and steps are rejected until the call stalls.  1e-4 is 20 x that floor."""
    model, g, _ = graph_of(name, golden)
    g = huber_closures(g, first)
    z = g['z'].copy()
    z[first::2, :2] += 1.5                                   # every other closure is an outlier
    g = dict(g, z=z)
    e, t = make_engine(model, g, losses=True), twin_of(model, g, losses=True)
    e.iterate(6, robustify=True, relinearise=True)
    t.iterate(6, relinearise=True, robustify=True)
    w, flag = e.weights()
    assert flag.any() and np.array_equal(flag, t.flag) and w.min() < 1.0
    t.w = w                                                  # the gradient at the device's own weights
    before = sweep_state(e)
    tol = 1e-4
    r = e.solve_map_nonlinear(tol_grad=tol, tol_step=0.0)
    x = e.map_mean()
    gn = float(np.linalg.norm(gradient(t, x)))
    print(name, 'reason', r.reason, 'outer', r.outer, f'|grad| {gn:.3e} (device {r.grad_norm:.3e}) energy {r.energy0:.6g} -> {r.energy:.6g}')
    assert r.reason == GRAD and r.converged and gn <= tol * (1 + 1e-6)
    assert close(r.energy0, e.energy()) and same_bits(before, sweep_state(e))
    assert np.array_equal(e.weights()[0], w)                 # the weights are fixed during the call


# ---- the sweep and the linear solver are untouched -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['se2_G25', 'se3_G28'])
def test_sweeps_and_solve_map_go_on_as_on_a_handle_that_never_solved(name):
    model, g, opts = graph_of(name, golden)
    a, b = make_engine(model, g), make_engine(model, g)
    ca, cb = a.iterate(5, relinearise=True), b.iterate(5, relinearise=True)
    assert np.array_equal(ca, cb)
    ra = a.solve_map_nonlinear(**opts)
    assert ra.accepted >= 1
    xa = a.map_mean()
    # the trace against the nonlinear MAP: the column is |means - x| formed from downloads
    u = a.iterate_until_nonlinear(4, map_distance=True, energy=True)
    v = b.iterate_until_nonlinear(4, energy=True)
    assert np.array_equal(u.relin_counts, v.relin_counts) and u.step.tobytes() == v.step.tobytes() and u.energy.tobytes() == v.energy.tobytes()
    want = np.linalg.norm(a.get_means() - xa.reshape(-1))
    assert abs(u.map_distance[-1] - want) <= 1e-9 * max(1.0, want) and abs(a.map_distance() - want) <= 1e-9 * max(1.0, want)
    ca, cb = a.iterate(3, relinearise=True), b.iterate(3, relinearise=True)
    assert np.array_equal(ca, cb) and same_bits(sweep_state(a), sweep_state(b))
    # the linear solver: one Gauss-Newton step at the sweeps' linearisation, bit-equal to the twin handle's
    ma, ia = a.solve_map()
    mb, ib = b.solve_map()
    assert ma.tobytes() == mb.tobytes() and ia == ib
    sa, _ = a.marginals(ids=[0, a.N - 1])
    sb, _ = b.marginals(ids=[0, b.N - 1])
    assert sa.tobytes() == sb.tobytes()


# ---- allocations and the live handle ----------------------------------------------------------------------------------------------------

def test_repeated_calls_allocate_nothing_and_a_new_generation_starts_over():
    from gbp_amd._capi import GbpError
    GBP_ESTATE = -5                                          # include/gbp_ba.h
    for name, grow in (('se2_G25', 'extend_se2'), ('se3_G28', 'extend_se3')):
        model, g, opts = graph_of(name, golden)
        e = make_engine(model, g)
        r0 = e.solve_map_nonlinear(**opts)
        n = e.alloc_count()
        for _ in range(3):
            r = e.solve_map_nonlinear(**opts)
            assert same_bits(result_bits(r), result_bits(r0))
        assert e.alloc_count() == n
        D, N = e.D, e.N
        mean = e.get_means().reshape(N, D)[-1] + 0.1
        lam = np.eye(D)
        z = np.zeros(D)
        z[0] = 0.5
        getattr(e, grow)([N - 1], [N], z[None], g['s'][:1], prior_eta=(lam @ mean)[None], prior_lam=lam[None])
        with pytest.raises(GbpError) as err:
            e.map_mean()
        assert err.value.code == GBP_ESTATE
        r = e.solve_map_nonlinear(**opts)
        assert e.map_mean().shape == (N + 1, D) and r.energy <= r.energy0 and e.alloc_count() == n
        e.retire([0, 1])
        with pytest.raises(GbpError) as err:
            e.map_mean()
        assert err.value.code == GBP_ESTATE
        before, n1 = sweep_state(e), e.alloc_count()
        with pytest.raises(GbpError) as err:
            e.solve_map_nonlinear(init='map', **opts)
        assert err.value.code == GBP_ESTATE and same_bits(before, sweep_state(e))
        r = e.solve_map_nonlinear(**opts)
        assert e.map_mean().shape == (N - 1, D) and r.energy <= r.energy0 and e.alloc_count() == n


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_bit_identical():
    from gbp_amd._capi import GbpError
    GBP_EINVAL, GBP_ESTATE = -1, -5                          # include/gbp_ba.h
    from gbp_amd.linear import LinearEngine
    model, g, opts = graph_of('se2_G25', golden)
    e = make_engine(model, g)
    e.iterate(3, relinearise=True)
    e.solve_map()
    before, x, n = sweep_state(e), e.map_mean(), e.alloc_count()
    bad = [dict(max_outer=-1), dict(init='map', lambda0=0.0), dict(lambda0=float('nan')), dict(lambda_up=1.0), dict(lambda_down=1.0), dict(lambda_down=0.0),
           dict(lambda_min=1.0, lambda0=0.5), dict(lambda_max=1e-6, lambda0=1e-4), dict(lambda_max=float('inf')), dict(tol_step=-1.0), dict(tol_grad=float('inf')),
           dict(tol_step=float('nan')), dict(rel_tol=0.0), dict(max_iters=-1), dict(check_every=0)]
    for kw in bad:
        with pytest.raises(GbpError) as err:
            e.solve_map_nonlinear(**kw)
        assert err.value.code == GBP_EINVAL, kw
        assert same_bits(before, sweep_state(e)) and e.map_mean().tobytes() == x.tobytes() and e.alloc_count() == n, kw
    lib, ct = e._lib, __import__('ctypes')
    from gbp_amd import _capi
    o = _capi.LinNlmapOpts(5, 2, 1e-4, 10.0, 0.1, 1e-12, 1e8, 0.0, 0.0, _capi.LinMapOpts(1e-12, 100, 8, 0))
    assert lib.gbp_lin_solve_map_nonlinear(e._h, ct.byref(o), None, None) == GBP_EINVAL          # unknown init
    o.init, o.cg.warm_start = 0, 1
    assert lib.gbp_lin_solve_map_nonlinear(e._h, ct.byref(o), None, None) == GBP_EINVAL          # the inner solves start at x
    assert same_bits(before, sweep_state(e)) and e.map_mean().tobytes() == x.tobytes()
    # GBP_ESTATE: not nonlinear; from the MAP without a solve.  (The third refusal of the header, init from the means without beliefs,
    # cannot be reached through the library: gbp_lin_set_nonlinear runs the belief stage, and no call takes beliefs away.)
    lin = LinearEngine(g['va'], g['vb'], np.zeros((e.F, 6)), np.tile(np.eye(6), (e.F, 1, 1)), g['prior_eta'], g['prior_lam'])
    lin.update_all_beliefs()
    lin.iterate(2)
    lin_state = lambda: list(lin.messages()) + list(lin.beliefs()) + [lin.get_means(), np.array(lin.alloc_count())]
    was = lin_state()
    with pytest.raises(GbpError) as err:
        lin.solve_map_nonlinear()
    assert err.value.code == GBP_ESTATE and same_bits(was, lin_state())
    fresh = make_engine(model, g)
    was, n0 = sweep_state(fresh), fresh.alloc_count()        # (sweep_state's joint products have made the linear solver's workspace)
    with pytest.raises(GbpError) as err:
        fresh.solve_map_nonlinear(init='map')
    assert err.value.code == GBP_ESTATE and same_bits(was, sweep_state(fresh)) and fresh.alloc_count() == n0
    with pytest.raises(GbpError) as err:
        fresh.map_mean()
    assert err.value.code == GBP_ESTATE
    # NULL opts are the documented defaults; max_outer == 0 leaves x = x0 with both energies filled
    i = _capi.LinNlmapInfo()
    assert lib.gbp_lin_solve_map_nonlinear(fresh._h, None, None, ct.byref(i)) == 0 and i.converged == 1
    z = make_engine(model, g)
    r = z.solve_map_nonlinear(max_outer=0)
    assert (r.outer, r.converged, r.reason) == (0, False, 0) and r.energy0 == r.energy and close(r.energy, z.energy())
    assert z.map_mean().reshape(-1).tobytes() == z.get_means().tobytes()


# ---- determinism ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['se2_reject', 'se3_reject', 'se3_ring258'])
def test_two_handles_are_bit_identical(name):
    model, g, opts = graph_of(name, golden)
    out = []
    for _ in range(2):
        e = make_engine(model, g)
        e.iterate(2, relinearise=True)
        r = e.solve_map_nonlinear(**opts)
        r2 = e.solve_map_nonlinear(init='map', **dict(opts, tol_grad=opts['tol_grad'] * 0.1))
        out.append(result_bits(r) + result_bits(r2) + [e.map_mean()] + sweep_state(e))
    assert same_bits(out[0], out[1])
