"""gbp_lin_solve_map_nonlinear_robust on the MI355X (include/gbp_lin.h; kernels in gbp_amd/csrc/gbp_lin_gn.hpp): the robust nonlinear
batch MAP of SE(2) and SE(3) chain / ring graphs by reweighted Levenberg-Marquardt, against the numpy twin of tests/lin_irls_cases.py
run with the same options, and for what the call must leave alone.  fp64 throughout.  test_linear_irls_cpu.py shows every M_f of the
compared runs to stay >= 1e-7 clear of its threshold at every reweight and every accept decision >= 1e-7 clear of dPhi = 0."""
import ctypes as ct

import numpy as np
import pytest

from lin_gn_cases import twin_of
from lin_irls_cases import CASES, IRLS_NONE, IRLS_WEIGHTS, X_TOL, graph_of, split, twin_run
from lin_nonlin_cases import SCHEDULE

pytestmark = pytest.mark.gpu

SUM_TOL = 1e-9                  # device sums against numpy: the bound of the energy column of test_linear_gn_gpu.py
LOSS = {0: None, 1: 'huber', 2: 'constant'}


def make_engine(model, g, losses=True):
    from gbp_amd.linear import LinearEngine
    make = LinearEngine.se2_pose_graph if model == 1 else LinearEngine.se3_pose_graph
    e = make(g['va'], g['vb'], g['z'], g['s'], g['prior_eta'], g['prior_lam'], SCHEDULE['beta'], SCHEDULE['num_undamped_iters'],
             SCHEDULE['min_linear_iters'], eta_damping=SCHEDULE['eta_damping'])
    if losses and 'loss' in g and len(g['loss']):
        e.set_robust([LOSS[int(l)] for l in g['loss']], g['thr'])
    return e


def sweep_state(e):
    """Everything the call must leave bit for bit, read through every getter: messages, beliefs, means, linpoint / iters / damping, THE
    HANDLE'S weights and flags (gbp_lin_get_weights), and the handle's eta_f, Lambda_f as the joint reads them."""
    out = list(e.messages()) + list(e.beliefs()) + [e.get_means()] + list(e.linearisation()) + list(e.weights())
    if e.N:
        out += [e.joint_eta(), e.joint_matvec(np.cos(np.arange(e.N * e.D) * 0.37))]
    return out


def same_bits(a, b):
    return len(a) == len(b) and all(np.asarray(x).shape == np.asarray(y).shape and np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def result_bits(r):
    return [np.array([r.rounds, r.outer, r.accepted, r.rejected, r.cg_iters, int(r.converged), r.reason, r.flagged]),
            np.array([r.energy0, r.energy, r.weight_change, r.move, r.grad_norm]), r.round_trace, r.lm_trace, r.weights, r.robust_flag]


def close(a, b, tol=SUM_TOL):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))))


# ---- against the twin, same options ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(CASES))
def test_run_equals_the_twin(name):
    """F in {0, 1, 63, 64, 65, 255, 256, 257} on chains, rings of 65 and 257, every lossy factor flagged / none / losses on a third,
    rounds with rejections and rounds that stall: rounds, reason and every round's flagged count, LM iterations and LM reason equal;
    flags equal at the end; the energy column within 1e-9; weights within 1e-9; the final x within X_TOL; the sweep's state bit for bit."""
    model, g, opts = graph_of(name)
    e, t = make_engine(model, g), twin_of(model, g, losses=True)
    before = sweep_state(e)
    r = e.solve_map_nonlinear_robust(**opts)
    x = e.map_mean()
    w = twin_run(t, t.mu, opts)
    rows = w['rows']
    if len(rows) == len(r.round_trace):
        print(name, 'energy gap', float(np.max(np.abs(r.round_trace[:, 0] - rows[:, 0]) / np.maximum(1.0, np.abs(rows[:, 0])))),
              'x gap', float(np.abs(x - w['x']).max() / max(1.0, np.abs(w['x']).max(initial=0.0))) if x.size else 0.0,
              'weight gap', float(np.abs(r.weights - w['weights']).max(initial=0.0)))
    print(name, 'rounds', r.rounds, 'outer', r.outer, 'rejected', r.rejected, 'reason', r.reason, 'flagged', r.round_trace[:, 1].astype(int).tolist(), 'cg', r.cg_iters)
    assert (r.rounds, r.outer, r.accepted, r.rejected, r.reason, r.converged, r.flagged) == (w['rounds'], w['outer'], w['accepted'], w['rejected'], w['reason'],
                                                                                             w['converged'], w['flagged']), name
    assert r.round_trace.shape == rows.shape and np.array_equal(r.round_trace[:, [1, 4, 5]], rows[:, [1, 4, 5]]), name   # flagged counts at every round
    assert close(r.round_trace[:, 0], rows[:, 0]), name                                    # the energy column
    assert close(r.round_trace[:, 2], rows[:, 2]) and close(r.round_trace[:, 3], rows[:, 3], X_TOL), name
    assert r.round_trace[0, 2] == 0.0 and r.round_trace[0, 3] == 0.0
    assert np.array_equal(r.robust_flag, w['flag']) and close(r.weights, w['weights']), name
    assert r.lm_trace.shape == w['lm_rows'].shape and np.array_equal(r.lm_trace[:, 4], w['lm_rows'][:, 4]) and close(r.lm_trace[:, 0], w['lm_rows'][:, 0]), name
    assert (r.energy0, r.energy) == (r.round_trace[0, 0], r.round_trace[-1, 0])
    if x.size:
        assert np.abs(x - w['x']).max() <= X_TOL * max(1.0, np.abs(w['x']).max()), name
    assert same_bits(before, sweep_state(e)), f"{name}: the sweep's state moved"
    if e.N and e.F:                                          # the handle's own weights are not the solver's: no sweep has made any yet
        assert np.all(e.weights()[0] == 1.0) and not e.weights()[1].any()
    if name.endswith('_stall'):
        assert r.round_trace[0, 5] == 3                      # GBP_LIN_NLMAP_STALL, and the loop went on
    if name.endswith('_chain0'):
        assert (r.rounds, r.outer, r.reason, r.converged) == (1, 0, IRLS_WEIGHTS, True)   # the prior means ARE the optimum: the gradient test ends the round
        e.solve_map(max_iters=0)                             # x = 0: one round of one exact step, then WEIGHTS
        r = e.solve_map_nonlinear_robust(init='map', **opts)
        assert (r.rounds, r.outer, r.accepted, r.reason, r.converged) == (1, 1, 1, IRLS_WEIGHTS, True) and r.lm_trace[0, 1] == 0.0
        assert np.abs(e.map_mean() - t.mu).max() <= 1e-12 * max(1.0, np.abs(t.mu).max())


def test_no_variables():
    from lin_gn_cases import _empty
    for model, D in ((1, 3), (2, 6)):
        e = make_engine(model, _empty(D))
        r = e.solve_map_nonlinear_robust()
        assert (r.rounds, r.outer, r.reason, r.converged, r.flagged) == (0, 0, IRLS_WEIGHTS, True, 0) and r.round_trace.shape == (1, 6) and not r.round_trace.any()
        assert e.map_mean().shape == (0, D)


# ---- without losses the call is solve_map_nonlinear -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['se2_ring65', 'se3_ring65', 'se2_chain257', 'se3_chain256'])
def test_without_flagged_factors_x_is_bit_equal_to_solve_map_nonlinear(name):
    """No losses set, and losses whose thresholds no factor reaches: every weight is 1, round 1's reweight finds weight_change == 0,
    the call ends after one round with reason WEIGHTS and its x, energy and LM trace are those of solve_map_nonlinear bit for bit."""
    model, g, opts = graph_of(name)
    rounds, lm = split(opts)
    lm = dict(lm, rel_tol=opts['rel_tol'], max_iters=opts['max_iters'])
    ref = make_engine(model, g, losses=False)
    p = ref.solve_map_nonlinear(**lm)
    xp = ref.map_mean()
    far = dict(g, thr=np.full(len(g['va']), 1e6))
    for graph, losses in ((g, False), (far, True)):
        e = make_engine(model, graph, losses=losses)
        r = e.solve_map_nonlinear_robust(**rounds, **lm)
        assert (r.rounds, r.reason, r.converged, r.flagged, r.weight_change) == (1, IRLS_WEIGHTS, True, 0, 0.0)
        assert e.map_mean().tobytes() == xp.tobytes()
        assert np.all(r.weights == 1.0) and not r.robust_flag.any()
        assert (r.outer, r.accepted, r.rejected, r.cg_iters) == (p.outer, p.accepted, p.rejected, p.cg_iters)
        assert r.lm_trace[:, 0].tobytes() == p.energy_trace.tobytes() and r.lm_trace[:, 3].tobytes() == p.dphi.tobytes() and r.energy0 == p.energy0


# ---- determinism, allocations, the live handle --------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['se2_ring257', 'se3_reject', 'se3_chain65'])
def test_two_handles_are_bit_identical(name):
    model, g, opts = graph_of(name)
    out = []
    for _ in range(2):
        e = make_engine(model, g)
        e.iterate(2, robustify=True, relinearise=True)
        r = e.solve_map_nonlinear_robust(**opts)
        r2 = e.solve_map_nonlinear_robust(init='map', **dict(opts, max_rounds=2))
        out.append(result_bits(r) + result_bits(r2) + [e.map_mean()] + sweep_state(e))
    assert same_bits(out[0], out[1])


def test_repeated_calls_allocate_nothing_and_the_call_follows_extend_and_shrink():
    model, g, opts = graph_of('se2_ring65')
    e = make_engine(model, g)
    e.iterate(3, robustify=True, relinearise=True)
    kept = e.weights()
    r0 = e.solve_map_nonlinear_robust(**opts)
    n = e.alloc_count()
    for _ in range(2):
        r = e.solve_map_nonlinear_robust(**opts)
        assert same_bits(result_bits(r), result_bits(r0))
    assert e.alloc_count() == n and same_bits(list(kept), list(e.weights()))
    # map_distance measures against the new x
    want = np.linalg.norm(e.get_means() - e.map_mean().reshape(-1))
    assert abs(e.map_distance() - want) <= 1e-9 * max(1.0, want)
    e.solve_map_nonlinear(**split(opts)[1])                 # the sibling shares the workspace: still nothing new
    assert e.alloc_count() == n
    D, N, F = e.D, e.N, e.F
    mean = e.get_means().reshape(N, D)[-1] + 0.1
    lam = np.eye(D)
    e.extend_se2([N - 1], [N], np.array([[0.5, 0.0, 0.0]]), g['s'][:1], prior_eta=(lam @ mean)[None], prior_lam=lam[None])
    r = e.solve_map_nonlinear_robust(**opts)
    assert e.map_mean().shape == (N + 1, D) and r.weights.shape == (F + 1,) and r.robust_flag.shape == (F + 1,) and r.weights[-1] == 1.0 and e.alloc_count() == n
    assert r.rounds >= 1 and 0 < r.flagged < F
    e.retire([0, 1])
    r = e.solve_map_nonlinear_robust(**opts)
    assert e.map_mean().shape == (N - 1, D) and r.weights.shape == (e.F,) and r.rounds >= 1 and e.alloc_count() == n
    want = np.linalg.norm(e.get_means() - e.map_mean().reshape(-1))
    assert abs(e.map_distance() - want) <= 1e-9 * max(1.0, want)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_bit_identical():
    from gbp_amd import _capi
    from gbp_amd._capi import GbpError
    from gbp_amd.linear import LinearEngine
    GBP_EINVAL, GBP_ESTATE = -1, -5                          # include/gbp_ba.h
    model, g, opts = graph_of('se2_ring65')
    e = make_engine(model, g)
    e.iterate(3, robustify=True, relinearise=True)
    e.solve_map()
    before, x, n = sweep_state(e), e.map_mean(), e.alloc_count()
    bad = [dict(max_rounds=-1), dict(tol_weight=-1.0), dict(tol_weight=float('nan')), dict(tol_move=-1e-3), dict(tol_move=float('inf')), dict(max_outer=-1),
           dict(lambda0=0.0), dict(lambda_up=1.0), dict(lambda_down=1.0), dict(lambda_min=1.0, lambda0=0.5), dict(lambda_max=float('inf')), dict(tol_step=-1.0),
           dict(tol_grad=float('nan')), dict(rel_tol=0.0), dict(max_iters=-1), dict(check_every=0)]
    for kw in bad:
        with pytest.raises(GbpError) as err:
            e.solve_map_nonlinear_robust(**kw)
        assert err.value.code == GBP_EINVAL, kw
        assert same_bits(before, sweep_state(e)) and e.map_mean().tobytes() == x.tobytes() and e.alloc_count() == n, kw
    lib = e._lib
    lm = _capi.LinNlmapOpts(5, 2, 1e-4, 10.0, 0.1, 1e-12, 1e8, 0.0, 0.0, _capi.LinMapOpts(1e-12, 100, 8, 0))
    o = _capi.LinIrlsOpts(3, 0, 1e-9, 1e-10, lm)
    assert lib.gbp_lin_solve_map_nonlinear_robust(e._h, ct.byref(o), None, None, None, None, None) == GBP_EINVAL      # unknown init
    o.lm.init, o.lm.cg.warm_start = 0, 1
    assert lib.gbp_lin_solve_map_nonlinear_robust(e._h, ct.byref(o), None, None, None, None, None) == GBP_EINVAL      # the inner solves start at x
    assert same_bits(before, sweep_state(e)) and e.map_mean().tobytes() == x.tobytes()
    # GBP_ESTATE: not nonlinear; from the MAP without a solve
    lin = LinearEngine(g['va'], g['vb'], np.zeros((e.F, 6)), np.tile(np.eye(6), (e.F, 1, 1)), g['prior_eta'], g['prior_lam'])
    lin.update_all_beliefs()
    lin.iterate(2)
    lin_state = lambda: list(lin.messages()) + list(lin.beliefs()) + [lin.get_means(), np.array(lin.alloc_count())]
    was = lin_state()
    with pytest.raises(GbpError) as err:
        lin.solve_map_nonlinear_robust()
    assert err.value.code == GBP_ESTATE and same_bits(was, lin_state())
    fresh = make_engine(model, g)
    was, n0 = sweep_state(fresh), fresh.alloc_count()
    with pytest.raises(GbpError) as err:
        fresh.solve_map_nonlinear_robust(init='map')
    assert err.value.code == GBP_ESTATE and same_bits(was, sweep_state(fresh)) and fresh.alloc_count() == n0
    # NULL opts are the documented defaults, every output optional; max_rounds == 0 leaves x = x0 and describes x0
    i = _capi.LinIrlsInfo()
    assert lib.gbp_lin_solve_map_nonlinear_robust(fresh._h, None, None, None, None, None, ct.byref(i)) == 0 and i.rounds >= 1 and i.rounds <= 20
    z, t = make_engine(model, g), twin_of(model, g, losses=True)
    r = z.solve_map_nonlinear_robust(max_rounds=0)
    w = twin_run(t, t.mu, dict(max_rounds=0))
    assert (r.rounds, r.outer, r.converged, r.reason) == (0, 0, False, IRLS_NONE) and r.round_trace.shape == (1, 6) and r.energy0 == r.energy
    assert z.map_mean().reshape(-1).tobytes() == z.get_means().tobytes()
    assert np.array_equal(r.robust_flag, w['flag']) and close(r.weights, w['weights']) and close(r.energy, w['energy'])
