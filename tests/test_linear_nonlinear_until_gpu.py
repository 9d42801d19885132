"""gbp_lin_iterate_until_nonlinear on the MI355X (include/gbp_lin.h; gbp_amd/csrc/gbp_lin_capi_until_nonlin.hip and the gated forms of
the stages in gbp_lin_nonlin.hpp / gbp_lin_sweep.hpp): the call against the host loop it replaces on a twin handle, bit for bit where
the contract says so; the freeze of the state at the deciding sweep for every check_every; the SETTLED bit at the sweeps the numpy model
of tests/lin_nonlin_until_cases.py gives; the reference's own runs (fixtures G25, G27); a live handle; the refusals; determinism.
tests/test_linear_nonlinear_until_cpu.py shows on the model alone that the freeze and SETTLED cases are usable."""
import ctypes as ct
import functools

import numpy as np
import pytest

from conftest import golden
from lin_map_cases import rel
from lin_nonlin_cases import PARITY, g25_graph, g25_schedule
from lin_nonlin_robust_cases import LOSS_NAME, g27_graph, g27_schedule
from lin_nonlin_until_cases import (BETA0_TOL, FREEZE, MAX_S, NAMES, SETTLED_PAIRS, STOP_NONE, STOP_STEP, TOL, TRACE_ENERGY, TRACE_MAP, UNTIL_SETTLED, case,
                                    freeze_sweep)

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5
SENTINEL, ISENT = -12345.5, -777
N_TWIN = 12
PLAIN_AND_ROBUST = [(n, r) for n in NAMES for r in (False, True) if not (n == 'nofactors' and r)]     # no factor: nothing to give a loss to


def make_engine(g, sched):
    from gbp_amd.linear import LinearEngine
    e = LinearEngine.se2_pose_graph(g['va'], g['vb'], g['z'], g['s'], g['prior_eta'], g['prior_lam'], sched['beta'],
                                    sched['num_undamped_iters'], sched['min_linear_iters'], eta_damping=sched['eta_damping'])
    if 'loss' in g:
        e.set_robust([LOSS_NAME[int(l)] for l in g['loss']], g['thr'])
    return e


def state(e):
    """Everything a sweep writes: both messages, beliefs, means, linpoint / iters_since_relin / damping, weights and flags.  eta_f and
    Lambda_f are seen through the joint's eta (the solvers read them where the relinearise stage writes them)."""
    return list(e.messages()) + list(e.beliefs()) + [e.get_means()] + list(e.linearisation()) + list(e.weights()) + [e.joint_eta()]


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def close(a, b):
    return abs(a - b) <= TOL * max(abs(b), 1.0)


def raw(e, max_iters, check_every=8, robustify=0, want=0, tol_step=0.0, tol_map=0.0, rows=None, counts=True, flagged=None):
    """The C call with sentinel-filled outputs of `rows` entries: (rc, trace, relin counts, robust counts, info)."""
    from gbp_amd import _capi
    o = _capi.LinUntilOpts(max_iters, check_every, robustify, want, tol_step, tol_map)
    i = _capi.LinUntilInfo(-1, -1, -1, -1)
    n = max(max_iters, 1) if rows is None else rows
    trace, rc, fc = np.full((n, 3), SENTINEL), np.full(n, ISENT, dtype=np.int32), np.full(n, ISENT, dtype=np.int32)
    give_f = bool(robustify) if flagged is None else flagged
    ret = e._lib.gbp_lin_iterate_until_nonlinear(e._h, ct.byref(o), _capi.dptr(trace), _capi.iptr(rc) if counts else None, _capi.iptr(fc) if give_f else None,
                                                 ct.byref(i))
    return ret, trace, rc, fc, i


def sweeps(e, n, robust):
    """n sweeps by the iterate calls: (relin counts, robust counts or None)."""
    out = e.iterate(n, robustify=robust, relinearise=True)
    return out if robust else (out, None)


def host_loop(e, n, robust, with_map=True):
    """The loop the call replaces: rows (n, 3) of step / energy / MAP distance, relin counts, robust counts."""
    rows, rc, fc = np.zeros((n, 3)), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    old = e.get_means()
    for i in range(n):
        c, f = sweeps(e, 1, robust)
        rc[i], fc[i] = c[0], (f[0] if robust else 0)
        mu = e.get_means()
        rows[i] = (np.max(np.abs(mu - old)) if mu.size else 0.0, e.energy(), e.map_distance() if with_map else np.nan)
        old = mu
    return rows, rc, fc


@functools.lru_cache(maxsize=None)
def recorded(name, robust, n=MAX_S):
    """A host loop's rows and counts over n sweeps of case `name` on the device: computed once, shared, never written to."""
    g, sched = case(name, robust)
    b = make_engine(g, sched)
    rows, rc, fc = host_loop(b, n, robust, with_map=False)
    b.close()
    for a in (rows, rc, fc):
        a.setflags(write=False)
    return rows, rc, fc


@functools.lru_cache(maxsize=None)
def model_sweep(name, robust):
    """The deciding sweep the numpy model proves usable for a freeze case."""
    return freeze_sweep(name, robust)[0]


# ---- 1. twin handles -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,robust', PLAIN_AND_ROBUST)
def test_trace_and_counts_match_the_host_loop_on_a_twin(name, robust):
    g, sched = case(name, robust)
    a, b = make_engine(g, sched), make_engine(g, sched)
    a.solve_map(); b.solve_map()
    r = a.iterate_until_nonlinear(N_TWIN, energy=True, map_distance=True, robustify=robust)
    rows, rc, fc = host_loop(b, N_TWIN, robust)
    assert (r.iters, r.converged, r.reason) == (N_TWIN, False, STOP_NONE)
    assert r.step.shape == r.energy.shape == r.map_distance.shape == r.relin_counts.shape == (N_TWIN,)
    assert np.array_equal(r.step, rows[:, 0]), f"step {r.step} vs {rows[:, 0]}"
    for i in range(N_TWIN):
        assert close(r.energy[i], rows[i, 1]), f"sweep {i + 1}: energy {r.energy[i]!r} vs {rows[i, 1]!r}"
        assert close(r.map_distance[i], rows[i, 2]), f"sweep {i + 1}: distance {r.map_distance[i]!r} vs {rows[i, 2]!r}"
    assert np.array_equal(r.relin_counts, rc) and r.relin_counts.dtype == np.int32
    if robust:
        assert np.array_equal(r.robust_counts, fc) and fc.any()   # some factor was flagged: the weights were re-made in the sweeps
    else:
        assert r.robust_counts is None
    if name == 'nofactors':
        assert not r.step.any() and not rc.any() and not r.energy.any()
    else:
        assert r.step[0] > 0 and rc.any()                    # (F1 converges to a step of exactly 0 within the twelve sweeps)
    assert same(state(a), state(b))
    plain = a.iterate_until_nonlinear(3)                     # columns not asked for
    assert plain.energy is None and plain.map_distance is None and plain.step.shape == plain.relin_counts.shape == (3,)
    a.close(); b.close()


def test_plain_sweeps_on_a_handle_with_losses_run_at_the_standing_weights():
    """robustify == 0 with losses set: the sweep of gbp_lin_iterate_nonlinear, the weighted factor stage and the weighted energy."""
    g, sched = case('ring65', True)
    a, b = make_engine(g, sched), make_engine(g, sched)
    sweeps(a, 3, True); sweeps(b, 3, True)
    w0 = a.weights()[0].copy()
    assert (w0 < 1).any()
    r = a.iterate_until_nonlinear(7, energy=True)
    rows, rc, _ = host_loop(b, 7, False, with_map=False)
    assert np.array_equal(r.step, rows[:, 0]) and np.array_equal(r.relin_counts, rc) and r.robust_counts is None
    assert all(close(x, y) for x, y in zip(r.energy, rows[:, 1]))
    assert np.array_equal(a.weights()[0], w0) and same(state(a), state(b))
    a.close(); b.close()


# ---- 2. the freeze ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('check_every', [1, 3, 8, 64])
@pytest.mark.parametrize('robust', [False, True])
@pytest.mark.parametrize('name', FREEZE)
def test_stop_on_step_freezes_the_state_at_the_deciding_sweep(name, robust, check_every):
    s = model_sweep(name, robust)
    rows, rc, fc = recorded(name, robust)
    assert s is not None and s % 3 and s % 8 and all(rows[s - 1, 0] < v for v in rows[:s - 1, 0])
    g, sched = case(name, robust)
    a, c = make_engine(g, sched), make_engine(g, sched)
    ret, trace, arc, afc, info = raw(a, MAX_S, check_every, int(robust), 0, tol_step=rows[s - 1, 0])
    sweeps(c, s, robust)
    assert ret == 0 and (info.iters, info.converged, info.reason) == (s, 1, STOP_STEP)
    assert same(state(a), state(c))
    assert np.array_equal(trace[:s, 0], rows[:s, 0]) and np.isnan(trace[:s, 1:]).all() and np.all(trace[s:] == SENTINEL)
    assert np.array_equal(arc[:s], rc[:s]) and np.all(arc[s:] == ISENT)
    if robust:
        assert np.array_equal(afc[:s], fc[:s]) and np.all(afc[s:] == ISENT)
    else:
        assert np.all(afc == ISENT)
    # the handle goes on from there like the twin
    assert np.array_equal(sweeps(a, 2, robust)[0], sweeps(c, 2, robust)[0]) and same(state(a), state(c))
    a.close(); c.close()


# ---- 3. settled ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,k,plain_stop,settled_stop', SETTLED_PAIRS)
def test_settled_waits_for_a_sweep_that_relinearises_nothing(name, k, plain_stop, settled_stop):
    rows, rc, _ = recorded(name, False, 60)
    assert rc[k - 1] > 0 and rc[settled_stop - 1] == 0
    g, sched = case(name)
    for want, stop in ((0, plain_stop), (UNTIL_SETTLED, settled_stop)):
        a, c = make_engine(g, sched), make_engine(g, sched)
        ret, trace, arc, _, info = raw(a, 60, 8, 0, want, tol_step=rows[k - 1, 0])
        assert ret == 0 and (info.iters, info.converged, info.reason) == (stop, 1, STOP_STEP), (want, info.iters)
        assert np.array_equal(trace[:stop, 0], rows[:stop, 0]) and np.array_equal(arc[:stop], rc[:stop]) and np.all(arc[stop:] == ISENT)
        sweeps(c, stop, False)
        assert same(state(a), state(c))
        a.close(); c.close()


def test_a_graph_that_relinearises_every_sweep_never_settles():
    g, sched = case('beta0')
    a, b = make_engine(g, sched), make_engine(g, sched)
    r = a.iterate_until_nonlinear(60, tol_step=BETA0_TOL, settled=True)
    assert (r.iters, r.converged, r.reason) == (60, False, STOP_NONE)
    assert r.relin_counts.tolist() == [0] + [a.F] * 59 and np.sum(r.step <= BETA0_TOL) > 50
    r = b.iterate_until_nonlinear(60, tol_step=BETA0_TOL)
    assert (r.iters, r.converged, r.reason) == (4, True, STOP_STEP)
    a.close(); b.close()


def test_settled_holds_back_the_map_rule_too():
    """tol_map generous enough for every sweep: without the bit the first sweep decides, with it the first that relinearises nothing --
    on hub9 the first sweep itself relinearises nothing (the linpoints are the means), so start from a handle one sweep on."""
    g, sched = case('hub9')
    rows, rc, _ = recorded('hub9', False, 60)
    first_quiet = 2 + int(np.nonzero(rc[1:] == 0)[0][0])      # 1-based, among the sweeps after the first
    assert rc[1] > 0 and first_quiet > 2
    for want, stop in ((TRACE_MAP, 1), (TRACE_MAP | UNTIL_SETTLED, first_quiet - 1)):
        a = make_engine(g, sched)
        a.solve_map()
        sweeps(a, 1, False)
        ret, trace, arc, _, info = raw(a, 20, 8, 0, want, tol_map=1e6)
        assert ret == 0 and (info.iters, info.converged, info.reason) == (stop, 1, 2), (want, info.iters)
        assert np.array_equal(arc[:stop], rc[1:1 + stop])
        a.close()


# ---- 4. the reference's own run --------------------------------------------------------------------------------------------------------

def _against_reference(e, r, means, energy, start):
    """energy and means-derived step of the reference's stored run, within the parity contract of tests/test_linear_nonlinear_gpu.py:
    rel() < PARITY on energy and means.  A step is a difference of two rows of means, each within PARITY * max |means| of the
    reference's, so it is within twice that of the reference's step."""
    n = means.shape[0]
    for i in range(n):
        assert rel(r.energy[i], energy[i]) < PARITY, f"sweep {i + 1}: energy {rel(r.energy[i], energy[i]):.3e}"
    prev = np.concatenate([start[None], means[:-1]])
    ref_step = np.max(np.abs(means - prev), axis=1)
    bound = 2 * PARITY * np.max(np.abs(means))
    assert r.step.shape == (n,) and np.max(np.abs(r.step - ref_step)) <= bound, f"step {np.max(np.abs(r.step - ref_step)):.3e} > {bound:.3e}"
    assert rel(e.get_means(), means[-1]) < PARITY


def test_reference_run_g25_in_one_call():
    g = golden('G25_se2_posegraph')
    sched, n = g25_schedule(g, 'main')
    e = make_engine(g25_graph(g), sched)
    start = e.get_means()
    r = e.iterate_until_nonlinear(n, energy=True)
    assert r.iters == n and r.relin_counts.tolist() == g['main_mask'].sum(1).tolist()
    _against_reference(e, r, g['main_means'], g['main_energy'], start)
    e.close()


def test_reference_run_g27_in_one_robust_call():
    g = golden('G27_se2_posegraph_robust')
    sched, n = g27_schedule(g)
    e = make_engine(g27_graph(g), sched)
    start = e.get_means()
    r = e.iterate_until_nonlinear(n, energy=True, robustify=True)
    assert r.iters == n and r.relin_counts.tolist() == g['mask'].sum(1).tolist() and r.robust_counts.tolist() == g['flag'].sum(1).tolist()
    _against_reference(e, r, g['means'], g['energy'], start)
    assert np.array_equal(e.weights()[1], g['flag'][-1].astype(bool))
    e.close()


# ---- 5. a live handle ------------------------------------------------------------------------------------------------------------------

def test_live_handle_extend_and_retire_between_calls():
    from gbp_amd import _capi
    from lin_nonlin_robust_cases import live_schedule
    g0, rounds = live_schedule(rounds=2)
    ext = rounds[0][0]
    sched = case('hub9')[1]
    a, b = make_engine(g0, sched), make_engine(g0, sched)
    a.solve_map()
    r = a.iterate_until_nonlinear(5, energy=True, map_distance=True)
    c, _ = sweeps(b, 5, False)
    assert np.array_equal(r.relin_counts, c) and same(state(a), state(b))
    a.iterate_until_nonlinear(5, energy=True, map_distance=True); sweeps(b, 5, False)
    count = a.alloc_count()
    a.iterate_until_nonlinear(5, energy=True, map_distance=True); sweeps(b, 5, False)
    assert a.alloc_count() == count and same(state(a), state(b))        # a repeated call of the same size allocates nothing
    for h in (a, b):
        h.extend_se2(ext['va'], ext['vb'], ext['z'], ext['s'], ext['prior_eta'], ext['prior_lam'])
    o = _capi.LinUntilOpts(3, 8, 0, TRACE_MAP, 0.0, 0.0)
    assert a._lib.gbp_lin_iterate_until_nonlinear(a._h, ct.byref(o), None, None, None, None) == ESTATE      # the solve is of the old graph
    assert same(state(a), state(b))
    r = a.iterate_until_nonlinear(6, energy=True)
    rows, rc, _ = host_loop(b, 6, False, with_map=False)
    assert np.array_equal(r.step, rows[:, 0]) and np.array_equal(r.relin_counts, rc) and same(state(a), state(b))
    a.solve_map()
    assert a.iterate_until_nonlinear(2, map_distance=True).map_distance.shape == (2,); sweeps(b, 2, False)
    for h in (a, b):
        h.retire([0])
    assert a._lib.gbp_lin_iterate_until_nonlinear(a._h, ct.byref(o), None, None, None, None) == ESTATE
    r = a.iterate_until_nonlinear(6, energy=True)
    rows, rc, _ = host_loop(b, 6, False, with_map=False)
    assert np.array_equal(r.step, rows[:, 0]) and np.array_equal(r.relin_counts, rc) and same(state(a), state(b))
    assert all(close(x, y) for x, y in zip(r.energy, rows[:, 1]))
    count = a.alloc_count()
    a.iterate_until_nonlinear(6, energy=True); sweeps(b, 6, False)
    assert a.alloc_count() == count and same(state(a), state(b))
    a.close(); b.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------

def test_every_refusal_leaves_the_handle_as_it_was():
    from gbp_amd import _capi
    from gbp_amd.linear import LinearEngine
    g, sched = case('ring65', True)
    a, b = make_engine(g, sched), make_engine(g, sched)
    sweeps(a, 2, True); sweeps(b, 2, True)
    count = a.alloc_count()
    nan, inf = float('nan'), float('inf')
    base = dict(max_iters=5, check_every=1, robustify=0, want=0, tol_step=0.0, tol_map=0.0)
    bad = [dict(max_iters=-1), dict(check_every=0), dict(robustify=2), dict(robustify=-1), dict(want=8), dict(want=-1), dict(tol_step=-1e-9), dict(tol_step=nan),
           dict(tol_step=inf), dict(tol_map=-1.0, want=TRACE_MAP), dict(tol_map=nan, want=TRACE_MAP), dict(tol_map=0.5), dict(tol_map=0.5, want=UNTIL_SETTLED)]
    for k in bad:
        assert raw(a, **dict(base, **k))[0] == EINVAL, k
    assert raw(a, **dict(base, flagged=True))[0] == EINVAL                 # robust_counts given with robustify == 0
    assert a._lib.gbp_lin_iterate_until_nonlinear(a._h, None, None, None, None, None) == EINVAL
    assert raw(a, **dict(base, want=TRACE_MAP))[0] == ESTATE                # no solve yet
    assert b'solve_map' in a._lib.gbp_last_error()
    nol = make_engine(*case('ring65'))
    assert raw(nol, **dict(base, robustify=1))[0] == ESTATE                 # no losses set
    lin = LinearEngine(g['va'], g['vb'], np.zeros((a.F, 6)), np.tile(np.eye(6), (a.F, 1, 1)), g['prior_eta'], g['prior_lam'])
    lin.update_all_beliefs()
    assert raw(lin, **base)[0] == ESTATE and b'nonlinear' in lin._lib.gbp_last_error()   # a linear handle
    uo = _capi.LinUntilOpts(5, 1, 0, 0, 1e-3, 0.0)
    assert a._lib.gbp_lin_iterate_until(a._h, ct.byref(uo), None, None) == ESTATE         # the old call still refuses a nonlinear handle
    uo4 = _capi.LinUntilOpts(5, 1, 0, UNTIL_SETTLED, 1e-3, 0.0)
    assert lin._lib.gbp_lin_iterate_until(lin._h, ct.byref(uo4), None, None) == EINVAL    # ... and the new bit on a linear one
    ret, trace, rc, fc, info = raw(a, 0, rows=2, robustify=1)               # max_iters == 0: nothing written
    assert ret == 0 and (info.iters, info.converged, info.reason) == (0, 0, STOP_NONE)
    assert np.all(trace == SENTINEL) and np.all(rc == ISENT) and np.all(fc == ISENT)
    assert a.alloc_count() == count and same(state(a), state(b))
    ca, cb = sweeps(a, 1, True), sweeps(b, 1, True)
    assert np.array_equal(ca[0], cb[0]) and same(state(a), state(b))
    # NULL outputs are legal
    o = _capi.LinUntilOpts(3, 8, 1, TRACE_ENERGY, 0.0, 0.0)
    assert a._lib.gbp_lin_iterate_until_nonlinear(a._h, ct.byref(o), None, None, None, None) == 0
    sweeps(b, 3, True)
    assert same(state(a), state(b))
    for h in (a, b, nol, lin):
        h.close()


def test_no_factors_converges_at_the_first_sweep():
    g, sched = case('nofactors')
    a = make_engine(g, sched)
    mu = a.get_means()
    ret, trace, rc, _, info = raw(a, 5, 8, 0, TRACE_ENERGY, tol_step=1e-300)
    assert ret == 0 and (info.iters, info.converged, info.reason) == (1, 1, STOP_STEP)
    assert trace[0, 0] == 0.0 and trace[0, 1] == 0.0 and np.isnan(trace[0, 2]) and np.all(trace[1:] == SENTINEL)
    assert rc[0] == 0 and np.all(rc[1:] == ISENT) and np.array_equal(a.get_means(), mu)
    a.close()


def test_the_call_marks_the_joint_stale():
    """After sweeps that relinearised, the next solve is a Gauss-Newton step at the new linearisation point, as after the iterate call."""
    g, sched = case('ring63')
    a, b = make_engine(g, sched), make_engine(g, sched)
    a.solve_map(); b.solve_map()
    r = a.iterate_until_nonlinear(4); sweeps(b, 4, False)
    assert r.relin_counts.any()
    ma, _ = a.solve_map(); mb, _ = b.solve_map()
    assert np.array_equal(ma, mb)
    a.close(); b.close()


# ---- 7. determinism --------------------------------------------------------------------------------------------------------------------

def test_two_handles_give_bit_identical_traces_and_counts():
    g, sched = case('ring257', True)
    out = []
    for _ in range(2):
        e = make_engine(g, sched)
        e.solve_map()
        r1 = e.iterate_until_nonlinear(9, energy=True, map_distance=True, robustify=True, check_every=4)
        r2 = e.iterate_until_nonlinear(7, energy=True, map_distance=True, settled=True)
        out.append([r1.step, r1.energy, r1.map_distance, r1.relin_counts, r1.robust_counts, r2.step, r2.energy, r2.map_distance, r2.relin_counts] + state(e))
        e.close()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(*out)) and out[0][4].any() and out[0][3].any()
