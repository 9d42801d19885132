"""gbp_lin_iterate_until (include/gbp_lin.h) on the GPU: the device-side trace and stop rule against the host loop it replaces
(iterate(1); get_means(); energy(); map_distance() on a twin handle), the freeze behind the deciding sweep for every check_every, the
places a reduction can drop something, the reference's own stdout trace, and the life cycle.  The deciding sweeps come from the numpy
model of tests/lin_until_cases.py, proved usable on the oracle alone by tests/test_linear_until_cpu.py."""
import ctypes as ct
import functools

import numpy as np
import pytest

from conftest import golden
from lin_until_cases import FIN_THREADS, MAX_S, STOP_MAP, STOP_NONE, STOP_STEP, TOL, TRACE_ENERGY, TRACE_MAP, displacement, graphs, map_of, oracle, run_model, usable_sweep

pytestmark = pytest.mark.gpu

GRAPHS = graphs()
EINVAL, ESTATE = -1, -5
SENTINEL = -7.25


def engine(g, robust=False):
    from gbp_amd.linear import LinearEngine
    o = oracle(g)
    e = LinearEngine(o.va, o.vb, o.fe0, o.fl0, o.pe, o.pl, factor_const=o.fc0)
    if robust:
        e.set_robust('huber', 2.0, o.sigma ** 2)
    e.update_all_beliefs()
    return e


def state(e):
    """Everything a sweep writes: both messages, beliefs, means, weights and flags."""
    return e.messages() + e.beliefs() + (e.get_means(),) + e.weights()


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def close(a, b):
    return abs(a - b) <= TOL * max(abs(b), 1.0)


def raw(e, max_iters, check_every=8, robustify=0, want=0, tol_step=0.0, tol_map=0.0, rows=None):
    """The C call with a sentinel-filled trace of `rows` rows: (rc, trace, info)."""
    from gbp_amd import _capi
    o = _capi.LinUntilOpts(max_iters, check_every, robustify, want, tol_step, tol_map)
    i = _capi.LinUntilInfo(-1, -1, -1, -1)
    trace = np.full((max(max_iters, 1) if rows is None else rows, 3), SENTINEL)
    rc = e._lib.gbp_lin_iterate_until(e._h, ct.byref(o), _capi.dptr(trace), ct.byref(i))
    return rc, trace, i


def host_loop(e, n, robust=False, with_map=True):
    """The loop the call replaces, on a twin: rows (n, 3) of step / energy / map distance."""
    rows = np.zeros((n, 3))
    old = e.get_means()
    for i in range(n):
        e.iterate(1, robustify=robust)
        mu = e.get_means()
        rows[i] = (np.max(np.abs(mu - old)) if mu.size else 0.0, e.energy(), e.map_distance() if with_map else np.nan)
        old = mu
    return rows


@functools.lru_cache(maxsize=None)
def recorded(name, robust):
    """B's rows over MAX_S sweeps on graph `name` (computed once, shared, never written to), and the sweeps the model proves usable."""
    g = GRAPHS[name]
    b = engine(g, robust)
    b.solve_map()
    rows = host_loop(b, MAX_S, robust)
    rows.setflags(write=False)
    m, _, _ = run_model(oracle(g, 'huber' if robust else None), MAX_S, x_map=map_of(g), robustify=robust)
    return rows, usable_sweep(m[:, 0]), usable_sweep(m[:, 2]), usable_sweep(m[:, 0], m[:, 2])


# ---- 1. twin handles -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('robust', [False, True])
@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_trace_matches_the_host_loop_on_a_twin(name, robust):
    n = 12
    a, b = engine(GRAPHS[name], robust), engine(GRAPHS[name], robust)
    a.solve_map(); b.solve_map()
    r = a.iterate_until(n, energy=True, map_distance=True, robustify=robust)
    rows = host_loop(b, n, robust)
    assert (r.iters, r.converged, r.reason) == (n, False, STOP_NONE)
    assert r.step.shape == r.energy.shape == r.map_distance.shape == (n,)
    assert np.array_equal(r.step, rows[:, 0]) and np.all(rows[:, 0] > 0)
    for i in range(n):
        assert close(r.energy[i], rows[i, 1]), f"sweep {i + 1}: energy {r.energy[i]!r} vs {rows[i, 1]!r}"
        assert close(r.map_distance[i], rows[i, 2]), f"sweep {i + 1}: distance {r.map_distance[i]!r} vs {rows[i, 2]!r}"
    assert same(state(a), state(b))
    if robust:
        assert a.weights()[1].any()                          # some factor was robust: the weights were re-made every sweep
    plain = a.iterate_until(3)                               # columns not asked for
    assert plain.energy is None and plain.map_distance is None and plain.step.shape == (3,)


# ---- 2. the freeze ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('check_every', [1, 3, 8, 64])
@pytest.mark.parametrize('robust', [False, True])
@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_stop_on_step_freezes_the_state_at_the_deciding_sweep(name, robust, check_every):
    rows, s, _, _ = recorded(name, robust)
    assert s is not None and s % 3 and s % 8 and all(rows[s - 1, 0] < v for v in rows[:s - 1, 0])
    a, c = engine(GRAPHS[name], robust), engine(GRAPHS[name], robust)
    rc, trace, info = raw(a, MAX_S, check_every, int(robust), 0, tol_step=rows[s - 1, 0])
    c.iterate(s, robustify=robust)
    assert rc == 0 and (info.iters, info.converged, info.reason) == (s, 1, STOP_STEP)
    assert same(state(a), state(c))
    assert np.array_equal(trace[:s, 0], rows[:s, 0]) and np.isnan(trace[:s, 1:]).all()
    assert np.all(trace[s:] == SENTINEL)


@pytest.mark.parametrize('check_every', [1, 3, 8, 64])
@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_stop_on_map_distance_and_step_first_when_both_are_met(name, check_every):
    rows, _, s, sb = recorded(name, False)
    assert s is not None and all(rows[s - 1, 2] < v for v in rows[:s - 1, 2])
    g = GRAPHS[name]
    a, c = engine(g), engine(g)
    a.solve_map()
    probe = a.iterate_until(MAX_S, map_distance=True, check_every=MAX_S)        # the device's own distances: the tolerance is one of them
    assert all(close(x, y) for x, y in zip(probe.map_distance, rows[:, 2]))
    a2 = engine(g)
    a2.solve_map()
    rc, trace, info = raw(a2, MAX_S, check_every, 0, TRACE_MAP, tol_map=probe.map_distance[s - 1])
    c.iterate(s)
    assert rc == 0 and (info.iters, info.converged, info.reason) == (s, 1, STOP_MAP)
    assert same(state(a2), state(c))
    assert np.array_equal(trace[:s, 2], probe.map_distance[:s]) and np.array_equal(trace[:s, 0], rows[:s, 0]) and np.all(trace[s:] == SENTINEL)
    # both tolerances met for the first time in one sweep: STEP
    assert sb is not None and all(rows[sb - 1, 0] < v for v in rows[:sb - 1, 0]) and all(probe.map_distance[sb - 1] < v for v in probe.map_distance[:sb - 1])
    a3, c3 = engine(g), engine(g)
    a3.solve_map()
    rc, trace, info = raw(a3, MAX_S, check_every, 0, TRACE_MAP, tol_step=rows[sb - 1, 0], tol_map=probe.map_distance[sb - 1])
    c3.iterate(sb)
    assert rc == 0 and (info.iters, info.converged, info.reason) == (sb, 1, STOP_STEP)
    assert same(state(a3), state(c3)) and np.all(trace[sb:] == SENTINEL)


# ---- 3. where a reduction can drop something -------------------------------------------------------------------------------------------

def consistent_chain(N, D, off=None, gross=None):
    """A chain whose measurements have zero residual at exactly representable positions, priors at the truth -- except variable `off`,
    whose prior mean is 1 too large, and factor `gross`, whose measurement is 50 off.  LinearEngine arguments."""
    rs = np.random.RandomState(N + D)
    x = np.round(rs.rand(N, D) * 64) / 8
    va, vb = np.arange(N - 1), np.arange(1, N)
    z = x[vb] - x[va]
    if gross is not None:
        z[gross] += 50.0
    J = np.hstack([-np.eye(D), np.eye(D)])
    fe, fl = (z @ J) / 0.25, np.ascontiguousarray(np.broadcast_to(J.T @ J / 0.25, (N - 1, 2 * D, 2 * D)))
    fc = 0.5 * np.einsum('fd,fd->f', z, z) / 0.25
    mean = x.copy()
    if off is not None:
        mean[off] += 1.0
    return (va, vb, fe, fl, mean / 9.0, np.ascontiguousarray(np.broadcast_to(np.eye(D) / 9.0, (N, D, D)))), fc


@pytest.mark.parametrize('D,N', [(6, 2102), (1, 40003), (1, 240003), (3, 5)])
def test_the_step_of_a_single_moving_variable_is_not_dropped(D, N):
    """More belief blocks than the finishing block has threads (d = 6: 2 variables per block, d = 1: 32), and more than 7 x that
    (N = 240003: 7501 blocks), from where a thread of the finishing block takes eight partials at a time; the one variable that moves
    being the first, the last, and the first of the last block; and a graph of 5 variables and 4 factors."""
    from gbp_amd.linear import LinearEngine
    vpw = 64 // (D + D * (D + 1) // 2)
    nblocks = -(-N // vpw)
    assert nblocks > FIN_THREADS or N == 5
    assert nblocks > 7 * FIN_THREADS or N < 200000
    for off in (0, N - 1, (nblocks - 1) * vpw):
        args, fc = consistent_chain(N, D, off=off)
        a, b = LinearEngine(*args, factor_const=fc), LinearEngine(*args, factor_const=fc)
        a.update_all_beliefs(); b.update_all_beliefs()
        before = b.get_means()
        r = a.iterate_until(1)
        b.iterate(1)
        moved = np.abs(b.get_means() - before)
        assert r.step[0] == np.max(moved) and r.step[0] > 1e-3
        assert np.argmax(moved) // D == off                  # the maximum sits where the test put it
        assert same(state(a), state(b))


def test_a_single_variable_without_factors_does_not_move():
    from gbp_amd.linear import LinearEngine
    pe, pl = np.array([[1.0, 2.0, 3.0]]), np.eye(3)[None] / 3.0
    a = LinearEngine([], [], np.zeros((0, 6)), np.zeros((0, 6, 6)), pe, pl, factor_const=np.zeros(0))
    a.update_all_beliefs()
    before = a.get_means()
    r = a.iterate_until(5, tol_step=1e-300, energy=True)
    assert (r.iters, r.converged, r.reason) == (1, True, STOP_STEP)            # F == 0: the step is exactly 0 from the first sweep
    assert r.step[0] == 0.0 and r.energy[0] == 0.0 and np.array_equal(a.get_means(), before)


@pytest.mark.parametrize('F', [257, 256 * FIN_THREADS + 1])
def test_the_energy_of_a_single_gross_factor_is_not_dropped(F):
    """More energy blocks than one (F across 256) and than the finishing block has threads (F across 256 x that), the one factor
    with a gross residual being the first and the last."""
    from gbp_amd.linear import LinearEngine
    for gross in (0, F - 1):
        args, fc = consistent_chain(F + 1, 1, gross=gross)
        a, b = LinearEngine(*args, factor_const=fc), LinearEngine(*args, factor_const=fc)
        a.update_all_beliefs(); b.update_all_beliefs()
        r = a.iterate_until(1, energy=True)
        b.iterate(1)
        want = b.energy()
        assert close(r.energy[0], want), f"{r.energy[0]!r} vs {want!r}"
        assert want > 50.0                                   # the gross factor's share, 0.5 r^2 / 0.25: every other factor has residual ~0


# ---- 4. the reference's own trace ------------------------------------------------------------------------------------------------------

def test_one_call_prints_the_reference_stdout_trace():
    """The 'Iteration i // Energy ... // Av distance of means from MAP ...' lines of the reference's own
    `ndim_posegraph.py --n_varnodes 100 --dim 3 --n_iters 20` run (fixture G8 stdout), character for character, from ONE call."""
    from gbp_amd.linear import LinearEngine
    from oracle.linear_oracle import toy_posegraph
    g8 = golden('G8_toy_linear')
    want = [ln for ln in str(g8['n100d3_stdout']).split('\n') if ln.startswith('Iteration')]
    va, vb, fe, fl, fc, pe, pl = toy_posegraph(100, 3, 10, 1.0, seed=0)
    e = LinearEngine(va, vb, fe, fl, pe, pl, factor_const=fc)
    e.update_all_beliefs()
    _, info = e.solve_map()
    assert info['converged']
    r = e.iterate_until(20, energy=True, map_distance=True)
    got = [f'Iteration {i}   //   Energy {r.energy[i]:.4f}   //   Av distance of means from MAP {r.map_distance[i]:4f}' for i in range(r.iters)]
    assert r.iters == 20 and got == want                     # ndim_posegraph.py:107-108


# ---- 5. life cycle ---------------------------------------------------------------------------------------------------------------------

def grow(e, g):
    """Two more variables hung on the end of the graph by three displacement factors."""
    D, N = e.D, e.N
    J = np.hstack([-np.eye(D), np.eye(D)])
    z = np.arange(3 * D, dtype=float).reshape(3, D) / 4
    e.extend([N - 1, N, N - 2], [N, N + 1, N + 1], z @ J, np.broadcast_to(J.T @ J, (3, 2 * D, 2 * D)), np.ones((2, D)), np.broadcast_to(np.eye(D) / 9.0, (2, D, D)),
             factor_const=0.5 * np.einsum('fd,fd->f', z, z))


@pytest.mark.parametrize('change', ['extend', 'shrink'])
@pytest.mark.parametrize('name', ['toy_d3', 'chain_d6', 'ring_d1'])
def test_map_column_needs_a_solve_after_a_change_of_the_graph(name, change):
    from gbp_amd import _capi
    g = GRAPHS[name]
    a, b = engine(g), engine(g)
    for e in (a, b):
        e.solve_map()
        e.iterate_until(4, energy=True, map_distance=True)   # the workspace exists, sized for the graph as it was
        if change == 'extend':
            grow(e, g)
        else:
            e.shrink(retire_vars=[0, 1, 2])
    before = state(a)
    with pytest.raises(_capi.GbpError) as err:
        a.iterate_until(4, map_distance=True)
    assert err.value.code == ESTATE and same(state(a), before)
    r0 = a.iterate_until(2, energy=True)                     # without the MAP column the call needs no solve
    assert r0.iters == 2 and close(r0.energy[1], a.energy())
    b.iterate(2)
    a.solve_map(); b.solve_map()
    r = a.iterate_until(6, energy=True, map_distance=True)
    rows = host_loop(b, 6)
    assert np.array_equal(r.step, rows[:, 0])
    assert all(close(x, y) for x, y in zip(r.energy, rows[:, 1])) and all(close(x, y) for x, y in zip(r.map_distance, rows[:, 2]))
    assert same(state(a), state(b))


def test_two_hundred_calls_reuse_one_workspace_and_two_handles_agree_bit_for_bit():
    g = GRAPHS['toy_d3']
    a, b, c = engine(g), engine(g), engine(g)
    for e in (a, b, c):
        e.solve_map()
    one = a.iterate_until(200, energy=True, map_distance=True)
    two = b.iterate_until(200, energy=True, map_distance=True)
    for col in ('step', 'energy', 'map_distance'):           # two identical handles: bit-identical traces
        assert np.array_equal(getattr(one, col), getattr(two, col))
    many = [c.iterate_until(1 + (i % 2), energy=True, map_distance=True) for i in range(200)]      # 300 sweeps in 200 calls
    got = np.concatenate([m.step for m in many]), np.concatenate([m.energy for m in many]), np.concatenate([m.map_distance for m in many])
    assert all(np.array_equal(x[:200], getattr(one, col)) for x, col in zip(got, ('step', 'energy', 'map_distance')))
    a.iterate_until(100)
    assert same(state(a), state(c))


def test_repeated_calls_allocate_nothing_and_a_change_of_the_graph_keeps_one_workspace():
    """Through the handle's allocation count: the first call makes the stop word, two partial arrays and the trace buffer; calls no
    longer than the longest seen make nothing; a longer one replaces the trace buffer; extend and shrink drop the two partial arrays
    and the next call re-makes them."""
    g = GRAPHS['chain_d6']
    e = engine(g)
    base = e.alloc_count()
    e.iterate_until(4, energy=True)
    assert e.alloc_count() == base + 4
    for i in range(200):
        e.iterate_until(1 + i % 4, energy=bool(i % 2))
        assert e.alloc_count() == base + 4
    e.iterate_until(9)                                       # a larger trace buffer replaces the smaller one
    assert e.alloc_count() == base + 4
    e.solve_map()
    with_map = e.alloc_count()
    e.iterate_until(9, energy=True, map_distance=True)
    assert e.alloc_count() == with_map
    grow(e, g)
    grown = e.alloc_count()                                  # the solver's workspace and the two partial arrays went with the old graph
    assert grown == base + 2
    e.iterate_until(3)
    e.iterate_until(9)
    assert e.alloc_count() == grown + 2
    e.shrink(retire_vars=[0])
    assert e.alloc_count() == grown
    e.iterate_until(2, energy=True)
    assert e.alloc_count() == grown + 2


def test_every_refusal_leaves_the_handle_as_it_was():
    from gbp_amd import _capi
    from gbp_amd.linear import LinearEngine
    g = GRAPHS['chain_d6']
    a, twin = engine(g), engine(g)
    inf, nan = float('inf'), float('nan')
    bad = [dict(max_iters=-1), dict(check_every=0), dict(robustify=2), dict(robustify=-1), dict(want=4), dict(want=-1), dict(tol_step=-1e-9), dict(tol_step=nan),
           dict(tol_step=inf), dict(tol_map=-1.0, want=TRACE_MAP), dict(tol_map=nan, want=TRACE_MAP), dict(tol_map=0.5)]
    for kw in bad:
        rc, trace, info = raw(a, **{'max_iters': 5, **kw})
        assert rc == EINVAL, kw
        assert np.all(trace == SENTINEL) and info.iters == -1
    assert a._lib.gbp_lin_iterate_until(a._h, None, None, None) == EINVAL
    for kw, why in ((dict(robustify=1), 'no losses'), (dict(want=TRACE_MAP), 'no solve'), (dict(want=TRACE_MAP, tol_map=1.0), 'no solve')):
        rc, trace, _ = raw(a, 5, **kw)
        assert rc == ESTATE and np.all(trace == SENTINEL), why
    o = oracle(g)
    fresh = LinearEngine(o.va, o.vb, o.fe0, o.fl0, o.pe, o.pl, factor_const=o.fc0)
    assert raw(fresh, 5)[0] == ESTATE                        # no beliefs yet
    rc, trace, info = raw(a, 0)                              # max_iters == 0: fine, and nothing happens
    assert rc == 0 and (info.iters, info.converged, info.reason) == (0, 0, STOP_NONE) and np.all(trace == SENTINEL)
    assert same(state(a), state(twin))
    ra, rt = a.iterate_until(9, energy=True), twin.iterate_until(9, energy=True)
    assert np.array_equal(ra.step, rt.step) and np.array_equal(ra.energy, rt.energy) and same(state(a), state(twin))
    assert a._lib.gbp_lin_iterate_until(a._h, ct.byref(_capi.LinUntilOpts(2, 8, 0, 0, 0.0, 0.0)), None, None) == 0      # trace and info may be NULL
    twin.iterate(2)
    assert same(state(a), state(twin))


def test_robust_call_marks_the_joint_stale_like_robustify():
    """After robust sweeps the next solve describes the joint at the new weights, as after iterate(n, robustify=True)."""
    g = GRAPHS['toy_d3_outliers']
    a, b = engine(g, True), engine(g, True)
    a.solve_map(); b.solve_map()
    a.iterate_until(7, robustify=True)
    b.iterate(7, robustify=True)
    assert b.weights()[1].any()
    assert np.array_equal(a.solve_map()[0], b.solve_map()[0])


# ---- 6. max_iters runs out -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('check_every', [1, 8])
@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_running_out_of_sweeps_is_not_an_error(name, check_every):
    rows, s, _, _ = recorded(name, False)
    a, c = engine(GRAPHS[name]), engine(GRAPHS[name])
    n = s - 1                                                # one sweep short of where this tolerance would have been met
    rc, trace, info = raw(a, n, check_every, 0, TRACE_ENERGY, tol_step=rows[s - 1, 0], rows=n + 2)
    c.iterate(n)
    assert rc == 0 and (info.iters, info.converged, info.reason) == (n, 0, STOP_NONE)
    assert same(state(a), state(c)) and np.array_equal(trace[:n, 0], rows[:n, 0]) and np.all(trace[n:] == SENTINEL)


# ---- 7. every d, and the wave and block edges of the gated and traced stages ----------------------------------------------------------

def stage_cases():
    """(d, N): for every d, N one short of two whole waves of the belief stage (64 // (d + d(d+1)/2) variables each), exactly two, and
    one over; and d = 1 with N = 131, whose F = 259 factors cross the 64-factor wave of the factor stage (a tail of 3) and the
    256-factor block of the energy and robustify stages."""
    out = []
    for d in range(1, 7):
        vpw = 64 // (d + d * (d + 1) // 2)
        out += [(d, 2 * vpw - 1), (d, 2 * vpw), (d, 2 * vpw + 1)]
    return out + [(1, 131)]


def skip_chain(d, N):
    """lin_until_cases.displacement on the chain with skips: factors (i, i + 1) and (i, i + 2), three of the measurements outliers."""
    rs = np.random.RandomState(100 * d + N)
    return displacement(f'chain_d{d}_n{N}', np.concatenate([np.arange(N - 1), np.arange(N - 2)]), np.concatenate([np.arange(1, N), np.arange(2, N)]),
                        rs.rand(N, d) * 10, 0.5, 7 * d + N, outliers=3)


@pytest.mark.parametrize('robust', [False, True])
@pytest.mark.parametrize('d,N', stage_cases())
def test_every_d_at_the_wave_and_block_edges_matches_the_plain_sweeps_on_a_twin(d, N, robust):
    """The gated and traced forms of every stage against the plain ones, for every d the engine is instantiated for: A makes four
    sweeps in one call with both extra columns, B four calls of one plain sweep each."""
    g = skip_chain(d, N)
    assert len(g['va']) == 2 * N - 3 and N <= 131
    a, b = engine(g, robust), engine(g, robust)
    a.solve_map(); b.solve_map()
    rc, trace, info = raw(a, 4, 8, int(robust), TRACE_ENERGY | TRACE_MAP)
    rows = host_loop(b, 4, robust)
    assert rc == 0 and info.iters == 4 and info.reason == STOP_NONE
    assert same(state(a), state(b))
    assert np.array_equal(trace[:, 0], rows[:, 0])
    for i in range(4):
        assert close(trace[i, 1], rows[i, 1]), f"sweep {i + 1}: energy {trace[i, 1]!r} vs {rows[i, 1]!r}"
        assert close(trace[i, 2], rows[i, 2]), f"sweep {i + 1}: distance {trace[i, 2]!r} vs {rows[i, 2]!r}"
    if robust:
        assert a.weights()[1].any() and np.any(a.weights()[0] != 1.0)      # the outliers did their work: weights other than 1
