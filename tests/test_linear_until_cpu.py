"""gbp_lin_iterate_until (include/gbp_lin.h) on a CPU: the C ABI boundary, the numpy model of tests/lin_until_cases.py, the engine's
per-variable and finishing routines (gbp_amd/csrc/gbp_lin_until.hpp) compiled for the host through tests/hostmath/lin_until_shim.hip
against that model, and -- on the oracle alone -- the proof that every graph of tests/test_linear_until_gpu.py has a deciding sweep
its freeze tests can use.  The GPU side is tests/test_linear_until_gpu.py."""
import ctypes as ct
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from lin_until_cases import (FIN_THREADS, MAX_S, STOP_MAP, STOP_NONE, STOP_STEP, TRACE_ENERGY, TRACE_MAP, decide, emulate_finish_sum, graphs, map_of,
                             oracle, run_model, step_of, usable_sweep)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostmath', 'lin_until_shim.hip')
LIB = os.path.join(HERE, 'hostmath', 'liblin_until_shim.so')
CSRC = os.path.join(REPO, 'gbp_amd', 'csrc')
GRAPHS = graphs()


def hipcc():
    return shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def capi():
    from gbp_amd import build, _capi
    build.build()
    return _capi


def test_until_symbol_is_declared_exported_and_bound(capi):
    lib = capi.load()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'gbp_lin.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+gbp_lin_iterate_until\s*\(', header)
    assert hasattr(lib, 'gbp_lin_iterate_until')
    res, args = capi.SIGNATURES['gbp_lin_iterate_until']
    assert res is ct.c_int and args == [ct.c_void_p, ct.c_void_p, ct.POINTER(ct.c_double), ct.c_void_p]
    for name, code in (('TRACE_ENERGY', 1), ('TRACE_MAP', 2), ('STOP_NONE', 0), ('STOP_STEP', 1), ('STOP_MAP', 2)):
        assert re.search(r'#define\s+GBP_LIN_%s\s+%d\b' % (name, code), header)
        assert getattr(capi, 'LIN_' + name) == code
    assert ct.sizeof(capi.LinUntilOpts) == 32 and ct.sizeof(capi.LinUntilInfo) == 16
    assert [f for f, _ in capi.LinUntilOpts._fields_] == ['max_iters', 'check_every', 'robustify', 'want', 'tol_step', 'tol_map']
    assert 'gbp_lin_capi_until.hip' in __import__('gbp_amd.build', fromlist=['SOURCES']).SOURCES


def test_until_refuses_a_null_handle(capi):
    lib = capi.load()
    o = capi.LinUntilOpts(1, 1, 0, 0, 0.0, 0.0)
    assert lib.gbp_lin_iterate_until(None, ct.byref(o), None, None) == -1
    assert b'NULL handle' in lib.gbp_last_error()


def test_linear_engine_has_iterate_until(capi):
    from gbp_amd.linear import LinearEngine
    p = inspect.signature(LinearEngine.iterate_until).parameters
    assert list(p) == ['self', 'max_iters', 'tol_step', 'tol_map', 'energy', 'map_distance', 'robustify', 'check_every']
    assert [p[k].default for k in list(p)[2:]] == [0.0, 0.0, False, False, False, 8]


# ---- the model ------------------------------------------------------------------------------------------------------------------------

def test_model_stop_rule():
    assert decide(1.0, 1.0, 0.0, 0.0) == STOP_NONE                       # both off
    assert decide(0.5, 9.0, 0.5, 0.0) == STOP_STEP and decide(np.nextafter(0.5, 1), 9.0, 0.5, 0.0) == STOP_NONE     # <=, not <
    assert decide(9.0, 0.5, 0.0, 0.5) == STOP_MAP and decide(9.0, None, 0.0, 0.5) == STOP_NONE
    assert decide(0.1, 0.1, 0.5, 0.5) == STOP_STEP                       # STEP is tested first
    assert decide(0.0, 0.0, 0.0, 0.0) == STOP_NONE                       # a tolerance of 0 is off, even at a step of exactly 0


@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_model_is_the_host_loop(name):
    """run_model's rows are what the loop iterate(1); get_means(); energy(); distance gives on a second oracle, and its state after
    a stop is the state after that many plain sweeps."""
    g = GRAPHS[name]
    x = map_of(g)
    a, b = oracle(g), oracle(g)
    rows, iters, reason = run_model(a, 12, x_map=x)
    assert iters == 12 and reason == STOP_NONE
    for i in range(12):
        old = b.mu.copy()
        b.synchronous_iteration()
        assert rows[i, 0] == step_of(b.mu, old) and rows[i, 1] == b.energy() and rows[i, 2] == np.linalg.norm(b.mu - x)
    c, d = oracle(g), oracle(g)
    rows2, iters2, reason2 = run_model(c, 12, tol_step=rows[6, 0], x_map=x)
    d.iterate(iters2)
    assert reason2 == STOP_STEP and iters2 <= 7 and np.array_equal(rows2, rows[:iters2]) and np.array_equal(c.mu, d.mu)


@pytest.mark.parametrize('robust', [False, True])
@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_every_gpu_graph_has_a_usable_deciding_sweep(name, robust):
    """What tests/test_linear_until_gpu.py's freeze tests rest on, proved on the oracle alone: a sweep s <= 40, no multiple of 3 or
    8, whose step is strictly below every earlier step, so that tol_step = step_s stops exactly there; the same for the MAP distance
    (plain sweeps); and the graph is healthy."""
    g = GRAPHS[name]
    x = map_of(g)
    o = oracle(g, 'huber' if robust else None)
    rows, _, _ = run_model(o, MAX_S, x_map=x, robustify=robust)
    assert np.all(np.isfinite(rows)) and np.max(np.abs(o.mu)) < 1e3
    for col, tol_name in ((0, 'tol_step'),) + (() if robust else ((2, 'tol_map'),)):
        s = usable_sweep(rows[:, col])
        assert s is not None and s <= MAX_S and s % 3 and s % 8, f"{name}: column {col} has no usable sweep"
        assert all(rows[s - 1, col] < v for v in rows[:s - 1, col])
        assert rows[s - 1, col] > 1e-9                       # far above rounding: the device's own sequence decides the same way
        o2 = oracle(g, 'huber' if robust else None)
        _, iters, reason = run_model(o2, MAX_S, x_map=x, robustify=robust, **{tol_name: rows[s - 1, col]})
        assert iters == s and reason == (STOP_STEP if col == 0 else STOP_MAP)
    if not robust:                                           # a sweep that meets both tolerances for the first time: STEP wins
        s = usable_sweep(rows[:, 0], rows[:, 2])
        assert s is not None, f"{name}: no sweep at which step and distance are both below all earlier ones"
        o3 = oracle(g)
        _, iters, reason = run_model(o3, MAX_S, x_map=x, tol_step=rows[s - 1, 0], tol_map=rows[s - 1, 2])
        assert iters == s and reason == STOP_STEP


# ---- the engine's routines on the host --------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def shim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ('gbp_lin_until.hpp', 'gbp_lin_sweep.hpp', 'gbp_lin_robust.hpp', 'gbp_lin_handle.hpp', 'gbp_math.hpp')]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        tmp = f'{LIB}.{os.getpid()}.tmp'
        subprocess.check_call([hipcc(), '--offload-host-only', '-O1', '-std=c++17', '-shared', '-fPIC', '-o', tmp, SRC])
        os.replace(tmp, LIB)
    so = ct.CDLL(LIB)
    i, d, dp = ct.c_int, ct.c_double, ct.POINTER(ct.c_double)
    so.lin_until_threads.argtypes, so.lin_until_threads.restype = [], i
    so.lin_until_vars.argtypes, so.lin_until_vars.restype = [i, i, dp, dp, dp, dp, dp], None
    so.lin_until_finish.argtypes, so.lin_until_finish.restype = [i, dp, i, dp, i, d, d, dp], i
    return so


def _dp(a):
    return None if a is None else a.ctypes.data_as(ct.POINTER(ct.c_double))


def host_finish(so, step_part, sq_part, en_part, want, tol_step=0.0, tol_map=0.0):
    bel = np.ascontiguousarray(np.concatenate([step_part, sq_part, [0.0]]))
    en = np.ascontiguousarray(np.concatenate([en_part, [0.0]]))
    row = np.zeros(3)
    reason = so.lin_until_finish(len(step_part), _dp(bel), len(en_part), _dp(en), want, tol_step, tol_map, _dp(row))
    return row, reason


def test_shim_reports_the_thread_count_the_cases_assume(shim):
    assert shim.lin_until_threads() == FIN_THREADS


@pytest.mark.parametrize('D', [1, 2, 3, 4, 5, 6])
def test_host_per_variable_values(shim, D):
    rs = np.random.RandomState(60 + D)
    n = 50
    new, old, x = rs.randn(n, D), rs.randn(n, D), rs.randn(n, D)
    old[3] = new[3]                                          # a variable that did not move: step exactly 0
    step, sq = np.zeros(n), np.zeros(n)
    shim.lin_until_vars(D, n, _dp(new), _dp(old), _dp(x), _dp(step), _dp(sq))
    assert np.array_equal(step, np.max(np.abs(new - old), axis=1)) and step[3] == 0.0
    assert np.allclose(sq, np.sum((new - x) ** 2, axis=1), rtol=1e-14, atol=0)
    shim.lin_until_vars(D, n, _dp(new), _dp(old), None, _dp(step), _dp(sq))
    assert np.array_equal(sq, np.zeros(n))
    new[7, D - 1] = np.nan                                   # a NaN mean is not dropped (numpy's max keeps it too)
    shim.lin_until_vars(D, n, _dp(new), _dp(old), None, _dp(step), _dp(sq))
    assert np.isnan(step[7]) and not np.isnan(np.delete(step, 7)).any()


@pytest.mark.parametrize('nb', [0, 1, 5, FIN_THREADS - 1, FIN_THREADS, FIN_THREADS + 1, 2 * FIN_THREADS + 77,
                                7 * FIN_THREADS, 7 * FIN_THREADS + 1, 8 * FIN_THREADS + 5, 17 * FIN_THREADS + 300])
def test_host_finish_at_partial_counts_around_the_block(shim, nb):
    """Partial counts below, equal to and above the finishing block's thread count, and below, at and above the 7 x that from which a
    thread's strided loop takes eight partials at a time (one batch, one batch and a tail, two batches and a tail); the largest step
    in every slot that a strided loop, a batch or a tree could drop: first, last, the last slot of the first round, the first of the
    second, the last slot of a batch's first and last rounds, the first slot behind the batches (the tail)."""
    rs = np.random.RandomState(nb)
    ne = max(nb // 3, 1) if nb else 0
    if nb > 7 * FIN_THREADS:
        ne = nb - 3                                          # the energy column through the batched loop too, with another count
    sq, en = rs.rand(nb), rs.rand(ne) * 100
    both = TRACE_ENERGY | TRACE_MAP
    batches = (nb - 7 * FIN_THREADS + 8 * FIN_THREADS - 1) // (8 * FIN_THREADS) if nb > 7 * FIN_THREADS else 0    # of thread 0
    slots = {0, nb - 1, FIN_THREADS - 1, FIN_THREADS, 7 * FIN_THREADS, 8 * FIN_THREADS - 1, 8 * FIN_THREADS, 8 * FIN_THREADS * batches, 8 * FIN_THREADS * batches + 3}
    for at in sorted(slots & set(range(nb))) or [None]:
        step = rs.rand(nb)
        if at is not None:
            step[at] = 3.5
        row, reason = host_finish(shim, step, sq, en, both)
        assert row[0] == (np.max(step) if nb else 0.0) and reason == STOP_NONE
        assert row[1] == emulate_finish_sum(en) and row[2] == np.sqrt(emulate_finish_sum(sq))       # the kernel's own order, bit for bit
        assert abs(row[1] - np.sum(en)) <= 1e-12 * max(np.sum(en), 1) and abs(row[2] - np.sqrt(np.sum(sq))) <= 1e-12 * max(np.sqrt(np.sum(sq)), 1)
    row, reason = host_finish(shim, rs.rand(nb), sq, en, 0)
    assert np.isnan(row[1]) and np.isnan(row[2]) and reason == STOP_NONE                            # columns not asked for


def test_host_finish_decides_like_the_model(shim):
    rs = np.random.RandomState(4)
    step, sq, en = rs.rand(300), rs.rand(300), rs.rand(40)
    m, dist = float(np.max(step)), float(np.sqrt(emulate_finish_sum(sq)))
    both = TRACE_ENERGY | TRACE_MAP
    for tol_step, tol_map in ((0.0, 0.0), (m, 0.0), (np.nextafter(m, 0), 0.0), (0.0, dist), (0.0, np.nextafter(dist, 0)), (m, dist), (np.nextafter(m, 0), dist)):
        _, reason = host_finish(shim, step, sq, en, both, tol_step, tol_map)
        assert reason == decide(m, dist, tol_step, tol_map), (tol_step, tol_map)
    _, reason = host_finish(shim, np.zeros(0), np.zeros(0), np.zeros(0), TRACE_ENERGY, 1e-300, 0.0)
    assert reason == STOP_STEP                               # no variables: the step is 0 and any positive tol_step is met


@pytest.mark.parametrize('name', sorted(GRAPHS))
def test_host_routines_reproduce_the_model_rows(shim, name):
    """Every sweep of the model: the per-variable routine over the oracle's old and new means, grouped into the belief stage's blocks
    (64 / (d + P) variables each), then the finishing routine: the step bit for bit, the distance to rounding."""
    g = GRAPHS[name]
    x = map_of(g)
    o = oracle(g)
    D = o.D
    vpw = 64 // (D + D * (D + 1) // 2)
    for _ in range(8):
        old = o.mu.copy()
        o.synchronous_iteration()
        step, sq = np.zeros(o.N), np.zeros(o.N)
        shim.lin_until_vars(D, o.N, _dp(np.ascontiguousarray(o.mu)), _dp(old), _dp(np.ascontiguousarray(x)), _dp(step), _dp(sq))
        blocks = [slice(b, b + vpw) for b in range(0, o.N, vpw)]
        row, _ = host_finish(shim, np.array([step[b].max() for b in blocks]), np.array([sq[b].sum() for b in blocks]), np.array([o.energy()]), TRACE_ENERGY | TRACE_MAP)
        assert row[0] == step_of(o.mu, old)
        assert row[1] == o.energy() and abs(row[2] - np.linalg.norm(o.mu - x)) <= 1e-12 * max(np.linalg.norm(o.mu - x), 1)


def test_host_routines_under_address_and_undefined_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main), compiled with the host sanitizers and run as a process of its own."""
    exe = str(tmp_path / 'lin_until_main')
    subprocess.check_call([hipcc(), '--offload-host-only', '-O1', '-g', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', '-DLIN_UNTIL_SHIM_MAIN', '-o', exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and 'lin_until_shim OK' in r.stdout, out[-3000:]
    assert 'AddressSanitizer' not in out and 'runtime error:' not in out, out[-3000:]
