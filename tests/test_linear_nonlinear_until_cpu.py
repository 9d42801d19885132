"""gbp_lin_iterate_until_nonlinear (include/gbp_lin.h) on a CPU: the C ABI boundary; on the numpy model of
tests/lin_nonlin_until_cases.py alone, the proof that every case the freeze tests of tests/test_linear_nonlinear_until_gpu.py use has a
deciding sweep clear of both discontinuous tests of a sweep, and the SETTLED cases; and the engine's decision routine
(until_row_settled, gbp_amd/csrc/gbp_lin_until.hpp) compiled for the host through tests/hostmath/lin_nonlin_until_shim.hip against that
model."""
import ctypes as ct
import inspect
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO
from lin_nonlin_until_cases import (BETA0_TOL, FREEZE, MARGIN, SETTLED_PAIRS, STOP_MAP, STOP_NONE, STOP_STEP, TRACE_ENERGY, TRACE_MAP, UNTIL_SETTLED, case, decide,
                                    freeze_sweep, run_model, settled_decide, twin)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostmath', 'lin_nonlin_until_shim.hip')
LIB = os.path.join(HERE, 'hostmath', 'liblin_nonlin_until_shim.so')
CSRC = os.path.join(REPO, 'gbp_amd', 'csrc')


def hipcc():
    return shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def capi():
    from gbp_amd import build, _capi
    build.build()
    return _capi


def test_symbol_is_declared_exported_and_bound(capi):
    lib = capi.load()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'gbp_lin.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+gbp_lin_iterate_until_nonlinear\s*\(', header)
    assert hasattr(lib, 'gbp_lin_iterate_until_nonlinear')
    res, args = capi.SIGNATURES['gbp_lin_iterate_until_nonlinear']
    ip, dp = ct.POINTER(ct.c_int32), ct.POINTER(ct.c_double)
    assert res is ct.c_int and args == [ct.c_void_p, ct.c_void_p, dp, ip, ip, ct.c_void_p]
    assert re.search(r'#define\s+GBP_LIN_UNTIL_SETTLED\s+4\b', header) and capi.LIN_UNTIL_SETTLED == 4
    assert ct.sizeof(capi.LinUntilOpts) == 32 and ct.sizeof(capi.LinUntilInfo) == 16
    assert [f for f, _ in capi.LinUntilOpts._fields_] == ['max_iters', 'check_every', 'robustify', 'want', 'tol_step', 'tol_map']
    assert 'gbp_lin_capi_until_nonlin.hip' in __import__('gbp_amd.build', fromlist=['SOURCES']).SOURCES


def test_refuses_a_null_handle(capi):
    lib = capi.load()
    o = capi.LinUntilOpts(1, 1, 0, 0, 0.0, 0.0)
    assert lib.gbp_lin_iterate_until_nonlinear(None, ct.byref(o), None, None, None, None) == -1
    assert b'NULL handle' in lib.gbp_last_error()


def test_linear_engine_has_iterate_until_nonlinear(capi):
    from gbp_amd.linear import LinearEngine, UntilResult
    p = inspect.signature(LinearEngine.iterate_until_nonlinear).parameters
    assert list(p) == ['self', 'max_iters', 'tol_step', 'tol_map', 'energy', 'map_distance', 'robustify', 'settled', 'check_every']
    assert [p[k].default for k in list(p)[2:]] == [0.0, 0.0, False, False, False, False, 8]
    q = inspect.signature(LinearEngine.iterate_until).parameters               # the linear call keeps its exact parameter list
    assert list(q) == ['self', 'max_iters', 'tol_step', 'tol_map', 'energy', 'map_distance', 'robustify', 'check_every']
    r = inspect.signature(UntilResult.__init__).parameters
    assert list(r) == ['self', 'iters', 'converged', 'reason', 'step', 'energy', 'map_distance', 'relin_counts', 'robust_counts']
    assert r['relin_counts'].default is None and r['robust_counts'].default is None
    old = UntilResult(3, True, 1, None, None, None)                             # six positional parameters still construct it
    assert old.relin_counts is None and old.robust_counts is None


# ---- the model ------------------------------------------------------------------------------------------------------------------------

def test_model_settled_rule():
    assert settled_decide(0.1, None, 0.5, 0.0, 0, True) == STOP_STEP and settled_decide(0.1, None, 0.5, 0.0, 3, True) == STOP_NONE
    assert settled_decide(0.1, None, 0.5, 0.0, 3, False) == STOP_STEP            # bit clear: the count is not looked at
    assert settled_decide(9.0, 0.1, 0.0, 0.5, 1, True) == STOP_NONE and settled_decide(9.0, 0.1, 0.0, 0.5, 0, True) == STOP_MAP
    assert settled_decide(0.1, 0.1, 0.5, 0.5, 0, True) == STOP_STEP              # STEP before MAP


@pytest.mark.parametrize('robust', [False, True])
@pytest.mark.parametrize('name', FREEZE)
def test_every_freeze_case_has_a_usable_deciding_sweep(name, robust):
    """What the freeze tests of the GPU file rest on, on the twin alone: a deciding sweep s, no multiple of 3 or 8, whose step is a
    strict minimum so far, and a run that stays >= MARGIN clear of `dist > beta` and of `M > t` before every sweep up to s."""
    s, tol, rows, rc, fc, robust_margin, dist_margin = freeze_sweep(name, robust)
    assert s is not None, f"{name}: no usable sweep"
    assert s % 3 != 0 and s % 8 != 0 and all(rows[s - 1, 0] < v for v in rows[:s - 1, 0])
    assert rows[s - 1, 0] > 1e-9                              # far above rounding: the device's own sequence decides the same way
    assert dist_margin >= MARGIN and robust_margin >= MARGIN, f"{name}: margins {dist_margin:.3e} (dist > beta), {robust_margin:.3e} (M > t)"
    assert np.all(np.isfinite(rows[:, :2]))
    g, sched = case(name, robust)
    a, b = twin(g, sched), twin(g, sched)
    rows2, rc2, fc2, iters, reason = run_model(a, 40, tol_step=tol, robustify=robust)
    assert iters == s and reason == STOP_STEP
    assert np.array_equal(rows2[:, :2], rows[:s, :2]) and np.array_equal(rc2, rc[:s]) and np.array_equal(fc2, fc[:s])
    b.iterate(s, relinearise=True, robustify=robust)          # the model's state after the stop is that of s sweeps
    assert np.array_equal(a.mu, b.mu) and np.array_equal(a.linpoint, b.linpoint) and np.array_equal(a.w, b.w)
    if robust:
        assert fc[:s].any()                                   # some factor was flagged: the losses act in the case


@pytest.mark.parametrize('name,k,plain_stop,settled_stop', SETTLED_PAIRS)
def test_settled_moves_the_deciding_sweep(name, k, plain_stop, settled_stop):
    """tol_step = the step of sweep k, in which some factor relinearises: without SETTLED the call stops there, with it at the first
    later sweep that meets the tolerance and relinearises nothing."""
    g, sched = case(name)
    rows, rc, _, _, _ = run_model(twin(g, sched), 60)
    tol = rows[k - 1, 0]
    assert rc[k - 1] > 0 and all(rows[k - 1, 0] < v for v in rows[:k - 1, 0])
    if name == 'hub9':
        assert rc[k - 1] == 6
    _, _, _, iters, reason = run_model(twin(g, sched), 60, tol_step=tol)
    assert (iters, reason) == (plain_stop, STOP_STEP)
    _, rc2, _, iters, reason = run_model(twin(g, sched), 60, tol_step=tol, settled=True)
    assert (iters, reason) == (settled_stop, STOP_STEP) and rc2[-1] == 0
    # the sweeps between met the tolerance or relinearised -- each one that met it did relinearise
    assert all(rc[i] > 0 for i in range(k - 1, settled_stop - 1) if rows[i, 0] <= tol)
    # the deciding comparisons are far from rounding: no other step within 1e-6 (relative) of the tolerance up to the settled stop
    assert min(abs(v - tol) for i, v in enumerate(rows[:settled_stop, 0]) if i != k - 1) > 1e-6 * tol


def test_beta0_never_settles():
    g, sched = case('beta0')
    rows, rc, _, iters, reason = run_model(twin(g, sched), 60, tol_step=BETA0_TOL, settled=True)
    assert rc.tolist() == [0] + [28] * 59 and (iters, reason) == (60, STOP_NONE)
    assert rows[0, 0] > 2 * BETA0_TOL and np.sum(rows[:, 0] <= BETA0_TOL) > 50
    _, _, _, iters, reason = run_model(twin(g, sched), 60, tol_step=BETA0_TOL)
    assert (iters, reason) == (4, STOP_STEP) and abs(rows[3, 0] - BETA0_TOL) > 1e-3 and abs(rows[2, 0] - BETA0_TOL) > 1e-3


# ---- the engine's decision routine on the host ------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def shim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ('gbp_lin_until.hpp', 'gbp_lin_handle.hpp', 'gbp_math.hpp')] + [os.path.join(REPO, 'include', 'gbp_lin.h')]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        tmp = f'{LIB}.{os.getpid()}.tmp'
        subprocess.check_call([hipcc(), '--offload-host-only', '-O1', '-std=c++17', '-shared', '-fPIC', '-o', tmp, SRC])
        os.replace(tmp, LIB)
    so = ct.CDLL(LIB)
    i, d, dp = ct.c_int, ct.c_double, ct.POINTER(ct.c_double)
    so.lin_nl_until_settled_bit.argtypes, so.lin_nl_until_settled_bit.restype = [], i
    so.lin_nl_until_decide.argtypes, so.lin_nl_until_decide.restype = [i, d, d, i, i, d, d, d, dp], i
    so.lin_nl_until_decide_block.argtypes, so.lin_nl_until_decide_block.restype = [i, d, d, i, d, d, d, dp], i
    so.lin_nl_until_row.argtypes, so.lin_nl_until_row.restype = [i, d, d, d, d, d, dp], i
    return so


def _row():
    r = np.full(3, -7.0)
    return r, r.ctypes.data_as(ct.POINTER(ct.c_double))


def same_row(a, b):
    return all(x == y or (np.isnan(x) and np.isnan(y)) for x, y in zip(a, b))


def test_host_decision_matches_the_model(shim):
    """count 0 and > 0, bit set and clear, pointer NULL, every combination of tolerances met and not met (STEP before MAP), columns
    asked for and not: the reason is the model's, the row is until_row's, and with the bit clear or the pointer NULL so is the reason."""
    assert shim.lin_nl_until_settled_bit() == UNTIL_SETTLED
    step, dist, en = 0.25, 0.5, 3.0
    sq = dist * dist
    for want_cols, bit, count, has, tol_step, tol_map in itertools.product(
            (0, TRACE_ENERGY, TRACE_MAP, TRACE_ENERGY | TRACE_MAP), (0, UNTIL_SETTLED), (0, 1, 257), (0, 1),
            (0.0, step, np.nextafter(step, 0)), (0.0, dist, np.nextafter(dist, 0))):
        want = want_cols | bit
        row, p = _row()
        got = shim.lin_nl_until_decide(want, tol_step, tol_map, has, count, step, sq, en, p)
        old, q = _row()
        plain = shim.lin_nl_until_row(want_cols, tol_step, tol_map, step, sq, en, q)
        assert plain == decide(step, dist if want & TRACE_MAP else None, tol_step, tol_map) != -1
        model = settled_decide(step, dist if want & TRACE_MAP else None, tol_step, tol_map, count if has else 0, bool(bit))
        assert got == model, (want, count, has, tol_step, tol_map)
        assert same_row(row, old) and row[0] == step
        assert np.isnan(row[1]) == (not want & TRACE_ENERGY) and np.isnan(row[2]) == (not want & TRACE_MAP)
        if not bit or not has:
            assert got == plain
        if has:
            blk, r = _row()
            assert shim.lin_nl_until_decide_block(want, tol_step, tol_map, count, step, sq, en, r) == got and same_row(blk, row)
    # both met in one sweep: STEP wins; a relinearising sweep under the bit decides neither
    row, p = _row()
    assert shim.lin_nl_until_decide(TRACE_MAP, 1.0, 1.0, 1, 0, step, sq, en, p) == STOP_STEP
    assert shim.lin_nl_until_decide(TRACE_MAP | UNTIL_SETTLED, 1.0, 1.0, 1, 5, step, sq, en, p) == STOP_NONE
    assert shim.lin_nl_until_decide(TRACE_MAP | UNTIL_SETTLED, 0.0, 1.0, 1, 0, step, sq, en, p) == STOP_MAP


def test_host_decision_with_a_nan_step(shim):
    """A NaN step meets no tolerance (the comparison is false), with and without the bit; the row keeps the NaN."""
    for want in (0, UNTIL_SETTLED):
        for count in (0, 2):
            row, p = _row()
            assert shim.lin_nl_until_decide(want, 1e300, 0.0, 1, count, np.nan, 0.0, 0.0, p) == STOP_NONE and np.isnan(row[0])
    row, p = _row()
    assert shim.lin_nl_until_row(0, 1e300, 0.0, np.nan, 0.0, 0.0, p) == STOP_NONE and np.isnan(row[0])
    # ... while the distance can still decide a settled sweep
    assert shim.lin_nl_until_decide(TRACE_MAP | UNTIL_SETTLED, 1e300, 1.0, 1, 0, np.nan, 0.25, 0.0, p) == STOP_MAP


@pytest.mark.parametrize('name,k,plain_stop,settled_stop', SETTLED_PAIRS)
def test_host_decision_over_a_model_run(shim, name, k, plain_stop, settled_stop):
    """The routine fed the model's steps and counts sweep by sweep stops where the model does."""
    g, sched = case(name)
    rows, rc, _, _, _ = run_model(twin(g, sched), 60)
    tol = rows[k - 1, 0]
    for bit, want_stop in ((0, plain_stop), (UNTIL_SETTLED, settled_stop)):
        row, p = _row()
        reasons = [shim.lin_nl_until_decide(bit, tol, 0.0, 1, int(rc[i]), rows[i, 0], 0.0, 0.0, p) for i in range(60)]
        assert reasons.index(STOP_STEP) + 1 == want_stop
