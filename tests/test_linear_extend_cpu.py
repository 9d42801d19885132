"""Growing a live linear graph (include/gbp_lin.h: gbp_lin_extend / gbp_lin_get_sizes) on a CPU: the C ABI boundary, the grown numpy
oracle of tests/lin_extend_cases.py against the reference's own staged run (fixture G23), and the engine's placement routines
(gbp_amd/csrc/gbp_lin_extend.hpp) compiled for the host through tests/hostmath/lin_extend_shim.hip against np.lexsort.  The GPU side
is tests/test_linear_extend_gpu.py."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, golden
from lin_extend_cases import TOL, csr, full_graph, grow, schedules
from lin_map_cases import rel
from oracle.linear_oracle import LinearOracleBatched

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostmath', 'lin_extend_shim.hip')
LIB = os.path.join(HERE, 'hostmath', 'liblin_extend_shim.so')
CSRC = os.path.join(REPO, 'gbp_amd', 'csrc')
SCHEDULES = schedules()


def hipcc():
    return shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def capi():
    from gbp_amd import build, _capi
    build.build()
    return _capi


def test_extend_symbols_are_declared_exported_and_bound(capi):
    lib = capi.load()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'gbp_lin.h')).read(), flags=re.S)
    ip, vp = ct.POINTER(ct.c_int32), ct.c_void_p
    want = {'gbp_lin_extend': [vp, vp], 'gbp_lin_get_sizes': [vp, ip, ip]}
    for name, args in want.items():
        assert re.search(r'\bint\s+%s\s*\(' % name, header), f"{name} is not declared in include/gbp_lin.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert capi.SIGNATURES[name] == (ct.c_int, args)
    assert re.search(r'\}\s*gbp_lin_extend_desc_t\s*;', header)
    dp = ct.POINTER(ct.c_double)
    assert [(n, t) for n, t in capi.LinExt._fields_] == [
        ('n_new_vars', ct.c_int32), ('n_new_factors', ct.c_int32), ('var_a', ip), ('var_b', ip), ('factor_eta', dp), ('factor_lam', dp),
        ('factor_const', dp), ('prior_eta', dp), ('prior_lam', dp), ('loss', ip), ('threshold', dp), ('noise_var', dp)]
    assert 'gbp_lin_capi_extend.hip' in __import__('gbp_amd.build', fromlist=['SOURCES']).SOURCES


def test_extend_entry_points_refuse_a_null_handle(capi):
    lib = capi.load()
    d = capi.LinExt()
    n, f = ct.c_int32(), ct.c_int32()
    assert lib.gbp_lin_extend(None, ct.byref(d)) == -1
    assert b'NULL handle' in lib.gbp_last_error()
    assert lib.gbp_lin_get_sizes(None, ct.byref(n), ct.byref(f)) == -1
    assert b'NULL handle' in lib.gbp_last_error()


def test_linear_engine_has_the_extend_methods(capi):
    import inspect
    from gbp_amd.linear import LinearEngine
    for m in ('extend', 'sizes', 'extend_from_factor_graph'):
        assert callable(getattr(LinearEngine, m))
    par = inspect.signature(LinearEngine.extend).parameters
    assert list(par)[1:] == ['var_a', 'var_b', 'factor_eta', 'factor_lam', 'prior_eta', 'prior_lam', 'factor_const', 'loss', 'threshold', 'noise_var']
    assert par['threshold'].default == 2.0 and par['loss'].default is None


# ---- the grown oracle against the reference --------------------------------------------------------------------------------------------

def test_grown_oracle_reproduces_the_reference_staged_run():
    """Fixture G23: ndim_posegraph.py's graph (n = 50, dim = 3, M = 5) built by the reference's classes for 30 variables, swept 10
    times, grown by 10 variables and their factors, update_all_beliefs(), 10 sweeps, and again.  Means and beliefs right after every
    growth and after its sweeps, and the energy."""
    g = golden('G23_toy_linear_grown')
    va, vb, z, pe, pl = g['va'], g['vb'], g['meas'], g['prior_eta'], g['prior_lam']
    D = pe.shape[1]
    J = np.hstack([-np.eye(D), np.eye(D)])
    fe, fl, fc = z @ J, np.tile(J.T @ J, (len(va), 1, 1)), 0.5 * np.einsum('fd,fd->f', z, z)      # sigma = 1
    o, n0, f0 = None, 0, 0
    for s, (n, f) in enumerate(zip(g['stage_n'], g['stage_f'])):
        assert np.all(np.maximum(va[f0:f], vb[f0:f]) < n) and f > f0
        if o is None:
            o = LinearOracleBatched(va[:f], vb[:f], fe[:f], fl[:f], pe[:n], pl[:n], factor_const=fc[:f])
            o.update_all_beliefs()
        else:
            o = grow(o, va[f0:f], vb[f0:f], fe[f0:f], fl[f0:f], pe[n0:n], pl[n0:n], fc[f0:f])
        assert (o.N, o.F) == (n, f)
        assert rel(o.get_means(), g[f's{s}_grown_means']) < TOL
        assert rel(o.beliefs()[0], g[f's{s}_grown_bel_eta']) < TOL and rel(o.beliefs()[1], g[f's{s}_grown_bel_lam']) < TOL
        o.iterate(10)
        assert rel(o.get_means(), g[f's{s}_means']) < TOL, f"stage {s}: means {rel(o.get_means(), g[f's{s}_means']):.3e}"
        assert rel(o.beliefs()[0], g[f's{s}_bel_eta']) < TOL and rel(o.beliefs()[1], g[f's{s}_bel_lam']) < TOL
        want = float(g[f's{s}_energy'])
        assert abs(o.energy() - want) <= TOL * abs(want), f"stage {s}: energy {o.energy()!r} vs {want!r}"
        n0, f0 = n, f
    assert (o.N, o.F) == (50, len(va))


def test_grow_keeps_old_beliefs_bit_identical():
    """The helper itself, not the engine: grow() carries the messages over so that an old variable's belief in the ORACLE adds the
    same messages in the same order, then zeros.  (The engine's side of this is asserted in tests/test_linear_extend_gpu.py.)"""
    name, N0, (va, vb), steps, damping = SCHEDULES[0]
    rs = np.random.RandomState(1)
    from lin_extend_cases import generic_fc, random_priors
    o = LinearOracleBatched(va, vb, *generic_fc(rs, 3, len(va))[:2], *random_priors(rs, N0, 3), eta_damping=damping)
    o.update_all_beliefs(); o.iterate(3)
    _, a, b = steps[2]                                     # ids in [0, N0 + 4)
    fe, fl, fc = generic_fc(rs, 3, len(a))
    g = grow(o, a, b, fe, fl, *random_priors(rs, 4, 3), fc)
    assert np.array_equal(g.bel_eta[:N0], o.bel_eta) and np.array_equal(g.bel_lam[:N0], o.bel_lam) and np.array_equal(g.mu[:N0], o.mu)
    assert np.array_equal(g.bel_eta[N0:], g.pe[N0:])


# ---- the engine's placement routines on the host ----------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def shim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ('gbp_lin_extend.hpp', 'gbp_lin_handle.hpp', 'gbp_math.hpp')]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        tmp = f'{LIB}.{os.getpid()}.tmp'
        subprocess.check_call([hipcc(), '--offload-host-only', '-O1', '-std=c++17', '-shared', '-fPIC', '-o', tmp, SRC])
        os.replace(tmp, LIB)
    so = ct.CDLL(LIB)
    i, ip = ct.c_int, ct.POINTER(ct.c_int32)
    so.lin_extend_place.argtypes, so.lin_extend_place.restype = [i, i, i, i] + [ip] * 11, None
    so.lin_extend_lower_bound.argtypes, so.lin_extend_lower_bound.restype = [ip, i, i], i
    return so


def place(so, N, va, vb, dN, a, b):
    """The shim on one growth step of the graph (N, va, vb), whose CSR is the lexsort one: (vptr, vadj, epos_a, epos_b, enew)."""
    ip = ct.POINTER(ct.c_int32)
    F, dF = len(va), len(a)
    vptr, vadj, _, _ = csr(N, va, vb)
    arr = lambda x, n: np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.int32), np.zeros(max(n - len(x), 0), dtype=np.int32)]))
    ins = [arr(va, 1), arr(vb, 1), arr(vptr, 1), arr(vadj, 1), arr(a, 1), arr(b, 1)]
    outs = [np.full(max(n, 1), -1, dtype=np.int32) for n in (N + dN + 1, 2 * (F + dF), F + dF, F + dF, 2 * F)]
    so.lin_extend_place(N, F, dN, dF, *[x.ctypes.data_as(ip) for x in ins + outs])
    return [o[:n] for o, n in zip(outs, (N + dN + 1, 2 * (F + dF), F + dF, F + dF, 2 * F))]


@pytest.mark.parametrize('sched', SCHEDULES, ids=[s[0] for s in SCHEDULES])
def test_host_placement_matches_lexsort_step_by_step(shim, sched):
    """After every step of every schedule: vptr, vadj, epos_a, epos_b exactly those of np.lexsort((factor, variable)) on the grown
    graph, and every old edge -- the row of vmsg that moves with it -- at the position its (factor, side) has there."""
    _, N, (va, vb), steps, _ = sched
    va, vb = np.asarray(va, dtype=np.int64), np.asarray(vb, dtype=np.int64)
    for dN, a, b in steps:
        vptr, vadj, ea, eb, enew = place(shim, N, va, vb, dN, a, b)
        _, old_adj, old_ea, old_eb = csr(N, va, vb)
        N, va, vb = N + dN, np.concatenate([va, a]), np.concatenate([vb, b])
        wptr, wadj, wea, web = csr(N, va, vb)
        assert np.array_equal(vptr, wptr) and np.array_equal(vadj, wadj) and np.array_equal(ea, wea) and np.array_equal(eb, web)
        F0 = len(old_ea)
        assert np.array_equal(enew[old_ea], wea[:F0]) and np.array_equal(enew[old_eb], web[:F0])
        assert np.array_equal(vadj[enew], old_adj)
    assert (N, len(va)) == full_graph(sched)[:1] + (len(full_graph(sched)[1]),)


def test_host_placement_on_random_growth(shim):
    """200 random steps on one graph, from empty: sizes 0..40 of both kinds, ids anywhere in the grown range."""
    rs = np.random.RandomState(23)
    N, va, vb = 0, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    for step in range(200):
        dN = int(rs.randint(0, 5)) if N else 2 + int(rs.randint(0, 5))
        dF = int(rs.randint(0, 41)) if step % 7 else 0
        a = rs.randint(0, N + dN, dF)
        b = (a + 1 + rs.randint(0, N + dN - 1, dF)) % (N + dN)
        vptr, vadj, ea, eb, enew = place(shim, N, va, vb, dN, a, b)
        N, va, vb = N + dN, np.concatenate([va, a]), np.concatenate([vb, b])
        wptr, wadj, wea, web = csr(N, va, vb)
        assert np.array_equal(vptr, wptr) and np.array_equal(vadj, wadj) and np.array_equal(ea, wea) and np.array_equal(eb, web), f"step {step}"
        F0 = len(va) - dF
        assert np.array_equal(enew[csr(N - dN, va[:F0], vb[:F0])[2]], wea[:F0])


def test_host_lower_bound(shim):
    ip = ct.POINTER(ct.c_int32)
    keys = np.array([0, 0, 2, 2, 2, 5, 9], dtype=np.int32)
    for v in range(-1, 12):
        assert shim.lin_extend_lower_bound(keys.ctypes.data_as(ip), len(keys), v) == int(np.searchsorted(keys, v, side='left'))
    assert shim.lin_extend_lower_bound(keys.ctypes.data_as(ip), 0, 3) == 0
