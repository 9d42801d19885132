"""The batch MAP of the linear engine (include/gbp_lin.h: gbp_lin_joint_matvec / joint_eta / solve_map / get_map / map_distance) on a
CPU: the C ABI boundary, and the solver's own per-factor and per-variable routines (gbp_amd/csrc/gbp_lin_map.hpp) compiled for the
host through tests/hostmath/lin_map_shim.hip and driven through a whole block-Jacobi PCG in plain loops, against the dense joint
(np.linalg.solve) and a numpy PCG.  The GPU side is tests/test_linear_map_gpu.py."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, golden
from lin_map_cases import (ITER_CAP, TOL, dense_joint, numpy_pcg, pack, random_generic_graph, rel, scaled_displacement_graph,
                           shapes)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostmath', 'lin_map_shim.hip')
LIB = os.path.join(HERE, 'hostmath', 'liblin_map_shim.so')
CSRC = os.path.join(REPO, 'gbp_amd', 'csrc')
NEW = ['gbp_lin_joint_matvec', 'gbp_lin_joint_eta', 'gbp_lin_solve_map', 'gbp_lin_get_map', 'gbp_lin_map_distance']


def hipcc():
    return shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def capi():
    from gbp_amd import build, _capi
    build.build()
    return _capi


def test_map_symbols_are_declared_exported_and_bound(capi):
    lib = capi.load()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'gbp_lin.h')).read(), flags=re.S)
    dp, vp = ct.POINTER(ct.c_double), ct.c_void_p
    want = {'gbp_lin_joint_matvec': [vp, dp, dp], 'gbp_lin_joint_eta': [vp, dp], 'gbp_lin_solve_map': [vp, vp, vp],
            'gbp_lin_get_map': [vp, dp], 'gbp_lin_map_distance': [vp, dp]}
    for name in NEW:
        assert re.search(r'\bint\s+%s\s*\(' % name, header), f"{name} is not declared in include/gbp_lin.h"
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = capi.SIGNATURES[name]
        assert res is ct.c_int and args == want[name]
    assert 'double rel_tol; int32_t max_iters, check_every, warm_start;' in header
    assert 'int32_t iters, converged; double rel_residual, eta_norm;' in header
    assert ct.sizeof(capi.LinMapOpts) == 24 and ct.sizeof(capi.LinMapInfo) == 24
    assert lib.gbp_abi_version() == 3


def test_map_entry_points_refuse_a_null_handle(capi):
    lib = capi.load()
    out = (ct.c_double * 4)()
    assert lib.gbp_lin_joint_matvec(None, out, out) == -1
    assert lib.gbp_lin_joint_eta(None, out) == -1
    assert lib.gbp_lin_solve_map(None, None, None) == -1
    assert lib.gbp_lin_get_map(None, out) == -1
    assert lib.gbp_lin_map_distance(None, out) == -1
    assert b'NULL handle' in lib.gbp_last_error()


def test_linear_engine_has_the_map_methods(capi):
    from gbp_amd.linear import LinearEngine
    for m in ('joint_matvec', 'joint_eta', 'solve_map', 'map_mean', 'map_distance'):
        assert callable(getattr(LinearEngine, m))


# ---- the solver's routines on the host ------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def shim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ('gbp_lin_map.hpp', 'gbp_lin_handle.hpp', 'gbp_math.hpp')]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        tmp = f'{LIB}.{os.getpid()}.tmp'
        subprocess.check_call([hipcc(), '--offload-host-only', '-O1', '-std=c++17', '-shared', '-fPIC', '-o', tmp, SRC])
        os.replace(tmp, LIB)
    so = ct.CDLL(LIB)
    i, d = ct.c_int, ct.c_double
    ip, dp = ct.POINTER(ct.c_int32), ct.POINTER(ct.c_double)
    graph = [i, i, i, ip, ip, dp, dp, dp, ip, ip, ip, ip]
    so.lin_map_pcg.argtypes, so.lin_map_pcg.restype = graph + [d, i, dp, dp], i
    so.lin_map_joint.argtypes, so.lin_map_joint.restype = graph + [dp, dp, dp], None
    return so


def graph_args(g):
    ip, dp = ct.POINTER(ct.c_int32), ct.POINTER(ct.c_double)
    return [g['D'], g['N'], g['F']] + [g[k].ctypes.data_as(ip) for k in ('va', 'vb')] + [g[k].ctypes.data_as(dp) for k in ('feta', 'flam', 'prior')] + \
           [g[k].ctypes.data_as(ip) for k in ('vptr', 'vadj', 'epos_a', 'epos_b')]


def host_pcg(so, g, rel_tol=1e-12, max_iters=ITER_CAP):
    dp = ct.POINTER(ct.c_double)
    x, r = np.zeros((g['N'], g['D'])), ct.c_double()
    it = so.lin_map_pcg(*graph_args(g), rel_tol, max_iters, x.ctypes.data_as(dp), ct.byref(r))
    return x, it, r.value


def host_joint(so, g, x):
    dp = ct.POINTER(ct.c_double)
    x = np.ascontiguousarray(x, dtype=float)
    y, eta = np.zeros_like(x), np.zeros_like(x)
    so.lin_map_joint(*graph_args(g), x.ctypes.data_as(dp), y.ctypes.data_as(dp), eta.ctypes.data_as(dp))
    return y, eta


def check_graph(so, name, va, vb, fe, fl, pe, pl):
    N, D = pe.shape
    g = pack(va, vb, fe, fl, pe, pl)
    eta, lam = dense_joint(va, vb, fe, fl, pe, pl)
    x = np.random.RandomState(1).randn(N, D)
    y, e = host_joint(so, g, x)
    assert rel(y, lam @ x.reshape(-1)) < TOL, f"{name}: matvec {rel(y, lam @ x.reshape(-1)):.3e}"
    assert rel(e, eta) < TOL, f"{name}: eta {rel(e, eta):.3e}"
    mu, it, r = host_pcg(so, g)
    want = np.linalg.solve(lam, eta)
    _, it_np = numpy_pcg(lam, eta, D)
    print(f"MAP host d={D} {name}: cond {np.linalg.cond(lam):.1f} iters {it} (numpy {it_np}) rel_residual {r:.2e} err {rel(mu, want):.2e}")
    assert it < ITER_CAP and it_np < ITER_CAP
    assert rel(mu, want) < TOL, f"{name}: {rel(mu, want):.3e}"
    assert abs(it - it_np) <= 1, f"{name}: {it} iterations against numpy's {it_np}"
    assert r <= 2e-12


@pytest.mark.parametrize('D', [1, 2, 3, 4, 5, 6])
def test_host_pcg_matches_the_dense_solve_and_the_numpy_pcg(shim, D):
    """Every shape of the GPU test, and the random generic graph of test_random_pairwise_graphs_all_sizes."""
    for name, *g in shapes(D):
        check_graph(shim, name, *g)
    check_graph(shim, 'generic', *random_generic_graph(D))


@pytest.mark.parametrize('n,dim,key', [(100, 3, 'n100d3_map_mu'), (50, 6, 'defaults_map_mu')])
def test_host_pcg_reproduces_the_reference_map(shim, n, dim, key):
    """The reference's own joint_distribution_cov means (fixture G8)."""
    from oracle.linear_oracle import toy_posegraph
    va, vb, fe, fl, _, pe, pl = toy_posegraph(n, dim, 10, 1.0, seed=0)
    mu, it, r = host_pcg(shim, pack(va, vb, fe, fl, pe, pl))
    want = golden('G8_toy_linear')[key]
    print(f"MAP host G8 {key}: iters {it} rel_residual {r:.2e} err {rel(mu, want):.2e}")
    assert it < ITER_CAP and r <= 2e-12 and rel(mu, want) < TOL


def test_scaled_graph_is_in_the_condition_range_and_solves_on_the_host(shim):
    """The scaling case of the GPU test: 1e3 <= cond <= 1e4 as numpy reports it, means 1e6 from the origin; at rel_tol 1e-10 the
    error is within cond * 2e-10."""
    va, vb, fe, fl, pe, pl = scaled_displacement_graph()
    eta, lam = dense_joint(va, vb, fe, fl, pe, pl)
    cond = np.linalg.cond(lam)
    assert 1e3 <= cond <= 1e4, cond
    want = np.linalg.solve(lam, eta)
    assert np.min(np.abs(want)) > 9e5
    mu, it, r = host_pcg(shim, pack(va, vb, fe, fl, pe, pl), rel_tol=1e-10, max_iters=2000)
    err = np.linalg.norm(mu.reshape(-1) - want) / np.linalg.norm(want)
    print(f"MAP host scaled: cond {cond:.1f} iters {it} rel_residual {r:.2e} err {err:.2e}")
    assert r <= 2e-10 and err <= cond * 2e-10


def test_host_routines_under_address_and_undefined_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main: rings of every d through the whole PCG), compiled with the host sanitizers
    and run as a process of its own."""
    exe = str(tmp_path / 'lin_map_main')
    subprocess.check_call([hipcc(), '--offload-host-only', '-O1', '-g', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', '-DLIN_MAP_SHIM_MAIN', '-o', exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and 'lin_map_shim OK' in r.stdout, out[-3000:]
    assert 'AddressSanitizer' not in out and 'runtime error:' not in out, out[-3000:]
