"""Exact marginal covariances of the linear engine (include/gbp_lin.h: gbp_lin_solve_marginals) on a CPU: the C ABI boundary, and the
solver's own per-(item, column) routines (gbp_amd/csrc/gbp_lin_marg.hpp) compiled for the host through tests/hostmath/lin_marg_shim.hip
and driven through whole multi-column block-Jacobi PCGs in plain loops, against np.linalg.inv of the dense joint.  Every right-hand
side is a unit vector and the solver stops at a true residual of 1e-12, so |x - x*|_inf <= |Lambda^-1| 1e-12 <= cond * 1e-12 * max|x*|
(max |Sigma| >= |Lambda^-1|_2 / (N d) is cruder than needed: the measured errors are printed); TOL = 1e-9 needs cond < 1e3, which this
file asserts with numpy for every graph that this file and tests/test_linear_marginals_gpu.py use.  The GPU side is that file."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, golden
from lin_map_cases import TOL, dense_joint, pack, rel, shapes
from lin_marg_cases import chain, diag_blocks, sub

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostmath', 'lin_marg_shim.hip')
LIB = os.path.join(HERE, 'hostmath', 'liblin_marg_shim.so')
CSRC = os.path.join(REPO, 'gbp_amd', 'csrc')
COND_MAX = 1e3


def hipcc():
    return shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def capi():
    from gbp_amd import build, _capi
    build.build()
    return _capi


def test_marginals_symbol_is_declared_exported_and_bound(capi):
    lib = capi.load()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'gbp_lin.h')).read(), flags=re.S)
    dp, ip, vp = ct.POINTER(ct.c_double), ct.POINTER(ct.c_int32), ct.c_void_p
    assert re.search(r'\bint\s+gbp_lin_solve_marginals\s*\(', header), "gbp_lin_solve_marginals is not declared in include/gbp_lin.h"
    assert hasattr(lib, 'gbp_lin_solve_marginals'), "gbp_lin_solve_marginals is not exported"
    res, args = capi.SIGNATURES['gbp_lin_solve_marginals']
    assert res is ct.c_int and args == [vp, ip, ct.c_int32, vp, dp, dp, vp]
    assert 'int32_t iters, converged, batches, reserved; double rel_residual;' in header
    assert re.search(r'#define\s+GBP_LIN_MARG_COLS\s+8\b', header) and capi.LIN_MARG_COLS == 8
    assert ct.sizeof(capi.LinMargInfo) == 24
    assert lib.gbp_abi_version() == 3


def test_marginals_refuse_a_null_handle(capi):
    lib = capi.load()
    out = (ct.c_double * 4)()
    ids = (ct.c_int32 * 1)(0)
    assert lib.gbp_lin_solve_marginals(None, ids, 1, None, out, None, None) == -1
    assert b'NULL handle' in lib.gbp_last_error()
    assert lib.gbp_lin_solve_marginals(None, None, 0, None, None, None, None) == -1


def test_linear_engine_has_the_marginal_methods(capi):
    from gbp_amd.linear import LinearEngine
    for m in ('marginals', 'belief_covariances'):
        assert callable(getattr(LinearEngine, m))


# ---- the solver's routines on the host ------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def shim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ('gbp_lin_marg.hpp', 'gbp_lin_map.hpp', 'gbp_lin_handle.hpp', 'gbp_math.hpp')]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        tmp = f'{LIB}.{os.getpid()}.tmp'
        subprocess.check_call([hipcc(), '--offload-host-only', '-O1', '-std=c++17', '-shared', '-fPIC', '-o', tmp, SRC])
        os.replace(tmp, LIB)
    so = ct.CDLL(LIB)
    i, d = ct.c_int, ct.c_double
    ip, dp = ct.POINTER(ct.c_int32), ct.POINTER(ct.c_double)
    so.lin_marg_solve.argtypes = [i, i, i, ip, ip, dp, dp, dp, ip, ip, ip, ip, ip, i, d, i, dp, dp, dp]
    so.lin_marg_solve.restype = i
    return so


def host_marginals(so, g, ids, joint=False, rel_tol=1e-12, max_iters=400):
    ip, dp = ct.POINTER(ct.c_int32), ct.POINTER(ct.c_double)
    D = g['D']
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    M = ids.shape[0]
    sigma = np.full((M, D, D), np.nan)
    sj = np.full((M * D, M * D), np.nan) if joint else None
    r = ct.c_double()
    args = [D, g['N'], g['F']] + [g[k].ctypes.data_as(ip) for k in ('va', 'vb')] + [g[k].ctypes.data_as(dp) for k in ('feta', 'flam', 'prior')] + \
           [g[k].ctypes.data_as(ip) for k in ('vptr', 'vadj', 'epos_a', 'epos_b')]
    it = so.lin_marg_solve(*args, ids.ctypes.data_as(ip), M, rel_tol, max_iters, sigma.ctypes.data_as(dp),
                           None if sj is None else sj.ctypes.data_as(dp), ct.byref(r))
    return sigma, sj, it, r.value


@pytest.mark.parametrize('D', [1, 2, 3, 4, 5, 6])
def test_host_multi_column_pcg_matches_the_dense_inverse(shim, D):
    """Every shape of the GPU test: all variables (N d no multiple of 8 on most: the last batch is padded, and the shim checks that
    the padded columns stay exactly zero), and the joint block over a few ids in descending order."""
    for name, va, vb, fe, fl, pe, pl in shapes(D):
        N = pe.shape[0]
        _, lam = dense_joint(va, vb, fe, fl, pe, pl)
        cond = np.linalg.cond(lam)
        assert cond < COND_MAX, f"{name}: cond {cond:.1f}"
        S = np.linalg.inv(lam)
        g = pack(va, vb, fe, fl, pe, pl)
        sigma, _, it, r = host_marginals(shim, g, np.arange(N))
        err = rel(sigma, diag_blocks(S, range(N), D))
        print(f"marginals host d={D} {name}: cond {cond:.1f} iters {it} rel_residual {r:.2e} err {err:.2e}")
        assert it >= 0 and r <= 2e-12 and err < TOL, f"{name}: {it} {r:.3e} {err:.3e}"
        ids = [N - 1, 0] if N < 4 else [N - 1, N // 2, 1, 0]
        sg, sj, it, r = host_marginals(shim, g, ids, joint=True)
        assert it >= 0 and r <= 2e-12 and rel(sj, sub(S, ids, D)) < TOL, name
        assert np.array_equal(diag_blocks(sj, range(len(ids)), D), sg), name


@pytest.mark.parametrize('D', [1, 3, 6])
def test_host_columns_far_past_convergence_stay_finite(shim, D):
    """The hub and the isolated variable of the star in one batch, against a tolerance nobody can meet: the loop ends only when every
    residual of the recurrence is exactly zero or after 1000 iterations per batch, so every column's scalars run down through the
    denormals (map_ratio gives 0 only for 0 / 0).  The answer is as exact as at 1e-12."""
    name, va, vb, fe, fl, pe, pl = next(s for s in shapes(D) if s[0] == 'star')
    N = pe.shape[0]
    ids = [N - 1, 0]
    S = np.linalg.inv(dense_joint(va, vb, fe, fl, pe, pl)[1])
    _, sj, it, r = host_marginals(shim, pack(va, vb, fe, fl, pe, pl), ids, joint=True, rel_tol=1e-300, max_iters=1000)
    print(f"marginals host d={D} star hub + isolated, rel_tol 1e-300: iters {it} rel_residual {r:.2e} err {rel(sj, sub(S, ids, D)):.2e}")
    assert it > 0 and np.isfinite(sj).all() and r <= 2e-12 and rel(sj, sub(S, ids, D)) < TOL


@pytest.mark.parametrize('n,dim,tag', [(100, 3, 'n100d3'), (50, 6, 'defaults')])
def test_host_marginals_reproduce_the_reference_sigma(shim, n, dim, tag):
    """The reference's own joint_distribution_cov sigma (fixture G21).  np.linalg.inv of the dense joint is within 1e-13 of it (printed),
    so the reference is not the looser side and the bound stays TOL."""
    from oracle.linear_oracle import toy_posegraph
    va, vb, fe, fl, _, pe, pl = toy_posegraph(n, dim, 10, 1.0, seed=0)
    g21 = golden('G21_toy_linear_sigma')
    _, lam = dense_joint(va, vb, fe, fl, pe, pl)
    cond = np.linalg.cond(lam)
    assert cond < COND_MAX
    S = np.linalg.inv(lam)
    ids = g21[f'{tag}_joint_ids']
    assert list(ids) == [0, 7, n - 1]
    ref_gap = max(rel(diag_blocks(S, range(n), dim), g21[f'{tag}_sigma_diag']), rel(sub(S, ids, dim), g21[f'{tag}_sigma_joint']))
    sigma, _, it, r = host_marginals(shim, pack(va, vb, fe, fl, pe, pl), np.arange(n))
    _, sj, _, _ = host_marginals(shim, pack(va, vb, fe, fl, pe, pl), ids, joint=True)
    print(f"marginals host G21 {tag}: cond {cond:.1f} |inv(dense) - reference| {ref_gap:.2e} iters {it} rel_residual {r:.2e} "
          f"err {rel(sigma, g21[f'{tag}_sigma_diag']):.2e} joint {rel(sj, g21[f'{tag}_sigma_joint']):.2e}")
    assert 2 * ref_gap < TOL
    assert r <= 2e-12 and rel(sigma, g21[f'{tag}_sigma_diag']) < TOL and rel(sj, g21[f'{tag}_sigma_joint']) < TOL


def test_the_chain_of_the_gpu_test_is_well_conditioned():
    va, vb, fe, fl, _, pe, pl = chain()
    _, lam = dense_joint(va, vb, fe, fl, pe, pl)
    assert np.linalg.cond(lam) < COND_MAX


def test_host_routines_under_address_and_undefined_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main: rings of every d, four ids in descending order with the joint block),
    compiled with the host sanitizers and run as a process of its own."""
    exe = str(tmp_path / 'lin_marg_main')
    subprocess.check_call([hipcc(), '--offload-host-only', '-O1', '-g', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', '-DLIN_MARG_SHIM_MAIN', '-o', exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and 'lin_marg_shim OK' in r.stdout, out[-3000:]
    assert 'AddressSanitizer' not in out and 'runtime error:' not in out, out[-3000:]
