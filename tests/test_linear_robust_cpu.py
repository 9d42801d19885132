"""The robust losses of the linear engine (include/gbp_lin.h: gbp_lin_set_robust / robustify / iterate_robust / get_weights) on a CPU:
the C ABI boundary, the numpy oracle of tests/lin_robust_cases.py against the reference's own run (fixture G22), and the engine's
per-factor weight routine (gbp_amd/csrc/gbp_lin_robust.hpp) compiled for the host through tests/hostmath/lin_robust_shim.hip against
that oracle.  The GPU side is tests/test_linear_robust_gpu.py."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, golden
from lin_map_cases import random_pairs, random_priors, rel
from lin_robust_cases import LOSSES, TOL, RobustOracle, g22_graph, generic_jz, mixed_losses, pack_robust, robust_weight

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostmath', 'lin_robust_shim.hip')
LIB = os.path.join(HERE, 'hostmath', 'liblin_robust_shim.so')
CSRC = os.path.join(REPO, 'gbp_amd', 'csrc')
NEW = ['gbp_lin_set_robust', 'gbp_lin_robustify', 'gbp_lin_iterate_robust', 'gbp_lin_get_weights']
G22_SWEEPS = 30


def hipcc():
    return shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def capi():
    from gbp_amd import build, _capi
    build.build()
    return _capi


def test_robust_symbols_are_declared_exported_and_bound(capi):
    lib = capi.load()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'gbp_lin.h')).read(), flags=re.S)
    dp, ip, vp = ct.POINTER(ct.c_double), ct.POINTER(ct.c_int32), ct.c_void_p
    want = {'gbp_lin_set_robust': [vp, ip, dp, dp], 'gbp_lin_robustify': [vp], 'gbp_lin_iterate_robust': [vp, ct.c_int32],
            'gbp_lin_get_weights': [vp, dp, ip]}
    for name in NEW:
        assert re.search(r'\bint\s+%s\s*\(' % name, header), f"{name} is not declared in include/gbp_lin.h"
        assert hasattr(lib, name), f"{name} is not exported"
        res, args = capi.SIGNATURES[name]
        assert res is ct.c_int and args == want[name]
    for name, code in (('NONE', 0), ('HUBER', 1), ('CONSTANT', 2)):
        assert re.search(r'#define\s+GBP_LIN_LOSS_%s\s+%d\b' % (name, code), header)
    assert capi.LIN_LOSS == {None: 0, 'huber': 1, 'constant': 2}


def test_robust_entry_points_refuse_a_null_handle(capi):
    lib = capi.load()
    w, flag = (ct.c_double * 4)(), (ct.c_int32 * 4)()
    assert lib.gbp_lin_set_robust(None, flag, w, w) == -1
    assert lib.gbp_lin_robustify(None) == -1
    assert lib.gbp_lin_iterate_robust(None, 1) == -1
    assert lib.gbp_lin_get_weights(None, w, flag) == -1
    assert b'NULL handle' in lib.gbp_last_error()


def test_linear_engine_has_the_robust_methods(capi):
    import inspect
    from gbp_amd.linear import LinearEngine
    for m in ('set_robust', 'robustify_all_factors', 'weights'):
        assert callable(getattr(LinearEngine, m))
    assert inspect.signature(LinearEngine.set_robust).parameters['threshold'].default == 2.0
    for m in ('synchronous_iteration', 'iterate'):
        assert inspect.signature(getattr(LinearEngine, m)).parameters['robustify'].default is False


# ---- the numpy oracle against the reference ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('loss', ['huber', 'constant'])
@pytest.mark.parametrize('tag', ['n100d3', 'defaults'])
def test_oracle_reproduces_the_reference_robust_run(tag, loss):
    """Fixture G22: the reference's own robustify_loss / compute_messages, its linpoint moved to the belief means before every sweep.
    Weights and flags of every factor in every sweep, the energy of every sweep, the final means and beliefs."""
    g = golden('G22_toy_linear_robust')
    va, vb, J, z, sigma, pe, pl = g22_graph(g, tag, loss)
    o = RobustOracle(va, vb, J, z, sigma, pe, pl, loss, 2.0)
    o.update_all_beliefs()
    for s in range(G22_SWEEPS):
        o.synchronous_iteration(robustify=True)
        assert np.array_equal(o.flag, g[f'{tag}_{loss}_flag'][s].astype(bool)), f"sweep {s}: flags"
        assert rel(o.w, 1.0 / g[f'{tag}_{loss}_var'][s]) < TOL, f"sweep {s}: weights {rel(o.w, 1.0 / g[f'{tag}_{loss}_var'][s]):.3e}"
        e, want = o.energy(), g[f'{tag}_{loss}_energy'][s]
        assert abs(e - want) <= TOL * abs(want), f"sweep {s}: energy {e!r} vs {want!r}"
    assert o.flag.any() and not o.flag.all()
    assert rel(o.get_means(), g[f'{tag}_{loss}_means']) < TOL
    eta, lam = o.beliefs()
    assert rel(eta, g[f'{tag}_{loss}_bel_eta']) < TOL and rel(lam, g[f'{tag}_{loss}_bel_lam']) < TOL


# ---- the engine's weight routine on the host --------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def shim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ('gbp_lin_robust.hpp', 'gbp_lin_handle.hpp', 'gbp_math.hpp')]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        tmp = f'{LIB}.{os.getpid()}.tmp'
        subprocess.check_call([hipcc(), '--offload-host-only', '-O1', '-std=c++17', '-shared', '-fPIC', '-o', tmp, SRC])
        os.replace(tmp, LIB)
    so = ct.CDLL(LIB)
    i, d = ct.c_int, ct.c_double
    ip, dp = ct.POINTER(ct.c_int32), ct.POINTER(ct.c_double)
    so.lin_robust_weights.argtypes, so.lin_robust_weights.restype = [i, i, i, ip, ip, dp, dp, dp, dp, ip, dp, dp, dp, ip, dp], None
    so.lin_robust_weight_of.argtypes, so.lin_robust_weight_of.restype = [i, d, d, d, ip], d
    return so


def host_weights(so, o):
    """(w, flag, e) of the shim at the oracle's current means."""
    ip, dp = ct.POINTER(ct.c_int32), ct.POINTER(ct.c_double)
    g = pack_robust(o)
    w, flag, e = np.zeros(o.F), np.zeros(o.F, dtype=np.int32), np.zeros(o.F)
    so.lin_robust_weights(g['D'], g['N'], g['F'], g['va'].ctypes.data_as(ip), g['vb'].ctypes.data_as(ip), g['feta'].ctypes.data_as(dp),
                          g['flam'].ctypes.data_as(dp), g['fconst'].ctypes.data_as(dp), g['bel'].ctypes.data_as(dp), g['loss'].ctypes.data_as(ip),
                          g['thr'].ctypes.data_as(dp), g['nvar'].ctypes.data_as(dp), w.ctypes.data_as(dp), flag.ctypes.data_as(ip), e.ctypes.data_as(dp))
    return w, flag.astype(bool), e


@pytest.mark.parametrize('D', [1, 2, 3, 4, 5, 6])
def test_host_weights_on_random_jacobians_of_every_rank(shim, D):
    """J of m x 2d for m = 1 .. 2d, and a rank-deficient one (a repeated row); the three losses mixed per factor; means random."""
    rs = np.random.RandomState(40 + D)
    N, per = 12, 14
    Js, zs = [], []
    for m in list(range(1, 2 * D + 1)) + ['deficient']:
        rows = 2 * D if m == 'deficient' else m
        J, z, _ = generic_jz(rs, D, per, rows=2 * D)            # padded with zero rows to 2d: the same factor
        J[:, rows:], z[:, rows:] = 0.0, 0.0
        if m == 'deficient' and D > 0:
            J[:, -1], z[:, -1] = J[:, 0], z[:, 0]             # a consistent repeated measurement: rank 2d - 1
        Js.append(J); zs.append(z)
    J, z = np.concatenate(Js), np.concatenate(zs)
    F = J.shape[0]
    va, vb = random_pairs(rs, N, F)
    pe, pl = random_priors(rs, N, D)
    o = RobustOracle(va, vb, J, z, 0.5 + rs.rand(F), pe, pl, mixed_losses(rs, F), 1.0 + 2.0 * rs.rand(F))
    o.mu = rs.randn(N, D)
    o.robustify_all_factors()
    w, flag, e = host_weights(shim, o)
    M = o.mahalanobis()
    assert set(o.loss) == set(LOSSES) and o.flag.any() and not o.flag.all()
    assert np.min(np.abs(M - o.thr)) > 1e-6                    # nobody on the threshold: the flags are decided
    assert np.array_equal(flag, o.flag)
    assert rel(e, 0.5 * M ** 2) < TOL, f"M^2 / 2: {rel(e, 0.5 * M ** 2):.3e}"
    assert np.max(np.abs(w - o.w) / o.w) < TOL, f"weights: {np.max(np.abs(w - o.w) / o.w):.3e}"


@pytest.mark.parametrize('loss', ['huber', 'constant'])
def test_host_weight_at_and_around_the_threshold_and_at_zero(shim, loss):
    """M exactly at t is not robust (M > t, gbp.py:313, 323); one ulp above is; M = 0 and a residual form that rounds below zero are
    not, and none of them divides by zero."""
    code = {'huber': 1, 'constant': 2}[loss]
    flag = ct.c_int32(7)
    for t in (2.0, 1.5, 3.0):
        e_at = 0.5 * t * t                                   # exact in binary for these t: sqrt(2 e) == t
        assert shim.lin_robust_weight_of(code, t, 0.25, e_at, ct.byref(flag)) == 1.0 and flag.value == 0
        e_up = np.nextafter(0.5 * np.nextafter(t, 4.0) ** 2, 1e9)
        w = shim.lin_robust_weight_of(code, t, 0.25, e_up, ct.byref(flag))
        M = np.sqrt(2 * e_up)
        assert M > t and flag.value == 1 and abs(w - robust_weight(loss, t, 0.25, M)[0]) <= 1e-12
    for e in (0.0, -0.0, -1e-13):
        assert shim.lin_robust_weight_of(code, 2.0, 0.25, e, ct.byref(flag)) == 1.0 and flag.value == 0
    assert shim.lin_robust_weight_of(0, 2.0, 0.25, 1e6, ct.byref(flag)) == 1.0 and flag.value == 0      # loss none: never robust


def test_host_weights_with_means_on_the_measurement(shim):
    """M = 0 through the whole routine: displacement factors whose means reproduce the measurement exactly."""
    rs = np.random.RandomState(5)
    N, D = 9, 3
    va, vb = np.arange(N - 1), np.arange(1, N)
    x = np.round(rs.rand(N, D) * 64) / 8                     # exact differences
    J = np.broadcast_to(np.hstack([-np.eye(D), np.eye(D)]), (N - 1, D, 2 * D)).copy()
    pe, pl = random_priors(rs, N, D)
    o = RobustOracle(va, vb, J, x[vb] - x[va], 0.5, pe, pl, ['huber', 'constant'] * 4, 2.0)
    o.mu = x
    w, flag, e = host_weights(shim, o)
    assert np.array_equal(w, np.ones(N - 1)) and not flag.any() and np.max(np.abs(e)) < 1e-12


@pytest.mark.parametrize('loss', ['huber', 'constant'])
def test_host_weights_reproduce_the_reference(shim, loss):
    """Fixture G22, every sweep: the shim's weights at the oracle's means (the oracle itself is pinned to G22 above)."""
    g = golden('G22_toy_linear_robust')
    va, vb, J, z, sigma, pe, pl = g22_graph(g, 'n100d3', loss)
    o = RobustOracle(va, vb, J, z, sigma, pe, pl, loss, 2.0)
    o.update_all_beliefs()
    for s in range(G22_SWEEPS):
        w, flag, _ = host_weights(shim, o)                   # what robustify is about to compute
        o.synchronous_iteration(robustify=True)
        assert np.array_equal(flag, g[f'n100d3_{loss}_flag'][s].astype(bool))
        assert rel(w, 1.0 / g[f'n100d3_{loss}_var'][s]) < TOL


def test_host_routines_under_address_and_undefined_sanitizers(tmp_path):
    """The shim as a stand-alone program (its own main: displacement rings of every d with outliers and mixed losses), compiled with
    the host sanitizers and run as a process of its own."""
    exe = str(tmp_path / 'lin_robust_main')
    subprocess.check_call([hipcc(), '--offload-host-only', '-O1', '-g', '-std=c++17', '-Xarch_host', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=undefined', '-DLIN_ROBUST_SHIM_MAIN', '-o', exe, SRC])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and 'lin_robust_shim OK' in r.stdout, out[-3000:]
    assert 'AddressSanitizer' not in out and 'runtime error:' not in out, out[-3000:]
