"""CPU-side checks of gbp_lin_solve_map_nonlinear (include/gbp_lin.h): the numpy twin of tests/lin_gn_cases.py against the reference's own
Gauss-Newton fixed point (fixture G29, tests/golden/make_g29.py); the twin's optimum against the gradient of Phi formed from the model's
Jacobian; the accept / reject / STALL paths; how far every accept decision of a GPU case stays from dPhi = 0; the spread that bounds the
device's final x; the host side of the new routines (tests/hostmath/lin_gn_shim.hip) against the twin; and the ABI."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, golden
from lin_extend_cases import csr
from lin_gn_cases import (CASES, CLEAR, DIAG_FLOOR, GOLDEN_CASES, GRAD, STALL, X_TOL, factor_energy, gradient, graph_of, joint_at, min_clearance, solve,
                          twin_of)
from lin_map_cases import rel
from lin_nonlin_cases import se2_h, se2_jac
from lin_se3_cases import se3_h, se3_jac
from test_linear_se3_cpu import model_points

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(REPO, 'gbp_amd', 'csrc')
SRC = os.path.join(HERE, 'hostmath', 'lin_gn_shim.hip')
LIB = os.path.join(HERE, 'hostmath', 'liblin_gn_shim.so')

# Measured: the twin's optimum (tol_grad 1e-9) against the last iterate of the reference's Gauss-Newton, max-norm relative to the largest
# entry: SE(2) ring 4.1e-14, SE(3) helix 3.2e-14; the energies 2.8e-14 and 2.0e-14.  The bound is 10 x the largest.
REF_TOL = 4.1e-13
ALL = list(CASES) + list(GOLDEN_CASES)


def _run(name, **more):
    model, g, opts = graph_of(name, golden)
    t = twin_of(model, g)
    return t, solve(t, t.mu, **dict(opts, **more))


# ---- the twin against the reference's fixed point -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,tag', [('se2_G25', 'se2'), ('se3_G28', 'se3')])
def test_twin_optimum_is_the_reference_fixed_point(name, tag):
    g = golden('G29_nonlinear_map')
    model, graph, _ = graph_of(name, golden)
    t = twin_of(model, graph)
    assert np.array_equal(t.mu, g[tag + '_x0'])                       # the reference started where the call starts: the prior means
    assert g[tag + '_steps'][-1] <= 1e-11 and len(g[tag + '_steps']) < 40
    r = solve(t, t.mu, tol_grad=1e-9, tol_step=0.0)
    gap, egap = rel(r['x'], g[tag + '_iterates'][-1]), rel(r['energy'], g[tag + '_energy'][-1])
    print(f"{name}: reason {r['reason']}, outer {r['outer']}, x gap {gap:.2e}, energy gap {egap:.2e}, energy0 gap {rel(r['energy0'], g[tag + '_energy'][0]):.2e}")
    assert r['reason'] == GRAD and r['converged']
    assert gap < REF_TOL and egap < REF_TOL and rel(r['energy0'], g[tag + '_energy'][0]) < 1e-12
    # with lambda -> 0 the first LM step is the reference's first Gauss-Newton step
    r1 = solve(t, t.mu, max_outer=1, lambda0=1e-12, lambda_min=1e-12, tol_grad=0.0, tol_step=0.0)
    assert rel(r1['x'], g[tag + '_iterates'][0]) < 1e-8


# ---- independent optimality ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ALL)
def test_gradient_from_the_jacobian_vanishes_at_the_twin_optimum(name):
    tol = 1e-7
    t, r = _run(name, tol_grad=tol, tol_step=0.0, max_outer=60, lambda_max=1e8)
    assert r['converged'] and r['reason'] == GRAD
    gn = float(np.linalg.norm(gradient(t, r['x'])))
    print(name, f"|grad| {gn:.3e} (solver's own {r['grad_norm']:.3e})")
    assert gn <= tol * (1 + 1e-6)
    if t.N and t.F:                                          # the solver's residual eta - Lambda x IS minus that gradient (taken at the start, where it is large)
        eta, L = joint_at(t, t.mu)
        assert rel(eta - L @ t.mu.reshape(-1), -gradient(t, t.mu).reshape(-1)) < 1e-9


def test_gradient_against_central_differences():
    for name in ('se2_hub70', 'se3_G28'):
        model, g, _ = graph_of(name, golden)
        t = twin_of(model, g)
        x = t.mu.copy()
        phi = lambda y: factor_energy(t, y) + float(np.sum(0.5 * np.einsum('vi,vij,vj->v', y, t.pl, y) - np.sum(t.pe * y, 1)))
        G, rs = gradient(t, x), np.random.RandomState(3)
        for _ in range(6):
            d = rs.normal(0, 1, x.shape)
            d /= np.linalg.norm(d)
            num = (phi(x + 1e-5 * d) - phi(x - 1e-5 * d)) / 2e-5
            assert abs(num - float(np.sum(G * d))) < 1e-5 * max(1.0, abs(num))


# ---- accept, reject, stall ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['se2_reject', 'se3_reject'])
def test_reject_cases_contain_rejections(name):
    t, r = _run(name)
    rows = r['rows']
    print(name, r['outer'], r['accepted'], r['rejected'], rows[:, 3])
    assert r['rejected'] >= 3 and r['accepted'] >= 3 and r['reason'] == GRAD
    assert rows[0, 4] == 1 and (rows[:, 3] > 1.0).sum() >= 3          # real rejections: dPhi far above rounding
    lam = rows[:, 1]
    for i in range(1, len(rows)):                                     # lambda is a product of the options
        assert lam[i] == (max(lam[i - 1] * 0.1, 1e-12) if rows[i - 1, 4] else lam[i - 1] * 10.0)
    assert np.all(rows[rows[:, 4] == 1, 3] < 0) and np.all(rows[rows[:, 4] == 0, 3] > 0)   # an accept is dPhi < 0, and nothing else is
    assert r['energy'] < r['energy0']


@pytest.mark.parametrize('name', ['se2_stall', 'se3_stall'])
def test_stall_cases_stall(name):
    t, r = _run(name)
    assert r['reason'] == STALL and not r['converged'] and r['rows'][-1, 4] == 0
    assert r['rows'][-1, 1] > 1e-6 and r['rows'][-2, 1] <= 1e-6       # the rejection that ended it was the first one above lambda_max
    assert np.array_equal(r['x'], solve(t, t.mu, **dict(graph_of(name, golden)[2], max_outer=r['outer'] - 1))['x'])


@pytest.mark.parametrize('name', ALL)
def test_gpu_cases_stay_clear_of_dphi_zero(name):
    """Every accept decision of the runs test_linear_gn_gpu.py compares exactly: |dPhi| >= CLEAR, from the means and from x0 = 0."""
    t, r = _run(name)
    c = min_clearance(r['rows'])
    print(name, r['outer'], r['accepted'], r['rejected'], r['reason'], f'{c:.3e}')
    assert c >= CLEAR
    if name.endswith('F0'):
        r0 = solve(t, np.zeros_like(t.mu), **graph_of(name, golden)[2])
        assert r0['outer'] == 1 and r0['accepted'] == 1 and min_clearance(r0['rows']) >= CLEAR and r0['reason'] == GRAD
        assert rel(r0['x'], t.mu) < 1e-13                             # the priors' own solution after one accepted step


def test_final_x_spread_between_inner_tolerances():
    """X_TOL: the twin's own spread of the final x between inner solves left at cg.rel_tol 1e-12 and at 1e-14, x 10."""
    worst = 0.0
    for name in ALL:
        model, g, opts = graph_of(name, golden)
        t = twin_of(model, g)
        if not t.N:
            continue
        a, b = solve(t, t.mu, perturb=1e-12, **opts), solve(t, t.mu, perturb=1e-14, **opts)
        assert np.array_equal(a['rows'][:, 4], b['rows'][:, 4])
        gap = float(np.abs(a['x'] - b['x']).max() / max(1.0, np.abs(b['x']).max()))
        print(name, f'{gap:.3e}')
        worst = max(worst, gap)
    print(f'worst {worst:.3e}')
    assert worst * 10 <= X_TOL and worst * 100 >= X_TOL * 0.1        # the constant is what was measured, neither tighter nor far looser


# ---- the host side of the new routines --------------------------------------------------------------------------------------------------------

def hipcc():
    return shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


@pytest.fixture(scope='module')
def shim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ('gbp_lin_gn.hpp', 'gbp_lin_map.hpp', 'gbp_lin_nonlin.hpp', 'gbp_lin_robust.hpp', 'gbp_lin_handle.hpp', 'gbp_math.hpp')]
    deps.append(os.path.join(REPO, 'include', 'gbp_lin.h'))
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        tmp = f'{LIB}.{os.getpid()}.tmp'
        subprocess.check_call([hipcc(), '--offload-host-only', '-O1', '-std=c++17', '-shared', '-fPIC', '-o', tmp, SRC])
        os.replace(tmp, LIB)
    so = ct.CDLL(LIB)
    i, d, dp, ip = ct.c_int, ct.c_double, ct.POINTER(ct.c_double), ct.POINTER(ct.c_int)
    so.lin_gn_diag_floor.argtypes, so.lin_gn_diag_floor.restype = [], d
    so.lin_gn_factors.argtypes, so.lin_gn_factors.restype = [i, i, i, ip, ip, dp, dp, dp, dp, dp, dp, dp, dp], None
    so.lin_gn_damp.argtypes, so.lin_gn_damp.restype = [i, i, i, ip, ip, dp, dp, dp, dp, d, dp], None
    so.lin_gn_diff.argtypes, so.lin_gn_diff.restype = [i, i, dp, dp, dp, dp], d
    return so


def _dp(a):
    return None if a is None else a.ctypes.data_as(ct.POINTER(ct.c_double))


def _ip(a):
    return a.ctypes.data_as(ct.POINTER(ct.c_int))


def _pack_prior(pe, pl):
    D = pe.shape[1]
    iu = np.triu_indices(D)
    return np.ascontiguousarray(np.concatenate([pe, pl[:, iu[0], iu[1]]], 1))


def _points(model):
    """Factor f joins variables 2 f and 2 f + 1, whose values are the seeded points of test_linear_se3_cpu.py (zero and tiny rotations,
    both sides of the series crossover, |w_a| past pi); SE(2): seeded poses with unwrapped headings."""
    if model == 2:
        x, z, s = model_points()
    else:
        rs = np.random.RandomState(7)
        x = rs.normal(0, 3, (200, 6))
        x[:, [2, 5]] = rs.uniform(-9, 9, (200, 2))
        x[:4, [2, 5]] = 0.0
        z, s = rs.normal(0, 2, (200, 3)), rs.uniform(0.5, 20.0, (200, 3))
    return x, z, s


@pytest.mark.parametrize('model,weighted', [(1, False), (2, False), (2, True)])
def test_host_routines_match_the_twin(shim, model, weighted):
    assert shim.lin_gn_diag_floor() == DIAG_FLOOR
    pts, z, s = _points(model)
    F, D = pts.shape[0], pts.shape[1] // 2
    N, P2 = 2 * F, D * (2 * D + 1)
    rs = np.random.RandomState(11)
    va, vb = np.arange(0, N, 2, dtype=np.int32), np.arange(1, N, 2, dtype=np.int32)
    x = np.ascontiguousarray(pts.reshape(N, D))
    w = rs.uniform(0.05, 1.0, F) if weighted else None
    h_fn, jac_fn = (se2_h, se2_jac) if model == 1 else (se3_h, se3_jac)
    # linearise-at-x with energy
    feta, flam, e_lin, e_only = np.full((2 * D, F), np.nan), np.full((P2, F), np.nan), np.full(F, np.nan), np.full(F, np.nan)
    shim.lin_gn_factors(model, N, F, _ip(va), _ip(vb), _dp(np.ascontiguousarray(z.T)), _dp(np.ascontiguousarray(s.T)), _dp(w), _dp(x), _dp(feta), _dp(flam),
                        _dp(e_lin), _dp(e_only))
    J, h = jac_fn(pts, s), h_fn(pts, s)
    b = np.einsum('fki,fi->fk', J, pts) + s * z - h
    want_eta, want_lam = np.einsum('fki,fk->fi', J, b), np.einsum('fki,fkj->fij', J, J)
    want_e = 0.5 * np.sum((h - s * z) ** 2, 1) * (w if weighted else 1.0)
    iu = np.triu_indices(2 * D)
    lam = np.zeros((F, 2 * D, 2 * D))
    lam[:, iu[0], iu[1]] = flam.T
    lam[:, iu[1], iu[0]] = flam.T

    def close(name, a, b_, tol=1e-12):
        a, b_ = a.reshape(a.shape[0], -1), b_.reshape(b_.shape[0], -1)
        gap = np.abs(a - b_).max(1) / np.maximum(1.0, np.abs(b_).max(1))
        assert np.all(np.isfinite(a)) and gap.max() < tol, f"{name}: {gap.max():.3e} at {gap.argmax()}"

    close('eta', feta.T, want_eta); close('lam', lam, want_lam); close('energy', e_lin[:, None], want_e[:, None]); close('energy-only', e_only[:, None], want_e[:, None])
    # the damped prior
    pl = np.array([np.diag(rs.uniform(0.0, 4.0, D)) for _ in range(N)])
    pl[:3] = 0.0                                             # nothing on the diagonal but the factor: and variable 0 of the all-zero points
    pe = rs.normal(0, 2, (N, D))
    prior = _pack_prior(pe, pl)
    vptr, vadj = (np.ascontiguousarray(a, dtype=np.int32) for a in csr(N, va, vb)[:2])
    lam_d = 0.37
    dprior = np.full_like(prior, np.nan)
    shim.lin_gn_damp(D, N, F, _ip(vptr), _ip(vadj), _dp(prior), _dp(np.ascontiguousarray(flam)), _dp(w), _dp(x), lam_d, _dp(dprior))
    ww = w if weighted else np.ones(F)
    dg = np.einsum('vii->vi', pl).copy()
    dg[va] += ww[:, None] * np.einsum('fii->fi', want_lam[:, :D, :D])
    dg[vb] += ww[:, None] * np.einsum('fii->fi', want_lam[:, D:, D:])
    dg = np.maximum(dg, DIAG_FLOOR)
    want = _pack_prior(pe + lam_d * dg * x, pl + lam_d * np.einsum('vi,ij->vij', dg, np.eye(D)))
    close('damped prior', dprior, want)
    # the prior difference
    xc = x + rs.normal(0, 1, x.shape) * 10.0 ** rs.uniform(-9, 0, (N, 1))
    diff = np.full(N, np.nan)
    mx = shim.lin_gn_diff(D, N, _dp(prior), _dp(x), _dp(np.ascontiguousarray(xc)), _dp(diff))
    want_d = np.sum((xc - x) * (np.einsum('vij,vj->vi', pl, 0.5 * (xc + x)) - pe), 1)
    assert mx == np.abs(xc - x).max()
    assert np.all(np.abs(diff - want_d) <= 1e-12 * np.maximum(1.0, np.abs(want_d)))
    # in difference form it does not cancel far from the origin: the same small step taken 1e8 away keeps its digits
    far = x + 1e8
    xf = np.ascontiguousarray(far + (xc - x))
    want_far = np.sum((xf - far) * (np.einsum('vij,vj->vi', pl, 0.5 * (xf + far)) - pe), 1)
    shim.lin_gn_diff(D, N, _dp(prior), _dp(np.ascontiguousarray(far)), _dp(xf), _dp(diff))
    assert np.all(np.abs(diff - want_far) <= 1e-12 * np.maximum(1.0, np.abs(want_far)))
    naive = 0.5 * np.einsum('vi,vij,vj->v', xf, pl, xf) - np.sum(pe * xf, 1) - (0.5 * np.einsum('vi,vij,vj->v', far, pl, far) - np.sum(pe * far, 1))
    assert np.abs(naive - want_far).max() > 1e3 * np.abs(diff - want_far).max()   # what Phi(x_c) - Phi(x) formed from two values would lose


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def capi():
    from gbp_amd import build, _capi
    build.build()
    return _capi


def test_struct_layouts_and_binding(capi):
    O, I = capi.LinNlmapOpts, capi.LinNlmapInfo
    assert ct.sizeof(O) == 8 + 7 * 8 + ct.sizeof(capi.LinMapOpts) == 88 and O.lambda0.offset == 8 and O.tol_grad.offset == 56 and O.cg.offset == 64
    assert ct.sizeof(I) == 6 * 4 + 4 * 8 == 56 and I.energy0.offset == 24
    text = open(os.path.join(REPO, 'include', 'gbp_lin.h')).read()
    for name, T in (('gbp_lin_nlmap_opts_t', O), ('gbp_lin_nlmap_info_t', I)):
        body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\} %s;' % name, text).group(1), flags=re.S)
        names = [n for decl in body.split(';') for n in re.findall(r'\*?\b([a-z_0-9]+)\s*(?:,|$)', decl.strip())]
        assert names == [f[0].rstrip('_') for f in T._fields_], name
    bare = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for k, v in (('FROM_MEANS', 0), ('FROM_MAP', 1), ('NONE', 0), ('STEP', 1), ('GRAD', 2), ('STALL', 3)):
        assert re.search(r'#define\s+GBP_LIN_NLMAP_%s\s+%d\b' % (k, v), bare) and getattr(capi, 'LIN_NLMAP_' + k) == v
    assert 'iteratively reweighted' in text.lower() and 'GN_DIAG_FLOOR' in text
    lib = capi.load()
    assert lib.gbp_lin_solve_map_nonlinear is not None
    from gbp_amd.linear import LinearEngine
    assert callable(LinearEngine.solve_map_nonlinear)
