"""CPU-side checks of the SE(3) relative-pose factor of the linear engine (include/gbp_lin.h, GBP_LIN_MODEL_SE3_BETWEEN): the twin's
Jacobian against central differences, the numpy twin of tests/lin_se3_cases.py against the reference's own run (fixture G28,
tests/golden/make_g28.py), the engine's model routines compiled for the host (tests/hostmath/lin_se3_shim.hip) against the twin -- and
the SE(2) routines through the same shim against the SE(2) twin --, the distance of every seeded GPU case from the thresholds, and the
header, struct layouts and binding."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, golden
from lin_map_cases import rel
from lin_nonlin_cases import se2_h, se2_jac
from lin_se3_cases import AXIS, CASES, SWEEPS, g28_graph, g28_schedule, robust_case, run_margins, se3_h, se3_jac, twin_of

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(REPO, 'gbp_amd', 'csrc')
SRC = os.path.join(HERE, 'hostmath', 'lin_se3_shim.hip')
LIB = os.path.join(HERE, 'hostmath', 'liblin_se3_shim.so')

# Observed maximum gaps of the twin from the reference over the three tags of G28 (relative, max-norm): means 2.7e-13, energy 3.5e-13,
# factors 2.7e-13, linpoints 2.7e-13, messages 3.7e-13, beliefs 1.1e-16, weights 1.2e-13.  The bound is <= 100 x the largest of them.
TWIN_TOL = 1e-11


# ---- the points every model check shares ----------------------------------------------------------------------------------------------

def _unit(rs, n):
    v = rs.normal(0, 1, (n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _so3_exp(w):
    from lin_se3_cases import coeffs, ik
    A, B, _ = coeffs(np.sum(w * w, 1))
    return ik(w, A, B)


def _so3_log(R):
    from lin_se3_cases import so3_log
    return so3_log(R)


def model_points():
    """x (n, 12), z (n, 6), s (n, 6): seeded; w_a = w_b = 0 exactly; |w| in 1e-9 .. 1e-4 and around the series crossover |w| = 0.2;
    |w_a| in (pi, 4.5); relative rotations |phi| up to 2.5."""
    rs = np.random.RandomState(2028)
    blocks = []

    def block(wa, phi):
        n = wa.shape[0]
        Rb = _so3_exp(wa) @ _so3_exp(phi)                    # w_b: the rotation vector of R_a Exp(phi), continued near w_a when small
        wb = _so3_log(Rb)
        x = np.concatenate([rs.normal(0, 3, (n, 3)), wa, rs.normal(0, 3, (n, 3)), wb], 1)
        blocks.append(x)

    block(np.zeros((4, 3)), np.zeros((4, 3)))                                              # everything exactly zero
    block(np.zeros((6, 3)), _unit(rs, 6) * rs.uniform(0.1, 2.5, (6, 1)))                   # w_a = 0, a real relative rotation
    mags = 10.0 ** rs.uniform(-9, -4, (40, 1))
    block(_unit(rs, 40) * mags, _unit(rs, 40) * 10.0 ** rs.uniform(-9, -4, (40, 1)))       # deep in the series on both sides
    block(_unit(rs, 30) * rs.uniform(0.19, 0.21, (30, 1)), _unit(rs, 30) * rs.uniform(0.19, 0.21, (30, 1)))   # the crossover th = 0.2
    block(_unit(rs, 60) * rs.uniform(np.pi, 4.5, (60, 1)), _unit(rs, 60) * rs.uniform(0.0, 2.5, (60, 1)))     # past pi
    block(_unit(rs, 80) * rs.uniform(0.0, 3.0, (80, 1)), _unit(rs, 80) * rs.uniform(0.0, 2.5, (80, 1)))
    x = np.concatenate(blocks)
    # past pi the principal Log of R_b is not near w_a: give w_b the continued value w_a + phi-ish by taking it as is -- h only needs R_b,
    # and J is taken at the w_b given; but keep some w_b past pi too
    far = slice(80, 140)
    x[far, 9:12] = x[far, 3:6] + _unit(rs, 60) * rs.uniform(0.0, 0.8, (60, 1))
    n = x.shape[0]
    z = np.concatenate([rs.normal(0, 2, (n, 3)), _unit(rs, n) * rs.uniform(0, 2.5, (n, 1))], 1)
    s = rs.uniform(0.5, 20.0, (n, 6))
    return x, z, s


def test_points_cover_what_they_should():
    x, _, _ = model_points()
    na, nb = np.linalg.norm(x[:, 3:6], axis=1), np.linalg.norm(x[:, 9:12], axis=1)
    phi = np.linalg.norm(se3_h(x, np.ones((x.shape[0], 6)))[:, 3:], axis=1)
    assert x.shape[0] >= 200
    assert np.sum((na == 0) & (nb == 0)) >= 4
    assert np.sum((na > 1e-9) & (na < 1e-4)) >= 30 and np.sum((na > 0.19) & (na < 0.2)) >= 5 and np.sum((na > 0.2) & (na < 0.21)) >= 5
    assert np.sum((na > np.pi) & (na < 4.5)) >= 50 and np.sum(nb > np.pi) >= 20
    assert phi.max() > 2.3 and phi.max() < 2.6


def test_jacobian_against_central_differences():
    """The bound of the issue: 1e-6 relative to the larger of 1 and the largest entry of the numerical Jacobian, step 1e-6."""
    x, _, s = model_points()
    J = se3_jac(x, s)
    num = np.zeros_like(J)
    step = 1e-6
    for i in range(12):
        d = np.zeros(12); d[i] = step
        num[:, :, i] = (se3_h(x + d, s) - se3_h(x - d, s)) / (2 * step)
    scale = np.maximum(1.0, np.abs(num).max(axis=(1, 2)))
    gap = np.abs(J - num).max(axis=(1, 2)) / scale
    print(f'worst gap {gap.max():.3e} at point {gap.argmax()}')
    assert gap.max() < 1e-6


# ---- the twin against the reference's own run ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', ['main', 'b0', 'robust'])
def test_twin_equals_the_reference_run(tag):
    """Masks, iters_since_relin, per-factor damping and robust flags exactly in every sweep; the rest within TWIN_TOL."""
    g = golden('G28_se3_posegraph')
    sched, sweeps = g28_schedule(g, tag)
    t = twin_of(g28_graph(g, tag), sched)
    robust = tag == 'robust'
    gaps = {}

    def gap(name, a, b):
        gaps[name] = max(gaps.get(name, 0.0), rel(a, b))

    for s in range(sweeps):
        out = t.synchronous_iteration(True, robust)
        mask = out[0] if robust else out
        assert np.array_equal(mask, g[f'{tag}_mask'][s].astype(bool)), f"sweep {s}: mask"
        assert np.array_equal(t.iters, g[f'{tag}_iters'][s]), f"sweep {s}: iters"
        assert np.array_equal(t.fdamp, g[f'{tag}_damp'][s]), f"sweep {s}: damping"
        if robust:
            assert np.array_equal(t.flag, g['robust_flag'][s].astype(bool)), f"sweep {s}: flags"
            gap('weights', t.w, g['robust_w'][s])
        gap('means', t.get_means(), g[f'{tag}_means'][s])
        gap('energy', t.energy(), g[f'{tag}_energy'][s])
        k = f'{tag}_s{s + 1}_'
        if k + 'feta' in g:                                  # the reference holds the factor times its weight
            gap('factor', t.feta * t.w[:, None], g[k + 'feta']); gap('factor', t.flam * t.w[:, None, None], g[k + 'flam'])
            gap('linpoint', t.linpoint, g[k + 'linpoint'])
            for name, a in zip(('msg_eta_a', 'msg_lam_a', 'msg_eta_b', 'msg_lam_b'), t.messages()):
                gap('messages', a, g[k + name])
            gap('beliefs', t.be, g[k + 'bel_eta']); gap('beliefs', t.bl, g[k + 'bel_lam'])
    print(tag, {k: f'{v:.2e}' for k, v in gaps.items()})
    assert set(gaps) >= {'means', 'energy', 'factor', 'linpoint', 'messages', 'beliefs'}
    for k, v in gaps.items():
        assert v < TWIN_TOL, f"{k}: {v:.3e}"
    if tag == 'main':
        eta, lam = t.joint()
        assert rel(np.linalg.solve(lam, eta), g['main_map_mu'].reshape(-1)) < 1e-9


def test_fixture_is_what_the_issue_describes():
    g = golden('G28_se3_posegraph')
    assert g['edges'].shape == (35, 2) and g['prior_eta'].shape == (30, 6) and g['z'].shape == (35, 6)
    assert np.array_equal(g['s'], np.tile([10.0, 10.0, 10.0, 20.0, 20.0, 20.0], (35, 1)))
    assert g['main_mask'].shape == (60, 35) and g['b0_mask'].shape == (15, 35) and g['robust_mask'].shape == (60, 35)
    assert g['b0_mask'].sum(1).tolist() == [0] + [35] * 14
    counts = g['main_mask'].sum(1)
    assert counts[0] == 0 and counts[1] == 35 and 100 < counts.sum() < 300
    w = g['truth'][:, 3:]
    ang = np.linalg.norm(w, axis=1)
    assert ang[0] == 0 and abs(ang[-1] - 4.5) < 1e-12 and np.all(np.diff(ang) > 0) and rel(w, ang[:, None] * AXIS) < 1e-15   # continuous, past pi
    assert np.linalg.norm(g['z'][:, 3:], axis=1).max() < np.pi and np.linalg.norm(g['robust_z'][:, 3:], axis=1).max() < np.pi
    assert np.count_nonzero(np.any(g['robust_z'] != g['z'], 1)) == 3 and g['loss'].tolist() == [0] * 29 + [1] * 6
    assert g['robust_flag'].any() and (g['robust_flag'][1:] != g['robust_flag'][:-1]).any() and not g['robust_flag'][:, :29].any()
    assert min(float(g['main_margin']), float(g['robust_margin']), float(g['robust_loss_margin'])) >= 1e-7


# ---- the engine's model routines on the host ---------------------------------------------------------------------------------------------

def hipcc():
    return shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


@pytest.fixture(scope='module')
def shim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ('gbp_lin_nonlin.hpp', 'gbp_lin_robust.hpp', 'gbp_lin_handle.hpp', 'gbp_math.hpp')]
    deps.append(os.path.join(REPO, 'include', 'gbp_lin.h'))
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        tmp = f'{LIB}.{os.getpid()}.tmp'
        subprocess.check_call([hipcc(), '--offload-host-only', '-O1', '-std=c++17', '-shared', '-fPIC', '-o', tmp, SRC])
        os.replace(tmp, LIB)
    so = ct.CDLL(LIB)
    i, dp = ct.c_int, ct.POINTER(ct.c_double)
    so.lin_se3_dims.argtypes, so.lin_se3_dims.restype = [i, i], i
    for fn in (so.lin_se3_eval, so.lin_se2_eval):
        fn.argtypes, fn.restype = [i] + [dp] * 8, None
    return so


def _run(fn, x, z, s, D):
    n = x.shape[0]
    P = D * (2 * D + 1)
    x, z, s = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, z, s))
    out = [np.full((n, D), np.nan), np.full((n, 2 * D), np.nan), np.full((n, P), np.nan), np.full(n, np.nan), np.full(n, np.nan)]
    fn(n, *(a.ctypes.data_as(ct.POINTER(ct.c_double)) for a in [x, z, s] + out))
    h, eta, pk, energy, m2 = out
    lam = np.zeros((n, 2 * D, 2 * D))
    iu = np.triu_indices(2 * D)                              # row-major upper triangle: the packed order
    lam[:, iu[0], iu[1]] = pk
    lam[:, iu[1], iu[0]] = pk
    return h, eta, lam, energy, m2


def _twin_values(h_fn, jac_fn, x, z, s):
    J, h = jac_fn(x, s), h_fn(x, s)
    b = np.einsum('fki,fi->fk', J, x) + s * z - h
    r = h - s * z
    return h, np.einsum('fki,fk->fi', J, b), np.einsum('fki,fkj->fij', J, J), 0.5 * np.sum(r * r, 1), np.sum(r * r, 1)


def _close(got, want, tol=1e-12):
    """Per point, relative to the larger of 1 and the point's largest entry."""
    for name, a, b in zip(('h', 'eta', 'lam', 'energy', 'm2'), got, want):
        a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
        gap = np.abs(a - b).max(1) / np.maximum(1.0, np.abs(b).max(1))
        assert np.all(np.isfinite(a)) and gap.max() < tol, f"{name}: {gap.max():.3e} at point {gap.argmax()}"


def test_host_se3_routines_match_the_twin(shim):
    assert (shim.lin_se3_dims(2, 0), shim.lin_se3_dims(2, 1), shim.lin_se3_dims(1, 0), shim.lin_se3_dims(1, 1)) == (6, 6, 3, 3)
    x, z, s = model_points()
    # moderate translations and weights: 1e-12 of the largest entry of a point is then far above the rounding of the two evaluations
    _close(_run(shim.lin_se3_eval, x, z, s, 6), _twin_values(se3_h, se3_jac, x, z, s))


def test_host_se2_routines_match_the_se2_twin(shim):
    """The templating changed nothing: the SE(2) routines through the same header equal lin_nonlin_cases' twin."""
    rs = np.random.RandomState(7)
    n = 200
    x = rs.normal(0, 3, (n, 6))
    x[:, [2, 5]] = rs.uniform(-9, 9, (n, 2))
    x[:4, [2, 5]] = 0.0
    z, s = rs.normal(0, 2, (n, 3)), rs.uniform(0.5, 20.0, (n, 3))
    _close(_run(shim.lin_se2_eval, x, z, s, 3), _twin_values(se2_h, se2_jac, x, z, s))


# ---- the seeded GPU cases ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_gpu_cases_stay_clear_of_the_threshold(name):
    """Every seeded case of test_linear_se3_gpu.py: the twin's distance from `dist > beta` is >= 1e-9 before every sweep, so the
    device's masks can be compared exactly and no GPU case is skipped or cut short."""
    _, build, sched = next(c for c in CASES if c[0] == name)
    dm, _ = run_margins(build(), sched, SWEEPS)
    print(name, f'{dm:.3e}')
    assert dm >= 1e-9


def test_robust_gpu_case_stays_clear_of_both_thresholds():
    g, sched = robust_case()
    dm, rm = run_margins(g, sched, SWEEPS, robustify=True)
    print(f'{dm:.3e} {rm:.3e}')
    assert dm >= 1e-9 and rm >= 1e-9
    t = twin_of(g, sched)
    _, flagged = t.iterate(SWEEPS, relinearise=True, robustify=True)
    assert flagged.max() > 0 and flagged.min() < (t.loss != 0).sum()


def test_live_gpu_case_stays_clear_of_both_thresholds():
    from lin_se3_cases import live_margins
    dm, rm = live_margins()
    print(f'{dm:.3e} {rm:.3e}')
    assert dm >= 1e-9 and rm >= 1e-9


def test_until_gpu_case_stays_clear_of_the_threshold():
    from lin_se3_cases import case
    g, sched = case('helix')
    dm, _ = run_margins(g, sched, 30)                        # test_iterate_until_* run up to 30 sweeps of it
    assert dm >= 1e-9


def test_cases_exercise_what_they_are_for():
    from lin_se3_cases import case
    g, sched = case('ring258')
    assert len(g['va']) == 258 and g['N'] == 129 and np.all(np.bincount(np.concatenate([g['va'], g['vb']])) == 4)
    counts = twin_of(g, sched).iterate(SWEEPS, relinearise=True)
    assert counts[0] == 0 and counts.max() == 258 and 0 < np.count_nonzero(counts) < SWEEPS
    g, _ = case('star70')
    assert np.bincount(np.concatenate([g['va'], g['vb']]))[0] == 70
    g, _ = case('zero')
    assert not g['truth'][:, 3:].any() and not g['z'][:, 3:].any()
    g, _ = case('tiny')
    assert rel(np.linalg.norm(g['truth'][:, 3:], axis=1), 1e-7) < 1e-6
    g, _ = case('helix')
    assert np.linalg.norm(g['truth'][:, 3:], axis=1).max() > np.pi


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def capi():
    from gbp_amd import build, _capi
    build.build()
    return _capi


def test_header_constant_and_binding(capi):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'gbp_lin.h')).read(), flags=re.S)
    assert re.search(r'#define\s+GBP_LIN_MODEL_SE2_BETWEEN\s+1\b', text) and re.search(r'#define\s+GBP_LIN_MODEL_SE3_BETWEEN\s+2\b', text)
    assert capi.LIN_MODEL_SE3_BETWEEN == 2 and capi.LIN_MODEL_SE2_BETWEEN == 1
    from gbp_amd.linear import LinearEngine
    assert callable(LinearEngine.se3_pose_graph) and callable(LinearEngine.extend_se3)
    full = open(os.path.join(REPO, 'include', 'gbp_lin.h')).read()
    assert 'NEVER WRAPPED' in full and 'below pi' in full                       # the domain rule is stated
    assert 'never wrapped' in LinearEngine.se3_pose_graph.__doc__ and 'below pi' in LinearEngine.se3_pose_graph.__doc__


def test_struct_layouts_unchanged(capi):
    S = capi.LinNonlinear
    assert ct.sizeof(S) == 40 and [f[0] for f in S._fields_] == ['model', 'num_undamped_iters', 'min_linear_iters', 'reserved', 'beta', 'measurement', 'sqrt_info']
    assert (S.beta.offset, S.measurement.offset, S.sqrt_info.offset) == (16, 24, 32)
    E = capi.LinExtNonlinear
    assert ct.sizeof(E) == 8 + 6 * 8 and [f[0] for f in E._fields_] == ['n_new_vars', 'n_new_factors', 'var_a', 'var_b', 'measurement', 'sqrt_info', 'prior_eta', 'prior_lam']
    text = open(os.path.join(REPO, 'include', 'gbp_lin.h')).read()
    for name, T in (('gbp_lin_nonlinear_desc_t', S), ('gbp_lin_extend_nonlinear_desc_t', E)):
        body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\} %s;' % name, text).group(1), flags=re.S)
        names = [n for decl in body.split(';') for n in re.findall(r'\*?\b([a-z_]+)\s*(?:,|$)', decl.strip())]
        assert names == [f[0] for f in T._fields_], name
