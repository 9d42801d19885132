"""CPU-side checks of gbp_lin_solve_map_nonlinear_robust (include/gbp_lin.h): the numpy twin of tests/lin_irls_cases.py against the
reference's own robustify + Gauss-Newton fixed point (fixture G30, tests/golden/make_g30.py); the host side of the reweight lane
(tests/hostmath/lin_irls_shim.hip) against the twin; the order of the stop tests; how far every M_f of a GPU case stays from its
threshold, every accept decision from dPhi = 0 and every tested gradient from tol_grad; the spread that bounds the device's final x;
and the ABI."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, golden
from lin_gn_cases import STALL, min_clearance, twin_of
from lin_irls_cases import (CASES, CLEAR, GRAD_CLEAR, IRLS_MOVE, IRLS_NONE, IRLS_WEIGHTS, X_TOL, g30_graph, graph_of, solve_robust, twin_run, weights_at)
from lin_map_cases import rel
from lin_nonlin_cases import se2_h, se2_jac
from lin_nonlin_robust_cases import CONSTANT, HUBER, NONE
from lin_se3_cases import se3_h, se3_jac
from test_linear_se3_cpu import model_points

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(REPO, 'gbp_amd', 'csrc')
SRC = os.path.join(HERE, 'hostmath', 'lin_irls_shim.hip')
LIB = os.path.join(HERE, 'hostmath', 'liblin_irls_shim.so')

# Measured: the twin's fixed point against the reference's last round (fixture G30), max-norm relative to the largest entry: x 2.7e-9
# (SE(2) ring) and 1.0e-9 (SE(3) helix), the weights 1.3e-8 and 1.1e-8.  That is not rounding but where the two loops stop: the reference's
# undamped Gauss-Newton rounds go on to moves of 1e-10 (25 and 23 rounds, each contracting by about 0.4), while a Levenberg-Marquardt
# round tests Phi and cannot move below the floor of its decrease test (steps whose dPhi drowns in the rounding of E
# are rejected), so its rounds stop moving -- reason MOVE -- after 19 rounds each, a few 1e-9 from the reference's point.  The
# bound is 10 x the largest.
REF_TOL = 1.3e-7


# ---- the twin against the reference's fixed point -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', ['se2', 'se3'])
def test_twin_fixed_point_is_the_reference_fixed_point(tag):
    g30 = golden('G30_nonlinear_map_robust')
    model, graph = g30_graph(golden, tag)
    t = twin_of(model, graph, losses=True)
    mu, w, flag = g30[tag + '_mu'], g30[tag + '_w'], g30[tag + '_flag'].astype(bool)
    assert np.array_equal(t.mu, g30[tag + '_x0'])                     # the reference started where the call starts: the prior means
    assert len(mu) - 1 <= 30 and g30[tag + '_moves'][-1] <= 1e-10
    lossy = graph['loss'] != NONE
    assert flag[-1].any() and (lossy & ~flag[-1]).any()
    # the reference's rule: stop on the move alone; every round solved as far as the decrease test allows (a round that stalls goes on)
    r = solve_robust(t, t.mu, max_rounds=30, tol_weight=0.0, tol_move=1e-10, tol_grad=1e-9, tol_step=1e-12)
    xgap, wgap = rel(r['x'], mu[-1]), rel(r['weights'], w[-1])
    print(f"{tag}: rounds {r['rounds']} (reference {len(mu) - 1}), reason {r['reason']}, x gap {xgap:.2e}, weight gap {wgap:.2e}, "
          f"flagged per round {r['rows'][:, 1].astype(int).tolist()}")
    assert r['converged'] and r['reason'] == IRLS_MOVE
    assert xgap < REF_TOL and wgap < REF_TOL
    assert np.array_equal(r['flag'], flag[-1])
    # the per-round flagged counts: equal round for round; the reference's Gauss-Newton rounds go on for a few more (it has no decrease
    # test to stall on) and flag the same factors in all of them
    mine, ref = r['rows'][:, 1].astype(int).tolist(), flag.sum(1).tolist()
    assert len(mine) <= len(ref) and mine == ref[:len(mine)] and all(np.array_equal(f, flag[-1]) for f in flag[len(mine) - 1:])
    assert all(np.array_equal(a, b) for a, b in zip(r['flags'], flag))
    # the first reweight is at the same point exactly: the reference's weights to rounding
    assert rel(r['ws'][0], w[0]) < 1e-12 and np.array_equal(r['flags'][0], flag[0])


# ---- the host side of the reweight lane ---------------------------------------------------------------------------------------------------

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
    i, dp, ip = ct.c_int, ct.POINTER(ct.c_double), ct.POINTER(ct.c_int)
    so.lin_irls_reweight.argtypes, so.lin_irls_reweight.restype = [i, i, i, ip, ip, dp, dp, ip, dp, dp, i, dp, dp, dp, ip, dp, dp], i
    return so


def _dp(a):
    return None if a is None else a.ctypes.data_as(ct.POINTER(ct.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(ct.POINTER(ct.c_int))


def _points(model):
    """The seeded points of test_linear_se3_cpu.py (SE(2): the seeded poses of test_linear_gn_cpu.py), factor f joining variables 2 f
    and 2 f + 1."""
    if model == 2:
        return model_points()
    rs = np.random.RandomState(7)
    x = rs.normal(0, 3, (200, 6))
    x[:, [2, 5]] = rs.uniform(-9, 9, (200, 2))
    x[:4, [2, 5]] = 0.0
    return x, rs.normal(0, 2, (200, 3)), rs.uniform(0.5, 20.0, (200, 3))


@pytest.mark.parametrize('model', [1, 2])
def test_host_reweight_lane_matches_the_twin(shim, model):
    pts, z, s = _points(model)
    z = z.copy()
    F, D = pts.shape[0], pts.shape[1] // 2
    N, P2 = 2 * F, D * (2 * D + 1)
    h_fn, jac_fn = (se2_h, se2_jac) if model == 1 else (se3_h, se3_jac)
    h = h_fn(pts, s)
    z[1] = h[1] / s[1]                                       # M = 0: never above a positive threshold
    m = np.linalg.norm(s * z - h, axis=1)
    rs = np.random.RandomState(13)
    loss = np.array([(HUBER, CONSTANT, NONE)[f % 3] for f in range(F)], dtype=np.int32)
    loss[0], loss[1], loss[2] = HUBER, CONSTANT, NONE
    thr = np.where(rs.uniform(size=F) < 0.5, m * rs.uniform(0.2, 0.9, F), m * rs.uniform(1.1, 3.0, F))   # flagged and not, for both losses
    thr[0] = m[0]                                            # M EXACTLY at the threshold: not flagged (M > t is strict)
    thr[1] = 0.5
    thr[2] = 1e-9                                            # a factor at NONE: 1 / 0 whatever the threshold
    va, vb = np.arange(0, N, 2, dtype=np.int32), np.arange(1, N, 2, dtype=np.int32)
    x = np.ascontiguousarray(pts.reshape(N, D))
    zt, st = np.ascontiguousarray(z.T), np.ascontiguousarray(s.T)

    def run(loss_, thr_, first, w_in):
        feta, flam = np.full((2 * D, F), np.nan), np.full((P2, F), np.nan)
        w, flag, e, ch = w_in.copy(), np.full(F, -1, np.int32), np.full(F, np.nan), np.full(F, np.nan)
        n = shim.lin_irls_reweight(model, N, F, _ip(va), _ip(vb), _dp(zt), _dp(st), _ip(loss_), _dp(thr_), _dp(x), first, _dp(feta), _dp(flam), _dp(w), _ip(flag),
                                   _dp(e), _dp(ch))
        return n, feta, flam, w, flag, e, ch

    # the lane's own M (the device's arithmetic) decides the flag at the threshold: M exactly at t means equal in ITS arithmetic, so the
    # threshold of factor 0 is taken from the lane: e = w 0.5 M^2 with w = 1 at a huge threshold
    _, _, _, _, _, e_plain, _ = run(None, None, 1, np.full(F, np.nan))
    thr[0] = np.sqrt(2.0 * e_plain[0])
    flag_w = (loss != NONE) & (m > thr)
    flag_w[0] = False
    safe = np.where(flag_w, m, 1.0)
    want_w = np.where(flag_w, np.where(loss == HUBER, (2 * thr * safe - thr * thr) / safe ** 2, 1.0 / safe ** 2), 1.0)
    assert flag_w.any() and (~flag_w & (loss != NONE)).any() and flag_w[loss == HUBER].any() and flag_w[loss == CONSTANT].any()
    old = rs.uniform(0.1, 1.0, F)
    n, feta, flam, w, flag, e, ch = run(loss, thr, 0, old)

    def close(name, a, b_, tol=1e-12):
        a, b_ = a.reshape(a.shape[0], -1), b_.reshape(b_.shape[0], -1)
        gap = np.abs(a - b_).max(1) / np.maximum(1.0, np.abs(b_).max(1))
        assert np.all(np.isfinite(a)) and gap.max() < tol, f"{name}: {gap.max():.3e} at {gap.argmax()}"

    assert np.array_equal(flag != 0, flag_w) and n == int(flag_w.sum())
    assert flag[0] == 0 and w[0] == 1.0 and flag[1] == 0 and w[1] == 1.0 and e[1] == 0.0 and flag[2] == 0 and w[2] == 1.0
    close('w', w[:, None], want_w[:, None])
    close('energy', e[:, None], (want_w * 0.5 * m * m)[:, None])
    close('change', ch[:, None], np.abs(want_w - old)[:, None])
    J = jac_fn(pts, s)
    b = np.einsum('fki,fi->fk', J, pts) + s * z - h
    iu = np.triu_indices(2 * D)
    lam = np.zeros((F, 2 * D, 2 * D))
    lam[:, iu[0], iu[1]] = flam.T
    lam[:, iu[1], iu[0]] = flam.T
    close('eta', feta.T, np.einsum('fki,fk->fi', J, b)); close('lam', lam, np.einsum('fki,fkj->fij', J, J))     # the NOMINAL factor: the weight is apart
    # first: the old weights are not read and the change is 0
    n1, feta1, flam1, w1, flag1, e1, ch1 = run(loss, thr, 1, np.full(F, np.nan))
    assert n1 == n and not ch1.any() and w1.tobytes() == w.tobytes() and e1.tobytes() == e.tobytes() and feta1.tobytes() == feta.tobytes()
    # no losses set: every weight 1, nothing flagged, the same linearisation bit for bit
    n0, feta0, flam0, w0, flag0, e0, _ = run(None, None, 1, np.full(F, np.nan))
    assert n0 == 0 and not flag0.any() and np.all(w0 == 1.0) and feta0.tobytes() == feta.tobytes() and flam0.tobytes() == flam.tobytes()
    close('plain energy', e0[:, None], (0.5 * m * m)[:, None])


# ---- the order of the stop tests ---------------------------------------------------------------------------------------------------------

def test_weights_are_tested_before_the_move():
    """Without a flagged factor round 1's reweight finds weight_change == 0 AND, solved to a step of 0, a move within tol_move: WEIGHTS
    wins.  With the weight test off the same run ends in MOVE."""
    model, g, opts = graph_of('se2_none_flagged')
    t = twin_of(model, g, losses=True)
    lm = dict(tol_grad=1e-9, tol_step=1e-12)
    a = solve_robust(t, t.mu, max_rounds=5, tol_weight=1e-9, tol_move=1e9, **lm)
    assert (a['rounds'], a['reason'], a['converged']) == (1, IRLS_WEIGHTS, True) and a['weight_change'] == 0.0 and a['move'] <= 1e9
    b = solve_robust(t, t.mu, max_rounds=5, tol_weight=0.0, tol_move=1e9, **lm)
    assert (b['rounds'], b['reason'], b['converged']) == (1, IRLS_MOVE, True)
    assert np.array_equal(a['x'], b['x'])


def test_rounds_running_out_is_none_and_the_weights_are_those_of_the_final_x():
    model, g, opts = graph_of('se2_ring65')
    t = twin_of(model, g, losses=True)
    kept = t.w.copy()
    r = twin_run(t, t.mu, dict(opts, max_rounds=2))
    assert (r['rounds'], r['reason'], r['converged']) == (2, IRLS_NONE, False) and r['rows'].shape == (3, 6)
    w, flag, _ = weights_at(t, r['x'])
    assert np.array_equal(r['weights'], w) and np.array_equal(r['flag'], flag) and not r['rows'][-1, 4:].any()
    assert np.array_equal(t.w, kept)                         # the handle's own weights are not the solver's
    z = twin_run(t, t.mu, dict(opts, max_rounds=0))
    assert z['rounds'] == 0 and np.array_equal(z['x'], t.mu) and z['rows'].shape == (1, 6) and np.array_equal(z['weights'], weights_at(t, t.mu)[0])


def test_a_round_that_stalls_goes_on():
    model, g, opts = graph_of('se3_stall')
    t = twin_of(model, g, losses=True)
    r = twin_run(t, t.mu, opts)
    print('LM reasons per round', r['rows'][:, 5].tolist(), 'outer', r['rows'][:, 4].tolist(), 'reason', r['reason'])
    assert r['rows'][0, 5] == STALL and r['rounds'] >= 2 and r['rejected'] >= 3
    model, g, opts = graph_of('se3_reject')
    r = twin_run(twin_of(model, g, losses=True), t.mu, opts)
    assert r['rejected'] >= 3 and STALL not in r['rows'][:, 5]


# ---- the GPU cases are decidable ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(CASES))
def test_gpu_cases_stay_clear_of_every_decision(name):
    model, g, opts = graph_of(name)
    t = twin_of(model, g, losses=True)
    r = twin_run(t, t.mu, opts)
    grads = [abs(v - opts['tol_grad']) for gs in r['grads'] for v in gs]
    print(f"{name}: rounds {r['rounds']} outer {r['outer']} reason {r['reason']} flagged {r['rows'][:, 1].astype(int).tolist()} threshold margin "
          f"{min(r['margins'], default=np.inf):.2e} dPhi clearance {min_clearance(r['lm_rows']):.2e} gradient clearance {min(grads, default=np.inf):.2e}")
    assert min(r['margins'], default=np.inf) >= CLEAR and min_clearance(r['lm_rows']) >= CLEAR and min(grads, default=np.inf) >= GRAD_CLEAR


def test_cases_exercise_what_they_are_for():
    for tag in ('se2', 'se3'):
        run = lambda name: twin_run(*(lambda m, g, o: (twin_of(m, g, losses=True), twin_of(m, g, losses=True).mu, o))(*graph_of(name)))
        a, n, s = run(tag + '_all_flagged'), run(tag + '_none_flagged'), run(tag + '_some_lossy')
        assert np.all(a['rows'][:, 1] == 70) and not n['rows'][:, 1].any() and n['reason'] == IRLS_WEIGHTS and n['rounds'] == 1
        assert 0 < s['flagged'] < 70 and len(set(s['rows'][:, 1])) > 1                   # flags change between the rounds
    assert {len(graph_of(f'se3_chain{F}')[1]['va']) for F in (0, 1, 63, 64, 65, 255, 256, 257)} == {0, 1, 63, 64, 65, 255, 256, 257}
    assert len(graph_of('se2_ring257')[1]['va']) == 257 and len(graph_of('se3_ring65')[1]['va']) == 65


def test_final_x_spread_between_inner_tolerances():
    """What bounds the device's final x: the twin's own spread between runs whose dense solves are moved by vectors of residual
    1e-12 |eta| and 1e-14 |eta|.  X_TOL is 10 x the largest, and the runs make the same decisions."""
    worst = 0.0
    for name in CASES:
        model, g, opts = graph_of(name)
        t = twin_of(model, g, losses=True)
        if not t.N:
            continue
        a, b = twin_run(t, t.mu, opts, perturb=1e-12), twin_run(t, t.mu, opts, perturb=1e-14)
        assert a['rows'].shape == b['rows'].shape and np.array_equal(a['rows'][:, [1, 4, 5]], b['rows'][:, [1, 4, 5]]), name
        worst = max(worst, float(np.abs(a['x'] - b['x']).max() / max(1.0, np.abs(b['x']).max())))
    print(f'largest spread {worst:.3e}, X_TOL {X_TOL:.3e}')
    assert worst <= X_TOL / 10 and X_TOL <= 20 * worst


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def capi():
    from gbp_amd import build, _capi
    build.build()
    return _capi


def test_struct_layouts_and_binding(capi):
    O, I = capi.LinIrlsOpts, capi.LinIrlsInfo
    assert ct.sizeof(O) == 8 + 2 * 8 + ct.sizeof(capi.LinNlmapOpts) == 112 and O.tol_weight.offset == 8 and O.lm.offset == 24
    assert ct.sizeof(I) == 8 * 4 + 5 * 8 == 72 and I.energy0.offset == 32
    text = open(os.path.join(REPO, 'include', 'gbp_lin.h')).read()
    for name, T in (('gbp_lin_irls_opts_t', O), ('gbp_lin_irls_info_t', I)):
        body = re.sub(r'/\*.*?\*/', '', re.search(r'typedef struct \{([^}]*)\} %s;' % name, text).group(1), flags=re.S)
        names = [n for decl in body.split(';') for n in re.findall(r'\*?\b([a-z_0-9]+)\s*(?:,|$)', decl.strip())]
        assert names == [f[0] for f in T._fields_], name
    bare = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for k, v in (('NONE', 0), ('WEIGHTS', 1), ('MOVE', 2)):
        assert re.search(r'#define\s+GBP_LIN_IRLS_%s\s+%d\b' % (k, v), bare) and getattr(capi, 'LIN_IRLS_' + k) == v
    lib = capi.load()
    assert lib.gbp_lin_solve_map_nonlinear_robust is not None
    from gbp_amd.linear import LinearEngine
    assert callable(LinearEngine.solve_map_nonlinear_robust)
