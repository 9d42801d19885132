"""CPU-side checks of robust losses on the nonlinear (SE(2) relative-pose) path of the linear engine: the numpy twin of
tests/lin_nonlin_robust_cases.py against the reference's own robust relinearising run (fixture G27, tests/golden/make_g27.py), the
distance of every seeded GPU case from both discontinuous tests of a sweep, what the cases cover, and the header and binding of the new
ABI (include/gbp_lin.h)."""
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden
from lin_map_cases import rel
from lin_nonlin_robust_cases import CASES, EXTREME, MARGIN, NONE, SWEEPS, g27_graph, g27_schedule, live_schedule, robust_twin, run_margins
from test_linear_nonlinear_cpu import TWIN_TOL


def test_twin_equals_the_reference_run():
    """Flags, relinearisation masks, iters_since_relin and per-factor damping exactly in every sweep; weights, means, energy, the
    factors as the reference holds them (nominal times weight), linpoints, messages and beliefs within TWIN_TOL."""
    g = golden('G27_se2_posegraph_robust')
    sched, sweeps = g27_schedule(g)
    t = robust_twin(g27_graph(g), sched)
    gaps = {}

    def gap(name, a, b):
        gaps[name] = max(gaps.get(name, 0.0), rel(a, b))

    for s in range(sweeps):
        mask, flag = t.synchronous_iteration(True, True)
        assert np.array_equal(flag, g['flag'][s].astype(bool)), f"sweep {s}: flags"
        assert np.array_equal(mask, g['mask'][s].astype(bool)), f"sweep {s}: mask"
        assert np.array_equal(t.iters, g['iters'][s]), f"sweep {s}: iters"
        assert np.array_equal(t.fdamp, g['damp'][s]), f"sweep {s}: damping"
        gap('weights', t.w, g['w'][s])
        gap('means', t.get_means(), g['means'][s])
        gap('energy', t.energy(), g['energy'][s])
        k = f's{s + 1}_'
        if k + 'feta' in g:
            gap('factor', t.feta * t.w[:, None], g[k + 'feta']); gap('factor', t.flam * t.w[:, None, None], g[k + 'flam'])
            gap('linpoint', t.linpoint, g[k + 'linpoint'])
            for name, a in zip(('msg_eta_a', 'msg_lam_a', 'msg_eta_b', 'msg_lam_b'), t.messages()):
                gap('messages', a, g[k + name])
            gap('beliefs', t.be, g[k + 'bel_eta']); gap('beliefs', t.bl, g[k + 'bel_lam'])
    print({k: f'{v:.2e}' for k, v in gaps.items()})
    assert set(gaps) == {'weights', 'means', 'energy', 'factor', 'linpoint', 'messages', 'beliefs'}
    for k, v in gaps.items():
        assert v < TWIN_TOL, f"{k}: {v:.3e}"


def test_fixture_is_what_the_issue_describes():
    g = golden('G27_se2_posegraph_robust')
    g25 = golden('G25_se2_posegraph')
    assert g['edges'].shape == (35, 2) and g['prior_eta'].shape == (30, 3)
    if int(g['seed']) == int(g25['seed']):
        assert np.array_equal(g['edges'], g25['edges']) and np.array_equal(g['prior_eta'], g25['prior_eta'])
        assert np.count_nonzero(np.abs(g['z'] - g25['z']).max(1)) == 3               # three corrupted closures
    assert not g['loss'][:29].any() and g['loss'][29:].all() and set(g['loss'][29:].tolist()) == {1, 2}
    assert np.all(g['threshold'][g['loss'] == 1] == 2.0)
    assert float(g['robust_margin']) >= MARGIN and float(g['dist_margin']) >= MARGIN
    flags = g['flag'][:, 29:].astype(bool)
    assert flags.any() and (~flags.any(0)).any() and (flags[1:] != flags[:-1]).any()
    assert not g['flag'][:, :29].any() and np.all(g['w'][:, :29] == 1.0) and np.all(g['w'][g['flag'] == 0] == 1.0)
    assert np.all(g['w'][g['flag'] == 1] < 1.0)


@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_gpu_cases_stay_clear_of_both_thresholds(name):
    """Every seeded case of test_linear_nonlinear_robust_gpu.py: before every sweep the twin is >= 1e-7 away from `M > t` for every
    factor with a loss and from `dist > beta`, so flags, masks and counts can be compared exactly.  Except at the two extreme
    thresholds, some factor with a loss is flagged and some is left unflagged during the run."""
    _, build, sched = next(c for c in CASES if c[0] == name)
    g = build()
    rm, dm, flags = run_margins(g, sched, SWEEPS)
    print(name, f'robust {rm:.3e} distance {dm:.3e}')
    assert rm >= MARGIN and dm >= MARGIN
    lossy = g['loss'] != NONE
    assert lossy.any() and not flags[:, ~lossy].any()
    if name == 'never_flagged':
        assert not flags.any()
    elif name == 'all_flagged':
        assert flags[:, lossy].all()
    else:
        assert name not in EXTREME
        assert flags[:, lossy].any() and (~flags[:, lossy]).any()


def test_live_schedule_stays_clear_of_both_thresholds():
    g0, rounds = live_schedule()
    t = robust_twin(g0)
    rm = dm = np.inf
    for ext, (off, codes, thr), sweeps, shr in rounds:
        F0 = t.F
        t.extend(**ext)
        t.set_robust(codes, thr, first=F0 + off)
        for _ in range(sweeps):
            rm, dm = min(rm, t.robust_margin()), min(dm, t.margin())
            t.synchronous_iteration(True, True)
        if shr:
            t.shrink(**shr)
    print(f'robust {rm:.3e} distance {dm:.3e}')
    assert rm >= MARGIN and dm >= MARGIN


def test_twin_without_losses_is_the_plain_twin():
    """All weights 1: the robust sweep is the plain relinearising sweep, bit for bit."""
    from lin_nonlin_cases import CASES as PLAIN, twin_of
    _, build, sched = next(c for c in PLAIN if c[0] == 'ring65')
    g = build()
    a, b = robust_twin(g, sched), twin_of(g, sched)
    a.set_robust(NONE)
    ca, fa = a.iterate(SWEEPS, relinearise=True, robustify=True)
    cb = b.iterate(SWEEPS, relinearise=True)
    assert np.array_equal(ca, cb) and not fa.any()
    assert all(np.array_equal(x, y) for x, y in zip(a.messages(), b.messages())) and np.array_equal(a.mu, b.mu)


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------

NEW = ['gbp_lin_set_robust_nonlinear', 'gbp_lin_robustify_nonlinear', 'gbp_lin_iterate_nonlinear_robust']


@pytest.fixture(scope='module')
def capi():
    from gbp_amd import build, _capi
    build.build()
    return _capi


def test_new_symbols_declared_exported_and_bound(capi):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'gbp_lin.h')).read(), flags=re.S)
    lib = capi.load()
    for n in NEW:
        assert re.search(r'\bint\s+%s\s*\(' % n, text), f"{n} is not declared in include/gbp_lin.h"
        assert n in capi.SIGNATURES and hasattr(lib, n)
    assert len(capi.SIGNATURES['gbp_lin_set_robust_nonlinear'][1]) == 5 and len(capi.SIGNATURES['gbp_lin_iterate_nonlinear_robust'][1]) == 4


def test_null_handle_is_reported_not_crashed(capi):
    lib = capi.load()
    assert lib.gbp_lin_set_robust_nonlinear(None, 0, 0, None, None) == -1
    assert lib.gbp_lin_robustify_nonlinear(None) == -1
    assert lib.gbp_lin_iterate_nonlinear_robust(None, 1, None, None) == -1


def test_python_surface_routes_by_handle_kind():
    """iterate(n, robustify=True, relinearise=True) no longer raises before it reaches the library; set_robust takes `first`."""
    import inspect
    from gbp_amd.linear import LinearEngine
    assert 'first' in inspect.signature(LinearEngine.set_robust).parameters
    src = inspect.getsource(LinearEngine.iterate)
    assert 'gbp_lin_iterate_nonlinear_robust' in src and 'not supported' not in src
