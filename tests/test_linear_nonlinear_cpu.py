"""CPU-side checks of the nonlinear (SE(2) relative-pose) path of the linear engine: the numpy twin of tests/lin_nonlin_cases.py against
the reference's own run (fixture G25, tests/golden/make_g25.py), the distance of every seeded GPU case from the relinearisation
threshold, and the header, struct layout and binding of the new ABI (include/gbp_lin.h)."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from conftest import REPO, golden
from lin_map_cases import rel
from lin_nonlin_cases import CASES, SWEEPS, g25_graph, g25_schedule, run_margin, twin_of

# Observed maximum gaps of the twin from the reference over both tags of G25 (relative, max-norm): means 3.1e-13, energy 3.4e-12,
# factors 2.0e-13, linpoints 3.1e-13, messages 1.1e-13, beliefs 2.2e-16 (the anchored pose's prior of 1e6 sets the scale of what an
# inverse against a solve may differ by).  The bound is <= 100 x the largest of them.
TWIN_TOL = 1e-10


@pytest.mark.parametrize('tag', ['main', 'b0'])
def test_twin_equals_the_reference_run(tag):
    """Masks, iters_since_relin and per-factor damping exactly in every sweep; means, energy, factors, messages and beliefs tightly."""
    g = golden('G25_se2_posegraph')
    sched, sweeps = g25_schedule(g, tag)
    t = twin_of(g25_graph(g), sched)
    gaps = {}

    def gap(name, a, b):
        gaps[name] = max(gaps.get(name, 0.0), rel(a, b))

    for s in range(sweeps):
        mask = t.synchronous_iteration()
        assert np.array_equal(mask, g[f'{tag}_mask'][s].astype(bool)), f"sweep {s}: mask"
        assert np.array_equal(t.iters, g[f'{tag}_iters'][s]), f"sweep {s}: iters"
        assert np.array_equal(t.fdamp, g[f'{tag}_damp'][s]), f"sweep {s}: damping"
        gap('means', t.get_means(), g[f'{tag}_means'][s])
        gap('energy', t.energy(), g[f'{tag}_energy'][s])
        k = f'{tag}_s{s + 1}_'
        if k + 'feta' in g:
            gap('factor', t.feta, g[k + 'feta']); gap('factor', t.flam, g[k + 'flam']); gap('linpoint', t.linpoint, g[k + 'linpoint'])
            for name, a in zip(('msg_eta_a', 'msg_lam_a', 'msg_eta_b', 'msg_lam_b'), t.messages()):
                gap('messages', a, g[k + name])
            gap('beliefs', t.be, g[k + 'bel_eta']); gap('beliefs', t.bl, g[k + 'bel_lam'])
    print(tag, {k: f'{v:.2e}' for k, v in gaps.items()})
    assert set(gaps) == {'means', 'energy', 'factor', 'linpoint', 'messages', 'beliefs'}
    for k, v in gaps.items():
        assert v < TWIN_TOL, f"{k}: {v:.3e}"
    if tag == 'main':
        eta, lam = t.joint()
        mu = np.linalg.solve(lam, eta)
        assert rel(mu, g['main_map_mu']) < 1e-9                                 # cond(Lambda) ~ 1e6: not the sweep's tolerance
        assert float(g['main_margin']) >= 1e-7


def test_fixture_is_what_the_issue_describes():
    g = golden('G25_se2_posegraph')
    assert g['edges'].shape == (35, 2) and g['prior_eta'].shape == (30, 3)
    assert g['main_mask'].shape == (60, 35) and g['b0_mask'].shape == (15, 35)
    counts = g['main_mask'].sum(1)
    assert counts[0] == 0 and counts[1] == 35 and 100 < counts.sum() < 250      # nothing can move before the first sweep; then all
    assert g['b0_mask'].sum(1).tolist() == [0] + [35] * 14                      # dist is exactly 0 before the first sweep
    assert np.ptp(g['truth'][:, 2]) > 2 * np.pi                                 # headings are not wrapped


@pytest.mark.parametrize('name', [c[0] for c in CASES])
def test_gpu_cases_stay_clear_of_the_threshold(name):
    """Every seeded case of test_linear_nonlinear_gpu.py: the twin's distance from `dist > beta` is >= 1e-9 before every sweep, so the
    device's masks can be compared exactly and no GPU case is skipped or cut short."""
    _, build, sched = next(c for c in CASES if c[0] == name)
    m = run_margin(build(), sched, SWEEPS)
    print(name, f'{m:.3e}')
    assert m >= 1e-9


def test_twin_relinearises_in_the_cases():
    """The cases exercise what they are for: some factors relinearise, not all in every sweep."""
    _, build, sched = next(c for c in CASES if c[0] == 'ring129')
    t = twin_of(build(), sched)
    counts = t.iterate(SWEEPS, relinearise=True)
    assert counts[0] == 0 and counts.max() == t.F and 0 < np.count_nonzero(counts) < SWEEPS


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------

NEW = ['gbp_lin_set_nonlinear', 'gbp_lin_relinearise', 'gbp_lin_iterate_nonlinear', 'gbp_lin_get_linearisation']


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
    assert re.search(r'#define\s+GBP_LIN_MODEL_SE2_BETWEEN\s+1\b', text) and capi.LIN_MODEL_SE2_BETWEEN == 1


def test_nonlinear_desc_matches_header_layout(capi):
    # 4 int32, 1 double, 2 pointers on LP64, in the header's order
    S = capi.LinNonlinear
    assert ct.sizeof(S) == 16 + 8 + 16
    assert [f[0] for f in S._fields_] == ['model', 'num_undamped_iters', 'min_linear_iters', 'reserved', 'beta', 'measurement', 'sqrt_info']
    assert (S.beta.offset, S.measurement.offset, S.sqrt_info.offset) == (16, 24, 32)
    text = open(os.path.join(REPO, 'include', 'gbp_lin.h')).read()
    body = re.search(r'typedef struct \{([^}]*)\} gbp_lin_nonlinear_desc_t;', text).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = re.findall(r'\*?\b([a-z_]+)\s*;', body)
    assert names == [f[0] for f in S._fields_]


def test_null_handle_is_reported_not_crashed(capi):
    lib = capi.load()
    assert lib.gbp_lin_set_nonlinear(None, None) == -1
    assert lib.gbp_lin_relinearise(None, None) == -1
    assert lib.gbp_lin_iterate_nonlinear(None, 1, None) == -1
    assert lib.gbp_lin_get_linearisation(None, None, None, None) == -1
