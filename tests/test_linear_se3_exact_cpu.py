"""The SE(3) and SE(2) factor models against exact arithmetic on a CPU: fixture G31 (tests/golden/make_g31.py -- the models from their
definitions in 60-digit mpmath, independent of the engine's closed forms and of the numpy twin) holds what its docstring says and
regenerates to the bit; the engine's model routines compiled for the host (tests/hostmath/lin_se3_shim.hip) and the numpy twin of
tests/lin_se3_cases.py both equal it within bounds derived from rounding, block by block, up to pi - |phi| = 1e-8."""
import importlib.util
import os

import numpy as np
import pytest

from conftest import GOLDEN
from lin_nonlin_cases import se2_b, se2_h, se2_jac
from lin_se3_cases import se3_h, se3_jac
from lin_se3_exact_cases import QUANTITIES, blocks, exact, fixture, gaps, report_and_check
from test_linear_se3_cpu import _run, _twin_values, shim                            # noqa: F401  (shim: the fixture that builds the host library)


@pytest.fixture(scope='module')
def g():
    return fixture()


def _norms(g):
    x = g['x']
    return np.linalg.norm(x[:, 3:6], axis=1), np.linalg.norm(x[:, 9:12], axis=1), np.linalg.norm(g['phi'], axis=1)


def test_fixture_covers_what_it_should(g):
    x, s, names = g['x'], g['s'], [str(n) for n in g['classes']]
    n = x.shape[0]
    na, nb, phi = _norms(g)
    count = dict(blocks(g))
    assert 256 < n < 512 and n % 256 != 0                                     # past one 256-lane block of the relinearise stage, a ragged tail
    assert all(len(count[k]) > 0 for k in names) and sum(len(v) for v in count.values()) == n
    # the classes of model_points() (test_linear_se3_cpu.py)
    assert np.sum((na == 0) & (nb == 0)) >= 4 and np.sum((na == 0) & (phi > 0.1)) >= 6
    assert np.sum((na > 1e-9) & (na < 1e-4)) >= 20 and np.sum((na > 0.19) & (na < 0.2)) >= 5 and np.sum((na > 0.2) & (na < 0.21)) >= 5
    assert np.sum((na > np.pi) & (na < 4.5)) >= 40 and np.sum(nb > np.pi) >= 20
    assert phi[count['general']].max() > 2.0 and phi[count['general']].max() <= 2.5
    # near pi: every gap, >= 8 points each, the axes and the three kinds of w_a
    for gap in (0.5, 1e-1, 1e-2, 1e-3, 1e-4, 1e-6, 1e-8):
        idx = count[f'pi-{gap:g}']
        got = np.pi - phi[idx]
        assert len(idx) >= 8 and np.all(np.abs(got - gap) <= 1e-6 * gap + 4e-15) and np.all(phi[idx] < np.pi), (gap, got)
        ax = g['phi'][idx] / phi[idx, None]
        small = np.sort(np.abs(ax), axis=1)
        assert np.sum((small[:, 0] < 1e-12) & (small[:, 1] < 1e-12)) >= 3                      # along a coordinate axis
        assert np.sum((small[:, 0] < 1e-12) & (small[:, 1] > 1e-3)) >= 1                       # one component 0 ...
        assert np.sum((small[:, 0] > 1e-10) & (small[:, 0] < 1e-8)) >= 1                       # ... or 1e-9
        assert np.sum(small[:, 0] > 1e-3) >= 3                                                  # random
        assert np.sum(na[idx] == 0) >= 2 and np.sum((na[idx] > 0.3) & (na[idx] < 3)) >= 2 and np.sum((na[idx] > np.pi) & (na[idx] < 4.5)) >= 2
    exact0 = count['pi-1e-08'][np.any(g['x'][count['pi-1e-08'], 9:12] == 0.0, axis=1)]
    assert len(exact0) >= 1                                                   # a component of w_b exactly 0 beside pi
    # 2 pi on both sides and up to 7
    idx = count['twopi']
    for nw in (na[idx], nb[idx]):
        assert np.sum((nw < 2 * np.pi) & (nw > 2 * np.pi - 1e-3)) >= 3 and np.sum((nw > 2 * np.pi) & (nw < 2 * np.pi + 1e-3)) >= 3
        assert np.sum(nw > 6.5) >= 1 and nw.max() <= 7.0
    # t = |w|^2 a few ulp either side of 0.04, as a double computes it; and t subnormal / underflowed
    idx = count['ulp04']
    for w in (x[idx, 3:6], x[idx, 9:12]):
        t = w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1] + w[:, 2] * w[:, 2]
        assert np.all(np.abs(t - 0.04) < 5e-17) and np.sum(t < 0.04) >= 3 and np.sum(t >= 0.04) >= 3
    idx = count['tiny']
    t = np.sum(x[idx, 3:6] ** 2, axis=1)
    assert np.sum(t == 0.0) >= 2 and np.sum((t > 0.0) & (t < 2.3e-308)) >= 2 and np.all(np.abs(x[idx, 3:6]).max(1) > 0)
    # the translation classes
    tn = np.linalg.norm(x[:, 6:9] - x[:, 0:3], axis=1)
    assert np.all(tn[count['bigt']] > 1e3) and s[count['bigt'], :3].max() <= 1.0 and s[count['bigt'], :3].min() >= 1e-3
    assert np.all(s[count['bigs']] == 20.0) and np.all(tn[count['bigs']] < 10.0)
    # every relative rotation is inside the domain, and every measured one (a z_w at or past pi is refused)
    assert phi.max() < np.pi and np.linalg.norm(g['z'][:, 3:], axis=1).max() < np.pi
    # the factor behind the robust view of the GPU test: every Mahalanobis distance far above its threshold of 1e-6
    assert g['m2'].min() > 1e-2 and g['se2_m2'].min() > 1e-2
    # SE(2): every signed angle on both ends
    th = g['se2_x'][:, [2, 5]]
    want = sorted({sg * v for v in (0.0, 1e-9, 1.0, 9.0, 1e3, 1e6) for sg in (1.0, -1.0)})
    assert 36 <= th.shape[0] <= 48 and sorted(set(th[:, 0])) == want and sorted(set(th[:, 1])) == want


def test_fixture_regenerates_to_the_bit(g):
    """Every 16th point recomputed with mpmath equals the committed file bit for bit; so do the seeded points themselves."""
    spec = importlib.util.spec_from_file_location('make_g31', os.path.join(GOLDEN, 'make_g31.py'))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    assert [str(n) for n in g['classes']] == mk.CLASSES
    for prefix, fn, n in (('', mk.exact_se3, g['x'].shape[0]), ('se2_', mk.exact_se2, g['se2_x'].shape[0])):
        for i in range(0, n, 16):
            for k, v in fn(g[prefix + 'x'][i], g[prefix + 'z'][i], g[prefix + 's'][i]).items():
                assert np.asarray(v, dtype=np.float64).tobytes() == np.ascontiguousarray(g[prefix + k][i]).tobytes(), f'{prefix}{k} of point {i}'
    x2, z2, s2 = mk.se2_points()
    assert all(a.tobytes() == g[k].tobytes() for a, k in ((x2, 'se2_x'), (z2, 'se2_z'), (s2, 'se2_s')))


def test_exact_jacobian_is_consistent(g):
    """eta_f, Lambda_f, energy and m2 of the fixture are what its own h and J give in double, to double rounding: the file hangs together."""
    J, h, x, z, s = g['J'], g['h'], g['x'], g['z'], g['s']
    b = np.einsum('fki,fi->fk', J, x) + s * z - h
    r = h - s * z
    got = (h, np.einsum('fki,fk->fi', J, b), np.einsum('fki,fkj->fij', J, J), 0.5 * np.sum(r * r, 1), np.sum(r * r, 1))
    gap = gaps(got, exact(g))
    assert all(gap[q].max() < 64 * 2.0 ** -52 for q in QUANTITIES), {q: gap[q].max() for q in QUANTITIES}
    assert np.all(g['J'][:, 0:3, 9:12] == 0) and np.all(g['J'][:, 3:6, 0:3] == 0) and np.all(g['J'][:, 3:6, 6:9] == 0)


def test_host_se3_routines_equal_exact_arithmetic(shim, g):
    """The engine's routines on the host against the fixture, per block: h within 64 eps, eta_f, Lambda_f, energy and m2 within 256 eps
    of the larger of 1 and the point's largest exact entry -- the blocks beside pi and beside 2 pi included."""
    report_and_check('host SE(3)', gaps(_run(shim.lin_se3_eval, g['x'], g['z'], g['s'], 6), exact(g)), blocks(g))


def test_twin_equals_exact_arithmetic(g):
    report_and_check('twin SE(3)', gaps(_twin_values(se3_h, se3_jac, g['x'], g['z'], g['s']), exact(g)), blocks(g))


def test_host_se2_routines_equal_exact_arithmetic(shim, g):
    parts = [('se2', np.arange(g['se2_x'].shape[0]))]
    report_and_check('host SE(2)', gaps(_run(shim.lin_se2_eval, g['se2_x'], g['se2_z'], g['se2_s'], 3), exact(g, 'se2_')), parts)
    x, z, s = g['se2_x'], g['se2_z'], g['se2_s']
    J, h = se2_jac(x, s), se2_h(x, s)
    b, r = se2_b(J, x, z, s), h - s * z                      # the twin's own b: J x0 + diag(s) z - h summed term by term cancels at theta = 1e6
    twin = (h, np.einsum('fki,fk->fi', J, b), np.einsum('fki,fkj->fij', J, J), 0.5 * np.sum(r * r, 1), np.sum(r * r, 1))
    report_and_check('twin SE(2)', gaps(twin, exact(g, 'se2_')), parts)
