"""The device instance of the SE(3) and SE(2) factor models, point by point, against exact arithmetic (fixture G31, tests/golden/make_g31.py):
one handle in which the n points are n disjoint pairs of variables, with identity prior precision and the point as prior information,
so that every factor is linearised AT its point.  eta_f comes back through joint_eta() minus the prior, Lambda_f column by column
through twelve joint_matvec calls (the pairs are disjoint: one call reads one column of every factor), the energy through energy() on
one small handle per block, and the device's eval through the Huber weights of a threshold far below every Mahalanobis distance.  The
bounds are those of the CPU test (lin_se3_exact_cases.py): 256 eps of the larger of 1 and the point's largest exact entry.  The views
add roundings of their own -- joint_eta() adds the prior, of the size of the point, to eta_f: at most 21 eps on these points --, which
the bounds cover.  The range kernel of extend_se3 / extend_se2 is checked bit for bit against the whole handle."""
import numpy as np
import pytest

from lin_se3_cases import SCHEDULE
from lin_se3_exact_cases import F_TOL, blocks, fixture, gaps, report_and_check
from test_linear_se3_gpu import same_bits, state

pytestmark = pytest.mark.gpu

THRESHOLD = 1e-6                # the Huber threshold: test_fixture_covers_what_it_should keeps every Mahalanobis distance above 0.1


def pairs_engine(D, x, z, s, first=0, count=None):
    """Pairs first .. first + count - 1 of the points as a handle of 2 count variables: prior_lam = I, prior_eta = the point."""
    from gbp_amd.linear import LinearEngine
    count = x.shape[0] - first if count is None else count
    sl = slice(first, first + count)
    va = 2 * np.arange(count, dtype=np.int32)
    make = LinearEngine.se3_pose_graph if D == 6 else LinearEngine.se2_pose_graph
    return make(va, va + 1, z[sl], s[sl], x[sl].reshape(2 * count, D), np.tile(np.eye(D), (2 * count, 1, 1)), SCHEDULE['beta'],
                SCHEDULE['num_undamped_iters'], SCHEDULE['min_linear_iters'], eta_damping=SCHEDULE['eta_damping'])


def tail(D, x, z, s, first):
    """The arguments of extend_se3 / extend_se2 that append the pairs from `first` on."""
    n = x.shape[0] - first
    va = 2 * np.arange(first, first + n, dtype=np.int32)
    return va, va + 1, z[first:], s[first:], x[first:].reshape(2 * n, D), np.tile(np.eye(D), (2 * n, 1, 1))


def device_factors(e, D, x):
    """(eta_f (n, 2 D), Lambda_f (n, 2 D, 2 D)) of every pair as the solvers read them, the prior taken off."""
    n = x.shape[0]
    eta = e.joint_eta().reshape(n, 2 * D) - x
    lam = np.zeros((n, 2 * D, 2 * D))
    for k in range(2 * D):
        v = np.zeros((n, 2 * D))
        v[:, k] = 1.0
        lam[:, :, k] = e.joint_matvec(v).reshape(n, 2 * D) - v
    return eta, lam


def device_m2(e):
    """The squared Mahalanobis distance of every factor from its Huber weight w = (2 t M - t^2) / M^2 (gbp_lin_robust.hpp), every
    factor flagged: M = t (1 + sqrt(1 - w)) / w, the root above t."""
    e.set_robust('huber', THRESHOLD)
    e.robustify_all_factors()
    w, flag = e.weights()
    assert flag.all() and np.all((w > 0) & (w < 1e-4))
    m = THRESHOLD * (1.0 + np.sqrt(1.0 - w)) / w
    return m * m


def check_model(D, x, z, s, want_eta, want_lam, want_energy, want_m2, parts, what):
    n = x.shape[0]
    e = pairs_engine(D, x, z, s)
    lp, it, dm = e.linearisation()
    assert lp.tobytes() == np.ascontiguousarray(x).tobytes(), "identity priors: every factor is linearised at its point, bit for bit"
    assert np.all(it == 1) and not dm.any() and e.get_means().tobytes() == np.ascontiguousarray(x).tobytes()
    eta, lam = device_factors(e, D, x)
    assert np.array_equal(lam, np.swapaxes(lam, 1, 2))                       # one stored entry behind both halves
    # the range kernel: a third of the pairs at create, the rest appended
    part = pairs_engine(D, x, z, s, 0, n // 3)
    (part.extend_se3 if D == 6 else part.extend_se2)(*tail(D, x, z, s, n // 3))
    assert part.sizes() == e.sizes() == (2 * n, n)
    assert same_bits(state(part), state(e)), "factors linearised over a range differ from those linearised with the whole graph"
    part.close()
    m2 = device_m2(e)
    e.close()
    report_and_check(what, gaps((eta, lam, m2), (want_eta, want_lam, want_m2), names=('eta', 'lam', 'm2')), parts)
    # the energy: one small handle per block, so that no block's error hides in another's magnitude; the per-point bound summed
    bad = []
    for name, idx in parts:
        b = pairs_engine(D, x[idx], z[idx], s[idx])
        got, want = b.energy(), float(np.sum(want_energy[idx]))
        b.close()
        room = F_TOL * float(np.sum(np.maximum(1.0, want_energy[idx])))
        print(f'{what} {name:10s} energy {got!r} exact {want!r} gap / bound {abs(got - want) / room:.3f}')
        if not abs(got - want) < room:
            bad.append(f'{name}: {got!r} vs {want!r}, bound {room:.3e}')
    assert not bad, f'{what} energy: ' + '; '.join(bad)


def test_se3_device_model_equals_exact_arithmetic():
    """k_lin_relin<SE3> in its init mode, k_lin_relin_range<SE3>, k_lin_energy_nl<SE3> and the robustify lane on all points of G31 --
    two blocks of the relinearise stage with a ragged tail --, per block, the blocks beside pi and beside 2 pi included."""
    g = fixture()
    assert g['x'].shape[0] > 256 and g['x'].shape[0] % 256
    check_model(6, g['x'], g['z'], g['s'], g['eta'], g['lam'], g['energy'], g['m2'], blocks(g), 'device SE(3)')


def test_se2_device_model_equals_exact_arithmetic():
    """The SE(2) block the same way through se2_pose_graph: angles up to 1e6 on either end, never wrapped."""
    g = fixture()
    x = g['se2_x']
    check_model(3, x, g['se2_z'], g['se2_s'], g['se2_eta'], g['se2_lam'], g['se2_energy'], g['se2_m2'], [('se2', np.arange(x.shape[0]))], 'device SE(2)')
