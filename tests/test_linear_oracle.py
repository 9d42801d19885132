"""The linear-GBP oracle (oracle/linear_oracle.py) against fixture G8 = the reference's own ndim_posegraph.py run
(--n_varnodes 100 --dim 3 --n_iters 20): energies, distances to the batch MAP and final means."""
import numpy as np
import pytest

from conftest import golden
from oracle.linear_oracle import LinearOracle, toy_posegraph


def test_linear_oracle_reproduces_reference_trace():
    g8 = golden('G8_toy_linear')
    va, vb, fe, fl, fc, pe, pl = toy_posegraph(100, 3, 10, 1.0, seed=0)
    o = LinearOracle(va, vb, fe, fl, pe, pl, factor_const=fc)
    o.update_all_beliefs()
    mu_map = g8['n100d3_map_mu']
    energy, dist = [], []
    for _ in range(20):
        o.synchronous_iteration()
        energy.append(o.energy())
        dist.append(np.linalg.norm(o.get_means() - mu_map))
    assert np.allclose(energy, g8['n100d3_energy'], rtol=1e-6, atol=1e-3)      # fixture values are the printed 4 decimals
    assert np.allclose(dist, g8['n100d3_dist'], rtol=1e-5, atol=1e-5)
    assert np.allclose(o.get_means(), g8['n100d3_final_means'], rtol=1e-9, atol=1e-9)


def test_linear_oracle_damping_and_energy_identity():
    """Damped messages mix with the old eta only (gbp.py:368); the (eta_f, Lambda_f, const) energy equals the residual form."""
    va, vb, fe, fl, fc, pe, pl = toy_posegraph(12, 2, 3, 0.5, seed=1)
    o = LinearOracle(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=0.4)
    o.update_all_beliefs()
    o.iterate(3)
    e = 0.0
    rs = np.random.RandomState(1)                 # regenerate the measurements the same way toy_posegraph did
    mu0 = rs.rand(12, 2) * 10
    z = []
    pairs = []
    for i, m in enumerate(mu0):
        d = np.array([np.linalg.norm(m - m1) for m1 in mu0])
        for j in d.argsort()[1:4]:
            if [j, i] not in pairs:
                z.append(m - mu0[j] + rs.normal(0., 0.5, 2)); pairs.append([i, j])
    for f, (i, j) in enumerate(pairs):
        r = (o.mu[j] - o.mu[i]) - z[f]
        e += 0.5 * r @ r / 0.25
    assert np.isclose(o.energy(), e, rtol=1e-10)


def _random_graph(D, N, F, seed):
    rs = np.random.RandomState(seed)
    va = rs.randint(0, N, F)
    vb = (va + 1 + rs.randint(0, N - 1, F)) % N
    fe, fl, fc = [], [], []
    for _ in range(F):
        J = rs.randn(D + 1, 2 * D)
        z = rs.randn(D + 1)
        fe.append(J.T @ z); fl.append(J.T @ J); fc.append(0.5 * z @ z)
    A = rs.randn(N, D, D)
    pl = A @ A.transpose(0, 2, 1) + 2.0 * np.eye(D)
    return va, vb, np.array(fe), np.array(fl), np.array(fc), rs.randn(N, D), pl


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize('damping', [0.0, 0.3])
@pytest.mark.parametrize('D', [1, 2, 3, 4, 5, 6])
def test_batched_oracle_equals_the_per_factor_oracle(D, damping):
    """LinearOracleBatched (the reference for the million-factor GPU runs) is LinearOracle: same operands, same order."""
    from oracle.linear_oracle import LinearOracleBatched
    va, vb, fe, fl, fc, pe, pl = _random_graph(D, 30, 90, 100 + D)
    va[:3], vb[:3] = [4, 5, 4], [5, 4, 5]            # duplicate pair in both orientations
    o = LinearOracle(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=damping)
    b = LinearOracleBatched(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=damping)
    for g in (o, b):
        g.update_all_beliefs()
        g.iterate(8)
    for x, y in zip(b.beliefs(), o.beliefs()):
        assert _rel(x, y) < 1e-13
    for x, y in zip(b.messages(), o.messages()):
        assert _rel(x, y) < 1e-13
    assert _rel(b.get_means(), o.get_means()) < 1e-13
    assert abs(b.energy() - o.energy()) < 1e-12 * abs(o.energy())


def test_batched_oracle_reproduces_reference_trace():
    from oracle.linear_oracle import LinearOracleBatched
    g8 = golden('G8_toy_linear')
    va, vb, fe, fl, fc, pe, pl = toy_posegraph(100, 3, 10, 1.0, seed=0)
    o = LinearOracleBatched(va, vb, fe, fl, pe, pl, factor_const=fc)
    o.update_all_beliefs()
    mu_map = g8['n100d3_map_mu']
    energy, dist = [], []
    for _ in range(20):
        o.synchronous_iteration()
        energy.append(o.energy())
        dist.append(np.linalg.norm(o.get_means() - mu_map))
    assert np.allclose(energy, g8['n100d3_energy'], rtol=1e-6, atol=1e-3)
    assert np.allclose(dist, g8['n100d3_dist'], rtol=1e-5, atol=1e-5)
    assert np.allclose(o.get_means(), g8['n100d3_final_means'], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize('D', [1, 3, 6])
def test_residual_energy_matches_the_energy_identity_near_the_origin(D):
    """Exact residual energy == 0.5 x^T Lambda x - eta^T x + c where nothing cancels (origin, sigma = 1), at any means."""
    from oracle.linear_oracle import displacement_graph, residual_energy
    rs = np.random.RandomState(7 + D)
    N = 50
    va, vb = np.arange(N - 1), np.arange(1, N)
    J, z, fe, fl, fc, pe, pl = displacement_graph(va, vb, rs.rand(N, D) * 10, 1.0, rs)
    o = LinearOracle(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=0.2)
    o.update_all_beliefs()
    o.iterate(4)
    assert np.isclose(residual_energy(o.mu, va, vb, J, z, 1.0), o.energy(), rtol=1e-12)
    # a generic (non-displacement) factor with its own sigma per factor
    Js = rs.randn(va.shape[0], D + 1, 2 * D)
    zs = rs.randn(va.shape[0], D + 1)
    sig = 0.5 + rs.rand(va.shape[0])
    mu = rs.randn(N, D)
    want = 0.0
    for f in range(va.shape[0]):
        r = Js[f] @ np.concatenate([mu[va[f]], mu[vb[f]]]) - zs[f]
        want += 0.5 * r @ r / sig[f] ** 2
    assert np.isclose(residual_energy(mu, va, vb, Js, zs, sig), want, rtol=1e-12)
