"""The linear pairwise GBP engine (include/gbp_lin.h) at its edges: the wave / LDS-staging / reduction-block boundaries of
k_lin_factor, k_lin_belief and k_lin_energy, degree and adjacency shapes, an independent high-precision reference (the dense
joint solution on trees and at the loopy fixed point), million-factor rings, the energy far from the origin and the state / API
edges.  fp64 throughout: beliefs (eta, Lambda), both messages of every factor, means and energy to 1e-9 relative against the
numpy oracle (LinearOracleBatched, pinned to LinearOracle by tests/test_linear_oracle.py)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-9
EPS = np.finfo(np.float64).eps
SIGMAS = [(0.0, 1.0), (1e3, 0.1), (1e5, 0.01), (1e6, 0.001)]       # (offset of the map from the origin, measurement sigma)


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)) if b.size else 0.0


def vpw(D):
    """Variables per wave of k_lin_belief: 64 / (d + d(d+1)/2)."""
    return 64 // (D + D * (D + 1) // 2)


def generic_factors(rs, D, F):
    """Random linear factors over [a; b]: J (d+1) x 2d, so Lambda_f = J^T J is rank-deficient for d > 1, as a real factor is."""
    J = rs.randn(F, D + 1, 2 * D)
    z = rs.randn(F, D + 1)
    return np.einsum('fmi,fm->fi', J, z), np.einsum('fmi,fmj->fij', J, J), 0.5 * np.einsum('fm,fm->f', z, z)


def random_priors(rs, N, D):
    A = rs.randn(N, D, D)
    return rs.randn(N, D), A @ A.transpose(0, 2, 1) + 2.0 * np.eye(D)


def random_pairs(rs, N, F):
    va = rs.randint(0, N, F)
    return va, (va + 1 + rs.randint(0, N - 1, F)) % N


def ring(N, k):
    va = np.repeat(np.arange(N), k)
    return va, (va + np.tile(np.arange(1, k + 1), N)) % N


def run_both(va, vb, fe, fl, pe, pl, fc=None, damping=0.3, sweeps=10):
    from gbp_amd.linear import LinearEngine
    from oracle.linear_oracle import LinearOracleBatched
    e = LinearEngine(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=damping)
    o = LinearOracleBatched(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=damping)
    e.update_all_beliefs(); o.update_all_beliefs()
    e.iterate(sweeps); o.iterate(sweeps)
    return e, o


def assert_matches_oracle(e, o, sample=None, energy=True):
    """Beliefs, means and both messages of every factor (or of the factors in `sample`) to TOL; the energy to TOL relative
    (near the origin, where the oracle's expanded form does not cancel)."""
    for name, a, b in zip(('eta', 'lam'), e.beliefs(), o.beliefs()):
        assert rel(a, b) < TOL, f"belief {name}: {rel(a, b):.3e}"
    assert rel(e.get_means(), o.get_means()) < TOL, f"means: {rel(e.get_means(), o.get_means()):.3e}"
    for name, a, b in zip(('eta_a', 'lam_a', 'eta_b', 'lam_b'), e.messages(), o.messages()):
        if sample is not None:
            a, b = a[sample], b[sample]
        assert rel(a, b) < TOL, f"message {name}: {rel(a, b):.3e}"
    if energy:
        ee, eo = e.energy(), o.energy()
        assert abs(ee - eo) <= TOL * max(abs(eo), 1.0), f"energy {ee!r} vs {eo!r}"


# ---- layout boundaries ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('F', [1, 63, 64, 65, 128, 129, 255, 256, 257])
@pytest.mark.parametrize('D', [1, 2, 3, 4, 5, 6])
def test_factor_count_boundaries(D, F):
    """Full and partial waves of k_lin_factor and its LDS staging (64 / (d+P) records per store), and the 256-factor
    blocks of k_lin_energy."""
    rs = np.random.RandomState(1000 * D + F)
    N = 2 + F // 3
    va, vb = random_pairs(rs, N, F)
    fe, fl, fc = generic_factors(rs, D, F)
    pe, pl = random_priors(rs, N, D)
    e, o = run_both(va, vb, fe, fl, pe, pl, fc)
    assert_matches_oracle(e, o)


@pytest.mark.parametrize('dn', [-1, 0, 1])
@pytest.mark.parametrize('D', [1, 2, 3, 4, 5, 6])
def test_variable_count_boundaries(D, dn):
    """N = VPW k - 1, VPW k, VPW k + 1 around the waves of k_lin_belief (VPW = 32 / 12 / 7 / 4 / 3 / 2)."""
    rs = np.random.RandomState(2000 * D + dn + 5)
    N = vpw(D) * 5 + dn
    F = 2 * N + 3
    va, vb = random_pairs(rs, N, F)
    fe, fl, fc = generic_factors(rs, D, F)
    pe, pl = random_priors(rs, N, D)
    e, o = run_both(va, vb, fe, fl, pe, pl, fc)
    assert_matches_oracle(e, o)


# ---- degree and adjacency shapes -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('D', [1, 3, 6])
def test_degree_and_adjacency_shapes(D):
    """Isolated variables, every degree 1..9 (around the four-way unrolled accumulation), a hub of degree 2 000, one pair
    joined three times in both orientations, and sides a / b interleaved in every variable's adjacency."""
    rs = np.random.RandomState(30 + D)
    hub, n_leaf = 0, 2000
    leaves = np.arange(1, n_leaf + 1)
    pairs = [(hub, l) if i % 2 else (l, hub) for i, l in enumerate(leaves)]          # the hub alternates sides
    nxt = n_leaf + 1
    for k in range(1, 10):                                                          # u_k has exactly degree k
        u, nxt = nxt, nxt + 1
        for j, l in enumerate(rs.choice(leaves, k, replace=False)):
            pairs.append((u, l) if j % 2 else (l, u))
    p, q, nxt = nxt, nxt + 1, nxt + 2
    pairs += [(p, q), (q, p), (p, q)]                                               # duplicates, both orientations
    isolated = list(range(nxt, nxt + 5))
    N = nxt + 5
    pairs = [pairs[i] for i in rs.permutation(len(pairs))]                          # mixes the sides in factor-id order
    va, vb = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs])
    deg = np.bincount(np.concatenate([va, vb]), minlength=N)
    assert deg[hub] >= 2000 and all(d in deg for d in range(10)) and (deg[isolated] == 0).all()
    F = len(pairs)
    fe, fl, fc = generic_factors(rs, D, F)
    pe, pl = random_priors(rs, N, D)
    e, o = run_both(va, vb, fe, fl, pe, pl, fc)
    assert_matches_oracle(e, o)
    eta, lam = e.beliefs()
    assert np.array_equal(eta[isolated], pe[isolated]) and np.array_equal(lam[isolated], pl[isolated])


# ---- an independent high-precision reference -----------------------------------------------------------------------------

def joint_system(N, D, va, vb, fe, fl, pe, pl):
    """The joint information form over all variables, assembled from the factors as compat/gbp/gbp.py:83 does."""
    lam = np.zeros((N * D, N * D))
    eta = pe.reshape(-1).copy()
    for v in range(N):
        lam[v * D:(v + 1) * D, v * D:(v + 1) * D] += pl[v]
    for f in range(len(va)):
        idx = np.concatenate([np.arange(va[f] * D, (va[f] + 1) * D), np.arange(vb[f] * D, (vb[f] + 1) * D)])
        lam[np.ix_(idx, idx)] += fl[f]
        eta[idx] += fe[f]
    return eta, lam


def refined_solve(A, B, rounds=4):
    """A^-1 B in float64 with iterative refinement, residuals in long double."""
    Al, Bl = A.astype(np.longdouble), B.astype(np.longdouble)
    X = np.linalg.solve(A, B)
    for _ in range(rounds):
        R = Bl - Al @ X.astype(np.longdouble)
        X = X + np.linalg.solve(A, R.astype(np.float64))
    return X


def tree_diameter(N, va, vb):
    adj = [[] for _ in range(N)]
    for a, b in zip(va, vb):
        adj[a].append(b); adj[b].append(a)

    def far(s):
        dist = [-1] * N
        dist[s], todo = 0, [s]
        for v in todo:
            for w in adj[v]:
                if dist[w] < 0:
                    dist[w] = dist[v] + 1
                    todo.append(w)
        return int(np.argmax(dist)), max(dist)
    return far(far(0)[0])[1]


@pytest.mark.parametrize('shape', ['chain', 'tree'])
@pytest.mark.parametrize('D', [2, 5])
def test_tree_is_exact_against_the_joint_solution(D, shape):
    """On a tree with damping 0, GBP is exact after diameter + 2 sweeps: means and belief covariances against the dense
    joint solution Lambda_joint^-1 eta_joint, solved with iterative refinement."""
    rs = np.random.RandomState(40 + D + (shape == 'tree'))
    N = 60 if shape == 'chain' else 80
    if shape == 'chain':
        va, vb = np.arange(N - 1), np.arange(1, N)
    else:
        child = np.arange(1, N)
        parent = np.array([rs.randint(0, c) for c in child])
        flip = rs.rand(N - 1) < 0.5
        va, vb = np.where(flip, parent, child), np.where(flip, child, parent)
    fe, fl, fc = generic_factors(rs, D, N - 1)
    pe, pl = random_priors(rs, N, D)
    from gbp_amd.linear import LinearEngine
    e = LinearEngine(va, vb, fe, fl, pe, pl, factor_const=fc)
    e.update_all_beliefs()
    e.iterate(tree_diameter(N, va, vb) + 2)
    eta_j, lam_j = joint_system(N, D, va, vb, fe, fl, pe, pl)
    mu = refined_solve(lam_j, eta_j[:, None])[:, 0]
    cov = refined_solve(lam_j, np.eye(N * D))
    assert rel(e.get_means(), mu) < TOL, f"means vs joint MAP: {rel(e.get_means(), mu):.3e}"
    _, lam_b = e.beliefs()
    cov_b = np.linalg.inv(lam_b)
    cov_j = np.array([cov[v * D:(v + 1) * D, v * D:(v + 1) * D] for v in range(N)])
    assert rel(cov_b, cov_j) < TOL, f"belief covariances vs joint marginals: {rel(cov_b, cov_j):.3e}"


def test_loopy_ring_fixed_point_is_the_joint_map():
    """Loopy GBP on a Gaussian graph converges to the exact means: a k = 3 ring run to its fixed point (about 1 300 damped
    sweeps reach 1e-13 per sweep in the oracle)."""
    from gbp_amd.linear import LinearEngine
    from oracle.linear_oracle import displacement_graph
    rs = np.random.RandomState(50)
    N, D = 100, 3
    va, vb = ring(N, 3)
    J, z, fe, fl, fc, pe, pl = displacement_graph(va, vb, rs.rand(N, D) * 10, 1.0, rs)
    e = LinearEngine(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=0.3)
    e.update_all_beliefs()
    e.iterate(2000)
    before = e.get_means()
    e.iterate(1)
    after = e.get_means()
    step = float(np.max(np.abs(after - before)) / np.max(np.abs(after)))
    assert step < 1e-12, f"not converged: last sweep moved the means by {step:.3e}"
    eta_j, lam_j = joint_system(N, D, va, vb, fe, fl, pe, pl)
    mu = refined_solve(lam_j, eta_j[:, None])[:, 0]
    assert rel(after, mu) < 1e-8, f"fixed point vs joint MAP: {rel(after, mu):.3e}"


# ---- scale ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,D,k', [(200_000, 3, 5), (20_000, 6, 5)])
def test_large_ring_against_the_batched_oracle(N, D, k):
    """The tools/bench_linear.py ring (1M factors at d = 3) and a d = 6 ring of 100k factors, 10 damped sweeps: every belief
    and mean, and both messages of a seeded sample of 100k factors."""
    rs = np.random.RandomState(0)
    mu0 = rs.rand(N, D) * 10
    va, vb = ring(N, k)
    F = va.shape[0]
    z = mu0[vb] - mu0[va] + rs.normal(0, 1.0, (F, D))
    J = np.hstack([-np.eye(D), np.eye(D)])
    fe = z @ J
    fl = np.ascontiguousarray(np.broadcast_to(J.T @ J, (F, 2 * D, 2 * D)))
    fc = 0.5 * np.einsum('fd,fd->f', z, z)
    pl = np.ascontiguousarray(np.broadcast_to(np.eye(D) / 3.0, (N, D, D)))
    e, o = run_both(va, vb, fe, fl, mu0 / 3.0, pl, fc)
    sample = np.random.RandomState(1).choice(F, min(F, 100_000), replace=False)
    assert_matches_oracle(e, o, sample=sample)


# ---- energy far from the origin ------------------------------------------------------------------------------------------

def energy_bound(e_ref, fc):
    """1e-9 relative, plus the rounding the caller's float64 constants c_f already carry (4 eps sum c_f)."""
    return TOL * abs(e_ref) + 4 * EPS * float(np.sum(np.abs(fc)))


@pytest.mark.parametrize('off,sigma', SIGMAS)
@pytest.mark.parametrize('D', [2, 3, 6])
@pytest.mark.parametrize('shape', ['chain', 'ring'])
def test_energy_far_from_the_origin(shape, D, off, sigma):
    """linear_displacement factors on a map `off` from the origin with noise `sigma`, priors of ndim_posegraph.py
    (sigma 3 around the true positions): the engine's energy against the exact residual energy at the engine's OWN means
    (which isolates the energy kernel from the conditioning of the means)."""
    from gbp_amd.linear import LinearEngine
    from oracle.linear_oracle import displacement_graph, residual_energy
    rs = np.random.RandomState(60 + D)
    if shape == 'chain':
        N = 400
        va, vb = np.arange(N - 1), np.arange(1, N)
        damping, sweeps = 0.0, N + 1                       # exact on a chain: the energy is the small one at the MAP
    else:
        N = 120
        va, vb = ring(N, 2)
        damping, sweeps = 0.3, 200
    J, z, fe, fl, fc, pe, pl = displacement_graph(va, vb, off + rs.rand(N, D) * 10, sigma, rs)
    e = LinearEngine(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=damping)
    e.update_all_beliefs()
    e.iterate(sweeps)
    got = e.energy()
    ref = residual_energy(e.get_means(), va, vb, J, z, sigma)
    bound = energy_bound(ref, fc)
    print(f"ENERGY {shape} d={D} off={off:g} sigma={sigma:g}: E_ref {ref:.10g} |err| {abs(got - ref):.3e} bound {bound:.3e}")
    assert abs(got - ref) <= bound, f"energy {got!r} vs exact residual energy {ref!r}: |err| {abs(got - ref):.3e} > {bound:.3e}"


@pytest.mark.parametrize('off,sigma', SIGMAS)
def test_host_graph_energy_far_from_the_origin(off, sigma):
    """The same through the drop-in host graph (ndim_posegraph.py:67-91) moved to the device: the device energy against
    graph.energy(), the reference's residual form, evaluated at the device's means."""
    from conftest import REPO
    from gbp_amd.linear import LinearEngine
    compat = os.path.join(REPO, 'gbp_amd', 'compat')
    sys.path.insert(0, compat)
    try:
        from gbp import gbp
        from gbp.factors import linear_displacement
        rs = np.random.RandomState(3)
        n, dim = 30, 4
        mu0 = off + rs.rand(n, dim) * 10
        graph = gbp.FactorGraph(nonlinear_factors=False, eta_damping=0.2)
        for i in range(n):
            v = gbp.VariableNode(i, dim)
            v.prior.lam = np.eye(dim) / 9.0
            v.prior.eta = v.prior.lam @ mu0[i]
            graph.var_nodes.append(v)
        f = 0
        for i in range(n):
            for j in (i + 1, i + 5):
                if j < n:
                    a, b = graph.var_nodes[i], graph.var_nodes[j]
                    fac = gbp.Factor(f, [a, b], mu0[j] - mu0[i] + rs.normal(0, sigma, dim), sigma, linear_displacement.meas_fn,
                                     linear_displacement.jac_fn, loss=None, mahalanobis_threshold=2)
                    a.adj_factors.append(fac); b.adj_factors.append(fac); graph.factors.append(fac)
                    f += 1
        graph.update_all_beliefs()
        graph.compute_all_factors()
        e = LinearEngine.from_factor_graph(graph)
        e.update_all_beliefs()
        e.iterate(100)
        got = e.energy()
        mu = e.get_means().reshape(n, dim)
        for fac in graph.factors:                        # belief (eta = mu, Lambda = I): the host solve returns mu exactly
            for k, vid in enumerate(fac.adj_vIDs):
                fac.adj_beliefs[k].eta, fac.adj_beliefs[k].lam = mu[vid].copy(), np.eye(dim)
        ref = graph.energy()
        fc = [0.5 * float(fac.measurement @ fac.measurement) / fac.adaptive_gauss_noise_var for fac in graph.factors]
        bound = energy_bound(ref, fc)
        print(f"ENERGY host d={dim} off={off:g} sigma={sigma:g}: E_ref {ref:.10g} |err| {abs(got - ref):.3e} bound {bound:.3e}")
        assert abs(got - ref) <= bound, f"energy {got!r} vs graph.energy() {ref!r}: |err| {abs(got - ref):.3e} > {bound:.3e}"
    finally:
        sys.path.remove(compat)
        for m in [k for k in sys.modules if k == 'gbp' or k.startswith('gbp.') or k == 'utils' or k.startswith('utils.')]:
            del sys.modules[m]


# ---- state and API edges -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('D', [1, 4])
def test_no_factors(D):
    """F = 0: sweeps run, the energy is 0 and the means are the priors' own solution."""
    from gbp_amd.linear import LinearEngine
    rs = np.random.RandomState(70 + D)
    N = 37
    pe, pl = random_priors(rs, N, D)
    e = LinearEngine(np.zeros(0, int), np.zeros(0, int), np.zeros((0, 2 * D)), np.zeros((0, 2 * D, 2 * D)), pe, pl)
    e.update_all_beliefs()
    e.iterate(3)
    assert e.energy() == 0.0
    assert rel(e.get_means(), np.linalg.solve(pl, pe[..., None])[..., 0].reshape(-1)) < 1e-12
    eta, lam = e.beliefs()
    assert np.array_equal(eta, pe) and np.array_equal(lam, pl)


def _small_graph(D, seed, N=50, F=130):
    rs = np.random.RandomState(seed)
    va, vb = random_pairs(rs, N, F)
    fe, fl, fc = generic_factors(rs, D, F)
    pe, pl = random_priors(rs, N, D)
    return va, vb, fe, fl, fc, pe, pl


def _state(e):
    return [*e.beliefs(), e.get_means(), *e.messages(), np.array([e.energy()])]


def _bitwise_equal(s, t):
    return all(np.array_equal(a, b) for a, b in zip(s, t))


@pytest.mark.parametrize('D', [2, 5])
def test_state_edges(D):
    """Messages are zero before the first sweep; iterate(0) changes nothing; update_all_beliefs() twice is bitwise the same;
    factor_const=None is the energy without the constants."""
    from gbp_amd.linear import LinearEngine
    va, vb, fe, fl, fc, pe, pl = _small_graph(D, 80 + D)
    e = LinearEngine(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=0.3)
    e.update_all_beliefs()
    for m in e.messages():
        assert not m.any()
    s0 = _state(e)
    e.iterate(0)
    assert _bitwise_equal(_state(e), s0)
    e.iterate(4)
    s1 = _state(e)
    e.update_all_beliefs()
    s2 = _state(e)
    e.update_all_beliefs()
    assert _bitwise_equal(s2, _state(e))
    assert _bitwise_equal(s1, s2)                      # beliefs are a function of the messages alone
    n = LinearEngine(va, vb, fe, fl, pe, pl, factor_const=None, eta_damping=0.3)
    n.update_all_beliefs()
    n.iterate(4)
    assert _bitwise_equal(_state(n)[:-1], s1[:-1])
    assert abs((n.energy() + fc.sum()) - e.energy()) <= 1e-12 * (abs(e.energy()) + fc.sum())


def test_interleaved_engines_and_repeat_runs_are_bitwise_identical():
    """Two engines of different d interleaved give bitwise what each gives alone, and a second run of the same graph is
    bitwise the first (the engine has no atomics)."""
    from gbp_amd.linear import LinearEngine
    g3, g6 = _small_graph(3, 91, N=300, F=900), _small_graph(6, 92, N=200, F=700)

    def make(g):
        va, vb, fe, fl, fc, pe, pl = g
        e = LinearEngine(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=0.3)
        e.update_all_beliefs()
        return e
    alone = []
    for g in (g3, g6):
        e = make(g)
        e.iterate(12)
        alone.append(_state(e))
        e.close()
    a, b = make(g3), make(g6)
    for _ in range(4):
        a.iterate(3); b.iterate(3)
    assert _bitwise_equal(_state(a), alone[0]) and _bitwise_equal(_state(b), alone[1])
    again = make(g3)
    again.iterate(12)
    assert _bitwise_equal(_state(again), alone[0])
