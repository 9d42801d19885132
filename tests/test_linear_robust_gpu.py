"""The robust (Huber / constant) losses of the linear engine on the MI355X (include/gbp_lin.h: gbp_lin_set_robust / robustify /
iterate_robust / get_weights; kernels in gbp_amd/csrc/gbp_lin_robust.hpp): against the reference's own run (fixture G22), against the
numpy oracle of tests/lin_robust_cases.py on every kernel boundary, far from the origin against exact rational arithmetic, the joint
behind solve_map / marginals at the current weights, the effect on a ring with one gross outlier, and the state / option edges.
fp64 throughout, TOL = 1e-9 as in the other linear tests."""
import ctypes as ct
import os
import sys
from fractions import Fraction

import numpy as np
import pytest

from conftest import REPO, golden
from lin_map_cases import rel
from lin_robust_cases import TOL, RobustOracle, dense_weighted_joint, engine_args, g22_graph, robust_weight, shapes

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SIGMAS = [(0.0, 1.0), (1e3, 0.1), (1e5, 0.01), (1e6, 0.001)]       # as test_linear_edges_gpu.py::test_energy_far_from_the_origin
EINVAL, ESTATE = -1, -5


def make_engine(o):
    from gbp_amd.linear import LinearEngine
    args, kw, rob = engine_args(o)
    e = LinearEngine(*args, **kw)
    e.set_robust(*rob)
    return e


def assert_state_matches(e, o, what):
    """Weights, flags, both messages of every factor, beliefs, means and energy."""
    w, flag = e.weights()
    assert np.array_equal(flag, o.flag), f"{what}: flags differ at {np.nonzero(flag != o.flag)[0][:5]}"
    assert np.max(np.abs(w - o.w) / o.w) < TOL, f"{what}: weights {np.max(np.abs(w - o.w) / o.w):.3e}"
    for name, a, b in zip(('eta_a', 'lam_a', 'eta_b', 'lam_b'), e.messages(), o.messages()):
        assert rel(a, b) < TOL, f"{what}: message {name} {rel(a, b):.3e}"
    for name, a, b in zip(('eta', 'lam'), e.beliefs(), o.beliefs()):
        assert rel(a, b) < TOL, f"{what}: belief {name} {rel(a, b):.3e}"
    assert rel(e.get_means(), o.get_means()) < TOL, f"{what}: means"
    ee, eo = e.energy(), o.energy()
    assert abs(ee - eo) <= TOL * max(abs(eo), 1.0), f"{what}: energy {ee!r} vs {eo!r}"


# ---- the reference's own run --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('loss', ['huber', 'constant'])
@pytest.mark.parametrize('tag', ['n100d3', 'defaults'])
def test_reference_robust_run(tag, loss):
    """Fixture G22: weights and flags of every factor in every one of the 30 sweeps, the energy after each, the final beliefs and
    means, and solve_map at the final weights against joint_distribution_cov's mu."""
    from gbp_amd.linear import LinearEngine
    g = golden('G22_toy_linear_robust')
    va, vb, J, z, sigma, pe, pl = g22_graph(g, tag, loss)
    o = RobustOracle(va, vb, J, z, sigma, pe, pl, loss, 2.0)             # only to form (eta_f, Lambda_f, const_f)
    e = LinearEngine(va, vb, o.fe0, o.fl0, pe, pl, factor_const=o.fc0)
    e.set_robust(loss, 2.0, 1.0)
    e.update_all_beliefs()
    for s in range(30):
        e.synchronous_iteration(robustify=True)
        w, flag = e.weights()
        assert np.array_equal(flag, g[f'{tag}_{loss}_flag'][s].astype(bool)), f"sweep {s}: flags"
        assert rel(w, 1.0 / g[f'{tag}_{loss}_var'][s]) < TOL, f"sweep {s}: weights {rel(w, 1.0 / g[f'{tag}_{loss}_var'][s]):.3e}"
        got, want = e.energy(), g[f'{tag}_{loss}_energy'][s]
        assert abs(got - want) <= TOL * abs(want), f"sweep {s}: energy {got!r} vs {want!r}"
    assert rel(e.get_means(), g[f'{tag}_{loss}_means']) < TOL
    eta, lam = e.beliefs()
    assert rel(eta, g[f'{tag}_{loss}_bel_eta']) < TOL and rel(lam, g[f'{tag}_{loss}_bel_lam']) < TOL
    mu, info = e.solve_map()
    assert info['converged'] and rel(mu, g[f'{tag}_{loss}_map_mu']) < TOL, f"map: {rel(mu, g[f'{tag}_{loss}_map_mu']):.3e}"


# ---- against the numpy oracle --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('damping', [0.0, 0.4])
@pytest.mark.parametrize('D', [1, 2, 3, 4, 5, 6])
def test_robust_sweeps_match_the_oracle(D, damping):
    """F = 1, 63, 64, 65, 129 (wave tails of k_lin_factor, one and several blocks), a hub of degree 203 beside an isolated variable, a
    pair joined twice with different losses, rank-1 factors; the three losses mixed per factor; 10 robust sweeps, everything checked
    after each of them."""
    for name, N, va, vb, J, z, sigma, pe, pl, loss, thr in shapes(D):
        o = RobustOracle(va, vb, J, z, sigma, pe, pl, loss, thr, eta_damping=damping)
        e = make_engine(o)
        e.update_all_beliefs(); o.update_all_beliefs()
        seen = np.zeros(o.F, dtype=bool)
        for s in range(10):
            e.synchronous_iteration(robustify=True); o.synchronous_iteration(robustify=True)
            lossy = np.array([l is not None for l in o.loss])
            assert np.min(np.abs(o.mahalanobis() - o.thr)[lossy], initial=1.0) > 1e-7, f"{name}: a factor sits on its threshold"
            assert_state_matches(e, o, f"d={D} damping={damping} {name} sweep {s}")
            seen |= o.flag
        if o.F >= 63:
            assert seen.any() and not seen.all()
        e.close()


def test_plain_iterate_runs_at_the_weights_as_they_stand():
    """gbp_lin_iterate on a handle with losses: synchronous_iteration(robustify=False) -- the weights of the last robustify stay."""
    name, N, va, vb, J, z, sigma, pe, pl, loss, thr = shapes(3)[4]
    o = RobustOracle(va, vb, J, z, sigma, pe, pl, loss, thr, eta_damping=0.2)
    e = make_engine(o)
    e.update_all_beliefs(); o.update_all_beliefs()
    e.iterate(2); o.iterate(2)                               # weights still 1
    assert_state_matches(e, o, 'before any robustify')
    e.robustify_all_factors(); o.robustify_all_factors()
    w0, _ = e.weights()
    e.iterate(3); o.iterate(3)
    assert_state_matches(e, o, 'three plain sweeps at the weights')
    assert np.array_equal(e.weights()[0], w0) and (w0 < 1.0).any()


# ---- far from the origin ---------------------------------------------------------------------------------------------------------------

def exact_half_m2(mu, va, vb, z, sigma):
    """e_f = |x_b - x_a - z|^2 / (2 sigma^2) of every displacement factor, exactly (fractions.Fraction) from the float64 inputs."""
    out = np.zeros(len(va))
    s2 = Fraction(float(sigma)) ** 2
    for f in range(len(va)):
        r2 = Fraction(0)
        for k in range(mu.shape[1]):
            r = Fraction(float(mu[vb[f], k])) - Fraction(float(mu[va[f], k])) - Fraction(float(z[f, k]))
            r2 += r * r
        out[f] = float(r2 / (2 * s2))
    return out


@pytest.mark.parametrize('off,sigma', SIGMAS)
@pytest.mark.parametrize('D', [2, 3, 6])
def test_weights_far_from_the_origin(D, off, sigma):
    """A ring of linear_displacement factors on a map `off` from the origin with noise `sigma`, every seventh measurement 5 .. 30
    sigma off, losses huber / constant / none by turns: the weights against M evaluated exactly at the engine's OWN means.  The
    tolerance is the energy test's own error model per factor, |e_f - exact| <= TOL |e_f| + 4 EPS |const_f|, carried through w(M):
    w is monotone in e on either side of the threshold, so its error is at most |w(e +- de) - w(e)| (+ 4 EPS for its own rounding)."""
    from gbp_amd.linear import LinearEngine
    from oracle.linear_oracle import displacement_graph
    rs = np.random.RandomState(220 + D)
    N, t = 60, 2.0
    va = np.repeat(np.arange(N), 2)
    vb = (va + np.tile([1, 2], N)) % N
    F = len(va)
    x_true = off + rs.rand(N, D) * 10
    J, z, _, _, _, pe, pl = displacement_graph(va, vb, x_true, sigma, rs)
    out = np.arange(F) % 7 == 0
    z[out] += sigma * rs.uniform(5, 30, (int(out.sum()), 1)) * np.sign(rs.randn(int(out.sum()), D))
    fe, fl, fc = (z @ J) / sigma ** 2, np.ascontiguousarray(np.broadcast_to(J.T @ J / sigma ** 2, (F, 2 * D, 2 * D))), 0.5 * np.einsum('fd,fd->f', z, z) / sigma ** 2
    loss = [('huber', 'constant', None)[f % 3] for f in range(F)]
    e = LinearEngine(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=0.3)
    e.set_robust(loss, t, sigma ** 2)
    e.update_all_beliefs()
    lossy = np.array([l is not None for l in loss])

    def check(what):
        e.robustify_all_factors()                            # weights at the means read below
        w, flag = e.weights()
        mu = e.get_means().reshape(N, D)
        ex = exact_half_m2(mu, va, vb, z, sigma)
        de = TOL * np.abs(ex) + 4 * EPS * np.abs(fc)
        worst = 0.0
        for f in range(F):
            M, lo, hi = np.sqrt(2 * ex[f]), np.sqrt(2 * max(ex[f] - de[f], 0.0)), np.sqrt(2 * (ex[f] + de[f]))
            want, want_flag = robust_weight(loss[f], t, sigma ** 2, M)
            if loss[f] is not None:
                assert (lo > t) == (hi > t), f"{what}, factor {f}: M = {M!r} is within the energy's error of the threshold; pick another seed"
            bound = max(abs(robust_weight(loss[f], t, sigma ** 2, m)[0] - want) for m in (lo, hi)) + 4 * EPS
            assert bound < 1e-6, f"{what}, factor {f}: the error model allows {bound:.3e} on w"
            assert flag[f] == want_flag, f"{what}, factor {f}: flag {flag[f]} at M = {M!r}"
            assert abs(w[f] - want) <= bound, f"{what}, factor {f} ({loss[f]}): w {w[f]!r} vs {want!r}, |err| {abs(w[f] - want):.3e} > {bound:.3e}"
            worst = max(worst, abs(w[f] - want))
        print(f"WEIGHTS d={D} off={off:g} sigma={sigma:g} {what}: {int(flag.sum())} robust of {int(lossy.sum())} with a loss, worst |err| {worst:.3e}")
        return flag

    flag = check('at the prior means')                       # the true positions: the inliers sit at their noise, the outliers far out
    assert flag.any() and not flag[lossy].all() and not flag[~lossy].any()
    e.iterate(30, robustify=True)
    assert check('after 30 robust sweeps').any()             # (a stiff graph not yet converged: most factors are beyond 2 sigma here)


# ---- the joint at the current weights --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('D', [1, 3, 6])
def test_joint_follows_the_weights(D):
    """joint_matvec, joint_eta, solve_map and marginals against the dense weighted joint: with every weight 1, then -- on the same
    handle -- after a robustify.  Between the two get_map still returns the first solution; the second solve is bit-identical to that
    of a fresh handle brought to the same weights, so nothing of the first (preconditioner, joint eta) is reused."""
    name, N, va, vb, J, z, sigma, pe, pl, loss, thr = shapes(D)[3]       # f65
    o = RobustOracle(va, vb, J, z, sigma, pe, pl, loss, thr, eta_damping=0.1)
    x = np.random.RandomState(D).randn(N, D)

    def check(e, w, what):
        eta, lam = dense_weighted_joint(o, w)
        assert rel(e.joint_matvec(x), lam @ x.reshape(-1)) < TOL, f"{what}: matvec"
        assert rel(e.joint_eta(), eta) < TOL, f"{what}: eta"
        mu, info = e.solve_map()
        assert info['converged'] and rel(mu, np.linalg.solve(lam, eta)) < TOL, f"{what}: map {rel(mu, np.linalg.solve(lam, eta)):.3e}"
        ids = [0, N // 2, N - 1]
        sig, sj, minfo = e.marginals(ids, joint=True)
        idx = np.concatenate([np.arange(v * D, (v + 1) * D) for v in ids])
        inv = np.linalg.inv(lam)
        assert minfo['converged'] and rel(sj, inv[np.ix_(idx, idx)]) < TOL, f"{what}: marginals {rel(sj, inv[np.ix_(idx, idx)]):.3e}"
        assert rel(sig, np.array([inv[v * D:(v + 1) * D, v * D:(v + 1) * D] for v in ids])) < TOL
        return mu, info

    def bring(e):
        e.update_all_beliefs()
        e.iterate(3)
        e.robustify_all_factors()

    e = make_engine(o)
    mu1, _ = check(e, np.ones(o.F), 'weights 1')
    bring(e)
    o.update_all_beliefs(); o.iterate(3); o.robustify_all_factors()
    w, _ = e.weights()
    assert np.max(np.abs(w - o.w) / o.w) < TOL and (w < 0.9).any()
    assert np.array_equal(e.map_mean(), mu1), "get_map between the solves must still return the first solution"
    mu2, info2 = check(e, w, 'after robustify')
    assert rel(mu2, mu1) > 1e-6                              # the weights moved the solution: a stale joint would show
    fresh = make_engine(o)
    bring(fresh)
    assert np.array_equal(fresh.weights()[0], w)
    mu3, info3 = fresh.solve_map()
    assert np.array_equal(mu3, mu2) and info3 == info2
    e.set_robust(None)                                       # cleared: the plain joint again
    mu4, _ = e.solve_map()
    assert np.array_equal(mu4, mu1)


# ---- the effect ------------------------------------------------------------------------------------------------------------------------

def test_one_gross_outlier_on_a_ring():
    """A ring of displacement factors (every variable joined to its next two neighbours: one bad closure cannot spread evenly round
    it) with one closure measured 50 sigma off: the MAP of the robustified graph (robust sweeps, then one solve at their weights: a
    step of iteratively reweighted least squares) is nearer the ground truth than the plain MAP."""
    from gbp_amd.linear import LinearEngine
    from oracle.linear_oracle import displacement_graph
    rs = np.random.RandomState(50)
    N, D, sigma = 40, 3, 0.1
    va = np.repeat(np.arange(N), 2)
    vb = (va + np.tile([1, 2], N)) % N
    F = len(va)
    x_true = rs.rand(N, D) * 10
    _, z, _, _, _, pe, pl = displacement_graph(va, vb, x_true, sigma, rs)
    z[F - 1] += 50 * sigma / np.sqrt(D)                      # |offset| = 50 sigma
    Jd = np.hstack([-np.eye(D), np.eye(D)])
    fe, fl, fc = (z @ Jd) / sigma ** 2, np.ascontiguousarray(np.broadcast_to(Jd.T @ Jd / sigma ** 2, (F, 2 * D, 2 * D))), 0.5 * np.einsum('fd,fd->f', z, z) / sigma ** 2
    e = LinearEngine(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=0.2)
    e.update_all_beliefs()
    plain, _ = e.solve_map()
    e.set_robust('huber', 2.0)
    e.iterate(30, robustify=True)
    robust, info = e.solve_map()
    w, flag = e.weights()
    d_plain, d_robust = np.linalg.norm(plain - x_true), np.linalg.norm(robust - x_true)
    print(f"OUTLIER ring: |plain MAP - truth| {d_plain:.4f}, |robust MAP - truth| {d_robust:.4f}, w[outlier] {w[F - 1]:.4f}, robust factors {int(flag.sum())}")
    assert info['converged'] and flag[F - 1] and w[F - 1] < 1.0
    assert d_robust < d_plain


# ---- state and options -----------------------------------------------------------------------------------------------------------------

def small_graph(D=2, fc=True):
    name, N, va, vb, J, z, sigma, pe, pl, loss, thr = shapes(D)[1]       # f63
    return RobustOracle(va, vb, J, z, sigma, pe, pl, loss, thr, eta_damping=0.3)


def test_argument_and_state_errors():
    from gbp_amd import _capi
    from gbp_amd.linear import LinearEngine
    o = small_graph()
    args, kw, (loss, thr, nvar) = engine_args(o)
    e = LinearEngine(*args, **kw)
    lib, h, F = e._lib, e._h, o.F
    ip, dp = ct.POINTER(ct.c_int32), ct.POINTER(ct.c_double)
    codes = np.array([_capi.LIN_LOSS[l] for l in loss], dtype=np.int32)
    ones = np.ones(F)

    def set_robust(c, t, n):
        return lib.gbp_lin_set_robust(h, None if c is None else c.ctypes.data_as(ip), None if t is None else t.ctypes.data_as(dp),
                                      None if n is None else n.ctypes.data_as(dp))
    # before losses / beliefs
    assert lib.gbp_lin_robustify(h) == ESTATE and lib.gbp_lin_iterate_robust(h, 1) == ESTATE       # no losses set
    w, flag = e.weights()
    assert np.array_equal(w, ones) and not flag.any()
    bad = codes.copy(); bad[5] = 3
    assert set_robust(bad, ones, ones) == EINVAL
    bad[5] = -1
    assert set_robust(bad, ones, ones) == EINVAL
    assert set_robust(codes, None, ones) == EINVAL
    for v in (0.0, -1.0, np.nan, np.inf):
        t = ones.copy(); t[int(np.nonzero(codes)[0][0])] = v
        assert set_robust(codes, t, ones) == EINVAL
        n = ones.copy(); n[int(np.nonzero(codes == 2)[0][0])] = v
        assert set_robust(codes, ones, n) == EINVAL
    assert set_robust(codes, ones, None) == EINVAL                                                   # a constant loss without noise_var
    hub = np.where(codes == 2, 1, codes).astype(np.int32)
    assert set_robust(hub, ones, None) == 0                                                          # huber only: noise_var may be NULL
    t = ones.copy(); t[codes == 0] = -5.0                                                            # not read where the loss is none
    assert set_robust(codes, t, ones) == 0
    assert lib.gbp_lin_robustify(h) == ESTATE and lib.gbp_lin_iterate_robust(h, 1) == ESTATE       # losses, but no beliefs yet
    e.update_all_beliefs()
    assert lib.gbp_lin_iterate_robust(h, -1) == EINVAL
    assert lib.gbp_lin_get_weights(h, None, None) == EINVAL
    assert lib.gbp_lin_iterate_robust(h, 0) == 0 and lib.gbp_lin_robustify(h) == 0
    assert lib.gbp_lin_get_weights(h, ones.ctypes.data_as(dp), None) == 0                            # the flags are optional
    assert set_robust(None, None, None) == 0
    assert lib.gbp_lin_robustify(h) == ESTATE                                                        # cleared
    with pytest.raises(ValueError):
        e.set_robust('cauchy')
    with pytest.raises(ValueError):
        e.set_robust(['huber'] * (F - 1))
    # a handle without the factors' constants cannot evaluate M
    e2 = LinearEngine(*args, eta_damping=0.3)
    with pytest.raises(_capi.GbpError) as err:
        e2.set_robust('huber')
    assert err.value.code == EINVAL and 'factor_const' in str(err.value)
    e2.set_robust([None] * F)                                # no loss anywhere: nothing to evaluate
    e2.set_robust(None)


def test_clearing_the_losses_restores_the_plain_sweeps_bit_for_bit():
    from gbp_amd.linear import LinearEngine
    o = small_graph(3)
    args, kw, rob = engine_args(o)
    e, fresh = LinearEngine(*args, **kw), LinearEngine(*args, **kw)
    e.set_robust(*rob)
    e.set_robust(None)
    for g in (e, fresh):
        g.update_all_beliefs()
        g.iterate(7)
    for a, b in zip(e.messages() + e.beliefs() + (e.get_means(),), fresh.messages() + fresh.beliefs() + (fresh.get_means(),)):
        assert np.array_equal(a, b)
    assert e.energy() == fresh.energy()
    # and with losses set but every weight still 1 the robust kernel computes the same bits (times 1 is exact)
    e.set_robust(*rob)
    e.iterate(2); fresh.iterate(2)
    for a, b in zip(e.messages() + e.beliefs(), fresh.messages() + fresh.beliefs()):
        assert np.array_equal(a, b)


def test_two_identical_robust_runs_are_bit_identical():
    o = small_graph(6)
    runs = []
    for _ in range(2):
        e = make_engine(o)
        e.update_all_beliefs()
        e.iterate(8, robustify=True)
        e.iterate(2)
        mu, _ = e.solve_map()
        runs.append(e.messages() + e.beliefs() + e.weights() + (e.get_means(), np.array(e.energy()), mu))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    assert runs[0][6].min() < 1.0


def test_a_graph_without_factors():
    from gbp_amd.linear import LinearEngine
    rs = np.random.RandomState(0)
    pe, pl = rs.randn(3, 2), np.tile(2.0 * np.eye(2), (3, 1, 1))
    e = LinearEngine([], [], np.zeros((0, 4)), np.zeros((0, 4, 4)), pe, pl, factor_const=np.zeros(0))
    e.set_robust([], 2.0, 1.0)
    e.update_all_beliefs()
    e.robustify_all_factors()
    e.iterate(3, robustify=True)
    w, flag = e.weights()
    assert w.shape == (0,) and flag.shape == (0,) and e.energy() == 0.0
    assert np.allclose(e.get_means().reshape(3, 2), pe / 2.0)
    mu, info = e.solve_map()
    assert info['converged'] and np.allclose(mu, pe / 2.0)
    e.set_robust(None)
    e.iterate(1)


def test_from_factor_graph_takes_the_losses_of_the_host_graph():
    """A drop-in host graph (ndim_posegraph.py:67-91) whose factors carry loss='huber' / 'constant' / None: the device picks the losses
    up (they were ignored before), and its robust sweeps match the host graph driven as fixture G22 drives the reference -- every
    factor.linpoint set to its adjacent belief means before synchronous_iteration(robustify=True)."""
    from gbp_amd.linear import LinearEngine
    compat = os.path.join(REPO, 'gbp_amd', 'compat')
    sys.path.insert(0, compat)
    try:
        from gbp import gbp
        from gbp.factors import linear_displacement
        rs = np.random.RandomState(4)
        n, dim, std = 25, 3, 0.5
        mu0 = rs.rand(n, dim) * 10
        graph = gbp.FactorGraph(nonlinear_factors=False, eta_damping=0.2)
        for i in range(n):
            v = gbp.VariableNode(i, dim)
            v.prior.lam = np.eye(dim) / 9.0
            v.prior.eta = v.prior.lam @ mu0[i]
            graph.var_nodes.append(v)
        f = 0
        for i in range(n):
            for j in (i + 1, i + 4):
                if j < n:
                    a, b = graph.var_nodes[i], graph.var_nodes[j]
                    z = mu0[j] - mu0[i] + rs.normal(0.0, std, dim) + (8.0 * std if f % 6 == 0 else 0.0)
                    fac = gbp.Factor(f, [a, b], z, std, linear_displacement.meas_fn, linear_displacement.jac_fn,
                                     loss=('huber', 'constant', None)[f % 3], mahalanobis_threshold=1.5 + 0.5 * (f % 2))
                    a.adj_factors.append(fac); b.adj_factors.append(fac)
                    graph.factors.append(fac)
                    f += 1
        graph.update_all_beliefs()
        graph.compute_all_factors()
        e = LinearEngine.from_factor_graph(graph)
        e.update_all_beliefs()
        for s in range(8):
            for fac in graph.factors:
                fac.linpoint = np.concatenate([np.linalg.solve(b.lam, b.eta) for b in fac.adj_beliefs])
            graph.synchronous_iteration(robustify=True)
            e.synchronous_iteration(robustify=True)
            w, flag = e.weights()
            want = np.array([fac.gauss_noise_var / fac.adaptive_gauss_noise_var for fac in graph.factors])
            assert np.array_equal(flag, np.array([fac.robust_flag for fac in graph.factors])), f"sweep {s}"
            assert np.max(np.abs(w - want) / want) < TOL, f"sweep {s}"
        assert flag.any() and not flag.all()
        assert rel(e.get_means(), graph.get_means()) < TOL
        assert abs(e.energy() - graph.energy()) <= TOL * abs(graph.energy())
        with pytest.raises(ValueError):                      # the host graph is rescaled by now: the device wants nominal factors
            LinearEngine.from_factor_graph(graph)
    finally:
        sys.path.remove(compat)
        for m in [k for k in sys.modules if k == 'gbp' or k.startswith('gbp.') or k == 'utils' or k.startswith('utils.')]:
            del sys.modules[m]
