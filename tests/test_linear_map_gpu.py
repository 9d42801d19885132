"""The batch MAP of the linear engine on the GPU (include/gbp_lin.h: joint_matvec / joint_eta / solve_map / get_map / map_distance --
FactorGraph.joint_distribution_inf / _cov, gbp.py:94-144, by block-Jacobi conjugate gradients): against the reference's own MAP
(fixture G8), against the dense joint assembled from the same arrays and np.linalg.solve on every layout boundary of the kernels, on a
badly scaled graph, and at its option / state edges.  fp64; TOL is the linear tests' 1e-9: the solver stops at a relative residual of
1e-12 and |x - x*| / |x*| <= cond * rel_residual with cond < 1e3 on every graph here but the scaling one, which carries its own bound.
The same routines run on a CPU in tests/test_linear_map_cpu.py."""
import numpy as np
import pytest

from conftest import golden
from lin_map_cases import (ITER_CAP, TOL, dense_joint, random_generic_graph, rel, scaled_displacement_graph, shapes)

pytestmark = pytest.mark.gpu


def engine(va, vb, fe, fl, pe, pl, **kw):
    from gbp_amd.linear import LinearEngine
    return LinearEngine(va, vb, fe, fl, pe, pl, **kw)


@pytest.fixture(scope='module')
def toy():
    """toy_posegraph(100, 3): arrays, the dense joint, and one engine with a cold solve done."""
    from oracle.linear_oracle import toy_posegraph
    va, vb, fe, fl, fc, pe, pl = toy_posegraph(100, 3, 10, 1.0, seed=0)
    eta, lam = dense_joint(va, vb, fe, fl, pe, pl)
    return dict(args=(va, vb, fe, fl, pe, pl), fc=fc, eta=eta, lam=lam)


# ---- the reference's MAP --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,dim,key', [(100, 3, 'n100d3_map_mu'), (50, 6, 'defaults_map_mu')])
def test_solve_map_matches_the_reference_joint_distribution_cov(n, dim, key):
    from oracle.linear_oracle import toy_posegraph
    va, vb, fe, fl, fc, pe, pl = toy_posegraph(n, dim, 10, 1.0, seed=0)
    e = engine(va, vb, fe, fl, pe, pl, factor_const=fc)
    mu, info = e.solve_map()
    want = golden('G8_toy_linear')[key]
    eta, lam = dense_joint(va, vb, fe, fl, pe, pl)
    true_res = np.linalg.norm(eta - lam @ mu.reshape(-1)) / np.linalg.norm(eta)
    print(f"MAP G8 {key}: {info} err {rel(mu, want):.2e} residual in numpy {true_res:.2e}")
    assert rel(mu, want) < TOL
    assert info['converged'] and info['iters'] <= ITER_CAP and info['rel_residual'] <= 1e-12
    assert true_res <= 2e-12
    assert abs(info['eta_norm'] - np.linalg.norm(eta)) <= 1e-12 * np.linalg.norm(eta)
    assert np.array_equal(e.map_mean(), mu)


# ---- matvec, eta and the solve against the dense joint ----------------------------------------------------------------------------------

def check_against_dense(name, va, vb, fe, fl, pe, pl):
    N, D = pe.shape
    e = engine(va, vb, fe, fl, pe, pl)
    eta, lam = dense_joint(va, vb, fe, fl, pe, pl)
    x = np.random.RandomState(1).randn(N, D)
    y = e.joint_matvec(x)
    assert rel(y, lam @ x.reshape(-1)) < TOL, f"{name}: matvec {rel(y, lam @ x.reshape(-1)):.3e}"
    assert rel(e.joint_eta(), eta) < TOL, f"{name}: eta {rel(e.joint_eta(), eta):.3e}"
    mu, info = e.solve_map(max_iters=ITER_CAP)
    want = np.linalg.solve(lam, eta)
    print(f"MAP d={D} {name}: {info} err {rel(mu, want):.2e}")
    assert info['converged'] and info['iters'] <= ITER_CAP and info['rel_residual'] <= 1e-12, f"{name}: {info}"
    assert rel(mu, want) < TOL, f"{name}: {rel(mu, want):.3e}"
    return e, info


@pytest.mark.parametrize('D', [1, 2, 3, 4, 5, 6])
def test_matvec_eta_and_solve_against_the_dense_joint(D):
    """N = 3 without factors, N = 2 with one, factor counts around a wave (63, 64, 65, 129), variable counts that are no multiple of
    anything (33, 67), a hub of degree 203 beside degrees 0..5, a pair joined three times in both orientations, rank-1 factors."""
    for name, *g in shapes(D):
        e, info = check_against_dense(name, *g)
        if name == 'n3_f0':
            assert info['iters'] <= 1                      # no factors: the MAP is the prior means
            assert rel(e.map_mean(), np.linalg.solve(g[5], g[4][..., None])[..., 0]) < 1e-12


@pytest.mark.parametrize('D', [1, 2, 3, 4, 5, 6])
def test_solve_on_the_random_generic_graphs(D):
    check_against_dense('generic', *random_generic_graph(D))


def test_zero_eta_gives_zero_in_no_iterations():
    _, va, vb, fe, fl, pe, pl = shapes(3)[2]
    e = engine(va, vb, np.zeros_like(fe), fl, np.zeros_like(pe), pl)
    mu, info = e.solve_map()
    assert not mu.any() and info['converged'] and info['iters'] == 0 and info['eta_norm'] == 0.0


# ---- scaling --------------------------------------------------------------------------------------------------------------------------

def test_means_a_million_from_the_origin():
    """Displacement factors of sigma 0.1 under priors of sigma 1.5, 1e6 from the origin: 1e3 <= cond <= 1e4."""
    va, vb, fe, fl, pe, pl = scaled_displacement_graph()
    eta, lam = dense_joint(va, vb, fe, fl, pe, pl)
    cond = np.linalg.cond(lam)
    assert 1e3 <= cond <= 1e4
    want = np.linalg.solve(lam, eta)
    e = engine(va, vb, fe, fl, pe, pl)
    mu, info = e.solve_map(rel_tol=1e-10)
    err = np.linalg.norm(mu.reshape(-1) - want) / np.linalg.norm(want)
    print(f"MAP scaled: cond {cond:.1f} {info} err {err:.2e} bound {cond * 2e-10:.2e}")
    assert info['converged'] and info['rel_residual'] <= 1e-10
    assert err <= cond * 2e-10


# ---- distance to the MAP --------------------------------------------------------------------------------------------------------------

def test_map_distance_is_the_reference_trace(toy):
    g8 = golden('G8_toy_linear')
    e = engine(*toy['args'], factor_const=toy['fc'])
    e.solve_map()
    e.update_all_beliefs()
    e.iterate(1)
    d1 = e.map_distance()
    e.iterate(19)
    d20 = e.map_distance()
    want = np.linalg.norm(e.get_means() - e.map_mean().reshape(-1))
    print(f"MAP distance after 1 / 20 sweeps: {d1:.6f} / {d20:.6f}; numpy {want:.6f}; reference {g8['n100d3_dist'][-1]:.6f}")
    assert abs(d20 - want) <= 1e-12 * want
    assert np.allclose(d20, g8['n100d3_dist'][-1], rtol=1e-5, atol=1e-5)
    assert np.allclose(d1, g8['n100d3_dist'][0], rtol=1e-5, atol=1e-5)
    assert d20 < d1


# ---- options and states ---------------------------------------------------------------------------------------------------------------

def test_running_out_of_iterations_is_not_an_error(toy):
    e = engine(*toy['args'])
    mu, info = e.solve_map(max_iters=2)
    assert not info['converged'] and info['iters'] == 2 and info['rel_residual'] > 1e-12
    assert np.isfinite(mu).all() and mu.any()
    true_res = np.linalg.norm(toy['eta'] - toy['lam'] @ mu.reshape(-1)) / np.linalg.norm(toy['eta'])
    assert abs(info['rel_residual'] - true_res) <= 1e-9 * true_res        # the TRUE residual of the iterate reached
    _, info0 = e.solve_map(max_iters=0)
    assert not info0['converged'] and info0['iters'] == 0 and abs(info0['rel_residual'] - 1.0) < 1e-12


def test_two_solves_are_bit_identical(toy):
    e = engine(*toy['args'])
    a, ia = e.solve_map()
    b, ib = e.solve_map()
    assert np.array_equal(a, b) and ia == ib
    f = engine(*toy['args'])
    f.joint_matvec(np.ones((100, 3)))                      # the workspace was made by another call, and used in between
    c, ic = f.solve_map()
    assert np.array_equal(a, c) and ia == ic


def test_warm_start_from_the_beliefs(toy):
    from gbp_amd import _capi
    e = engine(*toy['args'])
    with pytest.raises(_capi.GbpError) as ei:
        e.solve_map(warm_start=True)                       # no beliefs yet
    assert ei.value.code == -5
    cold, icold = e.solve_map()
    e.update_all_beliefs()
    e.iterate(200)
    warm, iwarm = e.solve_map(warm_start=True)
    print(f"MAP cold {icold} warm {iwarm}")
    assert iwarm['converged'] and iwarm['iters'] <= icold['iters']
    assert rel(warm, cold) < TOL


def test_state_and_option_errors(toy):
    from gbp_amd import _capi
    e = engine(*toy['args'])
    for call in (e.map_mean, e.map_distance):
        with pytest.raises(_capi.GbpError) as ei:
            call()                                         # before a solve
        assert ei.value.code == -5
    e.solve_map()
    with pytest.raises(_capi.GbpError) as ei:
        e.map_distance()                                   # a solve, but no beliefs
    assert ei.value.code == -5
    for bad in (dict(rel_tol=0.0), dict(rel_tol=-1e-3), dict(max_iters=-1), dict(check_every=0)):
        with pytest.raises(_capi.GbpError) as ei:
            e.solve_map(**bad)
        assert ei.value.code == -1, bad
    assert e._lib.gbp_lin_joint_eta(e._h, None) == -1 and e._lib.gbp_lin_get_map(e._h, None) == -1
    assert e._lib.gbp_lin_map_distance(e._h, None) == -1 and e._lib.gbp_lin_joint_matvec(e._h, None, None) == -1
    assert e._lib.gbp_lin_solve_map(e._h, None, None) == 0  # NULL options are the defaults, NULL info is allowed


def test_sweeps_do_not_see_the_solver(toy):
    """beliefs() and messages() bit for bit, with and without solves and products in between the sweeps."""
    def run(with_solver):
        e = engine(*toy['args'], factor_const=toy['fc'], eta_damping=0.3)
        e.update_all_beliefs()
        e.iterate(5)
        if with_solver:
            e.solve_map()
            e.joint_matvec(np.ones((100, 3)))
            e.map_distance()
            e.solve_map(warm_start=True, check_every=1)
        e.iterate(5)
        return [*e.beliefs(), *e.messages(), e.get_means(), np.array([e.energy()])]
    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)
