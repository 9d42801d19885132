"""Exact marginal covariances of the linear engine on the GPU (include/gbp_lin.h: gbp_lin_solve_marginals -- the sigma of
FactorGraph.joint_distribution_cov, gbp.py:128-144, by block-Jacobi conjugate gradients on 8 unit right-hand sides at a time): against
the reference's own sigma (fixture G21), against np.linalg.inv of the dense joint on every layout boundary of the kernels, against the
belief covariances on a tree, and at its option / state edges.

fp64; TOL is the linear tests' 1e-9 by the argument of tests/test_linear_map_gpu.py: every right-hand side has norm 1, the solver stops at
a true residual of 1e-12, and |x - x*| <= cond * residual * |x*| with cond < 1e3 on every graph used here -- shapes(D) for D = 1..6
(worst: the star, 169 ... 780), the two toy graphs (58, 98) and the chain; tests/test_linear_marginals_cpu.py asserts that bound with
numpy for each of them.  For G21, np.linalg.inv of the dense joint and the reference's sigma agree to the last bit (the CPU test
prints and bounds the gap), so the reference is not the looser side and the bound stays TOL.  Measured errors are printed; they are
1e-16 ... 2e-13.  The same routines run on a CPU in tests/test_linear_marginals_cpu.py."""
import ctypes as ct

import numpy as np
import pytest

from conftest import golden
from lin_map_cases import TOL, dense_joint, rel, shapes
from lin_marg_cases import chain, diag_blocks, sub

pytestmark = pytest.mark.gpu


def engine(va, vb, fe, fl, pe, pl, **kw):
    from gbp_amd.linear import LinearEngine
    return LinearEngine(va, vb, fe, fl, pe, pl, **kw)


@pytest.fixture(scope='module')
def toy():
    """toy_posegraph(100, 3): arrays and the dense inverse, computed once and left unchanged."""
    from oracle.linear_oracle import toy_posegraph
    va, vb, fe, fl, fc, pe, pl = toy_posegraph(100, 3, 10, 1.0, seed=0)
    _, lam = dense_joint(va, vb, fe, fl, pe, pl)
    S = np.linalg.inv(lam)
    S.setflags(write=False)
    lam.setflags(write=False)
    return dict(args=(va, vb, fe, fl, pe, pl), fc=fc, lam=lam, S=S)


@pytest.fixture(scope='module')
def cases():
    """shapes(D) with the dense inverse of each joint, made on first use per D."""
    memo = {}

    def get(D):
        if D not in memo:
            memo[D] = [(name, g, np.linalg.inv(dense_joint(*g)[1])) for name, *g in shapes(D)]
        return memo[D]
    return get


def case(cases, D, name):
    return next((g, S) for n, g, S in cases(D) if n == name)


def ok(info):
    return info['converged'] and info['rel_residual'] <= 1e-12


# ---- the reference's sigma ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,dim,tag', [(100, 3, 'n100d3'), (50, 6, 'defaults')])
def test_marginals_match_the_reference_joint_distribution_cov(n, dim, tag):
    from oracle.linear_oracle import toy_posegraph
    va, vb, fe, fl, fc, pe, pl = toy_posegraph(n, dim, 10, 1.0, seed=0)
    g21 = golden('G21_toy_linear_sigma')
    e = engine(va, vb, fe, fl, pe, pl, factor_const=fc)
    sigma, info = e.marginals()
    ids = g21[f'{tag}_joint_ids']
    sg, sj, ij = e.marginals(ids, joint=True)
    print(f"marginals G21 {tag}: {info} err {rel(sigma, g21[f'{tag}_sigma_diag']):.2e}; joint {ij} err {rel(sj, g21[f'{tag}_sigma_joint']):.2e}")
    assert ok(info) and info['batches'] == -(-n * dim // 8)
    assert rel(sigma, g21[f'{tag}_sigma_diag']) < TOL
    assert ok(ij) and ij['batches'] == -(-3 * dim // 8)
    assert rel(sj, g21[f'{tag}_sigma_joint']) < TOL
    assert np.array_equal(sg, sigma[ids])


# ---- against the dense inverse --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('D', [1, 2, 3, 4, 5, 6])
def test_marginals_of_all_variables_against_the_dense_inverse(cases, D):
    """N = 3 without factors, N = 2 with one, factor counts that are no multiple of 8 and sit around a wave (63, 64, 65, 129), variable
    counts with N d no multiple of 8 (33, 67: the last batch is padded), a hub of degree 203 beside an isolated variable, a pair joined
    three times in both orientations, rank-1 factors."""
    for name, g, S in cases(D):
        N = g[4].shape[0]
        e = engine(*g)
        sigma, info = e.marginals()
        err = rel(sigma, diag_blocks(S, range(N), D))
        print(f"marginals d={D} {name}: {info} err {err:.2e}")
        assert ok(info) and info['batches'] == -(-N * D // 8), f"{name}: {info}"
        assert err < TOL, f"{name}: {err:.3e}"
        if name == 'n3_f0':
            assert info['iters'] <= info['batches']        # no factors: one iteration per batch is exact
            assert rel(sigma, np.linalg.inv(g[5])) < 1e-12


# ---- ids ------------------------------------------------------------------------------------------------------------------------------

def check_ids(g, S, ids, batches):
    D = g[4].shape[1]
    e = engine(*g)
    sigma, sj, info = e.marginals(ids, joint=True)
    want = sub(S, ids, D)
    asym = float(np.max(np.abs(sj - sj.T)) / np.max(np.abs(want)))
    print(f"marginals d={D} ids {list(ids)}: {info} err {rel(sj, want):.2e} asymmetry {asym:.2e}")
    assert ok(info) and info['batches'] == batches, info
    assert rel(sj, want) < TOL and rel(sigma, diag_blocks(S, ids, D)) < TOL
    assert asym < TOL                                       # not symmetrised
    assert np.array_equal(diag_blocks(sj, range(len(ids)), D), sigma)
    only, i2 = e.marginals(ids)                             # without the joint block: the same bits
    assert np.array_equal(only, sigma) and i2 == info


def test_a_single_id_has_fewer_live_columns_than_a_batch(cases):
    for D in (1, 3, 6):
        g, S = case(cases, D, 'n33')
        check_ids(g, S, [17], 1)


def test_ids_in_descending_order(cases):
    g, S = case(cases, 3, 'n67')
    check_ids(g, S, [66, 40, 39, 5, 0], 2)


def test_the_hub_and_the_isolated_variable(cases):
    g, S = case(cases, 3, 'star')
    N = g[4].shape[0]
    check_ids(g, S, [N - 1, 0], 1)
    e = engine(*g)
    _, sj, _ = e.marginals([N - 1, 0], joint=True)
    assert not sj[:3, 3:].any() and not sj[3:, :3].any()   # an isolated variable is independent of the rest, exactly
    assert rel(sj[:3, :3], np.linalg.inv(g[5][N - 1])) < 1e-12


@pytest.mark.parametrize('D', [1, 3, 6])
def test_columns_that_converge_at_very_different_rates(cases, D):
    """One batch holds the isolated variable's columns, exact after one iteration, and the hub's, which take some twenty; nothing is
    frozen, so the finished columns keep iterating on residuals that shrink towards underflow.  Residuals read every iteration; then a
    tolerance nobody can meet, 600 iterations on: the finished columns' scalars pass through the denormals to 0 / 0 -> 0, the true
    residual restarts the recurrence whenever all claim to be done, and the answer stays finite and as exact as before."""
    g, S = case(cases, D, 'star')
    N = g[4].shape[0]
    ids = [N - 1, 0]
    want = sub(S, ids, D)
    e = engine(*g)
    _, sj, info = e.marginals(ids, joint=True, check_every=1)
    assert ok(info) and rel(sj, want) < TOL, info
    _, sl, il = e.marginals(ids, joint=True, check_every=1, rel_tol=1e-300, max_iters=600)
    print(f"marginals d={D} star hub + isolated: {info} err {rel(sj, want):.2e}; 600 iterations on: {il} err {rel(sl, want):.2e}")
    assert not il['converged'] and il['iters'] == 600 * il['batches']
    assert np.isfinite(sl).all() and il['rel_residual'] < 1e-12 and rel(sl, want) < TOL
    assert not sl[:D, D:].any() and not sl[D:, :D].any()


@pytest.mark.parametrize('D,ids', [(2, [3, 9, 1, 22]), (4, [12, 2])])
def test_exactly_eight_columns_need_no_padding(cases, D, ids):
    """f65 has 23 variables; 4 x 2 and 2 x 4 columns fill one batch."""
    g, S = case(cases, D, 'f65')
    check_ids(g, S, ids, 1)


# ---- GBP's own covariances ------------------------------------------------------------------------------------------------------------

def test_belief_covariances_are_the_marginals_on_a_tree():
    """GBP is exact on trees: after 12 sweeps of a 12-variable chain every message has crossed it."""
    va, vb, fe, fl, fc, pe, pl = chain()
    e = engine(va, vb, fe, fl, pe, pl, factor_const=fc)
    e.update_all_beliefs()
    e.iterate(12)
    sigma, info = e.marginals()
    gap = rel(e.belief_covariances(), sigma)
    print(f"marginals chain: {info} |belief covariance - marginal| {gap:.2e}")
    assert ok(info) and gap < TOL
    assert e.belief_covariances().shape == (12, 3, 3)


def test_belief_covariances_are_not_the_marginals_on_a_loopy_graph(toy):
    e = engine(*toy['args'], factor_const=toy['fc'])
    e.update_all_beliefs()
    e.iterate(50)
    sigma, info = e.marginals()
    gap = rel(e.belief_covariances(), sigma)
    print(f"marginals toy graph after 50 sweeps: |belief covariance - marginal| {gap:.3e} (relative to the largest entry); "
          f"means from the MAP {np.max(np.abs(e.get_means() - e.solve_map()[0].reshape(-1))):.2e}")
    assert ok(info) and rel(sigma, diag_blocks(toy['S'], range(100), 3)) < TOL
    assert gap > TOL


# ---- determinism and isolation --------------------------------------------------------------------------------------------------------

def test_two_calls_are_bit_identical_and_the_map_is_left_alone(toy):
    e = engine(*toy['args'])
    mu, _ = e.solve_map()
    a, ja, ia = e.marginals([5, 99, 0, 42], joint=True)
    b, jb, ib = e.marginals([5, 99, 0, 42], joint=True)
    assert np.array_equal(a, b) and np.array_equal(ja, jb) and ia == ib
    assert np.array_equal(e.map_mean(), mu)                 # still solved, the same bits
    f = engine(*toy['args'])                                # a handle whose first solver call is this one
    c, jc, ic = f.marginals([5, 99, 0, 42], joint=True)
    assert np.array_equal(a, c) and np.array_equal(ja, jc) and ia == ic
    from gbp_amd import _capi
    with pytest.raises(_capi.GbpError) as ei:
        f.map_mean()                                        # marginals are no MAP solve
    assert ei.value.code == -5


def test_sweeps_do_not_see_the_marginals(toy):
    """beliefs(), messages() and energy() bit for bit, with and without marginals in between the sweeps."""
    def run(with_marginals):
        e = engine(*toy['args'], factor_const=toy['fc'], eta_damping=0.3)
        e.update_all_beliefs()
        e.iterate(5)
        if with_marginals:
            e.marginals([3, 1, 50])
            e.marginals([7], joint=True, check_every=1)
        e.iterate(5)
        return [*e.beliefs(), *e.messages(), e.get_means(), np.array([e.energy()])]
    for a, b in zip(run(False), run(True)):
        assert np.array_equal(a, b)


# ---- options and states ---------------------------------------------------------------------------------------------------------------

def test_running_out_of_iterations_is_not_an_error(cases):
    """max_iters = 2: the columns come back as they are, and rel_residual is numpy's worst column residual of those columns."""
    g, _ = case(cases, 3, 'n33')
    lam = dense_joint(*g)[1]
    e = engine(*g)
    sigma, sj, info = e.marginals(joint=True, max_iters=2)
    assert not info['converged'] and info['batches'] == 13 and info['iters'] == 2 * 13
    assert np.isfinite(sj).all() and np.isfinite(sigma).all() and sj.any()
    worst = np.max(np.linalg.norm(np.eye(99) - lam @ sj, axis=0))
    print(f"marginals max_iters=2: {info} worst column residual in numpy {worst:.6e}")
    assert info['rel_residual'] > 1e-12 and abs(info['rel_residual'] - worst) <= 1e-9 * worst
    _, info0 = e.marginals([4], max_iters=0)
    assert not info0['converged'] and info0['iters'] == 0 and info0['rel_residual'] == 1.0


def test_no_ids_and_the_errors(toy):
    from gbp_amd import _capi
    e = engine(*toy['args'])
    sigma, sj, info = e.marginals([], joint=True)
    assert sigma.shape == (0, 3, 3) and sj.shape == (0, 0)
    assert info == {'iters': 0, 'converged': True, 'batches': 0, 'rel_residual': 0.0}
    raw = _capi.LinMargInfo(9, 9, 9, 9, 9.0)
    assert e._lib.gbp_lin_solve_marginals(e._h, None, 0, None, None, None, ct.byref(raw)) == 0
    assert (raw.iters, raw.converged, raw.batches, raw.reserved, raw.rel_residual) == (0, 1, 0, 0, 0.0)
    for bad in ([1, 1], [0, 5, 0], [-1], [100], [3, 100]):
        with pytest.raises(_capi.GbpError) as ei:
            e.marginals(bad)
        assert ei.value.code == -1, bad
    with pytest.raises(ValueError):
        e.marginals([2 ** 32 + 1])                          # would wrap to the valid id 1 in int32
    for bad in (dict(rel_tol=0.0), dict(max_iters=-1), dict(check_every=0)):
        with pytest.raises(_capi.GbpError) as ei:
            e.marginals([0], **bad)
        assert ei.value.code == -1, bad
    out = np.zeros((1, 3, 3))
    ids = np.zeros(1, dtype=np.int32)
    warm = _capi.LinMapOpts(1e-12, 100, 8, 1)
    assert e._lib.gbp_lin_solve_marginals(e._h, _capi.iptr(ids), 1, ct.byref(warm), _capi.dptr(out), None, None) == -1
    assert e._lib.gbp_lin_solve_marginals(e._h, _capi.iptr(ids), 1, None, None, None, None) == -1      # NULL sigma
    assert e._lib.gbp_lin_solve_marginals(e._h, None, 1, None, _capi.dptr(out), None, None) == -1      # NULL ids
    assert not out.any()
    assert e._lib.gbp_lin_solve_marginals(e._h, _capi.iptr(ids), 1, None, _capi.dptr(out), None, None) == 0   # NULL options and info
    assert rel(out[0], toy['S'][:3, :3]) < TOL
