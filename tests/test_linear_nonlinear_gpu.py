"""The nonlinear (SE(2) relative-pose) path of the linear engine on the MI355X (include/gbp_lin.h: gbp_lin_set_nonlinear / relinearise /
iterate_nonlinear / get_linearisation; kernels in gbp_amd/csrc/gbp_lin_nonlin.hpp): against the reference's own run (fixture G25) with
the relinearisation masks compared exactly, against the numpy twin of tests/lin_nonlin_cases.py on the shapes where a kernel can go
wrong, the schedule's edges, the solvers at the current linearisation point, and the refusals.  fp64 throughout.
Every seeded case here is shown by test_linear_nonlinear_cpu.py to stay >= 1e-9 clear of the threshold `dist > beta`."""
import ctypes as ct

import numpy as np
import pytest

from conftest import golden
from lin_map_cases import rel
from lin_nonlin_cases import CASES, PARITY, SCHEDULE, SWEEPS, TOL, g25_graph, g25_schedule, hub, twin_of

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5


def make_engine(g, sched):
    from gbp_amd.linear import LinearEngine
    return LinearEngine.se2_pose_graph(g['va'], g['vb'], g['z'], g['s'], g['prior_eta'], g['prior_lam'], sched['beta'],
                                       sched['num_undamped_iters'], sched['min_linear_iters'], eta_damping=sched['eta_damping'])


def case(name):
    _, build, sched = next(c for c in CASES if c[0] == name)
    return build(), sched


def state(e):
    """Everything a sweep writes, for bit-for-bit comparisons."""
    return list(e.messages()) + list(e.beliefs()) + [e.get_means()] + list(e.linearisation())


def same_bits(a, b):
    return all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def assert_matches_twin(e, t, what, tol=TOL):
    lp, it, dm = e.linearisation()
    assert np.array_equal(it, t.iters), f"{what}: iters differ at {np.nonzero(it != t.iters)[0][:5]}"
    assert np.array_equal(dm, t.fdamp), f"{what}: damping differs at {np.nonzero(dm != t.fdamp)[0][:5]}"
    assert rel(lp, t.linpoint) < tol, f"{what}: linpoint {rel(lp, t.linpoint):.3e}"
    for name, a, b in zip(('eta_a', 'lam_a', 'eta_b', 'lam_b'), e.messages(), t.messages()):
        assert rel(a, b) < tol, f"{what}: message {name} {rel(a, b):.3e}"
    for name, a, b in zip(('eta', 'lam'), e.beliefs(), t.beliefs()):
        assert rel(a, b) < tol, f"{what}: belief {name} {rel(a, b):.3e}"
    assert rel(e.get_means(), t.get_means()) < tol, f"{what}: means {rel(e.get_means(), t.get_means()):.3e}"
    ee, et = e.energy(), t.energy()
    assert abs(ee - et) <= tol * max(abs(et), 1.0), f"{what}: energy {ee!r} vs {et!r}"


# ---- the reference's own run --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('tag', ['main', 'b0'])
def test_reference_run_sweep_by_sweep(tag):
    """G25 one sweep per call: the mask of every sweep from linearisation() (iters == 0), the count, iters and per-factor damping
    exactly; factors' linpoints, messages and beliefs at the stored sweeps, the energy trace and the means within the parity contract
    against the reference, and everything within TOL of the twin."""
    g = golden('G25_se2_posegraph')
    sched, sweeps = g25_schedule(g, tag)
    graph = g25_graph(g)
    e, t = make_engine(graph, sched), twin_of(graph, sched)
    assert_matches_twin(e, t, f'{tag} after set_nonlinear')
    worst = {}

    def gap(name, a, b, tol=PARITY):
        worst[name] = max(worst.get(name, 0.0), rel(a, b))
        assert rel(a, b) < tol, f"{name}: {rel(a, b):.3e}"

    for s in range(sweeps):
        counts = e.iterate(1, relinearise=True)
        t.synchronous_iteration()
        lp, it, dm = e.linearisation()
        want = g[f'{tag}_mask'][s].astype(bool)
        assert np.array_equal(it == 0, want), f"sweep {s}: mask differs at {np.nonzero((it == 0) != want)[0][:5]}"
        assert counts.tolist() == [int(want.sum())], f"sweep {s}: count {counts} vs {want.sum()}"
        assert np.array_equal(it, g[f'{tag}_iters'][s]) and np.array_equal(dm, g[f'{tag}_damp'][s]), f"sweep {s}: iters / damping"
        gap('means', e.get_means(), g[f'{tag}_means'][s])
        gap('energy', e.energy(), g[f'{tag}_energy'][s])
        k = f'{tag}_s{s + 1}_'
        if k + 'linpoint' in g:
            gap('linpoint', lp, g[k + 'linpoint'])
            for name, a in zip(('msg_eta_a', 'msg_lam_a', 'msg_eta_b', 'msg_lam_b'), e.messages()):
                gap('messages', a, g[k + name])
            eta, lam = e.beliefs()
            gap('beliefs', eta, g[k + 'bel_eta']); gap('beliefs', lam, g[k + 'bel_lam'])
            # eta_f, Lambda_f as the solvers see them: the joint's eta, and its product with a fixed vector, against the fixture's factors
            je, jl = dense_joint(graph, g[k + 'feta'], g[k + 'flam'])
            x = np.cos(np.arange(je.size) * 0.37)
            gap('factors', e.joint_eta().reshape(-1), je); gap('factors', e.joint_matvec(x).reshape(-1), jl @ x)
            assert_matches_twin(e, t, f'{tag} sweep {s + 1}')
    print(tag, 'worst gaps against the reference', {k: f'{v:.2e}' for k, v in worst.items()})
    e.close()


def dense_joint(graph, feta, flam):
    N = graph['N']
    eta, lam = graph['prior_eta'].reshape(-1).copy(), np.zeros((3 * N, 3 * N))
    for v in range(N):
        lam[3 * v:3 * v + 3, 3 * v:3 * v + 3] = graph['prior_lam'][v]
    for f, (a, b) in enumerate(zip(graph['va'], graph['vb'])):
        ix = np.concatenate([np.arange(3) + 3 * a, np.arange(3) + 3 * b])
        eta[ix] += feta[f]
        lam[np.ix_(ix, ix)] += flam[f]
    return eta, lam


def test_reference_run_in_one_call_and_solves():
    """G25 in ONE iterate(60): the per-sweep counts equal the fixture's, the final state equals the sweep-by-sweep run's end; then the
    solvers at the final linearisation point: solve_map against joint_distribution_cov's mu, marginals against its diagonal blocks."""
    g = golden('G25_se2_posegraph')
    for tag in ('main', 'b0'):
        sched, sweeps = g25_schedule(g, tag)
        e = make_engine(g25_graph(g), sched)
        counts = e.iterate(sweeps, relinearise=True)
        assert counts.tolist() == g[f'{tag}_mask'].sum(1).tolist(), f"{tag}: counts"
        lp, it, dm = e.linearisation()
        assert np.array_equal(it, g[f'{tag}_iters'][-1]) and np.array_equal(dm, g[f'{tag}_damp'][-1])
        assert rel(lp, g[f'{tag}_s{sweeps}_linpoint']) < PARITY and rel(e.get_means(), g[f'{tag}_means'][-1]) < PARITY
        if tag == 'main':
            mu, info = e.solve_map()
            assert info['converged'] and rel(mu, g['main_map_mu']) < PARITY, f"map {rel(mu, g['main_map_mu']):.3e}"
            sigma, minfo = e.marginals()
            assert minfo['converged'] and rel(sigma, g['main_map_sigma_diag']) < PARITY, f"marginals {rel(sigma, g['main_map_sigma_diag']):.3e}"
            print('map', rel(mu, g['main_map_mu']), 'marginals', rel(sigma, g['main_map_sigma_diag']))
        e.close()


# ---- against the twin ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['F1', 'hub9', 'turns40', 'chain63', 'ring63', 'chain64', 'ring64', 'chain65', 'ring65', 'chain129', 'ring129'])
def test_shapes_match_the_twin(name):
    """F = 1; 63, 64, 65, 129 on a chain and a ring with closures (the tail of a wave of k_lin_factor, lanes past the end of a block
    of k_lin_relin); a variable with 9 factors (the belief stage's 4-wide loop and its tail); theta of 40 turns + 1e-3.  One call of
    SWEEPS sweeps: counts and the end state against the twin; and SWEEPS calls of one sweep end bit for bit where the one call did."""
    g, sched = case(name)
    if name == 'hub9':
        assert np.bincount(np.concatenate([g['va'], g['vb']])).max() == 9
    e, e1, t = make_engine(g, sched), make_engine(g, sched), twin_of(g, sched)
    counts = e.iterate(SWEEPS, relinearise=True)
    want = t.iterate(SWEEPS, relinearise=True)
    assert np.array_equal(counts, want), f"counts {counts} vs {want}"
    assert_matches_twin(e, t, name)
    single = [int(e1.iterate(1, relinearise=True)[0]) for _ in range(SWEEPS)]
    assert single == counts.tolist()
    assert same_bits(state(e), state(e1)), "n sweeps in one call differ from n calls of one sweep"
    e.close(); e1.close()


def test_beta_infinite_is_the_plain_sweep():
    """beta = +inf, graph damping 0: nothing relinearises, every factor's damping stays 0, and the state is bit for bit that of the
    plain gbp_lin_iterate."""
    g, _ = case('ring65')
    sched = dict(SCHEDULE, beta=np.inf, eta_damping=0.0)
    a, b = make_engine(g, sched), make_engine(g, sched)
    counts = a.iterate(12, relinearise=True)
    b.iterate(12)
    assert counts.tolist() == [0] * 12
    assert same_bits(state(a)[:8], state(b)[:8])             # messages, beliefs, means, linpoints
    assert not a.linearisation()[2].any()
    assert np.array_equal(a.linearisation()[1], np.full(a.F, 13)) and np.array_equal(b.linearisation()[1], np.ones(b.F))   # iters untouched by the plain sweep
    a.close(); b.close()


def test_beta_zero_relinearises_everything():
    """beta = 0, min_linear_iters = 0: every factor relinearises in every sweep -- except the first after set_nonlinear, where the
    linpoint IS the belief means and dist is exactly 0, as in the reference (fixture G25, tag b0: [0, 35, 35, ...])."""
    g, sched = case('beta0')
    e, t = make_engine(g, sched), twin_of(g, sched)
    counts = e.iterate(SWEEPS, relinearise=True)
    assert counts.tolist() == [0] + [e.F] * (SWEEPS - 1)
    t.iterate(SWEEPS, relinearise=True)
    assert_matches_twin(e, t, 'beta0')
    e.close()


def test_min_linear_iters_spaces_the_relinearisations():
    g, sched = case('minlin5')
    e, t = make_engine(g, sched), twin_of(g, sched)
    last = np.full(e.F, -100)
    total = 0
    for s in range(SWEEPS):
        n = int(e.iterate(1, relinearise=True)[0])
        mask = t.synchronous_iteration()
        it = e.linearisation()[1]
        assert np.array_equal(it == 0, mask) and n == mask.sum()
        assert np.all(s - last[it == 0] >= 5), f"sweep {s}: a factor relinearised twice within 5 sweeps"
        last[it == 0] = s
        total += n
    assert total > e.F                                        # some factor did relinearise twice
    e.close()


@pytest.mark.parametrize('und', [0, 1, 4])
def test_num_undamped_iters(und):
    """The per-factor damping against the twin's, exactly, after every sweep.  Kept from the reference: iters starts at 1 and is
    incremented before the test, so before its first relinearisation a factor never meets num_undamped_iters <= 1; with 0 the switch
    fires only in the very sweep a factor relinearises."""
    g, sched = case(f'undamped{und}')
    e, t = make_engine(g, sched), twin_of(g, sched)
    seen = set()
    for s in range(SWEEPS):
        e.iterate(1, relinearise=True); t.synchronous_iteration()
        lp, it, dm = e.linearisation()
        assert np.array_equal(dm, t.fdamp) and np.array_equal(it, t.iters), f"sweep {s}"
        assert set(np.unique(dm)) <= {0.0, sched['eta_damping']}
        if und == 0:
            assert np.all(dm[it == 0] == sched['eta_damping'])
        seen |= set(np.unique(dm))
    assert seen == {0.0, sched['eta_damping']}
    assert_matches_twin(e, t, f'undamped{und}')
    e.close()


def test_plain_iterate_on_a_nonlinear_handle():
    """gbp_lin_iterate = synchronous_iteration(local_relin=False): no relinearisation, the graph-level damping, iters untouched."""
    g, sched = case('ring64')
    e, t = make_engine(g, sched), twin_of(g, sched)
    e.iterate(3, relinearise=True); t.iterate(3, relinearise=True)
    e.iterate(4); t.iterate(4)
    assert_matches_twin(e, t, 'after plain sweeps')
    e.close()


def test_solves_follow_the_linearisation_point():
    """The joint is that of the current linearisation point: a relinearise() that relinearised something changes the next solve (one
    Gauss-Newton step, equal to the twin's dense solve); one that relinearised nothing leaves it bit for bit."""
    g, sched = case('ring63')
    sched = dict(sched, min_linear_iters=1)                   # iters is 1 after set_nonlinear and the plain sweep leaves it there
    e, t = make_engine(g, sched), twin_of(g, sched)
    e.iterate(2); t.iterate(2)                                # the means leave the linearisation points
    mu0, _ = e.solve_map()
    n = e.relinearise()
    assert n == int(t.relinearise_factors().sum()) and n > 0
    mu1, info = e.solve_map()
    eta, lam = t.joint()
    assert info['converged'] and rel(mu1, np.linalg.solve(lam, eta)) < 1e-6       # rel_tol 1e-12 on the residual, cond <= 1e6
    assert rel(e.joint_eta().reshape(-1), eta) < TOL
    assert np.max(np.abs(mu1 - mu0)) > 1e-6, "the solve did not see the new linearisation point"
    assert e.relinearise() == 0                               # iters is 0 where it relinearised, dist <= beta elsewhere
    t.relinearise_factors()
    mu2, _ = e.solve_map()
    assert mu2.tobytes() == mu1.tobytes()
    assert_matches_twin(e, t, 'after relinearise alone')      # iters moved, the damping did not switch
    e.close()


def test_energy_is_the_nonlinear_one():
    g, sched = case('ring65')
    e, t = make_engine(g, dict(sched, beta=np.inf)), twin_of(g, dict(sched, beta=np.inf))
    e.iterate(6, relinearise=True); t.iterate(6, relinearise=True)      # means far from linpoints that never move
    en, lin = t.energy(), t.linearised_energy()
    assert abs(en - lin) > 1e-3 * en, "the case does not tell the two energies apart"
    assert abs(e.energy() - en) <= TOL * en
    e.close()


def test_two_handles_are_bit_identical():
    g, sched = case('ring129')
    out = []
    for _ in range(2):
        e = make_engine(g, sched)
        c = [e.iterate(5, relinearise=True), np.array([e.relinearise()]), e.iterate(7, relinearise=True)]
        out.append(state(e) + c + [np.array([e.energy()])])
        e.close()
    assert same_bits(out[0], out[1])


# ---- refusals and resources -------------------------------------------------------------------------------------------------------------

def test_out_of_scope_calls_are_refused_and_change_nothing():
    from gbp_amd import _capi
    g, sched = case('ring64')
    a, b = make_engine(g, sched), make_engine(g, sched)
    a.iterate(2, relinearise=True); b.iterate(2, relinearise=True)
    lib, F = a._lib, a.F
    loss, thr = np.ones(F, dtype=np.int32), np.full(F, 2.0)
    uo = _capi.LinUntilOpts(5, 1, 0, 0, 1e-3, 0.0)
    ext, shr = _capi.LinExt(), _capi.LinShrink()
    ids = np.zeros(1, dtype=np.int32)
    shr.n_retire_vars, shr.retire_vars, shr.fold = 1, _capi.iptr(ids), 1
    calls = {'set_robust': lambda: lib.gbp_lin_set_robust(a._h, _capi.iptr(loss), _capi.dptr(thr), None),
             'robustify': lambda: lib.gbp_lin_robustify(a._h), 'iterate_robust': lambda: lib.gbp_lin_iterate_robust(a._h, 1),
             'iterate_until': lambda: lib.gbp_lin_iterate_until(a._h, ct.byref(uo), None, None),
             'extend': lambda: lib.gbp_lin_extend(a._h, ct.byref(ext)), 'shrink': lambda: lib.gbp_lin_shrink(a._h, ct.byref(shr))}
    for name, call in calls.items():
        assert call() == ESTATE, name
        assert b'nonlinear' in lib.gbp_last_error(), name
    assert a.sizes() == b.sizes()
    ca, cb = a.iterate(1, relinearise=True), b.iterate(1, relinearise=True)
    assert np.array_equal(ca, cb) and same_bits(state(a), state(b))
    a.close(); b.close()


def test_set_nonlinear_validates_before_it_changes_anything():
    from gbp_amd import _capi
    from gbp_amd.linear import LinearEngine
    g, sched = case('ring63')
    F, N = g['va'].shape[0], g['N']
    z, s = np.ascontiguousarray(g['z']), np.ascontiguousarray(g['s'])

    def desc(model=1, und=4, minlin=2, beta=0.05, zz=z, ss=s):
        return _capi.LinNonlinear(model, und, minlin, 0, beta, _capi.dptr(zz), _capi.dptr(ss))

    e = LinearEngine(g['va'], g['vb'], np.zeros((F, 6)), np.zeros((F, 6, 6)), g['prior_eta'], g['prior_lam'], factor_const=np.zeros(F))
    lib = e._lib
    bad = s.copy(); bad[F // 2, 1] = 0.0
    inf = s.copy(); inf[0, 0] = np.inf
    neg = -s
    for name, d in (('model', desc(model=7)), ('null z', desc(zz=None)), ('null s', desc(ss=None)), ('s = 0', desc(ss=bad)), ('s = inf', desc(ss=inf)),
                    ('s < 0', desc(ss=neg)), ('beta', desc(beta=-1.0)), ('beta nan', desc(beta=np.nan)), ('und', desc(und=-1)), ('minlin', desc(minlin=-1))):
        assert lib.gbp_lin_set_nonlinear(e._h, ct.byref(d)) == EINVAL, name
    assert lib.gbp_lin_set_nonlinear(e._h, None) == EINVAL
    # a linear handle: the three other calls are refused
    n = ct.c_int32()
    assert lib.gbp_lin_relinearise(e._h, ct.byref(n)) == ESTATE
    assert lib.gbp_lin_iterate_nonlinear(e._h, 1, None) == ESTATE
    assert lib.gbp_lin_get_linearisation(e._h, None, None, None) == ESTATE
    # losses set
    e.set_robust('huber', 2.0)
    assert lib.gbp_lin_set_nonlinear(e._h, ct.byref(desc())) == ESTATE
    e.set_robust(None)
    count = e.alloc_count()
    assert lib.gbp_lin_set_nonlinear(e._h, ct.byref(desc())) == 0
    assert e.alloc_count() == count + 6                       # z, s, linpoint, iters, damping, counts
    assert lib.gbp_lin_set_nonlinear(e._h, ct.byref(desc())) == ESTATE     # twice
    assert lib.gbp_lin_iterate_nonlinear(e._h, -1, None) == EINVAL
    # the handle made step by step is the handle of se2_pose_graph
    ref = make_engine(g, dict(sched, eta_damping=0.0))
    assert same_bits(state(e), state(ref))
    e.close(); ref.close()
    # dofs != 3
    e2 = LinearEngine([0], [1], np.zeros((1, 4)), np.zeros((1, 4, 4)), np.zeros((2, 2)), np.tile(np.eye(2), (2, 1, 1)))
    z1, s1 = np.zeros((1, 3)), np.ones((1, 3))
    assert lib.gbp_lin_set_nonlinear(e2._h, ct.byref(desc(zz=z1, ss=s1))) == EINVAL
    e2.close()


def test_repeated_calls_allocate_nothing():
    g, sched = case('ring63')
    e = make_engine(g, sched)
    base = e.alloc_count()
    e.iterate(1, relinearise=True)
    assert e.alloc_count() == base                            # one slot exists from set_nonlinear
    e.iterate(9, relinearise=True)
    assert e.alloc_count() == base                            # the counts buffer grew: replaced, not added
    for n in (9, 3, 1, 0):
        e.iterate(n, relinearise=True); e.relinearise(); e.energy(); e.linearisation()
    assert e.alloc_count() == base
    e.close()


def test_empty_graph_and_no_factors():
    from gbp_amd.linear import LinearEngine
    g = hub()
    e = LinearEngine.se2_pose_graph([], [], np.zeros((0, 3)), np.zeros((0, 3)), g['prior_eta'], g['prior_lam'], 0.05, 4, 2)
    assert e.iterate(3, relinearise=True).tolist() == [0, 0, 0] and e.relinearise() == 0 and e.energy() == 0.0
    assert rel(e.get_means(), np.linalg.solve(g['prior_lam'], g['prior_eta'][:, :, None]).reshape(-1)) < TOL
    e.close()
