"""GPU parity of gbp_lin_extend (include/gbp_lin.h): a live linear handle grown on the device against the numpy oracle grown the same
way (tests/lin_extend_cases.py: grow(), pinned to the reference's staged run by fixture G23 in tests/test_linear_extend_cpu.py).
fp64; the sweep has no thresholds, so messages, beliefs, means and energy are asserted at the linear tests' TOL = 1e-9 relative, and
whatever the call promises to keep is asserted bit for bit."""
import ctypes as ct

import numpy as np
import pytest

from lin_extend_cases import TOL, generic_fc, grow, random_priors, robust_parts, schedules
from lin_map_cases import dense_joint, rel
from lin_robust_cases import RobustOracle, dense_weighted_joint
from oracle.linear_oracle import LinearOracleBatched

pytestmark = pytest.mark.gpu

SCHEDULES = schedules()
DIMS = [1, 3, 6]
GBP_EINVAL, GBP_ESTATE = -1, -5


def engine(*a, **k):
    from gbp_amd.linear import LinearEngine
    return LinearEngine(*a, **k)


def state(e):
    """Everything a sweep reads or writes, as the handle holds it."""
    return e.messages() + e.beliefs() + (e.get_means(),)


def same_bits(x, y):
    return all(np.array_equal(a, b) for a, b in zip(x, y))


def assert_close(e, o, what):
    for name, a, b in zip(('msg eta a', 'msg lam a', 'msg eta b', 'msg lam b'), e.messages(), o.messages()):
        assert rel(a, b) < TOL, f"{what}: {name} {rel(a, b):.3e}"
    for name, a, b in zip(('belief eta', 'belief lam'), e.beliefs(), o.beliefs()):
        assert rel(a, b) < TOL, f"{what}: {name} {rel(a, b):.3e}"
    assert rel(e.get_means(), o.get_means()) < TOL, f"{what}: means {rel(e.get_means(), o.get_means()):.3e}"
    got, want = e.energy(), o.energy()
    assert abs(got - want) <= TOL * abs(want), f"{what}: energy {got!r} vs {want!r}"


def start(D, sched, seed=0):
    """(engine, oracle, rs) of a schedule's initial graph, beliefs made."""
    name, N0, (va, vb), steps, damping = sched
    rs = np.random.RandomState(2300 + 10 * D + seed)
    fe, fl, fc = generic_fc(rs, D, len(va))
    pe, pl = random_priors(rs, N0, D)
    e = engine(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=damping)
    o = LinearOracleBatched(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=damping)
    e.update_all_beliefs(); o.update_all_beliefs()
    return e, o, rs


def step_data(rs, D, step):
    dN, a, b = step
    fe, fl, fc = generic_fc(rs, D, len(a))
    pe, pl = random_priors(rs, dN, D)
    return dict(va=a, vb=b, fe=fe, fl=fl, fc=fc, pe=pe, pl=pl)


def extend(e, s):
    e.extend(s['va'], s['vb'], s['fe'], s['fl'], s['pe'], s['pl'], factor_const=s['fc'])


# ---- every schedule, every size -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('D', DIMS)
@pytest.mark.parametrize('sched', SCHEDULES, ids=[s[0] for s in SCHEDULES])
def test_grown_handle_matches_the_grown_oracle(sched, D):
    """Sweeps before and after every growth step; across each call the old factors' messages and the old variables' belief records
    stay bit-identical, new variables hold their prior, and sizes() follows."""
    e, o, rs = start(D, sched)
    e.iterate(3); o.iterate(3)
    assert_close(e, o, 'before')
    for k, step in enumerate(sched[3]):
        s = step_data(rs, D, step)
        before, N0, F0 = state(e), e.N, e.F
        extend(e, s)
        o = grow(o, s['va'], s['vb'], s['fe'], s['fl'], s['pe'], s['pl'], s['fc'])
        assert e.sizes() == (o.N, o.F) == (e.N, e.F)
        after = state(e)
        assert same_bits([m[:F0] for m in before[:4]], [m[:F0] for m in after[:4]]), f"step {k}: old messages moved"
        assert all(not m[F0:].any() for m in after[:4]), f"step {k}: new messages are not zero"
        assert same_bits([b[:N0] for b in before[4:6]], [b[:N0] for b in after[4:6]]), f"step {k}: old beliefs changed"
        assert np.array_equal(before[6], after[6][:N0 * D]), f"step {k}: old means changed"
        touched = np.unique(np.concatenate([s['va'], s['vb']])).astype(int)
        alone = np.setdiff1d(np.arange(N0, e.N), touched)
        assert np.array_equal(after[4][alone], s['pe'][alone - N0]) and np.array_equal(np.triu(after[5][alone]), np.triu(s['pl'][alone - N0]))
        assert_close(e, o, f'step {k} grown')
        e.iterate(3); o.iterate(3)
        assert_close(e, o, f'step {k} swept')


@pytest.mark.parametrize('D', DIMS)
def test_grown_before_any_sweep_equals_created_whole_bit_for_bit(D):
    """A handle created small and grown to the full graph, then swept 20 times, against a handle created at full size: the same
    layout, so the same bits (messages and beliefs).  Two handles given the same schedule agree as well."""
    sched = SCHEDULES[1]                                     # tails, damped
    name, N0, (va, vb), steps, damping = sched
    grown = []
    for _ in range(2):
        e, _, rs = start(D, sched)
        parts = [step_data(rs, D, st) for st in steps]
        for s in parts:
            extend(e, s)
        e.iterate(20)
        grown.append(state(e))
    rs = np.random.RandomState(2300 + 10 * D)
    fe, fl, fc = generic_fc(rs, D, len(va))
    pe, pl = random_priors(rs, N0, D)
    cat = lambda first, key: np.concatenate([first] + [s[key] for s in parts])
    whole = engine(cat(va, 'va'), cat(vb, 'vb'), cat(fe, 'fe'), cat(fl, 'fl'), cat(pe, 'pe'), cat(pl, 'pl'), factor_const=cat(fc, 'fc'),
                   eta_damping=damping)
    whole.update_all_beliefs(); whole.iterate(20)
    assert same_bits(grown[0], grown[1])
    assert same_bits(grown[0], state(whole))


def test_growth_without_beliefs_makes_none():
    from gbp_amd import _capi
    name, N0, (va, vb), steps, damping = SCHEDULES[0]
    rs = np.random.RandomState(5)
    e = engine(va, vb, *generic_fc(rs, 3, len(va))[:2], *random_priors(rs, N0, 3))
    s = step_data(rs, 3, steps[0])
    e.extend(s['va'], s['vb'], s['fe'], s['fl'])
    with pytest.raises(_capi.GbpError) as err:
        e.iterate(1)
    assert err.value.code == GBP_ESTATE
    assert not e.beliefs()[0].any()


@pytest.mark.parametrize('D', DIMS)
def test_empty_and_refused_extends_change_nothing(D):
    """dN = dF = 0 is GBP_OK; an id out of range, a == b, a missing factor_const and a bad loss are GBP_EINVAL; after each the handle
    goes on bit-identically to an untouched twin over 5 sweeps."""
    from gbp_amd import _capi
    sched = SCHEDULES[0]
    e, _, rs = start(D, sched)
    twin, _, _ = start(D, sched)
    e.iterate(2); twin.iterate(2)
    s = step_data(rs, D, (2, np.array([0, 1]), np.array([3, e.N + 1])))
    e.extend([], [], np.zeros((0, 2 * D)), np.zeros((0, 2 * D, 2 * D)))
    assert e.sizes() == twin.sizes() and same_bits(state(e), state(twin))
    bad = [dict(s, vb=np.array([3, e.N + 2])), dict(s, vb=np.array([3, -1])), dict(s, va=np.array([3, 1])), dict(s, fc=None)]
    for b in bad:
        with pytest.raises(_capi.GbpError) as err:
            extend(e, b)
        assert err.value.code == GBP_EINVAL
    for kw in (dict(loss='huber', threshold=0.0), dict(loss='constant'), dict(loss=['huber', 'constant'], noise_var=[1.0, -1.0])):
        with pytest.raises(_capi.GbpError) as err:
            e.extend(s['va'], s['vb'], s['fe'], s['fl'], s['pe'], s['pl'], factor_const=s['fc'], **kw)
        assert err.value.code == GBP_EINVAL
    assert (e.N, e.F) == e.sizes() == twin.sizes()
    e.iterate(5); twin.iterate(5)
    assert same_bits(state(e), state(twin))
    extend(e, s)                                            # and the same step is accepted once it is valid
    assert e.sizes() == (twin.N + 2, twin.F + 2)


# ---- robust losses ----------------------------------------------------------------------------------------------------------------------

def robust_pair(D, rs, N, F, losses):
    from lin_map_cases import random_pairs
    va, vb = random_pairs(rs, N, F)
    J, z, sigma, loss, thr = robust_parts(rs, D, F, losses)
    pe, pl = random_priors(rs, N, D)
    o = RobustOracle(va, vb, J, z, sigma, pe, pl, loss, thr, eta_damping=0.2)
    e = engine(va, vb, o.fe0, o.fl0, pe, pl, factor_const=o.fc0, eta_damping=0.2)
    if losses:
        e.set_robust(loss, thr, sigma ** 2)
    e.update_all_beliefs(); o.update_all_beliefs()
    return e, o


def assert_robust_close(e, o, what):
    w, flag = e.weights()
    assert np.array_equal(flag, o.flag), f"{what}: flags"
    assert rel(w, o.w) < TOL, f"{what}: weights {rel(w, o.w):.3e}"
    assert_close(e, o, what)


@pytest.mark.parametrize('D', DIMS)
@pytest.mark.parametrize('case', ['mixed_then_losses', 'mixed_then_none', 'plain_then_losses'])
def test_robust_handle_grown(case, D):
    """A handle with mixed losses grown with and without `loss` for the new factors, and a handle without losses grown with them:
    weights, flags, energy and beliefs against the grown RobustOracle through iterate(n, robustify=True); old weights bit-identical
    across the call, new ones 1 / not robust."""
    rs = np.random.RandomState(2350 + D)
    N, F, dN, dF = 23, 63, 4, 66
    e, o = robust_pair(D, rs, N, F, losses=case != 'plain_then_losses')
    e.iterate(4, robustify=case != 'plain_then_losses'); o.iterate(4, robustify=True)
    assert_robust_close(e, o, 'before')
    a = rs.randint(0, N + dN, dF)
    b = (a + 1 + rs.randint(0, N + dN - 1, dF)) % (N + dN)
    J, z, sigma, loss, thr = robust_parts(rs, D, dF, losses=case != 'mixed_then_none')
    pe, pl = random_priors(rs, dN, D)
    w0, flag0 = e.weights()
    s2 = sigma ** 2
    fe, fl, fc = np.einsum('fmi,fm->fi', J, z) / s2[:, None], np.einsum('fmi,fmj->fij', J, J) / s2[:, None, None], 0.5 * np.einsum('fm,fm->f', z, z) / s2
    if case == 'mixed_then_none':
        e.extend(a, b, fe, fl, pe, pl, factor_const=fc)
    else:
        e.extend(a, b, fe, fl, pe, pl, factor_const=fc, loss=loss, threshold=thr, noise_var=s2)
    o = grow(o, a, b, pe=pe, pl=pl, J=J, z=z, sigma=sigma, loss=loss, threshold=thr)
    w1, flag1 = e.weights()
    assert np.array_equal(w1[:F], w0) and np.array_equal(flag1[:F], flag0)
    assert np.array_equal(w1[F:], np.ones(dF)) and not flag1[F:].any()
    assert_robust_close(e, o, 'grown')
    e.iterate(4, robustify=True); o.iterate(4, robustify=True)
    assert o.flag[:F].any() or o.flag[F:].any()
    assert_robust_close(e, o, 'swept')


# ---- solvers ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('D', DIMS)
def test_solvers_after_an_extend(D):
    """get_map and map_distance give GBP_ESTATE right after an extend; solve_map and marginals on the grown handle agree with the
    dense joint of the grown graph."""
    from gbp_amd import _capi
    sched = SCHEDULES[0]
    e, o, rs = start(D, sched)
    e.iterate(3)
    e.solve_map(); e.marginals(ids=[0, 5]); e.map_mean()
    for step in sched[3]:
        s = step_data(rs, D, step)
        extend(e, s)
        o = grow(o, s['va'], s['vb'], s['fe'], s['fl'], s['pe'], s['pl'], s['fc'])
    for call in (e.map_mean, e.map_distance):
        with pytest.raises(_capi.GbpError) as err:
            call()
        assert err.value.code == GBP_ESTATE
    eta, lam = dense_joint(o.va, o.vb, o.fe, o.fl, o.pe, o.pl)
    mu, info = e.solve_map()
    assert info['converged'] and info['rel_residual'] <= 1e-12
    assert rel(mu, np.linalg.solve(lam, eta)) < TOL
    assert abs(e.map_distance() - np.linalg.norm(e.get_means() - mu.reshape(-1))) <= 1e-9 * max(np.linalg.norm(mu), 1.0)
    ids = [0, e.N - 1, 7]
    sigma, sj, minfo = e.marginals(ids=ids, joint=True)
    S = np.linalg.inv(lam)
    idx = np.concatenate([np.arange(v * D, (v + 1) * D) for v in ids])
    assert minfo['converged'] and rel(sj, S[np.ix_(idx, idx)]) < TOL
    assert rel(sigma, np.array([S[v * D:(v + 1) * D, v * D:(v + 1) * D] for v in ids])) < TOL


def test_solver_on_a_grown_robust_handle_describes_the_current_weights():
    D = 3
    rs = np.random.RandomState(77)
    e, o = robust_pair(D, rs, 23, 63, losses=True)
    e.iterate(3, robustify=True); o.iterate(3, robustify=True)
    J, z, sigma, loss, thr = robust_parts(rs, D, 5)
    s2 = sigma ** 2
    a, b = np.array([0, 1, 2, 23, 24]), np.array([5, 23, 24, 24, 6])
    pe, pl = random_priors(rs, 2, D)
    e.extend(a, b, np.einsum('fmi,fm->fi', J, z) / s2[:, None], np.einsum('fmi,fmj->fij', J, J) / s2[:, None, None], pe, pl,
             factor_const=0.5 * np.einsum('fm,fm->f', z, z) / s2, loss=loss, threshold=thr, noise_var=s2)
    o = grow(o, a, b, pe=pe, pl=pl, J=J, z=z, sigma=sigma, loss=loss, threshold=thr)
    eta, lam = dense_weighted_joint(o, o.w)
    mu, info = e.solve_map()
    assert info['converged'] and rel(mu, np.linalg.solve(lam, eta)) < TOL


# ---- the drop-in layer --------------------------------------------------------------------------------------------------------------------

def test_extend_from_a_grown_host_factor_graph():
    """A host graph of the drop-in gbp.gbp classes grown after from_factor_graph (ndim_posegraph.py:67-88 again): the device follows
    with extend_from_factor_graph and matches the host graph's own update_all_beliefs() and sweeps."""
    import os
    import sys
    from conftest import REPO
    compat = os.path.join(REPO, 'gbp_amd', 'compat')
    sys.path.insert(0, compat)
    try:
        from gbp import gbp
        from gbp.factors import linear_displacement
        rs = np.random.RandomState(3)
        n, dim = 30, 4
        mu0 = rs.rand(n, dim) * 10
        graph = gbp.FactorGraph(nonlinear_factors=False, eta_damping=0.2)

        def add(lo, hi):
            for i in range(lo, hi):
                v = gbp.VariableNode(i, dim)
                v.prior.lam = np.eye(dim) / 3.0
                v.prior.eta = v.prior.lam @ mu0[i]
                graph.var_nodes.append(v)
            new = []
            for i in range(hi):
                for j in (i + 1, i + 5):
                    if lo <= j < hi:
                        a, b = graph.var_nodes[i], graph.var_nodes[j]
                        fac = gbp.Factor(len(graph.factors), [a, b], mu0[j] - mu0[i] + rs.normal(0, 0.3, dim), 0.3, linear_displacement.meas_fn,
                                         linear_displacement.jac_fn, loss=None, mahalanobis_threshold=2)
                        a.adj_factors.append(fac); b.adj_factors.append(fac); graph.factors.append(fac)
                        new.append(fac)
            graph.update_all_beliefs()
            for fac in new:
                fac.compute_factor()
            return len(new)
        add(0, 20)
        e = graph.device_engine()
        e.update_all_beliefs()
        for lo, hi in ((20, 26), (26, 30)):
            for _ in range(5):
                graph.synchronous_iteration()
            e.iterate(5)
            dF = add(lo, hi)
            assert e.extend_from_factor_graph(graph) == (hi - lo, dF)
            assert e.sizes() == (len(graph.var_nodes), len(graph.factors)) == (e.N, e.F)
            assert rel(e.get_means(), graph.get_means()) < TOL
        for _ in range(5):
            graph.synchronous_iteration()
        e.iterate(5)
        assert e.extend_from_factor_graph(graph) == (0, 0)
        assert rel(e.get_means(), graph.get_means()) < TOL
        assert abs(e.energy() - graph.energy()) <= TOL * abs(graph.energy())
        eta, lam = e.beliefs()
        assert rel(eta, np.array([v.belief.eta for v in graph.var_nodes])) < TOL
        assert rel(lam, np.array([v.belief.lam for v in graph.var_nodes])) < TOL
        graph.var_nodes[3].adj_factors.reverse()
        with pytest.raises(ValueError, match='ascending'):
            e.extend_from_factor_graph(graph)
        graph.var_nodes[3].adj_factors.reverse()
        last = graph.factors.pop()                         # something removed before the tail: positions no longer match
        with pytest.raises(ValueError, match='only grows'):
            e.extend_from_factor_graph(graph)
        graph.factors.append(last)
        a, b = graph.var_nodes[0], graph.var_nodes[9]
        fac = gbp.Factor(len(graph.factors) + 3, [a, b], mu0[9] - mu0[0], 0.3, linear_displacement.meas_fn, linear_displacement.jac_fn,
                         loss=None, mahalanobis_threshold=2)
        a.adj_factors.append(fac); b.adj_factors.append(fac); graph.factors.append(fac)
        with pytest.raises(ValueError, match='factorID'):      # refused before the factor itself is looked at
            e.extend_from_factor_graph(graph)
        assert e.sizes() == (30, len(graph.factors) - 1)
    finally:
        sys.path.remove(compat)
        for m in [k for k in sys.modules if k == 'gbp' or k.startswith('gbp.') or k == 'utils' or k.startswith('utils.')]:
            del sys.modules[m]


# ---- growth without a leak ------------------------------------------------------------------------------------------------------------------

def hip_runtime():
    for name in (None, 'libamdhip64.so.7', 'libamdhip64.so'):
        try:
            lib = ct.CDLL(name)
            lib.hipMemGetInfo, lib.hipMalloc, lib.hipFree
            return lib
        except (OSError, AttributeError):
            continue
    raise AssertionError("hipMemGetInfo not found in the process's HIP runtime")


def device_free(hip):
    free, total = ct.c_size_t(), ct.c_size_t()
    assert hip.hipMemGetInfo(ct.byref(free), ct.byref(total)) == 0
    return free.value


def allocation_granularity(hip):
    """The step in which hipMemGetInfo's free figure moves: 4 KiB blocks are allocated until it drops, and the drop is the step."""
    hip.hipMalloc.argtypes, hip.hipFree.argtypes = [ct.POINTER(ct.c_void_p), ct.c_size_t], [ct.c_void_p]
    base, held, step = device_free(hip), [], 0
    for _ in range(4096):
        q = ct.c_void_p()
        assert hip.hipMalloc(ct.byref(q), 4096) == 0
        held.append(q)
        step = base - device_free(hip)
        if step > 0:
            break
    for q in held:
        assert hip.hipFree(q) == 0
    assert step > 0
    return step


def test_two_hundred_extends_hold_one_generation():
    """A chain of 20 000 three-dof variables with losses on every factor, grown 200 times by one variable and one factor; every 20th
    step solves the MAP and a marginal first, so that the call also has those workspaces to drop.  Every extend replaces every array of
    the handle, so a call that kept ONE replaced array, the smallest per-factor one ([F] int32, 80 KB), would hold 16 MiB more at the end.
    The bound is taken in the test: what a handle created at the final size and put through the same calls takes, plus what two such
    creates differ by, plus 4 steps of the free figure (`allocation_granularity`, measured here): arrays smaller than a step share
    blocks of that size, and after 200 generations of allocate-new-then-free-old the survivors need not be packed as densely as a
    fresh handle's -- `a few allocations' granularity`, 4 taken as a few.  On the MI355X: step 2 MiB, so a margin of 8 MiB, half of
    what the smallest leak adds."""
    hip = hip_runtime()
    D, N, steps = 3, 20000, 200
    rs = np.random.RandomState(9)
    NF = N + steps
    fe, fl, fc = generic_fc(rs, D, NF - 1)
    pe, pl = random_priors(rs, NF, D)
    va, vb = np.arange(NF - 1), np.arange(1, NF)

    def solvers(e):
        e.solve_map(max_iters=2); e.marginals(ids=[0, e.N - 1], max_iters=2)

    def held(make):
        base = device_free(hip)
        e = make()
        e.iterate(1, robustify=True); solvers(e); e.sync()
        used = base - device_free(hip)
        e.close()
        return used

    def whole():
        e = engine(va, vb, fe, fl, pe, pl, factor_const=fc)
        e.set_robust('huber', 2.0)
        e.update_all_beliefs()
        return e

    def grown():
        e = engine(va[:N - 1], vb[:N - 1], fe[:N - 1], fl[:N - 1], pe[:N], pl[:N], factor_const=fc[:N - 1])
        e.set_robust('huber', 2.0)
        e.update_all_beliefs()
        for k in range(steps):
            f, v = N - 1 + k, N + k
            if k % 20 == 0:
                solvers(e)
            e.extend(va[f:f + 1], vb[f:f + 1], fe[f:f + 1], fl[f:f + 1], pe[v:v + 1], pl[v:v + 1], factor_const=fc[f:f + 1], loss='huber')
        assert e.sizes() == (NF, NF - 1)
        return e
    step = allocation_granularity(hip)
    first, second = held(whole), held(whole)
    got = held(grown)
    print(f"free-figure step {step} bytes; fresh {first} and {second} bytes, grown {got} bytes")
    assert first > 0
    assert got <= max(first, second) + abs(first - second) + 4 * step, (step, first, second, got)
