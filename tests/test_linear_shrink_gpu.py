"""GPU parity of gbp_lin_shrink (include/gbp_lin.h): a live linear handle shrunk on the device against the numpy oracle shrunk the same
way (tests/lin_shrink_cases.py: shrink(), pinned to the reference's shrunk run by fixture G24 and to exact marginalisation on a tree in
tests/test_linear_shrink_cpu.py).  fp64; messages, beliefs, means, energy and weights are asserted at the linear tests' TOL = 1e-9
relative, and whatever the call promises to keep is asserted bit for bit."""
import ctypes as ct

import numpy as np
import pytest

from lin_extend_cases import generic_fc, grow, random_priors
from lin_map_cases import dense_joint, rel
from lin_shrink_cases import TOL, plan, prefix_graphs, robust_oracle, schedules, shrink, tree
from oracle.linear_oracle import LinearOracleBatched

pytestmark = pytest.mark.gpu

SCHEDULES = schedules()
DIMS = [1, 3, 6]
MODES = ['never', 'on', 'cleared']                           # losses never set, set, set and cleared again
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
    assert e.sizes() == (o.N, o.F) == (e.N, e.F), what
    for name, a, b in zip(('msg eta a', 'msg lam a', 'msg eta b', 'msg lam b'), e.messages(), o.messages()):
        assert rel(a, b) < TOL, f"{what}: {name} {rel(a, b):.3e}"
    for name, a, b in zip(('belief eta', 'belief lam'), e.beliefs(), o.beliefs()):
        assert rel(a, b) < TOL, f"{what}: {name} {rel(a, b):.3e}"
    assert rel(e.get_means(), o.get_means()) < TOL, f"{what}: means {rel(e.get_means(), o.get_means()):.3e}"
    got, want = e.energy(), o.energy()
    assert abs(got - want) <= TOL * abs(want), f"{what}: energy {got!r} vs {want!r}"
    if hasattr(o, 'w'):
        w, flag = e.weights()
        assert np.array_equal(flag, o.flag), f"{what}: flags"
        assert rel(w, o.w) < TOL, f"{what}: weights {rel(w, o.w):.3e}"


def robust_pair(D, N, va, vb, damping, mode, seed=0):
    """(engine, RobustOracle) of a structure, beliefs made, 3 sweeps behind them; `mode` as MODES."""
    rs = np.random.RandomState(2400 + 10 * D + seed)
    o = robust_oracle(rs, D, N, va, vb, damping, 'on' if mode != 'never' else 'off')
    e = engine(o.va, o.vb, o.fe0, o.fl0, o.pe, o.pl, factor_const=o.fc0, eta_damping=damping)
    if mode != 'never':
        e.set_robust(o.loss, o.thr, o.sigma ** 2)
    e.update_all_beliefs(); o.update_all_beliefs()
    e.iterate(3, robustify=mode != 'never'); o.iterate(3, robustify=True)
    if mode == 'cleared':
        e.set_robust(None)
        o.loss = [None] * o.F
        o.w, o.flag = np.ones(o.F), np.zeros(o.F, dtype=bool)
        o.fe, o.fl = o.fe0.copy(), o.fl0.copy()
    return e, o


def plain_pair(D, N, va, vb, damping=0.0, seed=0, sweeps=0):
    rs = np.random.RandomState(2450 + 10 * D + seed)
    fe, fl, fc = generic_fc(rs, D, len(va))
    pe, pl = random_priors(rs, N, D)
    e = engine(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=damping)
    o = LinearOracleBatched(va, vb, fe, fl, pe, pl, factor_const=fc, eta_damping=damping)
    e.update_all_beliefs(); o.update_all_beliefs()
    e.iterate(sweeps); o.iterate(sweeps)
    return e, o


# ---- 1. every structural schedule against the model ------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('D', DIMS)
@pytest.mark.parametrize('sched', SCHEDULES, ids=[s[0] for s in SCHEDULES])
def test_shrunk_handle_matches_the_shrunk_oracle(sched, D, mode):
    """After every shrink, and after 5 further sweeps: everything within TOL of the model, the maps the model's; across each call the
    surviving factors' messages, weights and flags and the belief records of variables none of whose factors leaves stay bit-identical."""
    name, N0, (va, vb), steps, damping = sched
    e, o = robust_pair(D, N0, va, vb, damping, mode)
    assert_close(e, o, 'before')
    for k, (retire, drop, fold) in enumerate(steps):
        before, w0 = state(e), e.weights()
        vkeep, fkeep, _, _, _ = plan(o.N, o.va, o.vb, retire, drop)
        touched = np.zeros(o.N, dtype=bool)
        touched[o.va[~fkeep]] = True; touched[o.vb[~fkeep]] = True
        vm, fm = e.shrink(retire, drop, fold=bool(fold))
        o, vmap, fmap = shrink(o, retire, drop, bool(fold))
        assert vm.dtype == fm.dtype == np.int32 and np.array_equal(vm, vmap) and np.array_equal(fm, fmap), f"step {k}: maps"
        after, w1 = state(e), e.weights()
        assert same_bits([m[fkeep] for m in before[:4]], after[:4]), f"step {k}: surviving messages moved"
        assert np.array_equal(w0[0][fkeep], w1[0]) and np.array_equal(w0[1][fkeep], w1[1]), f"step {k}: surviving weights / flags"
        same = vkeep & ~touched
        assert same_bits([b[same] for b in before[4:6]], [b[vmap[same]] for b in after[4:6]]), f"step {k}: untouched beliefs changed"
        assert np.array_equal(before[6].reshape(-1, D)[same], after[6].reshape(-1, D)[vmap[same]])
        assert_close(e, o, f'step {k} shrunk')
        e.iterate(5, robustify=mode == 'on'); o.iterate(5, robustify=mode == 'on')
        assert_close(e, o, f'step {k} swept')
    if name == 'emptied':                                    # N' = F' = 0, and the emptied handle grows again
        assert e.sizes() == (0, 0)
        rs = np.random.RandomState(7)
        from lin_extend_cases import robust_parts
        J, z, sigma, loss, thr = robust_parts(rs, D, 5, losses=False)
        s2 = sigma ** 2
        pe, pl = random_priors(rs, 4, D)
        a, b = np.array([0, 1, 2, 3, 0]), np.array([1, 2, 3, 0, 2])
        e.extend(a, b, np.einsum('fmi,fm->fi', J, z) / s2[:, None], np.einsum('fmi,fmj->fij', J, J) / s2[:, None, None], pe, pl,
                 factor_const=0.5 * np.einsum('fm,fm->f', z, z) / s2)
        o = grow(o, a, b, pe=pe, pl=pl, J=J, z=z, sigma=sigma, loss=None, threshold=thr)
        assert_close(e, o, 'regrown')
        e.iterate(3); o.iterate(3)
        assert_close(e, o, 'regrown and swept')


# ---- 2. bit identity ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('D', DIMS)
@pytest.mark.parametrize('graph', prefix_graphs(), ids=[g[0] for g in prefix_graphs()])
def test_prefix_fold_keeps_every_surviving_belief_bit_for_bit(graph, D):
    """A chain and a ring built in pose order, the lowest-numbered variables retired: at every survivor the folded factors are a prefix
    of its adjacency list, so its belief is the same sum in the same order."""
    name, N, va, vb, retire = graph
    e, o = plain_pair(D, N, va, vb, damping=0.2, sweeps=4)
    before = state(e)
    vm, fm = e.retire(retire)
    after = state(e)
    keep = vm >= 0
    assert keep.sum() == N - len(retire) and (fm >= 0).sum() < len(va)
    assert same_bits([b[keep] for b in before[4:6]], after[4:6]), f"{name}: beliefs changed"
    assert np.array_equal(before[6].reshape(-1, D)[keep], after[6].reshape(-1, D))
    o, _, _ = shrink(o, retire=retire)
    assert_close(e, o, name)


@pytest.mark.parametrize('D', DIMS)
def test_shrunk_before_any_sweep_equals_created_from_the_survivors(D):
    """Messages are zero before the first sweep, so the fold adds zeros: the shrunk handle is the handle created from the survivors'
    arrays, bit for bit, sweep after sweep."""
    name, N, (va, vb), steps, damping = SCHEDULES[3]         # n33_31, damped
    retire = np.array([0, 17, 5])
    drop = np.array([2, 40, 41])
    e, o = plain_pair(D, N, va, vb, damping)
    vkeep, fkeep, _, vmap, _ = plan(N, va, vb, retire, drop)
    e.shrink(retire, drop)
    c = engine(vmap[o.va[fkeep]], vmap[o.vb[fkeep]], o.fe[fkeep], o.fl[fkeep], o.pe[vkeep], o.pl[vkeep], factor_const=o.fc[fkeep], eta_damping=damping)
    c.update_all_beliefs()
    assert e.sizes() == c.sizes()
    for sweep in range(6):
        assert same_bits(state(e), state(c)), f"after {sweep} sweeps"
        assert e.energy() == c.energy()
        e.iterate(1); c.iterate(1)


@pytest.mark.parametrize('D', DIMS)
def test_two_handles_given_the_same_calls_are_bit_identical(D):
    name, N, (va, vb), steps, damping = SCHEDULES[2]
    runs = []
    for _ in range(2):
        e, _ = plain_pair(D, N, va, vb, 0.4, sweeps=2)
        rs = np.random.RandomState(11)
        trace = []
        for k in range(4):
            dN, dF = 3, 6
            a = rs.randint(0, e.N + dN, dF)
            b = (a + 1 + rs.randint(0, e.N + dN - 1, dF)) % (e.N + dN)
            fe, fl, fc = generic_fc(rs, D, dF)
            e.extend(a, b, fe, fl, *random_priors(rs, dN, D), factor_const=fc)
            e.iterate(2)
            trace.append(state(e))
            maps = e.shrink(rs.permutation(e.N)[:3], rs.permutation(e.F)[:4], fold=bool(k % 2 == 0))
            trace.append(state(e) + maps)
            e.iterate(1)
        trace.append(state(e))
        runs.append(trace)
    assert all(same_bits(x, y) for x, y in zip(*runs))


# ---- 3. exactness on a tree, through the engine ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('D', DIMS)
def test_fold_is_exact_marginalisation_on_a_tree(D):
    """The chain with two leaves of the CPU check: after N + 2 undamped sweeps and the fold, solve_map and marginals(joint=True) of the
    shrunk handle equal the dense MAP and Lambda^-1 of the FULL graph restricted to the survivors."""
    rs = np.random.RandomState(2410 + D)
    N, va, vb, fe, fl, fc, pe, pl, retire = tree(rs, D)
    e = engine(va, vb, fe, fl, pe, pl, factor_const=fc)
    e.update_all_beliefs()
    e.iterate(N + 2)
    vm, _ = e.retire(retire)
    keep = np.flatnonzero(vm >= 0)
    eta, lam = dense_joint(va, vb, fe, fl, pe, pl)
    S = np.linalg.inv(lam)
    idx = np.concatenate([np.arange(v * D, (v + 1) * D) for v in keep])
    mu, info = e.solve_map()
    assert info['converged'] and rel(mu, (S @ eta)[idx]) < TOL, rel(mu, (S @ eta)[idx])
    sigma, sj, minfo = e.marginals(joint=True)
    assert minfo['converged'] and rel(sj, S[np.ix_(idx, idx)]) < TOL, rel(sj, S[np.ix_(idx, idx)])
    assert rel(sigma, np.array([S[v * D:(v + 1) * D, v * D:(v + 1) * D] for v in keep])) < TOL


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------

def raw_shrink(e, n_r, r, n_d, d, fold):
    """gbp_lin_shrink with the descriptor as given (the Python method cannot pass a NULL list with a count): the return code."""
    from gbp_amd import _capi
    ip = ct.POINTER(ct.c_int32)
    desc = _capi.LinShrink()
    keep = [None if x is None else np.ascontiguousarray(x, dtype=np.int32) for x in (r, d)]
    desc.n_retire_vars, desc.n_drop_factors, desc.fold = n_r, n_d, fold
    desc.retire_vars = None if keep[0] is None else keep[0].ctypes.data_as(ip)
    desc.drop_factors = None if keep[1] is None else keep[1].ctypes.data_as(ip)
    return e._lib.gbp_lin_shrink(e._h, ct.byref(desc))


@pytest.mark.parametrize('D', DIMS)
def test_refused_and_empty_shrinks_change_nothing(D):
    """Every GBP_EINVAL of the header, and both counts 0 (GBP_OK, identity maps): beliefs, messages, sizes and one further sweep equal
    those of a twin that never saw the call.  After a legal shrink map_mean / map_distance give GBP_ESTATE until a solve."""
    from gbp_amd import _capi
    name, N, (va, vb), steps, damping = SCHEDULES[2]
    e, _ = robust_pair(D, N, va, vb, 0.4, 'on')
    twin, _ = robust_pair(D, N, va, vb, 0.4, 'on')
    F = e.F
    e.solve_map(); twin.solve_map()
    bad = [(1, None, 0, None, 1), (0, None, 2, None, 1),                   # a NULL list with a positive count
           (-1, [0], 0, None, 1), (0, None, -3, [0], 1),                   # a negative count
           (2, [0, N], 0, None, 1), (1, [-1], 0, None, 1), (0, None, 1, [F], 1), (0, None, 2, [3, -2], 1),   # out of range
           (3, [4, 9, 4], 0, None, 1), (0, None, 2, [7, 7], 0),            # listed twice
           (1, [0], 0, None, 2), (1, [0], 1, [0], -1)]                     # fold not 0 or 1
    for args in bad:
        assert raw_shrink(e, *args) == GBP_EINVAL, args
        assert e._lib.gbp_last_error()
    vm, fm = e.shrink()
    assert np.array_equal(vm, np.arange(N)) and np.array_equal(fm, np.arange(F))
    assert e.sizes() == twin.sizes() == (N, F)
    assert same_bits(state(e) + e.weights(), state(twin) + twin.weights())
    assert np.array_equal(e.map_mean(), twin.map_mean())                   # the solver's state was left alone as well
    e.iterate(1, robustify=True); twin.iterate(1, robustify=True)
    assert same_bits(state(e) + e.weights(), state(twin) + twin.weights())
    e.retire([1])
    for call in (e.map_mean, e.map_distance):
        with pytest.raises(_capi.GbpError) as err:
            call()
        assert err.value.code == GBP_ESTATE
    mu, info = e.solve_map()
    assert info['converged'] and mu.shape == (N - 1, D)
    e.map_distance()


def test_shrink_without_beliefs_makes_none():
    from gbp_amd import _capi
    name, N, (va, vb), steps, damping = SCHEDULES[2]
    rs = np.random.RandomState(5)
    e = engine(va, vb, *generic_fc(rs, 3, len(va))[:2], *random_priors(rs, N, 3))
    e.retire([0, 1])
    with pytest.raises(_capi.GbpError) as err:
        e.iterate(1)
    assert err.value.code == GBP_ESTATE
    assert not e.beliefs()[0].any()


# ---- 5. one generation -------------------------------------------------------------------------------------------------------------------------

def test_two_hundred_window_steps_hold_one_generation():
    """A fixed-lag window over a ring of 10 000 three-dof poses (each joined to the two before it): 200 times extend (+3 variables, +6
    factors) then shrink (the 3 oldest retired, folded).  Every call replaces every array of the handle, so a call that kept ONE
    replaced array, the smallest per-factor one ([F] int32, 80 KB), would hold 30 MB more after step 200 than after step 10.  The device
    memory in use is read from hipMemGetInfo as tests/test_linear_extend_gpu.py does; the bound is 4 steps of that figure's
    granularity (2 MiB on the MI355X: 8 MiB), the allowance that test makes for survivors packed less densely.  The final state is within
    TOL of the model."""
    from test_linear_extend_gpu import allocation_granularity, device_free, hip_runtime
    hip = hip_runtime()
    D, N0, steps = 3, 10000, 200
    rs = np.random.RandomState(9)

    def pairs(lo, hi):
        a = np.concatenate([[j - 2, j - 1] for j in range(lo, hi)])
        return a, np.repeat(np.arange(lo, hi), 2)
    a0, b0 = pairs(2, N0)
    fe, fl, fc = generic_fc(rs, D, len(a0))
    pe, pl = random_priors(rs, N0, D)
    step = allocation_granularity(hip)
    base = device_free(hip)
    e = engine(a0, b0, fe, fl, pe, pl, factor_const=fc, eta_damping=0.2)
    o = LinearOracleBatched(a0, b0, fe, fl, pe, pl, factor_const=fc, eta_damping=0.2)
    e.update_all_beliefs(); o.update_all_beliefs()
    used = {}
    for k in range(1, steps + 1):
        a, b = pairs(e.N, e.N + 3)
        fe, fl, fc = generic_fc(rs, D, 6)
        pe, pl = random_priors(rs, 3, D)
        if k % 20 == 0:
            e.solve_map(max_iters=2); e.marginals(ids=[0, e.N - 1], max_iters=2)
        e.extend(a, b, fe, fl, pe, pl, factor_const=fc)
        o = grow(o, a, b, fe, fl, pe, pl, fc)
        if k % 10 == 1:
            e.iterate(1); o.iterate(1)
        e.retire([0, 1, 2])
        o, _, _ = shrink(o, retire=[0, 1, 2])
        assert e.sizes() == (N0, 2 * N0 - 3)
        if k in (10, steps):
            e.sync()
            used[k] = base - device_free(hip)
    print(f"free-figure step {step} bytes; in use after step 10: {used[10]} bytes, after step {steps}: {used[steps]} bytes")
    assert used[10] > 0
    assert used[steps] <= used[10] + 4 * step, (step, used)
    assert_close(e, o, 'after 200 window steps')
