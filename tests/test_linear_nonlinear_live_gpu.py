"""Growing and shrinking a live nonlinear (SE(2)) handle on the MI355X (include/gbp_lin.h: gbp_lin_extend_nonlinear /
gbp_lin_shrink_nonlinear; the range form of the relinearise kernel in gbp_amd/csrc/gbp_lin_nonlin.hpp): the reference's own grown run
(fixture G26), the shapes where a kernel can go wrong, what is kept bit for bit, the shrinks, a fixed-lag window, random schedules, and
the contract of the two calls -- against the numpy twin of tests/lin_nonlin_live_cases.py.  fp64 throughout.
Every schedule here is shown by test_linear_nonlinear_live_cpu.py to stay >= 1e-9 clear of the threshold `dist > beta`.

Worst gaps against the reference on G26, as printed by test_g26_on_the_device on an MI355X: see DESIGN section 8h."""
import ctypes as ct

import numpy as np
import pytest

from conftest import golden
from lin_map_cases import rel
from lin_nonlin_cases import PARITY, SCHEDULE, SWEEPS, TOL
from lin_nonlin_live_cases import (EDGE_CASES, FUZZ_SEEDS, SHRINK_CASES, converged_chain, fuzz_schedule, g26_graph, head, kept_state_case, live_twin,
                                   play_on_twin, tail, window_schedule)
from test_linear_nonlinear_gpu import assert_matches_twin, dense_joint, make_engine, same_bits, state

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -5


def play_on_engine(e, step):
    kind = step[0]
    if kind == 'extend':
        k = step[1]
        return e.extend_se2(k['va'], k['vb'], k['z'], k['s'], k['prior_eta'], k['prior_lam'])
    if kind == 'shrink':
        return e.shrink(step[1]['retire'], step[1]['drop'], step[1]['fold'])
    if kind == 'iterate':
        return e.iterate(step[1], relinearise=True)
    if kind == 'plain':
        return e.iterate(step[1])
    if kind == 'relin':
        return e.relinearise()
    if kind == 'energy':
        return e.energy()
    if kind == 'map':
        mu, info = e.solve_map()
        assert info['converged']
        return mu
    raise ValueError(kind)


def play(e, t, step, what):
    """One step on both; what it returns and the whole state afterwards are compared."""
    got, want = play_on_engine(e, step), play_on_twin(t, step)
    kind = step[0]
    if kind == 'shrink':
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), f"{what}: maps"
    elif kind == 'iterate':
        assert np.array_equal(got, want), f"{what}: counts {got} vs {want}"
    elif kind == 'relin':
        assert got == want, f"{what}: relinearised {got} vs {want}"
    elif kind == 'energy':
        assert abs(got - want) <= TOL * max(abs(want), 1.0), f"{what}: energy {got!r} vs {want!r}"
    elif kind == 'map':
        assert rel(got, want) < TOL, f"{what}: map {rel(got, want):.3e}"
    assert e.sizes() == (t.N, t.F) and (e.N, e.F) == (t.N, t.F), f"{what}: sizes {e.sizes()} vs {(t.N, t.F)}"
    assert_matches_twin(e, t, what)


def run_schedule(g, steps, name, sched=SCHEDULE):
    e, t = make_engine(g, sched), live_twin(g, sched)
    assert_matches_twin(e, t, f'{name} at the start')
    for i, step in enumerate(steps):
        play(e, t, step, f'{name} step {i} ({step[0]})')
    return e, t


# ---- 1. the reference's own grown run ---------------------------------------------------------------------------------------------------

def test_g26_on_the_device():
    """G26: the same schedule of extend_se2 and iterate(2, relinearise=True).  Masks, counts, iters and damping exactly; means,
    messages, linpoints, factors and energy within the parity contract; solve_map and marginals against the recorded joint."""
    g = golden('G26_se2_posegraph_grown')
    beta, damping, und, minlin, sweeps = g['cfg']
    sched = dict(beta=float(beta), num_undamped_iters=int(und), min_linear_iters=int(minlin), eta_damping=float(damping))
    full, start = g26_graph(g)
    e, t = make_engine(start, sched), live_twin(start, sched)
    appends = {int(s): (int(n), int(f)) for s, n, f in g['appends']}
    worst = {}

    def gap(name, a, b):
        worst[name] = max(worst.get(name, 0.0), rel(a, b))
        assert rel(a, b) < PARITY, f"{name}: {rel(a, b):.3e}"

    s = 0
    while s < int(sweeps):
        if s in appends:
            k = tail(full, e.N, e.F, *appends[s])[1]
            e.extend_se2(k['va'], k['vb'], k['z'], k['s'], k['prior_eta'], k['prior_lam'])
            t.extend(**k)
            assert e.sizes() == appends[s]
        counts = e.iterate(2, relinearise=True)
        t.iterate(2, relinearise=True)
        F = e.F
        assert F == int(g['sweep_f'][s + 1])
        assert counts.tolist() == g['mask'][s:s + 2, :F].sum(1).tolist(), f"sweeps {s}, {s + 1}: counts {counts}"
        lp, it, dm = e.linearisation()
        assert np.array_equal(it, g['iters'][s + 1, :F]) and np.array_equal(dm, g['damp'][s + 1, :F]), f"sweep {s + 1}: iters / damping"
        assert np.array_equal(it == 0, g['mask'][s + 1, :F].astype(bool))
        gap('energy', e.energy(), g['energy'][s + 1])
        s += 2
    lp, it, dm = e.linearisation()
    gap('means', e.get_means(), g['means']); gap('linpoint', lp, g['linpoint'])
    for name, a in zip(('msg_eta_a', 'msg_lam_a', 'msg_eta_b', 'msg_lam_b'), e.messages()):
        gap('messages', a, g[name])
    eta, lam = e.beliefs()
    gap('beliefs', eta, g['bel_eta']); gap('beliefs', lam, g['bel_lam'])
    je, jl = dense_joint(full, g['feta'], g['flam'])
    x = np.cos(np.arange(je.size) * 0.37)
    gap('factors', e.joint_eta().reshape(-1), je); gap('factors', e.joint_matvec(x).reshape(-1), jl @ x)
    assert_matches_twin(e, t, 'G26 at the end')
    mu, info = e.solve_map()
    assert info['converged']
    gap('map', mu, g['map_mu'])
    sigma, minfo = e.marginals()
    assert minfo['converged']
    gap('marginals', sigma, g['map_sigma_diag'])
    print('G26 worst gaps against the reference', {k: f'{v:.2e}' for k, v in worst.items()})
    e.close()


# ---- 2. shapes ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(EDGE_CASES))
def test_shapes_match_the_twin(name):
    """F 63 -> 65 and 255 -> 257; dF = 1; an isolated new pose (dF = 0); a closure alone (dN = 0); from one pose and no factor, pose by
    pose, to 10; a tenth factor onto the hub variable, which holds 9; the turns40 graph itself continued by three poses.  Each ends with SWEEPS relinearising sweeps."""
    g, steps = EDGE_CASES[name]
    e, t = run_schedule(g, steps, name)
    if name == 'onto_hub':                                   # pose 5 held 9 factors before the extend and holds 10 now
        assert np.bincount(np.concatenate([g['va'], g['vb']]))[5] == 9 and np.bincount(np.concatenate([t.va, t.vb]))[5] == 10
    e.close()


# ---- 3. kept state ------------------------------------------------------------------------------------------------------------------------

def test_extend_keeps_every_old_factor_and_variable():
    g, steps = kept_state_case()
    e, ref = make_engine(g, SCHEDULE), make_engine(g, SCHEDULE)
    e.iterate(5, relinearise=True); ref.iterate(5, relinearise=True)
    F0, N0 = e.F, e.N
    before = state(e)
    k = steps[1][1]
    e.extend_se2(k['va'], k['vb'], k['z'], k['s'], k['prior_eta'], k['prior_lam'])       # 4 closures, no new pose
    after = state(e)
    assert e.F == F0 + 4 and e.N == N0
    for i in (0, 1, 2, 3, 7, 8, 9):                            # messages, linpoint, iters, damping of the old factors
        assert after[i][:F0].tobytes() == before[i].tobytes(), f"state[{i}] of the old factors changed"
    for i in (4, 5, 6):                                        # beliefs and means: zero messages are added behind the old ones
        assert after[i].tobytes() == before[i].tobytes(), f"state[{i}] of the old variables changed"
    assert np.array_equal(after[8][F0:], np.ones(4)) and not after[9][F0:].any() and not any(after[i][F0:].any() for i in range(4))
    assert np.array_equal(after[7][F0:], np.concatenate([after[6].reshape(-1, 3)[k['va']], after[6].reshape(-1, 3)[k['vb']]], 1))
    # eta_f, Lambda_f of the old factors: the joint of the grown handle minus the new factors' own part is that of the never-extended one
    t = live_twin(g)
    t.iterate(5, relinearise=True)
    t.extend(**k)
    zero = np.zeros_like(t.feta); zero[F0:] = t.feta[F0:]
    zl = np.zeros_like(t.flam); zl[F0:] = t.flam[F0:]
    full = dict(N=N0, va=t.va, vb=t.vb, prior_eta=np.zeros((N0, 3)), prior_lam=np.zeros((N0, 3, 3)))
    ne, nlam = dense_joint(full, zero, zl)                    # the new factors alone
    x = np.cos(np.arange(3 * N0) * 0.37)
    assert rel(e.joint_eta().reshape(-1) - ne, ref.joint_eta().reshape(-1)) < TOL
    assert rel(e.joint_matvec(x).reshape(-1) - nlam @ x, ref.joint_matvec(x).reshape(-1)) < TOL
    # and bit for bit: with the new factors culled again the handle is the never-extended one
    e.cull(np.arange(F0, F0 + 4))
    assert same_bits(state(e), state(ref))
    assert e.joint_eta().tobytes() == ref.joint_eta().tobytes() and e.joint_matvec(x).tobytes() == ref.joint_matvec(x).tobytes()
    e.close(); ref.close()


@pytest.mark.parametrize('name,K', [('f63_65', 63), ('f255_257', 255), ('from_one_pose', 0), ('onto_hub', 18)])
def test_create_then_extend_is_create_whole(name, K):
    """A handle created with the first K factors and extended by the rest before any sweep is bit-identical to the handle created
    whole: eta_f and Lambda_f (through the joint), linpoint, iters, damping, beliefs -- and stays so through relinearising sweeps."""
    from lin_nonlin_cases import chain
    from lin_nonlin_live_cases import hub_plus
    g = {'f63_65': lambda: chain(66, seed=65), 'f255_257': lambda: chain(258, seed=257), 'from_one_pose': lambda: chain(10, seed=4), 'onto_hub': hub_plus}[name]()
    N0 = K + 1 if name != 'onto_hub' else 12
    whole, part = make_engine(g, SCHEDULE), make_engine(head(g, N0, K), SCHEDULE)
    k = tail(g, N0, K)[1]
    part.extend_se2(k['va'], k['vb'], k['z'], k['s'], k['prior_eta'], k['prior_lam'])
    x = np.cos(np.arange(3 * g['N']) * 0.37)
    for when in ('before any sweep', 'after 6 sweeps'):
        assert same_bits(state(whole), state(part)), when
        assert whole.joint_eta().tobytes() == part.joint_eta().tobytes() and whole.joint_matvec(x).tobytes() == part.joint_matvec(x).tobytes(), when
        ca, cb = whole.iterate(6, relinearise=True), part.iterate(6, relinearise=True)
        assert np.array_equal(ca, cb)
    whole.close(); part.close()


# ---- 4. shrink ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', sorted(SHRINK_CASES))
def test_shrinks_match_the_twin(name):
    """Retire the oldest pose with and without the fold; drop one closure; retire everything and grow again; F 65 -> 63; F 257 -> 255
    and 599 -> 199 with energy() before and after (fewer blocks of energy partials than the handle's buffer holds).  After each
    shrink the maps equal the twin's, the survivors' per-factor state is bit for bit what it was, and SWEEPS sweeps match the twin."""
    from lin_shrink_cases import plan
    g, steps = SHRINK_CASES[name]
    e, t = make_engine(g, SCHEDULE), live_twin(g, SCHEDULE)
    for i, step in enumerate(steps):
        if step[0] == 'shrink':
            before = state(e)
            fkeep = plan(t.N, t.va, t.vb, step[1]['retire'], step[1]['drop'])[1]
        play(e, t, step, f'{name} step {i} ({step[0]})')
        if step[0] == 'shrink':
            after = state(e)
            for j in (0, 1, 2, 3, 7, 8, 9):                    # messages, linpoint, iters, damping of the survivors
                assert after[j].tobytes() == before[j][fkeep].tobytes(), f"{name}: state[{j}] of the surviving factors changed"
    e.close()


def test_fold_of_a_converged_chain_leaves_the_survivors_beliefs():
    """beta = +inf (the factors stay at their first linearisation point: a linear chain), 60 sweeps, the oldest pose retired with the
    fold: on a tree with converged messages the fold is GBP's exact marginalisation, and the leaving factor is a prefix of its one
    survivor's adjacency list -- the survivors' belief records are bit for bit what they were."""
    g, sched = converged_chain(), dict(SCHEDULE, beta=np.inf)
    e, t = make_engine(g, sched), live_twin(g, sched)
    e.iterate(60, relinearise=True); t.iterate(60, relinearise=True)
    eta, lam = e.beliefs()
    mu = e.get_means().reshape(-1, 3)
    vmap, fmap = e.retire([0], fold=True)
    t.shrink(retire=[0], fold=True)
    eta1, lam1 = e.beliefs()
    assert eta1.tobytes() == eta[1:].tobytes() and lam1.tobytes() == lam[1:].tobytes() and e.get_means().tobytes() == mu[1:].tobytes()
    assert_matches_twin(e, t, 'after the fold')
    # converged: the next sweeps do not move the survivors either
    e.iterate(SWEEPS, relinearise=True); t.iterate(SWEEPS, relinearise=True)
    assert_matches_twin(e, t, 'sweeps after the fold')
    assert rel(e.get_means(), mu[1:]) < 1e-8
    e.close()


# ---- 5. a window ----------------------------------------------------------------------------------------------------------------------------

def test_fixed_lag_window():
    """40 steps of extend (one pose, its odometry, a closure every 7th), retire the oldest beyond 12 held, two relinearising sweeps;
    the twin after every step; the handle holds one generation; solve_map at the end against the twin's dense solve."""
    g, groups = window_schedule()
    e, t = make_engine(g, SCHEDULE), live_twin(g, SCHEDULE)
    allocs = {}
    for k, group in enumerate(groups, start=1):
        for step in group:
            play(e, t, step, f'window step {k} ({step[0]})')
        allocs[k] = e.alloc_count()
    assert (e.N, len(groups)) == (12, 40)
    assert allocs[40] == allocs[20], f"the handle grew: {allocs[20]} allocations after step 20, {allocs[40]} after step 40"
    mu, info = e.solve_map()
    eta, lam = t.joint()
    want = np.linalg.solve(lam, eta)
    print('window: solve_map against the dense solve', rel(mu, want))
    assert info['converged'] and rel(mu, want) < 1e-9, f"map {rel(mu, want):.3e}"
    e.close()


# ---- 6. fuzz --------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', FUZZ_SEEDS)
def test_random_schedules_match_the_twin(seed):
    g, steps = fuzz_schedule(seed)
    kinds = {s[0] for s in steps}
    assert len(steps) == 25 and {'extend', 'shrink', 'iterate'} <= kinds
    e, t = run_schedule(g, steps, f'fuzz {seed}')
    e.close()


# ---- 7. contract ----------------------------------------------------------------------------------------------------------------------------

def test_a_linear_handle_refuses_both_calls():
    from gbp_amd import _capi
    from gbp_amd.linear import LinearEngine
    g = kept_state_case()[0]
    F = len(g['va'])
    e = LinearEngine(g['va'], g['vb'], np.zeros((F, 6)), np.tile(np.eye(6), (F, 1, 1)), g['prior_eta'], g['prior_lam'])
    e.update_all_beliefs()
    e.iterate(2)
    before = list(e.messages()) + list(e.beliefs())
    ext, shr = _capi.LinExtNonlinear(), _capi.LinShrink()
    ids = np.zeros(1, dtype=np.int32)
    shr.n_retire_vars, shr.retire_vars, shr.fold = 1, _capi.iptr(ids), 1
    assert e._lib.gbp_lin_extend_nonlinear(e._h, ct.byref(ext)) == ESTATE and b'nonlinear' in e._lib.gbp_last_error()
    assert e._lib.gbp_lin_shrink_nonlinear(e._h, ct.byref(shr)) == ESTATE and b'nonlinear' in e._lib.gbp_last_error()
    assert e.sizes() == (g['N'], F) and same_bits(before, list(e.messages()) + list(e.beliefs()))
    e.close()


def test_invalid_descriptors_change_nothing():
    from gbp_amd import _capi
    g, steps = kept_state_case()
    a, b = make_engine(g, SCHEDULE), make_engine(g, SCHEDULE)
    a.iterate(3, relinearise=True); b.iterate(3, relinearise=True)
    lib, N, F = a._lib, a.N, a.F
    count = a.alloc_count()
    va, vb = np.array([0, 3], dtype=np.int32), np.array([N, 9], dtype=np.int32)       # one new pose, two factors
    z, s = np.zeros((2, 3)), np.tile([10.0, 10.0, 20.0], (2, 1))
    pe, pl = np.zeros((1, 3)), np.eye(3)[None].copy()

    def ext(dN=1, dF=2, a_=va, b_=vb, zz=z, ss=s, pe_=pe, pl_=pl):
        return _capi.LinExtNonlinear(dN, dF, _capi.iptr(a_), _capi.iptr(b_), _capi.dptr(zz), _capi.dptr(ss), _capi.dptr(pe_), _capi.dptr(pl_))

    def with_(arr, idx, val):
        out = arr.copy(); out[idx] = val
        return out

    bad_ext = {'null var_a': ext(a_=None), 'null var_b': ext(b_=None), 'null z': ext(zz=None), 'null s': ext(ss=None), 'null prior_eta': ext(pe_=None),
               'null prior_lam': ext(pl_=None), 'id out of range': ext(b_=with_(vb, 0, N + 1)), 'negative id': ext(a_=with_(va, 1, -1)),
               'a == b': ext(b_=with_(vb, 1, 3)), 'z nan': ext(zz=with_(z, (1, 2), np.nan)), 'z inf': ext(zz=with_(z, (0, 0), np.inf)),
               's = 0': ext(ss=with_(s, (1, 1), 0.0)), 's < 0': ext(ss=with_(s, (0, 2), -1.0)), 's inf': ext(ss=with_(s, (0, 0), np.inf)),
               'negative dN': ext(dN=-1), 'negative dF': ext(dF=-1)}
    for name, d in bad_ext.items():
        assert lib.gbp_lin_extend_nonlinear(a._h, ct.byref(d)) == EINVAL, name
    assert lib.gbp_lin_extend_nonlinear(a._h, None) == EINVAL

    def shr(retire=(), drop=(), fold=1, null=False):
        r, d = np.array(retire, dtype=np.int32), np.array(drop, dtype=np.int32)
        out = _capi.LinShrink()
        out.n_retire_vars, out.retire_vars = len(r), (None if null else _capi.iptr(r))
        out.n_drop_factors, out.drop_factors, out.fold = len(d), _capi.iptr(d), fold
        out._keep = (r, d)
        return out

    bad_shr = {'retire id out of range': shr(retire=[N]), 'negative retire id': shr(retire=[-1]), 'retire id twice': shr(retire=[2, 2]),
               'drop id out of range': shr(drop=[F]), 'null list': shr(retire=[1], null=True), 'fold 2': shr(retire=[1], fold=2)}
    for name, d in bad_shr.items():
        assert lib.gbp_lin_shrink_nonlinear(a._h, ct.byref(d)) == EINVAL, name
    assert lib.gbp_lin_shrink_nonlinear(a._h, None) == EINVAL
    assert a.sizes() == (N, F) and a.alloc_count() == count
    x = np.cos(np.arange(3 * N) * 0.37)
    assert same_bits(state(a), state(b)) and a.joint_eta().tobytes() == b.joint_eta().tobytes() and a.joint_matvec(x).tobytes() == b.joint_matvec(x).tobytes()
    ca, cb = a.iterate(2, relinearise=True), b.iterate(2, relinearise=True)
    assert np.array_equal(ca, cb) and same_bits(state(a), state(b))
    # nothing to do: GBP_OK, nothing changes, the maps are the identity
    assert lib.gbp_lin_extend_nonlinear(a._h, ct.byref(ext(dN=0, dF=0))) == 0
    vmap, fmap = a.shrink()
    assert vmap.tolist() == list(range(N)) and fmap.tolist() == list(range(F)) and same_bits(state(a), state(b))
    # the generic extend stays refused through the Python surface too
    with pytest.raises(_capi.GbpError):
        a.extend([0], [1], np.zeros((1, 6)), np.zeros((1, 6, 6)))
    assert a.sizes() == (N, F)
    a.close(); b.close()


def test_solver_results_are_dropped_by_both_calls():
    from gbp_amd import _capi
    g, steps = kept_state_case()
    e = make_engine(g, SCHEDULE)
    e.iterate(3, relinearise=True)
    k = steps[1][1]
    for call in (lambda: e.extend_se2(k['va'], k['vb'], k['z'], k['s']), lambda: e.retire([4])):
        e.solve_map()
        e.map_mean()
        call()
        with pytest.raises(_capi.GbpError) as err:
            e.map_mean()
        assert err.value.code == ESTATE
        mu, info = e.solve_map()
        assert info['converged'] and mu.shape == (e.N, 3)
    e.close()
