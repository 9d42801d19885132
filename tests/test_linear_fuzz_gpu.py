"""Random call schedules on a live linear handle (tests/lin_fuzz_cases.py): per (seed, d) six steps of 2 to 5 calls -- sweeps, robustify,
set_robust, solve_map, marginals, joint_matvec / joint_eta, update_all_beliefs, in an order nobody chose -- each closed by an extend, on
the handle under test `e` beside the host model (LinModel: a RobustOracle grown the same way) and a `shadow` handle that gets the same
schedule without its solver and read-only calls.  After every call:
  1. sizes, weights (TOL) and flags (equal), messages, beliefs, means and energy (TOL = 1e-9 relative, the linear tests' bound) against
     the model;
  2. joint_matvec / joint_eta (TOL), solve_map (converged, rel_residual <= 1e-12, mu at TOL), map_distance and marginals (sigma and
     sigma_joint at TOL, batches = ceil(len(ids) d / 8)) against the dense joint at the MODEL's weights;
  3. across a growing extend, bit for bit: old messages, old belief records, old weights and flags; new messages zero, new weights 1,
     new flags False;
  4. map_mean / map_distance give GBP_ESTATE exactly while the model has no solve behind it, robustify / iterate(robustify=True) exactly
     while it has no losses; map_mean returns the last solve's iterate bitwise whatever was called since;
  5. at the end of every step state(e) and e.weights() are the shadow's, bit for bit: the solvers leave the sweep alone;
  6. once per schedule a call the header refuses gives its code and leaves `e` bitwise on the shadow, and the next step is accepted;
  7. at the end, after set_robust(None), joint_eta, joint_matvec, a cold solve_map (with its iteration count) and marginals are bitwise
     those of a handle created whole from the final arrays: the grown layout is the one gbp_lin_create makes.
tests/test_linear_fuzz_cpu.py proves on the host alone that every default schedule is healthy and at least 1e-6 clear of every loss
threshold at every step, so no comparison here is conditional.  Seeds: lin_fuzz_cases.SEEDS, extended to GBP_LIN_FUZZ_SEEDS seeds for a
soak.  As measured on the MI355X over the 48 default cases: the MAP within 2.0e-12, marginals within 2.3e-13, every other quantity
within 1.3e-15 of the model; check 7 holds bitwise in all 48."""
import os

import numpy as np
import pytest

from lin_fuzz_cases import DIMS, GBP_ESTATE, MARGIN, REFUSALS, SEEDS, SHAPES, LinModel, healthy, random_schedule, refused_variant, tally
from lin_map_cases import rel

pytestmark = pytest.mark.gpu

TOL = 1e-9
N_SEEDS = int(os.environ.get('GBP_LIN_FUZZ_SEEDS', len(SEEDS)))
ALL_SEEDS = tuple(SEEDS) + tuple(range(max(SEEDS) + 1, max(SEEDS) + 1 + max(0, N_SEEDS - len(SEEDS))))
CASES = [(seed, D) for seed in ALL_SEEDS for D in DIMS]
WORST = {}          # quantity -> the worst gap seen over all cases
MET = {}            # (seed, D) -> tally of the shapes, from the model that followed the engine's own sizes and codes


def engine(*a, **k):
    from gbp_amd.linear import LinearEngine
    return LinearEngine(*a, **k)


def state(e):
    """Everything a sweep reads or writes, as the handle holds it."""
    return e.messages() + e.beliefs() + (e.get_means(),)


def same_bits(x, y):
    return len(x) == len(y) and all(np.asarray(a).shape == np.asarray(b).shape and np.array_equal(a, b) for a, b in zip(x, y))


def _gap(name, got, want, where):
    g = rel(got, want)
    WORST[name] = max(WORST.get(name, 0.0), g)
    assert g < TOL, f"{where}: {name} {g:.3e}"


def _raises(code, call, where):
    from gbp_amd import _capi
    with pytest.raises(_capi.GbpError) as err:
        call()
    assert err.value.code == code, (where, str(err.value))


def _do(e, op):
    """One call of the schedule on an engine; returns what the call returns."""
    a = op.args
    if op.kind == 'iterate':
        return e.iterate(a['n'], robustify=a['robustify'])
    if op.kind == 'robustify':
        return e.robustify_all_factors()
    if op.kind == 'update_beliefs':
        return e.update_all_beliefs()
    if op.kind == 'map_mean':
        return e.map_mean()
    if op.kind == 'marginals':
        return e.marginals(ids=a['ids'], joint=a['joint'])
    if op.kind == 'extend':
        kw = {}
        if a['loss'] is not None:
            kw = dict(loss=a['loss'], threshold=a['thr'], noise_var=a['sigma'] ** 2)
        return e.extend(a['va'], a['vb'], a['fe'], a['fl'], a['pe'], a['pl'], factor_const=a['fc'], **kw)
    raise ValueError(op.kind)


def _set_robust(e, m, a):
    """set_robust with the noise variances of ALL factors (the model holds them), which the constant loss reads."""
    if a['loss'] is None:
        e.set_robust(None)
    else:
        e.set_robust(a['loss'], a['thr'], m.o.sigma ** 2)


def _against_model(e, m, where):                                                                      # 1.
    o = m.o
    assert e.sizes() == (o.N, o.F) == (e.N, e.F), where
    w, flag = e.weights()
    assert np.array_equal(flag, o.flag), f"{where}: flags differ at {np.flatnonzero(flag != o.flag)}"
    _gap('weights', w, o.w, where)
    for name, a, b in zip(('msg eta a', 'msg lam a', 'msg eta b', 'msg lam b'), e.messages(), o.messages()):
        _gap(name, a, b, where)
    for name, a, b in zip(('belief eta', 'belief lam'), e.beliefs(), o.beliefs()):
        _gap(name, a, b, where)
    _gap('means', e.get_means(), o.get_means(), where)
    got, want = e.energy(), o.energy()
    g = abs(got - want) / abs(want) if want else abs(got)
    WORST['energy'] = max(WORST.get('energy', 0.0), g)
    assert g <= TOL, f"{where}: energy {got!r} vs {want!r}"


def _state_codes(e, m, last_mu, where):                                                               # 4.
    if m.solved:
        assert np.array_equal(e.map_mean(), last_mu), f"{where}: the last MAP iterate moved"
        e.map_distance()
    else:
        _raises(GBP_ESTATE, e.map_mean, where)
        _raises(GBP_ESTATE, e.map_distance, where)


def _solve(e, m, warm, where):                                                                        # 2.
    mu, info = e.solve_map(warm_start=warm)
    assert info['converged'] and info['rel_residual'] <= 1e-12, (where, info)
    want = m.map_mean()
    _gap('map', mu, want, where)
    dist, host = e.map_distance(), float(np.linalg.norm(e.get_means() - mu.reshape(-1)))
    gd = abs(dist - host) / max(float(np.linalg.norm(mu)), 1.0)
    WORST['map_distance'] = max(WORST.get('map_distance', 0.0), gd)
    assert gd <= 1e-9, (where, dist, host)
    assert np.array_equal(e.map_mean(), mu), where
    return mu


def _marginals(e, m, ids, joint, where):
    want, want_joint = m.marginals(ids)
    if joint:
        sigma, sj, info = e.marginals(ids=ids, joint=True)
        _gap('sigma_joint', sj, want_joint, where)
    else:
        sigma, info = e.marginals(ids=ids)
    assert info['converged'] and info['batches'] == -(-len(ids) * m.D // 8), (where, info)
    _gap('sigma', sigma, want, where)


def _joint(e, m, x, where):
    eta, lam = m.joint()
    _gap('joint_eta', e.joint_eta(), eta, where)
    _gap('joint_matvec', e.joint_matvec(x), lam @ x.reshape(-1), where)


def _growth_kept(before, after, N0, F0, D, where):                                                    # 3.
    (st0, w0, f0), (st1, w1, f1) = before, after
    assert same_bits([x[:F0] for x in st0[:4]], [x[:F0] for x in st1[:4]]), f"{where}: old messages moved"
    assert all(not x[F0:].any() for x in st1[:4]), f"{where}: new messages are not zero"
    assert same_bits([b[:N0] for b in st0[4:6]], [b[:N0] for b in st1[4:6]]), f"{where}: old beliefs changed"
    assert np.array_equal(st0[6], st1[6][:N0 * D]), f"{where}: old means changed"
    assert np.array_equal(w1[:F0], w0) and np.array_equal(f1[:F0], f0), f"{where}: old weights or flags changed"
    assert np.array_equal(w1[F0:], np.ones(len(w1) - F0)) and not f1[F0:].any(), f"{where}: new weights are not 1 / flags not False"


def _on_shadow(e, shadow, where):                                                                     # 5.
    assert e.sizes() == shadow.sizes(), where
    assert same_bits(state(e), state(shadow)), f"{where}: the state left the shadow's"
    assert same_bits(e.weights(), shadow.weights()), f"{where}: the weights left the shadow's"


def _refuse(e, m, shadow, seed, name, where):                                                         # 6.
    got, op, code = refused_variant(np.random.RandomState(seed), m, name)
    assert got == name
    _raises(code, lambda: _do(e, op), f'{where} refusal {name!r}')
    assert (e.N, e.F) == e.sizes() == (m.N, m.F), where
    _on_shadow(e, shadow, f'{where} after refusal {name!r}')


@pytest.mark.parametrize('seed,D', CASES)
def test_random_call_schedule(seed, D):
    s = random_schedule(seed, D)
    b = s.base
    m = LinModel(s)
    pair = []
    for _ in range(2):
        h = engine(b['va'], b['vb'], b['fe'], b['fl'], b['pe'], b['pl'], factor_const=b['fc'], eta_damping=b['damping'])
        if b['set_losses']:
            h.set_robust(b['loss'], b['thr'], b['sigma'] ** 2)
        h.update_all_beliefs()
        pair.append(h)
    e, shadow = pair
    last_mu, calls = None, 0
    _against_model(e, m, f'seed {seed} d {D} created')
    for k, ops in enumerate(s.steps):
        if s.refuse[0] == k:
            _refuse(e, m, shadow, seed, s.refuse[1], f'seed {seed} d {D} step {k}')
        for j, op in enumerate(ops):
            where = f'seed {seed} d {D} step {k} call {j} ({op.kind})'
            a = op.args
            N0, F0 = m.N, m.F
            kept = (state(e),) + e.weights() if op.kind == 'extend' else None
            margin_from = len(m.margins)
            code = m.apply(op)
            assert healthy(m) and min(m.margins[margin_from:], default=1.0) >= MARGIN, where        # given: test_linear_fuzz_cpu.py
            if code is not None:                                                                      # 4. a refused call of the schedule
                assert code == GBP_ESTATE and op.kind in ('iterate', 'robustify') and not m.losses_on
                _raises(code, lambda: _do(e, op), where)
            elif op.kind == 'set_robust':
                _set_robust(e, m, a)
                _set_robust(shadow, m, a)
            elif op.kind == 'solve_map':
                last_mu = _solve(e, m, a['warm'], where)
            elif op.kind == 'marginals':
                _marginals(e, m, a['ids'], a['joint'], where)
            elif op.kind == 'joint':
                _joint(e, m, a['x'], where)
            else:
                _do(e, op)
                _do(shadow, op)
            calls += 1
            _against_model(e, m, where)
            _state_codes(e, m, last_mu, where)
            if op.kind == 'extend' and (m.N, m.F) != (N0, F0):
                _growth_kept(kept, (state(e),) + e.weights(), N0, F0, D, where)
        _on_shadow(e, shadow, f'seed {seed} d {D} end of step {k}')
    # 7. the layout is the one gbp_lin_create makes
    where = f'seed {seed} d {D} against a handle created whole'
    e.set_robust(None)
    g = m.given
    fresh = engine(g['va'], g['vb'], g['fe'], g['fl'], g['pe'], g['pl'], factor_const=g['fc'], eta_damping=b['damping'])
    assert e.sizes() == fresh.sizes() == (m.N, m.F), where
    rs = np.random.RandomState(seed)
    x = rs.randn(m.N, D)
    assert np.array_equal(e.joint_eta(), fresh.joint_eta()), f'{where}: joint_eta'
    assert np.array_equal(e.joint_matvec(x), fresh.joint_matvec(x)), f'{where}: joint_matvec'
    (mu_e, info_e), (mu_f, info_f) = e.solve_map(), fresh.solve_map()
    assert info_e == info_f and info_e['converged'], (where, info_e, info_f)
    assert np.array_equal(mu_e, mu_f), f'{where}: solve_map'
    if m.N:
        ids = [int(v) for v in rs.permutation(m.N)[:min(m.N, 4)]]
        (sig_e, sj_e, minfo_e), (sig_f, sj_f, minfo_f) = e.marginals(ids=ids, joint=True), fresh.marginals(ids=ids, joint=True)
        assert minfo_e == minfo_f and minfo_e['converged'], (where, minfo_e, minfo_f)
        assert np.array_equal(sig_e, sig_f) and np.array_equal(sj_e, sj_f), f'{where}: marginals'
    for h in (e, shadow, fresh):
        h.close()
    MET[(seed, D)] = tally(s, m)
    print(f'LINFUZZ seed={seed} d={D}: N={m.N} F={m.F} calls={calls} robustifies={len(m.margins)} refusal={s.refuse[1]!r} '
          f'cold solve iters={info_e["iters"]}')


def test_linear_fuzz_tally(request):
    """(runs after the parametrised test above: same module, file order)  The worst gap per quantity against its bound, and the shapes
    the engine met over the default seeds -- every one of lin_fuzz_cases.SHAPES and every refusal."""
    if os.environ.get('PYTEST_XDIST_WORKER'):
        pytest.skip('the cases are spread over xdist workers (soak runs): the tally lives in the other processes')
    if request.config.getoption('keyword'):
        pytest.skip('-k selected a subset: the tally is incomplete by construction')
    assert sorted(MET) == sorted(CASES), f'cases that did not finish: {sorted(set(CASES) - set(MET))}'
    for name, g in sorted(WORST.items()):
        print(f'LINFUZZ worst gap {name}: {g:.3e} (bound {TOL:g})')
    total = {k: sum(MET[(seed, D)][k] for seed in SEEDS for D in DIMS) for k in SHAPES + REFUSALS}
    print('LINFUZZ shapes met on the device:', total)
    assert all(v >= 1 for v in total.values()), {k: v for k, v in total.items() if not v}
    assert max(WORST.values()) < TOL
