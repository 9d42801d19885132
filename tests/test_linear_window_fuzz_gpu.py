"""Random sliding-window schedules on a live linear handle (tests/lin_window_cases.py): per (seed, d) six steps of 2 to 4 calls drawn as
the call fuzz draws them, one extend and one shrink (random retire list, random drop list, either fold), on the handle under test beside
the host model (WindowModel: a RobustOracle grown by lin_extend_cases.grow() and shrunk by lin_shrink_cases.shrink()) and a twin handle
given the same calls.  After every call, with the checks of tests/test_linear_fuzz_gpu.py (imported, not restated):
  1. sizes, weights (TOL) and flags (equal), messages, beliefs, means and energy (TOL = 1e-9 relative) against the model;
  2. joint_matvec / joint_eta, solve_map, map_distance and marginals against the dense joint at the MODEL's weights -- after a shrink
     that is the joint of the shrunk graph with the folded priors;
  3. map_mean / map_distance give GBP_ESTATE exactly while the model has no solve behind it (a shrink that removes something forgets it);
  4. across a shrink: the maps are the model's, the surviving factors' messages, weights and flags bit for bit;
  5. at the end of every step the twin holds the same bits: no atomics, no race.
tests/test_linear_window_fuzz_cpu.py proves on the host alone that every chosen schedule is healthy and at least 1e-6 clear of every loss
threshold at every step, so no comparison here is conditional and no seed skips."""
import numpy as np
import pytest

from lin_fuzz_cases import MARGIN, healthy
from lin_window_cases import DIMS, SEEDS, WindowModel, window_schedule
from test_linear_fuzz_gpu import (_against_model, _do, _joint, _marginals, _raises, _set_robust, _solve, _state_codes, engine, same_bits,
                                  state)

pytestmark = pytest.mark.gpu

GBP_ESTATE = -5
CASES = [(seed, D) for seed in SEEDS for D in DIMS]


@pytest.mark.parametrize('seed,D', CASES)
def test_random_window_schedule(seed, D):
    s = window_schedule(seed, D)
    b = s.base
    m = WindowModel(s)
    pair = []
    for _ in range(2):
        h = engine(b['va'], b['vb'], b['fe'], b['fl'], b['pe'], b['pl'], factor_const=b['fc'], eta_damping=b['damping'])
        if b['set_losses']:
            h.set_robust(b['loss'], b['thr'], b['sigma'] ** 2)
        h.update_all_beliefs()
        pair.append(h)
    e, twin = pair
    last_mu, calls = None, 0
    _against_model(e, m, f'seed {seed} d {D} created')
    for k, ops in enumerate(s.steps):
        for j, op in enumerate(ops):
            where = f'seed {seed} d {D} step {k} call {j} ({op.kind})'
            a = op.args
            margin_from = len(m.margins)
            before = (state(e),) + e.weights() if op.kind == 'shrink' else None
            fkeep = None
            if op.kind == 'shrink':
                from lin_shrink_cases import plan
                fkeep = plan(m.N, m.o.va, m.o.vb, a['retire'], a['drop'])[1]
            code = m.apply(op)
            assert code is None, where
            assert healthy(m) and min(m.margins[margin_from:], default=1.0) >= MARGIN, where    # given: test_linear_window_fuzz_cpu.py
            if op.kind == 'set_robust':
                _set_robust(e, m, a); _set_robust(twin, m, a)
            elif op.kind == 'solve_map':
                last_mu = _solve(e, m, a['warm'], where)
                twin.solve_map(warm_start=a['warm'])
            elif op.kind == 'marginals':
                _marginals(e, m, a['ids'], a['joint'], where)
            elif op.kind == 'joint':
                _joint(e, m, a['x'], where)
            elif op.kind == 'shrink':
                maps = [h.shrink(a['retire'], a['drop'], fold=a['fold']) for h in (e, twin)]
                for vm, fm in maps:                                                               # 4.
                    assert np.array_equal(vm, m.maps[0]) and np.array_equal(fm, m.maps[1]), f'{where}: maps'
                st1, w1, f1 = (state(e),) + e.weights()
                assert same_bits([x[fkeep] for x in before[0][:4]], st1[:4]), f'{where}: surviving messages moved'
                assert np.array_equal(before[1][fkeep], w1) and np.array_equal(before[2][fkeep], f1), f'{where}: surviving weights or flags'
            else:
                _do(e, op); _do(twin, op)
            calls += 1
            _against_model(e, m, where)
            _state_codes(e, m, last_mu, where)
        assert e.sizes() == twin.sizes()
        assert same_bits(state(e), state(twin)) and same_bits(e.weights(), twin.weights()), f'seed {seed} d {D} end of step {k}: the twin differs'
    # the solvers on the final window: the dense joint of the shrunk graph at the model's weights
    where = f'seed {seed} d {D} final'
    _solve(e, m, False, where)
    if m.N:
        _marginals(e, m, [int(v) for v in np.random.RandomState(seed).permutation(m.N)[:min(m.N, 3)]], True, where)
    if not m.losses_on:
        _raises(GBP_ESTATE, e.robustify_all_factors, where)
    for h in (e, twin):
        h.close()
    print(f'LINWINDOW seed={seed} d={D}: N={m.N} F={m.F} calls={calls} robustifies={len(m.margins)}')
