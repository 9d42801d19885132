"""The random call schedules of tests/lin_fuzz_cases.py without a GPU: the generator is deterministic and draws only calls the header
allows (apart from the refusals it marks), the host model grown step by step is the oracle of the final graph, every default schedule
stays healthy and clear of the loss thresholds at every step -- so that tests/test_linear_fuzz_gpu.py may compare at every step of every
case, none left out -- and the default seeds meet every shape of lin_fuzz_cases.SHAPES and every refusal."""
import functools

import numpy as np
import pytest

from lin_fuzz_cases import (DIMS, EMPTY_SEED, MARGIN, N_STEPS, REFUSAL_CODE, REFUSALS, SEEDS, SHAPES, LinModel, Op, healthy, is_legal,
                            random_schedule, refused_variant, tally, threshold_margin)
from lin_robust_cases import RobustOracle

CASES = [(seed, D) for seed in SEEDS for D in DIMS]


@functools.lru_cache(maxsize=None)
def _schedule(seed, D):
    return random_schedule(seed, D)


@functools.lru_cache(maxsize=None)
def _run(seed, D):
    """The model through the schedule: (model, healthy at every step, smallest margin, largest |mean|, illegal calls drawn unmarked)."""
    s = _schedule(seed, D)
    m = LinModel(s)
    ok, big, unmarked, refused = healthy(m), 0.0, [], None
    for k, ops in enumerate(s.steps):
        if s.refuse is not None and s.refuse[0] == k:
            name, op, code = refused_variant(np.random.RandomState(seed), m, s.refuse[1])
            refused = (name, is_legal(m, op), code)
        for op in ops:
            why = is_legal(m, op)
            code = m.apply(op)
            if (why is not None) != bool(op.args.get('refused')) or (why is not None) != (code is not None):
                unmarked.append((k, op.kind, why, code))
            ok = ok and healthy(m)
            big = max(big, float(np.abs(m.o.mu).max()) if m.N else 0.0)
    return m, ok, min(m.margins, default=np.inf), big, unmarked, refused


def _same(a, b):
    if isinstance(a, np.ndarray):
        return np.array_equal(a, b)
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


@pytest.mark.parametrize('seed,D', CASES)
def test_generator_is_deterministic_and_legal(seed, D):
    a, b = _schedule(seed, D), random_schedule(seed, D)
    assert _same(tuple(a), tuple(b))
    assert len(a.steps) == N_STEPS and all(2 <= len(ops) - 1 <= 5 and ops[-1].kind == 'extend' for ops in a.steps)
    assert all(op.kind != 'extend' for ops in a.steps for op in ops[:-1])
    assert 0 <= a.base['N'] <= 30 and 0 <= len(a.base['va']) <= 69 and a.base['damping'] in (0.0, 0.4)
    for ops in a.steps:
        ext = ops[-1].args
        assert 0 <= len(ext['pe']) <= 4 and 0 <= len(ext['va']) <= 69
    if seed == EMPTY_SEED:
        first = a.steps[0][-1].args
        assert a.base['N'] == 0 and len(a.base['va']) == 0 and len(first['pe']) >= 2 and len(first['va']) >= 1
    m, _, _, _, unmarked, refused = _run(seed, D)
    assert not unmarked, unmarked
    assert m.N <= 55 and m.F <= 69 * (N_STEPS + 1)
    # the refusal of this schedule breaks the rule it names and nothing else knows better
    assert a.refuse is not None and refused[0] == a.refuse[1] and refused[1] == refused[0] and refused[2] == REFUSAL_CODE[refused[0]]


def test_every_refusal_is_an_argument_or_state_error_by_the_headers_rules():
    s = _schedule(1, 3)
    m = LinModel(s)
    for op in s.steps[0]:
        m.apply(op)
    m.apply(Op('set_robust', dict(loss=None, thr=np.zeros(m.F))))
    rs = np.random.RandomState(0)
    for name in REFUSALS:
        got, op, code = refused_variant(rs, m, name)
        assert got == name and is_legal(m, op) == name and code == REFUSAL_CODE[name]
    assert {refused_variant(rs, m)[0] for _ in range(200)} == set(REFUSALS)


def _final_losses(s):
    """The losses of the final graph by the header's rules alone: set_robust replaces them, NULL clears them, an extend appends `loss`
    or NONE and leaves old factors at NONE where losses were not set."""
    loss, on = (list(s.base['loss']) if s.base['set_losses'] else [None] * len(s.base['va'])), s.base['set_losses']
    for ops in s.steps:
        for op in ops:
            a = op.args
            if op.kind == 'set_robust':
                on = a['loss'] is not None
                loss = list(a['loss']) if on else [None] * len(loss)
            elif op.kind == 'extend':
                dF = len(a['va'])
                brings = a['loss'] is not None and dF > 0
                if brings and not on:
                    loss = [None] * len(loss)
                loss = loss + (list(a['loss']) if brings else [None] * dF)
                on = on or brings
    return loss, on


@pytest.mark.parametrize('seed,D', CASES)
def test_model_grown_without_sweeps_is_the_oracle_of_the_final_graph(seed, D):
    s = _schedule(seed, D)
    m = LinModel(s)
    cat = {k: [s.base[k]] for k in ('va', 'vb', 'J', 'z', 'sigma', 'pe', 'pl')}
    thr = s.base['thr']
    for ops in s.steps:
        for op in ops:
            if op.kind in ('set_robust', 'update_beliefs', 'extend'):
                assert m.apply(op) is None
            if op.kind == 'set_robust' and op.args['loss'] is not None:
                thr = op.args['thr']
            if op.kind == 'extend':
                for k in cat:
                    cat[k].append(op.args[k])
                thr = np.concatenate([thr, op.args['thr']])
    loss, on = _final_losses(s)
    assert m.losses_on == on and m.o.loss == loss and not m.solved and m.has_beliefs
    c = {k: np.concatenate(v) for k, v in cat.items()}
    whole = RobustOracle(c['va'], c['vb'], c['J'], c['z'], c['sigma'], c['pe'], c['pl'], loss, thr, eta_damping=s.base['damping'])
    whole.update_all_beliefs()
    assert (m.N, m.F) == (whole.N, whole.F)
    for x, y in zip(m.o.messages() + m.o.beliefs() + (m.o.get_means(),), whole.messages() + whole.beliefs() + (whole.get_means(),)):
        assert np.allclose(x, y, rtol=1e-12, atol=0.0)
    assert abs(m.o.energy() - whole.energy()) <= 1e-12 * abs(whole.energy())
    assert np.array_equal(m.o.w, np.ones(m.F)) and not m.o.flag.any()
    has = np.array([l is not None for l in loss], dtype=bool)
    assert np.array_equal(m.o.thr[has], thr[has])
    # what the engine is handed piece by piece is the oracle's nominal factor
    for k, ref in (('fe', whole.fe0), ('fl', whole.fl0), ('fc', whole.fc0), ('pe', whole.pe), ('pl', whole.pl)):
        assert np.allclose(m.given[k], ref, rtol=1e-12, atol=1e-300), k
    assert np.array_equal(m.given['va'], whole.va) and np.array_equal(m.given['vb'], whole.vb)


def test_every_default_schedule_is_healthy_and_clear_of_the_thresholds():
    """48 of 48: healthy at every step, and |M - t| / t >= 1e-6 at every robustify (a constant-loss weight jumps at the threshold).
    As drawn: 370 robustifies, smallest margin 1.3e-5, largest |mean| 9.8."""
    worst_margin, worst_mean, robustifies = np.inf, 0.0, 0
    for seed, D in CASES:
        m, ok, margin, big, _, _ = _run(seed, D)
        print(f'LINFUZZ host seed={seed} D={D}: N={m.N} F={m.F} healthy={ok} robustifies={len(m.margins)} margin={margin:.3e} max|mean|={big:.3g}')
        assert ok, (seed, D)
        assert margin >= MARGIN, (seed, D, margin)
        worst_margin, worst_mean, robustifies = min(worst_margin, margin), max(worst_mean, big), robustifies + len(m.margins)
    print(f'LINFUZZ host: {len(CASES)} schedules, {robustifies} robustifies, smallest margin {worst_margin:.3e}, largest |mean| {worst_mean:.3g}')
    assert robustifies >= len(CASES)
    assert threshold_margin(m) >= 0.0


def test_default_seeds_meet_every_shape():
    total = dict.fromkeys(SHAPES + REFUSALS, 0)
    for seed, D in CASES:
        t = tally(_schedule(seed, D), _run(seed, D)[0])
        assert set(t) == set(total)
        for k, v in t.items():
            total[k] += v
    print('LINFUZZ shapes over the default seeds:', total)
    assert all(v >= 1 for v in total.values()), {k: v for k, v in total.items() if not v}
    assert total['starts_empty'] == len(DIMS)
