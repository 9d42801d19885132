"""The random sliding-window schedules of tests/lin_window_cases.py without a GPU: the generator is deterministic, every call it draws is
legal for the handle the calls before it left (sizes followed through every extend and every shrink), and on every chosen seed the host
model alone stays healthy and at least lin_fuzz_cases.MARGIN clear of every loss threshold at every step -- so that
tests/test_linear_window_fuzz_gpu.py may compare after every call of every case, none skipped."""
import functools

import numpy as np
import pytest

from lin_fuzz_cases import MARGIN, healthy, is_legal
from lin_window_cases import DIMS, N_STEPS, SEEDS, WindowModel, window_schedule

CASES = [(seed, D) for seed in SEEDS for D in DIMS]


@functools.lru_cache(maxsize=None)
def _run(seed, D):
    s = window_schedule(seed, D)
    m = WindowModel(s)
    ok, illegal, sizes, shrunk = healthy(m), [], [], 0
    for k, ops in enumerate(s.steps):
        for op in ops:
            if op.kind == 'shrink':
                a = op.args
                ids_ok = (np.unique(a['retire']).size == len(a['retire']) and np.unique(a['drop']).size == len(a['drop'])
                          and all(0 <= v < m.N for v in a['retire']) and all(0 <= f < m.F for f in a['drop']))
                if not ids_ok:
                    illegal.append((k, 'shrink'))
                shrunk += bool(len(a['retire']) or len(a['drop']))
            elif is_legal(m, op) is not None:
                illegal.append((k, op.kind, is_legal(m, op)))
            if m.apply(op) is not None:
                illegal.append((k, op.kind, 'refused by the model'))
            ok = ok and healthy(m)
        sizes.append((m.N, m.F))
    return m, ok, min(m.margins, default=np.inf), illegal, sizes, shrunk


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
    a, b = window_schedule(seed, D), window_schedule(seed, D)
    assert _same(tuple(a), tuple(b))
    assert len(a.steps) == N_STEPS
    for ops in a.steps:
        assert 2 <= len(ops) - 2 <= 4 and ops[-2].kind == 'extend' and ops[-1].kind == 'shrink'
        assert all(op.kind not in ('extend', 'shrink') for op in ops[:-2])
    _, _, _, illegal, _, shrunk = _run(seed, D)
    assert not illegal, illegal
    assert shrunk >= 1


def test_every_chosen_seed_is_healthy_and_clear_of_the_thresholds():
    assert len(SEEDS) == 8
    robustifies, folds = 0, {True: 0, False: 0}
    for seed, D in CASES:
        m, ok, margin, _, sizes, _ = _run(seed, D)
        print(f'LINWINDOW host seed={seed} D={D}: sizes {sizes} healthy={ok} robustifies={len(m.margins)} margin={margin:.3e}')
        assert ok, (seed, D)
        assert margin >= MARGIN, (seed, D, margin)
        robustifies += len(m.margins)
        for ops in window_schedule(seed, D).steps:
            folds[ops[-1].args['fold']] += 1
    assert robustifies >= len(CASES) and min(folds.values()) >= 1
