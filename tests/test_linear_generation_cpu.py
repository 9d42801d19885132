"""The schedules of tests/lin_generation_cases.py played on the numpy models alone: they reach the sizes the GPU test counts on (an extend
with dN = 0 and one with dF = 0, F over 256 and back), and the SE(2) one stays clear of the relinearisation threshold before every sweep,
as every schedule of tests/lin_nonlin_live_cases.py must.  A condition on the seeds, not a measurement."""
import numpy as np
import pytest

from lin_generation_cases import KINDS, schedule
from lin_nonlin_live_cases import MARGIN


class NoEngine:
    """Stands in for the engine of a Player: takes every call and does nothing."""
    N = F = D = 0

    def __getattr__(self, name):
        return lambda *a, **k: None


@pytest.mark.parametrize('kind', KINDS)
def test_schedule_on_the_model(kind):
    from lin_generation_cases import Player
    start, steps = schedule(kind)
    p = Player(kind, NoEngine(), start())
    sizes, margin = [(p.m.N, p.m.F)], np.inf
    for step in steps:
        if kind == 'se2' and step[0] == 'sweep':
            for _ in range(step[1]):
                margin = min(margin, p.m.margin())
                p.m.synchronous_iteration()
        else:
            p.play(step)
        if step[0] in ('extend', 'shrink'):
            sizes.append((p.m.N, p.m.F))
    assert margin >= MARGIN, f"a factor comes within {margin:.2e} of beta"
    (n0, f0), (n1, f1), (n2, f2), (n3, f3), (n4, f4) = sizes
    assert n1 >= n0 and f1 >= f0 and n2 < n1 and f2 < f1 and n3 >= n2 and f3 >= f2 and n4 < n3 and f4 < f3
    assert min(n4, f4) > 0
    if kind == 'plain_f256':
        assert f0 <= 256 < f1 and f2 < 256 and n1 == n0                    # the partials of the energy grow once; dN = 0
    if kind in ('robust', 'se2'):
        assert f3 == f2 and n3 > n2                                         # dF = 0
    if kind == 'plain':
        assert n3 == n2 and f3 > f2                                         # dN = 0
