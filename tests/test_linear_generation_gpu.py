"""What a rebuild of a live linear handle could get wrong by forgetting one array in one list (gbp_amd/csrc/gbp_lin_generation.hpp:
lin_gen_columns and who walks it): a leak per rebuild, a stale pointer after the commit, an array left at the old stride.  One fixed
schedule per kind of handle (tests/lin_generation_cases.py) -- plain with factor_const, robust with mixed losses, losses set and cleared
(the stale arrays), plain with F over 256 and back, SE(2) nonlinear -- and after every step: the number of device allocations the handle
owns, and every observable against the numpy model of the kind at the existing suites' tolerances (TOL of lin_shrink_cases.py and
lin_nonlin_cases.py; the SE(2) schedule stays MARGIN clear of the relinearisation threshold, tests/test_linear_generation_cpu.py)."""
import numpy as np
import pytest

from gbp_amd._capi import GbpError
from lin_extend_cases import generic_fc
from lin_generation_cases import KINDS, Player, engine_of, schedule
from test_linear_nonlinear_gpu import assert_matches_twin
from test_linear_shrink_gpu import assert_close

pytestmark = pytest.mark.gpu

EINVAL = -1
# gbp_lin_get_alloc_count after create and after every step of the schedule, recorded from the library of the parent commit (5f3b56e),
# which spelled every array out by hand in each list
ALLOCS = {
    'plain': [15] * 8,
    'robust': [20] * 8,
    'cleared': [20, 20, 20, 15, 15, 15, 15, 20, 20],         # cleared, the next rebuild drops the five stale arrays; new losses bring five back
    'plain_f256': [15] * 8,                                  # the larger d_red replaces the smaller one
    'se2': [21] * 8,
}
CYCLES = 20


def compare(p, what):
    if p.kind == 'se2':
        assert p.e.sizes() == (p.m.N, p.m.F) == (p.e.N, p.e.F), what
        assert_matches_twin(p.e, p.m, what)
    else:
        assert_close(p.e, p.m, what)


def refused(p, call, what):
    """A call the library refuses leaves sizes, allocations and messages as they were (the messages bit for bit)."""
    e = p.e
    sizes, allocs, msgs = e.sizes(), e.alloc_count(), e.messages()
    with pytest.raises(GbpError) as err:
        call()
    assert err.value.code == EINVAL, what
    assert e.sizes() == sizes == (e.N, e.F) and e.alloc_count() == allocs, what
    assert all(a.tobytes() == b.tobytes() for a, b in zip(msgs, e.messages())), f"{what}: messages moved"


@pytest.mark.parametrize('kind', KINDS)
def test_schedule_allocations_observables_and_refusals(kind):
    start, steps = schedule(kind)
    model = start()
    p = Player(kind, engine_of(model, kind), model)
    e = p.e
    counts = [e.alloc_count()]
    compare(p, 'created')
    for i, step in enumerate(steps):
        p.play(step)
        counts.append(e.alloc_count())
        compare(p, f'step {i} ({step[0]})')
        if step[0] in ('extend', 'shrink'):
            N, D = e.N, e.D
            if kind == 'se2':
                refused(p, lambda: e.extend_se2([0], [N], np.zeros((1, 3)), np.ones((1, 3))), f'step {i}: extend, id out of range')
            else:
                fe, fl, fc = generic_fc(np.random.RandomState(1), D, 1)
                refused(p, lambda: e.extend([0], [N], fe, fl, factor_const=fc), f'step {i}: extend, id out of range')
            refused(p, lambda: e.shrink([0, 0]), f'step {i}: shrink, id listed twice')
            compare(p, f'step {i} after the refusals')
    print(f"{kind}: alloc counts {counts}")
    assert counts == ALLOCS[kind]
    sizes, held = e.sizes(), e.alloc_count()                  # a handle holds ONE generation, however often it is rebuilt
    for _ in range(CYCLES):
        p.cycle()
    assert e.sizes() == sizes and e.alloc_count() == held
    e.close()
