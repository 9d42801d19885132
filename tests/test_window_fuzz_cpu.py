"""The random window schedules of tests/window_fuzz_cases.py without a GPU: the generator is deterministic and legal, the reference's
object graph (NumpyBA through tests/window_host.py) follows every default seed with the sizes, maps and factor order the header
promises, the default seeds meet every shape the hand-built cases single out, and the host model alone stays healthy on at least 75 % of
the scheduled steps -- so that tests/test_window_fuzz_gpu.py, which compares an engine with the host graph only while it is healthy,
cannot quietly compare less."""
import functools

import numpy as np
import pytest

from window_fuzz_cases import (N_STEPS, REFUSALS, SEEDS, SHAPES, Graph, healthy, index_step, is_legal, make_host, random_schedule,
                               refused_variant, tally)
from window_host import window_step_numpy_ba

W = 50.0


def _same_batch(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ('cam_means', 'lmk_means', 'meas', 'cam_idx', 'lmk_idx'))


@functools.lru_cache(maxsize=None)
def _schedule(seed):
    return random_schedule(seed)


@functools.lru_cache(maxsize=None)
def _host_run(seed):
    """The host graph through the schedule: per step (Graph before, Step, host maps, Graph after, healthy after)."""
    from retire_host import graph_arrays
    s = _schedule(seed)
    nb = make_host(s.base, s.settings['loss'])
    out = []
    for step in s.steps:
        nb.iterate(step.sweeps)
        _, _, _, cam, lmk = graph_arrays(nb)
        before = Graph(nb.C, nb.L, cam, lmk)
        m = window_step_numpy_ba(nb, step.batch, step.cull, step.retire, step.lmks, step.fold, prior_weaker_factor=W)
        _, _, _, cam, lmk = graph_arrays(nb)
        out.append((before, step, m, Graph(nb.C, nb.L, cam, lmk), healthy(nb)))
    nb.iterate(4)
    return out, healthy(nb), nb.are()


@pytest.mark.parametrize('seed', SEEDS)
def test_generator_is_deterministic_and_legal(seed):
    a, b = _schedule(seed), random_schedule(seed)
    assert len(a.steps) == N_STEPS and a.refuse == b.refuse and a.settings == b.settings
    assert np.array_equal(a.base.cam_idx, b.base.cam_idx) and np.array_equal(a.base.meas, b.base.meas)
    assert 6 <= a.base.n_cams <= 12 and a.base.n_lmks <= 200 and a.graphs[0].cam.size == a.base.n_factors
    assert np.unique(a.base.cam_idx).size == a.base.n_cams and np.unique(a.base.lmk_idx).size == a.base.n_lmks
    for k, (x, y) in enumerate(zip(a.steps, b.steps)):
        assert (x.sweeps, x.fold, x.how, x.pushes) == (y.sweeps, y.fold, y.how, y.pushes) and _same_batch(x.batch, y.batch)
        assert np.array_equal(x.cull, y.cull) and np.array_equal(x.retire, y.retire) and np.array_equal(x.lmks, y.lmks)
        g = a.graphs[k]
        assert is_legal(g, x) is None, (k, is_legal(g, x))
        assert 1 <= x.sweeps <= 4 and len(x.retire) <= 2 and g.C - len(x.retire) >= 3 and x.how in ('step', 'calls')
        assert len(x.batch['cam_means']) <= 3 and a.graphs[k + 1].cam.size <= 1300 and a.graphs[k + 1].C <= 21
        # every kind of refusal is an argument error by the same rules
        for kind in range(len(REFUSALS)):
            name, (bt, cull, retire, lmks) = refused_variant(g, x, kind)
            bad = x._replace(batch=bt if bt is not None else dict(x.batch, cam_means=np.zeros((0, 6)), lmk_means=np.zeros((0, 3)),
                             meas=np.zeros((0, 2)), cam_idx=np.zeros(0, np.int32), lmk_idx=np.zeros(0, np.int32)), cull=cull, retire=retire, lmks=lmks)
            assert name in REFUSALS and is_legal(g, bad) is not None, (k, name)


@pytest.mark.parametrize('seed', SEEDS)
def test_host_model_follows_the_schedule(seed):
    s = _schedule(seed)
    run, _, _ = _host_run(seed)
    for k, (before, step, m, after, _) in enumerate(run):
        # the host graph is the graph the generator drew the step for, and its composed maps are the ones the rules give directly
        want = s.graphs[k]
        assert (before.C, before.L) == (want.C, want.L) and np.array_equal(before.cam, want.cam) and np.array_equal(before.lmk, want.lmk), k
        for name, x, y in zip(m._fields, m, s.maps[k]):
            np.testing.assert_array_equal(x, y, err_msg=f'step {k} {name}')
        # sizes are those the maps imply
        assert after.C == (m.cam_map >= 0).sum() + (m.new_cam_ids >= 0).sum(), k
        assert after.L == (m.lmk_map >= 0).sum() + (m.new_lmk_ids >= 0).sum(), k
        assert after.cam.size == (m.factor_map >= 0).sum() + (m.new_factor_ids >= 0).sum(), k
        # survivors keep their relative order
        for old in (m.cam_map, m.lmk_map, m.factor_map):
            alive = old[old >= 0]
            assert (np.diff(alive) > 0).all(), k
        # new and surviving factor ids together are a permutation
        ids = np.concatenate([m.factor_map, m.new_factor_ids])
        assert np.array_equal(np.sort(ids[ids >= 0]), np.arange(after.cam.size)), k
        # camera-major; inside a camera the old factors first (in their old order: monotone above), then the new ones in batch order
        assert (np.diff(after.cam) >= 0).all(), k
        is_new = np.zeros(after.cam.size, bool)
        is_new[m.new_factor_ids[m.new_factor_ids >= 0]] = True
        same_cam = after.cam[1:] == after.cam[:-1]
        assert not (same_cam & is_new[:-1] & ~is_new[1:]).any(), k
        nf = m.new_factor_ids
        full_c = np.concatenate([m.cam_map, m.new_cam_ids])
        bc = full_c[step.batch['cam_idx']]
        for c in np.unique(bc):
            assert (np.diff(nf[bc == c]) > 0).all(), (k, c)
        np.testing.assert_array_equal(after.cam[nf], bc)
        assert np.array_equal(after.cam, s.graphs[k + 1].cam) and np.array_equal(after.lmk, s.graphs[k + 1].lmk), k


def test_default_seeds_meet_every_shape():
    total = dict.fromkeys(SHAPES, 0)
    for seed in SEEDS:
        s = _schedule(seed)
        t = tally(zip(s.graphs, s.steps, s.maps))
        assert set(t) == set(SHAPES)
        for k, v in t.items():
            total[k] += v
    print('WINDOWFUZZ shapes over the default seeds:', total)
    assert all(total[k] >= 1 for k in SHAPES), total
    assert total['fold_above_64'] >= 2, total
    # the index model's tally is the host graph's
    seed = SEEDS[0]
    s = _schedule(seed)
    assert tally((b, st, m) for b, st, m, _, _ in _host_run(seed)[0]) == tally(zip(s.graphs, s.steps, s.maps))


def test_host_model_alone_meets_the_health_cap():
    """What the GPU test may compare: the steps up to the first unhealthy one of each seed."""
    compared = {}
    for seed in SEEDS:
        run, last, are = _host_run(seed)
        flags = [h for _, _, _, _, h in run]
        n = flags.index(False) if False in flags else len(flags)
        compared[seed] = n
        print(f'WINDOWFUZZ host seed={seed} healthy steps={n}/{N_STEPS} healthy after 4 more sweeps={last and n == N_STEPS} final ARE={are:.2f}')
        assert n >= 1, seed
    assert sum(compared.values()) >= 0.75 * N_STEPS * len(SEEDS), compared
