"""Random window schedules on a live BA handle (tests/window_fuzz_cases.py): five irregular steps per seed -- a keyframe batch, a cull
list, a camera list, a landmark list, taken as ONE gbp_ba_window_step or as the four calls -- on two engines (fused and general sweep)
beside the reference's object graph (NumpyBA through tests/window_host.py).  Per step:
  1. the six maps of both engines are the host's, exactly; sizes agree; check_layout() == 0; rebuild_count counts the rebuilds;
  2. while the host graph is healthy: beliefs and priors within 1e-7 of the host's (tests/test_window_step_gpu.py's bound for this
     comparison), relinearisation ages, damping and robust flags equal;
  3. a twin of the fused engine, started from its state blob, takes the step the OTHER way (calls for a step, a step for calls): factors,
     messages, relinearisation state and landmark priors bitwise, priors and beliefs 1e-12, beliefs 1e-9 after 3 more sweeps;
  4. on every second step a handle created from the resulting problem has the same plan, accepts the state blob and stays bitwise equal
     through 3 sweeps: the layout after rebuild n is the one gbp_ba_create makes;
  5. once per seed a step with an argument error the header documents is refused with GBP_EINVAL and leaves the blob untouched.
Seeds: window_fuzz_cases.SEEDS, extended to GBP_WINDOW_FUZZ_SEEDS seeds for a soak."""
import os

import numpy as np
import pytest

from conftest import rel_err_rows
from window_fuzz_cases import N_STEPS, SEEDS, SHAPES, Graph, healthy, make_host, random_schedule, refused_variant, tally
from window_host import EngineOps, four_calls, result_problem, window_step_numpy_ba

pytestmark = pytest.mark.gpu

W = 50.0
N_SEEDS = int(os.environ.get('GBP_WINDOW_FUZZ_SEEDS', len(SEEDS)))
ALL_SEEDS = tuple(SEEDS) + tuple(range(max(SEEDS) + 1, max(SEEDS) + 1 + max(0, N_SEEDS - len(SEEDS))))
COMPARED = {}       # seed -> steps compared against the host graph
MET = {}            # seed -> tally of the shapes, from the engine's own arrays and maps


@pytest.fixture(scope='module')
def lib():
    from gbp_amd import build
    build.build()
    from gbp_amd import _capi
    return _capi


def _engine(problem, **kw):
    from gbp_amd.engine import BAEngine
    e = BAEngine.from_problem(problem, **kw)
    e.generate_priors_var(W)
    e.update_all_beliefs()
    return e


def _bitwise(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _tuple(b):
    return None if b is None else (b['cam_means'], b['lmk_means'], b['meas'], b['cam_idx'], b['lmk_idx'])


def _batch_or_none(bt):
    return bt if bt is not None and (len(bt['cam_means']) or len(bt['lmk_means']) or len(bt['meas'])) else None


class _CountingOps(EngineOps):
    """EngineOps that counts the calls that change something (a call with an empty list does not rebuild)."""
    rebuilds = 0

    def extend(self, b):
        self.rebuilds += 1
        return super().extend(b)

    def cull(self, ids):
        self.rebuilds += len(ids) > 0
        return super().cull(ids)

    def retire(self, ids):
        self.rebuilds += len(ids) > 0
        return super().retire(ids)

    def retire_landmarks(self, ids, fold):
        self.rebuilds += len(ids) > 0
        return super().retire_landmarks(ids, fold)


def _take(e, step, how):
    """The step on engine e as one window step or as the four calls.  Returns (maps, rebuilds it must have cost)."""
    bt = _batch_or_none(step.batch)
    if how == 'step':
        m = e.window_step(cull=step.cull, retire=step.retire, retire_landmarks=step.lmks, fold_landmarks=step.fold, batch=_tuple(bt),
                          prior_weaker_factor=W)
        return m, int(bt is not None or len(step.cull) + len(step.retire) + len(step.lmks) > 0)
    ops = _CountingOps(e, prior_weaker_factor=W)
    return four_calls(ops, bt, step.cull, step.retire, step.lmks, step.fold), ops.rebuilds


def _same_maps(x, y, where):
    for name, a, b in zip(x._fields, x, y):
        np.testing.assert_array_equal(a, b, err_msg=f'{where}: {name}')


def _gap_to_host(e, nb, where):
    """test_window_step_gpu.py::_gap_to_host and ::_same_relin, and the robust flags; returns the worst gap"""
    ph = (np.array([v.prior.eta for v in nb.cams]), np.array([v.prior.lam for v in nb.cams]),
          np.array([v.prior.eta for v in nb.lmks]), np.array([v.prior.lam for v in nb.lmks]))
    worst = 0.0
    for what, mine, host in (('beliefs', e.beliefs(), nb.beliefs()), ('priors', e.priors(), ph)):
        for k, (a, h) in enumerate(zip(mine, host)):
            gap = rel_err_rows(a, h)
            print(f'WINDOWFUZZ {where}: {what} {k} gap to host {gap:.3e}')
            worst = max(worst, gap)
            assert gap < 1e-7, (where, what, k, gap)
    rs, fs = e.relin_state(), nb.graph.factors
    np.testing.assert_array_equal(rs['iters_since_relin'], [f.iters_since_relin for f in fs], err_msg=where)
    np.testing.assert_array_equal(rs['eta_damping'], [f.eta_damping for f in fs], err_msg=where)
    np.testing.assert_array_equal(rs['robust_flag'].astype(bool), [bool(f.robust_flag) for f in fs], err_msg=where)
    return worst


def _step_against_calls(a, b, where):
    """test_window_step_gpu.py::_equal_to_four_calls between two engines that took one step the two ways from one state (3 sweeps
    afterwards, on both); returns the worst gap of priors and beliefs right after the step"""
    assert (a.C, a.L, a.F) == (b.C, b.L, b.F) and a.plan_info() == b.plan_info() and b.check_layout() == 0, where
    fa, fb = a.factors(dense=False), b.factors(dense=False)
    for key in fa:
        if fa[key] is not None:
            assert _bitwise(fa[key], fb[key]), (where, key)
    for k, (x, y) in enumerate(zip(a.messages(), b.messages())):
        assert _bitwise(x, y), (where, 'messages', k)
    ra, rb = a.relin_state(), b.relin_state()
    for key in ra:
        assert _bitwise(ra[key], rb[key]), (where, key)
    np.testing.assert_array_equal(a.landmark_order(), b.landmark_order(), err_msg=where)
    pa, pb = a.priors(), b.priors()
    assert _bitwise(pa[2], pb[2]) and _bitwise(pa[3], pb[3]), where
    worst = 0.0
    for k, (x, y) in enumerate(zip(pa + a.beliefs(), pb + b.beliefs())):
        gap = rel_err_rows(x, y)
        worst = max(worst, gap)
        assert gap < 1e-12, (where, k, gap)
    a.iterate(3)
    b.iterate(3)
    for k, (x, y) in enumerate(zip(a.beliefs(), b.beliefs())):
        assert rel_err_rows(x, y) < 1e-9, (where, k)
    assert np.array_equal(a.iters_since_relin(), b.iters_since_relin()), where
    return worst


def _refused(lib, e, g, step, kind, where):
    name, (bt, cull, retire, lmks) = refused_variant(g, step, kind)
    blob, count, sizes = e.save_state(), e.rebuild_count(), (e.C, e.L, e.F)
    with pytest.raises(lib.GbpError) as ei:
        e.window_step(cull=cull, retire=retire, retire_landmarks=lmks, fold_landmarks=step.fold, batch=_tuple(_batch_or_none(bt)),
                      prior_weaker_factor=W)
    assert ei.value.code == -1, (where, name, str(ei.value))
    assert (e.C, e.L, e.F) == sizes and e.rebuild_count() == count and _bitwise(e.save_state(), blob), (where, name)


@pytest.mark.parametrize('seed', ALL_SEEDS)
def test_random_window_schedule(lib, monkeypatch, seed):
    s = random_schedule(seed)
    for key, value in s.settings['env'].items():
        monkeypatch.setenv(key, value)
    kw = dict(loss=s.settings['loss'], reorder_landmarks=s.settings['reorder_landmarks'])
    a, b, twin = _engine(s.base, fused=True, **kw), _engine(s.base, fused=False, **kw), _engine(s.base, fused=True, **kw)
    nb = make_host(s.base, s.settings['loss'])
    comparing, compared, worst_host, worst_twin, met = True, 0, 0.0, 0.0, []
    for k, step in enumerate(s.steps):
        where = f'seed {seed} step {k} ({step.how})'
        for g in (nb, a, b):
            g.iterate(step.sweeps)
        fac, means = a.factors(dense=False), a.means()
        before = Graph(a.C, a.L, fac['cam'], fac['lmk'])
        assert (before.C, before.L) == (s.graphs[k].C, s.graphs[k].L), where
        assert np.array_equal(before.cam, s.graphs[k].cam) and np.array_equal(before.lmk, s.graphs[k].lmk), where
        if k == s.refuse[0]:                                                                           # 5.
            _refused(lib, a, before, step, s.refuse[1], where)
        twin.load_state(a.save_state())
        counts = [a.rebuild_count(), b.rebuild_count()]
        mh = window_step_numpy_ba(nb, step.batch, step.cull, step.retire, step.lmks, step.fold, prior_weaker_factor=W)
        for j, e in enumerate((a, b)):                                                                 # 1.
            me, cost = _take(e, step, step.how)
            _same_maps(mh, me, f'{where} engine {"AB"[j]}')
            assert (e.C, e.L, e.F) == (nb.C, nb.L, len(nb.graph.factors)) and e.check_layout() == 0, where
            assert e.rebuild_count() == counts[j] + cost and (step.how == 'calls' or cost == 1), (where, cost)
        met.append((before, step, me))
        if comparing and healthy(nb):                                                                  # 2.
            worst_host = max(worst_host, _gap_to_host(a, nb, where + ' engine A'), _gap_to_host(b, nb, where + ' engine B'))
            compared += 1
        else:
            comparing = False
        mt, _ = _take(twin, step, 'calls' if step.how == 'step' else 'step')                           # 3.
        _same_maps(mh, mt, where + ' twin')
        blob = a.save_state()
        pair = (twin, a) if step.how == 'step' else (a, twin)                                          # (four calls, one step)
        worst_twin = max(worst_twin, _step_against_calls(*pair, where))
        a.load_state(blob)                                                                             # the 3 sweeps are not A's
        assert _bitwise(a.save_state(), blob), where
        if k % 2:                                                                                      # 4.
            f = _engine(result_problem(s.base.K, means[0], means[1], fac, step.batch, me), fused=True, **kw)
            assert a.plan_info() == f.plan_info() and a.info() == f.info(), where
            f.load_state(blob)
            twin.load_state(blob)
            twin.iterate(3)
            f.iterate(3)
            assert _bitwise(twin.save_state(), f.save_state()), where
            f.close()
    for g in (nb, a, b):
        g.iterate(4)
    if comparing and healthy(nb):
        where = f'seed {seed}, 4 sweeps after the last step'
        worst_host = max(worst_host, _gap_to_host(a, nb, where + ' engine A'), _gap_to_host(b, nb, where + ' engine B'))
    for e in (a, b, twin):
        e.close()
    print(f'WINDOWFUZZ seed={seed} steps compared={compared} worst host gap={worst_host:.3e} worst twin gap={worst_twin:.3e}')
    assert compared >= 1, seed
    COMPARED[seed], MET[seed] = compared, tally(met)


def test_window_fuzz_was_not_vacuous(request):
    """(runs after the parametrised test above: same module, file order)  All seeds ran, at least 75 % of the default seeds' steps were
    compared against the host graph -- the share tests/test_window_fuzz_cpu.py proves the host model alone allows -- and the device has
    met every shape."""
    if os.environ.get('PYTEST_XDIST_WORKER'):
        pytest.skip('the seeds are spread over xdist workers (soak runs): the tally lives in the other processes')
    if request.config.getoption('keyword'):
        pytest.skip('-k selected a subset: the tally is incomplete by construction')
    assert sorted(COMPARED) == sorted(ALL_SEEDS), f'seeds that did not finish: {sorted(set(ALL_SEEDS) - set(COMPARED))}'
    assert sum(COMPARED[x] for x in SEEDS) >= 0.75 * N_STEPS * len(SEEDS), COMPARED
    total = {k: sum(MET[x][k] for x in SEEDS) for k in SHAPES}
    print('WINDOWFUZZ shapes met on the device:', total)
    assert all(v >= 1 for v in total.values()) and total['fold_above_64'] >= 2, total
