"""Host side of gbp_lin_extend_nonlinear / gbp_lin_shrink_nonlinear (include/gbp_lin.h): the numpy twin with extend and shrink added
(tests/lin_nonlin_live_cases.py) reproduces the reference's own grown run (fixture G26, tests/golden/make_g26.py), and every seeded
schedule the GPU tests play -- the shapes, the shrinks, the window, the fuzz seeds -- stays clear of the relinearisation threshold."""
import numpy as np
import pytest

from conftest import golden
from lin_map_cases import rel
from lin_nonlin_cases import g25_schedule
from lin_nonlin_live_cases import MARGIN, all_schedules, g26_graph, live_twin, schedule_margin, tail

G26_TOL = 1e-10


def g26_schedule(g):
    beta, damping, und, minlin, sweeps = g['cfg']
    return dict(beta=float(beta), num_undamped_iters=int(und), min_linear_iters=int(minlin), eta_damping=float(damping)), int(sweeps)


def test_g26_is_what_the_generator_says():
    g = golden('G26_se2_posegraph_grown')
    assert float(g['margin']) >= 1e-7
    assert g['appends'].shape == (22, 3) and g['appends'][-1].tolist() == [44, 30, 34] and int(g['n0']) == 8 and int(g['f0']) == 7
    assert g25_schedule(golden('G25_se2_posegraph'), 'main')[0] == g26_schedule(g)[0]


def test_twin_reproduces_the_grown_reference_run():
    """Masks, iters and damping exactly, sweep by sweep; the energy of every sweep and everything stored at the end within 1e-10."""
    g = golden('G26_se2_posegraph_grown')
    sched, sweeps = g26_schedule(g)
    full, start = g26_graph(g)
    t = live_twin(start, sched)
    appends = {int(s): (int(n), int(f)) for s, n, f in g['appends']}
    for s in range(sweeps):
        if s in appends:
            t.extend(**tail(full, t.N, t.F, *appends[s])[1])
        mask = t.synchronous_iteration()
        F = int(g['sweep_f'][s])
        assert t.F == F
        assert np.array_equal(mask, g['mask'][s, :F].astype(bool)), f"sweep {s}: mask"
        assert np.array_equal(t.iters, g['iters'][s, :F]) and np.array_equal(t.fdamp, g['damp'][s, :F]), f"sweep {s}: iters / damping"
        assert abs(t.energy() - g['energy'][s]) <= G26_TOL * g['energy'][s], f"sweep {s}: energy"
    for name, a, b in (('means', t.get_means(), g['means']), ('feta', t.feta, g['feta']), ('flam', t.flam, g['flam']), ('linpoint', t.linpoint, g['linpoint']),
                       ('msg_eta_a', t.me[0], g['msg_eta_a']), ('msg_lam_a', t.ml[0], g['msg_lam_a']), ('msg_eta_b', t.me[1], g['msg_eta_b']),
                       ('msg_lam_b', t.ml[1], g['msg_lam_b']), ('bel_eta', t.be, g['bel_eta']), ('bel_lam', t.bl, g['bel_lam'])):
        assert rel(a, b) < G26_TOL, f"{name}: {rel(a, b):.3e}"
    eta, lam = t.joint()
    sigma = np.linalg.inv(lam)
    assert rel(sigma @ eta, g['map_mu']) < G26_TOL
    assert rel(np.array([sigma[3 * i:3 * i + 3, 3 * i:3 * i + 3] for i in range(t.N)]), g['map_sigma_diag']) < G26_TOL


@pytest.mark.parametrize('case', all_schedules(), ids=lambda c: c[0])
def test_schedules_stay_clear_of_the_threshold(case):
    """Before every relinearising sweep (and every relinearise()) of every schedule the GPU tests play: each factor allowed to
    relinearise whose distance is not exactly 0 is >= 1e-9 from `dist > beta`.  A condition on the seeds, not a measurement."""
    name, g, steps, sched = case
    m = schedule_margin(g, steps, sched)
    assert m >= MARGIN, f"{name}: a factor comes within {m:.2e} of beta"


def test_extend_keeps_the_old_state_and_shrink_gathers_it():
    """The twin's own contract: extend leaves every old factor's arrays as they were; shrink keeps the survivors' bit for bit and folds the
    stored message."""
    from lin_nonlin_live_cases import SHRINK_CASES, kept_state_case, play_on_twin
    g, steps = kept_state_case()
    t = live_twin(g)
    play_on_twin(t, steps[0])
    before = [a.copy() for a in (t.feta, t.flam, t.linpoint, t.iters, t.fdamp, t.me[0], t.ml[0], t.me[1], t.ml[1], t.be, t.bl)]
    play_on_twin(t, steps[1])
    F0, N0 = before[0].shape[0], before[-1].shape[0]
    after = (t.feta, t.flam, t.linpoint, t.iters, t.fdamp, t.me[0], t.ml[0], t.me[1], t.ml[1])
    assert all(np.array_equal(a[:F0], b) for a, b in zip(after, before[:9]))
    assert t.F == F0 + 4 and np.array_equal(t.iters[F0:], np.ones(4)) and not t.fdamp[F0:].any() and not t.me[0][F0:].any()
    assert rel(t.be[:N0], before[9]) < 1e-15 and np.array_equal(t.linpoint[F0:], t.adj_means()[F0:])
    g, steps = SHRINK_CASES['retire_fold']
    t = live_twin(g)
    play_on_twin(t, steps[0])
    pe1, m = t.pe[1].copy(), t.me[1][0].copy()
    lp = t.linpoint.copy()
    vmap, fmap = play_on_twin(t, steps[1])
    assert vmap.tolist() == [-1] + list(range(11)) and fmap.tolist() == [-1] + list(range(10))
    assert np.array_equal(t.pe[0], pe1 + m) and np.array_equal(t.linpoint, lp[1:])
