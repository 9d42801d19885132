"""oracle/exact_ba.py pinned to the reference: one sweep from fixture G4's `it1` state, a replay of G4 through its relinearising sweep
16 from G3's priors, and the exact run's independence of its working precision.  CPU only.

Fixture G13 is not replayed here: its two sequences are the reference's stage-wise calls (compute_all_factors with the damping on;
relinearise_factors followed by synchronous_iteration(local_relin=False)), and exact_ba restates synchronous_iteration(robustify=True,
local_relin=True) alone -- the one sweep the one-step comparisons run.  G13 stays pinned by tests/test_oracle_golden.py (C oracle) and
tests/test_stagewise_gpu.py (engine)."""
import os

import numpy as np
import pytest

import ba_regimes as BR
from conftest import DATA, golden, rel_err_rows
from oracle import exact_ba

BELIEFS = ('cam_eta', 'cam_lam', 'lmk_eta', 'lmk_lam')


def _vsmall():
    from gbp_amd.balio import read_bal
    p = read_bal(os.path.join(DATA, 'fr1desk_vsmall.txt'), native=False)
    order = np.argsort(p.cam_idx, kind='stable')                      # reference factor order (gbp_ba.py:128-130)
    g3 = golden('G3_priors_vsmall')
    return p, dict(K=np.asarray(p.K, dtype=np.float64), cam_prior_eta=g3['cam_prior_eta'], cam_prior_lam=g3['cam_prior_lam'],
                   lmk_prior_eta=g3['lmk_prior_eta'], lmk_prior_lam=g3['lmk_prior_lam'], z=p.meas[order],
                   cam=p.cam_idx[order].astype(np.int64), lmk=p.lmk_idx[order].astype(np.int64), adaptive_var=np.full(p.n_factors, 4.0))


def _g4_state(tag):
    p, st = _vsmall()
    g4 = golden('G4_trace_vsmall')
    for k in ('msg_cam_eta', 'msg_cam_lam', 'msg_lmk_eta', 'msg_lmk_lam', 'linpoint', 'iters_since_relin', 'eta_damping'):
        st[k] = g4[f'{tag}_{k}']
    return st, g4


def test_beliefs_of_a_stored_state_are_the_references():
    st, g4 = _g4_state('it1')
    got = exact_ba.beliefs(exact_ba._F64(), st)
    for k, a in zip(BELIEFS + ('cam_mu', 'lmk_mu'), got):
        assert rel_err_rows(a, g4['it1_' + k]) == 0.0, k


def test_one_step_from_g4():
    """G4 it1 -> it2 (fr1desk_vsmall, 1801 factors).  The reference's own rounding is ~3e-11 away from the exact sweep here (measured:
    exact vs it2 2.8e-11, yardstick vs it2 4.5e-11 -- cond(Lambda) amplifies the ulp-level differences of any other order of
    operations), so the yardstick is held at 1e-10 and the exact run at 1e-9."""
    st, g4 = _g4_state('it1')
    yd = exact_ba.sweep(st, sigma2=4.0)
    ex = exact_ba.sweep(st, sigma2=4.0, dps=40, relin=yd['relin'])
    assert not yd['relin'].any() and np.array_equal(ex['relin'], yd['relin'])
    for k in BELIEFS:
        assert rel_err_rows(yd[k], g4['it2_' + k]) < 1e-10, k
        assert rel_err_rows(ex[k], g4['it2_' + k]) < 1e-9, k
    for k in ('cam_mu', 'lmk_mu'):                     # means = inv(Lambda) eta: cond(Lambda) more sensitive (measured 3.4e-9)
        assert rel_err_rows(ex[k], g4['it2_' + k]) < 1e-7, k


def test_yardstick_replays_g4_through_a_relinearising_sweep():
    """From G3's priors and zero messages through replay_ba's schedule (iters_since_relin reset at sweeps 4 and 9) to sweep 16, which
    relinearises: the yardstick stays with the reference's beliefs and relinearisation counts.  Measured gap: 1.0e-9 after sweep 1
    (the first cavities are the weak priors alone), 2.3e-8 after sweep 16 -- the C oracle's is 1.4e-9 .. 2.1e-8 on the same trace
    (test_oracle_golden.py::test_g4_trace_vsmall): two float64 orders of operations part at cond(Lambda) x eps."""
    p, st = _vsmall()
    g4 = golden('G4_trace_vsmall')
    F = p.n_factors
    st.update(msg_cam_eta=np.zeros((F, 6)), msg_cam_lam=np.zeros((F, 6, 6)), msg_lmk_eta=np.zeros((F, 3)), msg_lmk_lam=np.zeros((F, 3, 3)),
              linpoint=np.concatenate([p.cam_means[st['cam']], p.lmk_means[st['lmk']]], axis=1), iters_since_relin=np.ones(F, np.int64),
              eta_damping=np.zeros(F))
    for i in range(16):
        if i in (3, 8):
            st['iters_since_relin'] = np.ones(F, np.int64)
        assert int((st['iters_since_relin'] == 0).sum()) == g4['n_relin'][i], i
        st = exact_ba.sweep(st, sigma2=4.0)
        for k in BELIEFS:
            if f'it{i + 1}_{k}' in g4:
                assert rel_err_rows(st[k], g4[f'it{i + 1}_{k}']) < 1e-7, (i + 1, k)
    assert st['relin'].sum() > 0
    assert np.array_equal(st['iters_since_relin'], g4['it16_iters_since_relin'])
    assert np.array_equal(st['eta_damping'], g4['it16_eta_damping'])


@pytest.mark.parametrize('name,kind', [('baseline', 'relin'), ('huber_outliers', 'damped'), ('weak_prior_1e6', 'damped')])
def test_exact_run_does_not_depend_on_its_precision(name, kind):
    """The same sweep at 40 and 60 digits agrees to 1e-30 (relative, per array): 40 digits are exact for every comparison here."""
    import mpmath
    r = {x.name: x for x in BR.regimes()}[name]
    st = _regime_state(r, kind)
    kw = dict(sigma2=r.kw.get('gauss_noise_std', 2.0) ** 2, loss=r.kw.get('loss'), nstds=r.kw.get('Nstds', 3.0), **BR.kind_kw(kind))
    a = exact_ba.sweep(st, dps=40, **kw)['_exact']
    b = exact_ba.sweep(st, dps=60, **kw)['_exact']
    ctx = mpmath.MPContext()
    ctx.dps = 60
    for k in a:
        x, y = a[k].reshape(-1), b[k].reshape(-1)
        num = max(abs(ctx.mpf(u) - ctx.mpf(v)) for u, v in zip(x, y))
        den = max(abs(ctx.mpf(v)) for v in y)
        assert num <= ctx.mpf('1e-30') * den, (k, float(num / den))


def _regime_state(r, kind, burn=3):
    """A state of a regime after `burn` yardstick sweeps (priors as generate_priors_var makes them)."""
    p = r.problem
    order = np.argsort(p.cam_idx, kind='stable')
    cam, lmk = p.cam_idx[order].astype(np.int64), p.lmk_idx[order].astype(np.int64)
    F, s2 = p.n_factors, r.kw.get('gauss_noise_std', 2.0) ** 2
    x0 = np.concatenate([p.cam_means[cam], p.lmk_means[lmk]], axis=1)
    _, J = exact_ba.meas_jac(exact_ba._F64(), x0, np.asarray(p.K, dtype=np.float64))
    fmax = np.einsum('fri,frj->fij', J, J).reshape(F, -1).max(axis=1) / s2
    cmax, lmax = np.zeros(p.n_cams), np.zeros(p.n_lmks)
    np.maximum.at(cmax, cam, fmax)
    np.maximum.at(lmax, lmk, fmax)
    cl = np.eye(6)[None] * (cmax / r.wf ** 2)[:, None, None]
    ll = np.eye(3)[None] * (lmax / r.wf ** 2)[:, None, None]
    st = dict(K=np.asarray(p.K, dtype=np.float64), cam_prior_eta=np.einsum('cij,cj->ci', cl, p.cam_means), cam_prior_lam=cl,
              lmk_prior_eta=np.einsum('lij,lj->li', ll, p.lmk_means), lmk_prior_lam=ll, z=p.meas[order], cam=cam, lmk=lmk,
              adaptive_var=np.full(F, s2), msg_cam_eta=np.zeros((F, 6)), msg_cam_lam=np.zeros((F, 6, 6)), msg_lmk_eta=np.zeros((F, 3)),
              msg_lmk_lam=np.zeros((F, 3, 3)), linpoint=x0, iters_since_relin=np.ones(F, np.int64), eta_damping=np.zeros(F))
    kw = dict(sigma2=s2, loss=r.kw.get('loss'), nstds=r.kw.get('Nstds', 3.0), **BR.kind_kw(kind))
    for _ in range(burn):
        st = exact_ba.sweep(st, **kw)
    if kind != 'damped':
        st['iters_since_relin'] = np.full(F, 8, np.int64)
    return st
