"""The BA sweep kernels against the exact sweep (oracle/exact_ba.py) at the numerical edges of tests/ba_regimes.py, one step at a time.

Per regime, path (fused / general / the library's choice) and comparison kind (ba_regimes.KINDS): burn-in through replay_ba's schedule,
the complete state read through the views, one more device sweep, then the exact (mpmath, 40 digits) and yardstick (the reference's
float64 maths) sweeps from the state read.  Criterion (ba_regimes.check): err(device, exact) <= min(C_RATIO err(yardstick, exact), CAP) + FLOOR
for the beliefs and the dense messages; mean errors in standard deviations of the exact belief.  The dense-remainder kind runs on the
general sweep only (Params::xtra)."""
import pytest

import ba_regimes as BR
from conftest import rel_err_rows

pytestmark = pytest.mark.gpu

REGIMES = {r.name: r for r in BR.regimes()}
CASES = [(n, path, kind) for n in REGIMES for path in ('fused', 'general', 'auto') for kind in BR.KINDS
         if not (kind == 'xtra' and path != 'general')]


def engine_one_step(regime, path, kind, burn=BR.BURN):
    from gbp_amd.engine import BAEngine
    from oracle import exact_ba
    fused = {'fused': True, 'general': False, 'auto': None}[path]
    g = BAEngine.from_problem(regime.problem, fused=fused, **regime.kw, **BR.kind_kw(kind))
    try:
        info, plan = g.info(), g.plan_info()
        if path == 'fused':
            assert info['fused'] and plan['fused']
        elif path == 'general':
            assert not info['fused'] and not plan['fused']
        else:
            # The library's own choice (gbp_capi.hip): the staged sweep only below 0.75 factors per camera-table row.  These graphs have
            # 16-64 factors and at most 8 table rows (one workgroup, <= 8 cameras): the fused sweep, like the forced one.
            assert not plan['staged_by_sparseness'] and plan['fused'] and info['fused'], plan
            assert regime.problem.n_factors >= 0.75 * plan['table_rows'], plan
        BR.prepare(g, regime, kind, burn)
        st = exact_ba.state_from_engine(g, g.K)
        g.synchronous_iteration(robustify=True, local_relin=True)
        ce, cl, le, ll = g.beliefs()
        me, ml, ne, nl = g.messages()
        cm, lm = g.means()
        rs = g.relin_state()
        nxt = dict(cam_eta=ce, cam_lam=cl, lmk_eta=le, lmk_lam=ll, cam_mu=cm, lmk_mu=lm, msg_cam_eta=me, msg_cam_lam=ml, msg_lmk_eta=ne,
                   msg_lmk_lam=nl, relin=rs['iters_since_relin'] == 0, robust_flag=rs['robust_flag'].astype(bool))
        if kind != 'damped':
            assert nxt['relin'].all()
        return BR.one_step(st, nxt, regime, kind, rel_err_rows)
    finally:
        g.close()


@pytest.mark.parametrize('name,path,kind', CASES)
def test_sweep_one_step_against_exact(name, path, kind):
    errs, maha = engine_one_step(REGIMES[name], path, kind)
    print(f'{name:18s} {path:8s} {kind:7s} ratio {BR.ratio(errs):7.3f}  worst {BR.worst(errs):.2e}  mean {max(maha["cam"][0], maha["lmk"][0]):.2e} sigma '
          f'(yardstick {max(maha["cam"][1], maha["lmk"][1]):.2e})')
    bad = BR.check(errs, maha)
    assert not bad, (name, path, kind, bad)


def test_sweep_one_step_after_one_sweep():
    """The baseline from a state one sweep old, on every path."""
    for path in ('fused', 'general', 'auto'):
        errs, maha = engine_one_step(REGIMES['baseline'], path, 'damped', burn=1)
        assert not BR.check(errs, maha), path

