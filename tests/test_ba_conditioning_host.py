"""The host-compiled factor core (HostBA: gbp_math.hpp + factor_core of gbp_kernels.hpp, tests/test_factor_math_host.py) against the
exact sweep (oracle/exact_ba.py) at the numerical edges of tests/ba_regimes.py, one step at a time: burn-in through replay_ba's schedule,
read the complete state, one more sweep on the host core, the same sweep exact (mpmath, 40 digits) and in the reference's own float64
maths (the yardstick).  The criterion is ba_regimes.check: the core may be C_RATIO times less accurate than the yardstick, and never more than CAP
away from the exact sweep.
What fails here is a loss of the covariance FORMULATION; the GPU file adds only what is device-specific (rcp, contraction, sum order)."""
import numpy as np
import pytest

import ba_regimes as BR
from conftest import rel_err_rows
from test_factor_math_host import HostBA, hm, unpack  # noqa: F401  (hm: the module fixture that builds the host library)

REGIMES = {r.name: r for r in BR.regimes()}


def host_state(h):
    """exact_ba's state dict from a HostBA (its arrays are the state)."""
    it = h.iters()
    return dict(K=h.K.copy(), cam_prior_eta=h.cpri[:, :6].copy(), cam_prior_lam=unpack(h.cpri[:, 6:], 6),
                lmk_prior_eta=h.lpri[:, :3].copy(), lmk_prior_lam=unpack(h.lpri[:, 3:], 3),
                msg_cam_eta=h.eC.copy(), msg_cam_lam=unpack(h.MC, 6), msg_lmk_eta=h.eL.copy(), msg_lmk_lam=unpack(h.ML, 3),
                linpoint=h.x0.copy(), z=h.z.copy(), cam=h.cam.copy(), lmk=h.lmk.copy(), adaptive_var=h.avar.copy(),
                iters_since_relin=it.astype(np.int64), eta_damping=np.where(h.st & 1, h.par['eta_damping'], 0.0))


def host_next(h, relin):
    ce, cl, le, ll = h.beliefs()
    return dict(cam_eta=ce, cam_lam=cl, lmk_eta=le, lmk_lam=ll, cam_mu=h.cam_mu, lmk_mu=h.lmk_mu,
                msg_cam_eta=h.eC, msg_cam_lam=unpack(h.MC, 6), msg_lmk_eta=h.eL, msg_lmk_lam=unpack(h.ML, 3),
                relin=relin, robust_flag=((h.st >> 1) & 1).astype(bool))


def host_one_step(lib, regime, kind, burn=BR.BURN):
    h = HostBA(lib, regime.problem, **regime.kw, **BR.kind_kw(kind))
    BR.prepare(h, regime, kind, burn)
    st = host_state(h)
    h.synchronous_iteration(robustify=True, local_relin=True)
    relin = h.iters() == 0
    return BR.one_step(st, host_next(h, relin), regime, kind, rel_err_rows)


@pytest.mark.parametrize('kind', BR.KINDS)
@pytest.mark.parametrize('name', list(REGIMES))
def test_host_core_one_step_against_exact(hm, name, kind):
    r = REGIMES[name]
    errs, maha = host_one_step(hm, r, kind)
    bad = BR.check(errs, maha)
    assert not bad, (name, kind, bad)


def test_host_core_one_step_after_one_sweep(hm):
    """The baseline from a state one sweep old (undamped messages fresh from zero)."""
    errs, maha = host_one_step(hm, REGIMES['baseline'], 'damped', burn=1)
    assert not BR.check(errs, maha)
