"""The host routines that gbp_lin_create, gbp_lin_extend, gbp_lin_set_robust, gbp_lin_set_nonlinear and gbp_lin_extend_nonlinear share
(gbp_amd/csrc/gbp_lin_generation.hpp), compiled for the host through tests/hostmath/lin_pack_shim.hip and run on a CPU: packing factors
and priors for upload against numpy.triu_indices, measurements against a numpy transpose, and the rules for a list of losses and for a
list of measurements against the message of every refusal the header documents, for both callers' prefixes."""
import ctypes as ct
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostmath', 'lin_pack_shim.hip')
LIB = os.path.join(HERE, 'hostmath', 'liblin_pack_shim.so')
CSRC = os.path.join(REPO, 'gbp_amd', 'csrc')
NONE, HUBER, CONSTANT = 0, 1, 2
EINVAL = -1
PREFIXES = ('factor', 'new factor')                        # gbp_lin_set_robust, gbp_lin_extend


@pytest.fixture(scope='module')
def shim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ('gbp_lin_generation.hpp', 'gbp_lin_handle.hpp')]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        tmp = f'{LIB}.{os.getpid()}.tmp'
        hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
        subprocess.check_call([hipcc, '--offload-host-only', '-O1', '-std=c++17', '-shared', '-fPIC', '-o', tmp, SRC])
        os.replace(tmp, LIB)
    so = ct.CDLL(LIB)
    i, ip, dp = ct.c_int, ct.POINTER(ct.c_int32), ct.POINTER(ct.c_double)
    so.lin_pack_factors_host.argtypes, so.lin_pack_factors_host.restype = [i, i, dp, dp, dp, dp], None
    so.lin_pack_priors_host.argtypes, so.lin_pack_priors_host.restype = [i, i, dp, dp, dp], None
    so.lin_check_losses_host.argtypes, so.lin_check_losses_host.restype = [ip, dp, dp, i, ct.c_char_p, ct.POINTER(ct.c_int)], i
    so.lin_check_measurements_host.argtypes, so.lin_check_measurements_host.restype = [dp, dp, i, ct.c_char_p], i
    so.lin_pack_measurements_host.argtypes, so.lin_pack_measurements_host.restype = [i, dp, dp, dp, dp], None
    so.lin_pack_last_error.argtypes, so.lin_pack_last_error.restype = [], ct.c_char_p
    return so


def dptr(a):
    return a.ctypes.data_as(ct.POINTER(ct.c_double))


@pytest.mark.parametrize('count', [0, 1, 5])
@pytest.mark.parametrize('D', [1, 3, 6])
def test_factors_are_packed_as_soa_upper_triangles(shim, D, count):
    """out_eta [2D][count] and out_lam [D(2D+1)][count]: row k of out_lam is entry triu_indices(2D)[k] of every factor's matrix.  The
    matrices are NOT symmetric here, so an entry taken from below the diagonal shows; the outputs start as NaN, so does one not written."""
    rs = np.random.RandomState(10 * D + count)
    D2, P2 = 2 * D, D * (2 * D + 1)
    eta, lam = rs.randn(count, D2), rs.randn(count, D2, D2)
    out_eta, out_lam = np.full((D2, count), np.nan), np.full((P2, count), np.nan)
    shim.lin_pack_factors_host(D, count, dptr(eta), dptr(lam), dptr(out_eta), dptr(out_lam))
    iu = np.triu_indices(D2)
    assert np.array_equal(out_eta, eta.T)
    assert np.array_equal(out_lam, lam[:, iu[0], iu[1]].T)


@pytest.mark.parametrize('count', [0, 1, 5])
@pytest.mark.parametrize('D', [1, 3, 6])
def test_priors_are_packed_as_records(shim, D, count):
    """out [count][D + D(D+1)/2]: eta, then the upper triangle in triu_indices(D) order."""
    rs = np.random.RandomState(100 + 10 * D + count)
    P = D * (D + 1) // 2
    eta, lam = rs.randn(count, D), rs.randn(count, D, D)
    out = np.full((count, D + P), np.nan)
    shim.lin_pack_priors_host(D, count, dptr(eta), dptr(lam), dptr(out))
    iu = np.triu_indices(D)
    assert np.array_equal(out[:, :D], eta)
    assert np.array_equal(out[:, D:], lam[:, iu[0], iu[1]])


def check(so, prefix, loss, thr, nvar):
    """(return code, any, message) of lin_check_losses on the lists; thr / nvar None = NULL."""
    loss = np.ascontiguousarray(loss, dtype=np.int32)
    thr = None if thr is None else np.ascontiguousarray(thr, dtype=np.float64)
    nvar = None if nvar is None else np.ascontiguousarray(nvar, dtype=np.float64)
    any_ = ct.c_int(-1)
    rc = so.lin_check_losses_host(loss.ctypes.data_as(ct.POINTER(ct.c_int32)), None if thr is None else dptr(thr), None if nvar is None else dptr(nvar),
                                  len(loss), prefix.encode(), ct.byref(any_))
    return rc, any_.value, so.lin_pack_last_error().decode()


# (loss, threshold, noise_var, the message after "<prefix> "): the refused factor is number 2 of 4 in every case; the factors before
# it are valid, the one after it would be refused too, so the message also pins the order
REFUSALS = [
    ('unknown loss', [HUBER, NONE, 7, 9], [2.0, 1.0, 1.0, 1.0], [1.0] * 4, "2: unknown loss 7"),
    ('negative loss code', [HUBER, NONE, -1, 9], [2.0, 1.0, 1.0, 1.0], [1.0] * 4, "2: unknown loss -1"),
    ('zero threshold', [HUBER, NONE, HUBER, HUBER], [2.0, -1.0, 0.0, 0.0], None, "2: the threshold must be positive"),
    ('negative threshold', [HUBER, NONE, CONSTANT, HUBER], [2.0, -1.0, -2.0, 0.0], [1.0] * 4, "2: the threshold must be positive"),
    ('NaN threshold', [CONSTANT, NONE, HUBER, HUBER], [2.0, np.nan, np.nan, 0.0], [1.0] * 4, "2: the threshold must be positive"),
    ('infinite threshold', [HUBER, NONE, HUBER, HUBER], [2.0, 1.0, np.inf, 0.0], None, "2: the threshold must be positive"),
    ('constant without noise_var', [HUBER, NONE, CONSTANT, CONSTANT], [2.0, 1.0, 1.5, 1.0], None, "2 has the constant loss: noise_var must be given"),
    ('zero noise_var', [CONSTANT, NONE, CONSTANT, CONSTANT], [2.0, 1.0, 1.5, 1.0], [1.0, -1.0, 0.0, 0.0], "2: noise_var must be positive"),
    ('negative noise_var', [HUBER, HUBER, CONSTANT, CONSTANT], [2.0, 1.0, 1.5, 1.0], [-1.0, np.nan, -3.0, 0.0], "2: noise_var must be positive"),
    ('NaN noise_var', [HUBER, NONE, CONSTANT, CONSTANT], [2.0, 1.0, 1.5, 1.0], [1.0, 1.0, np.nan, 0.0], "2: noise_var must be positive"),
]


@pytest.mark.parametrize('prefix', PREFIXES)
@pytest.mark.parametrize('case', REFUSALS, ids=[c[0].replace(' ', '_') for c in REFUSALS])
def test_loss_list_refusals_carry_the_callers_prefix(shim, case, prefix):
    _, loss, thr, nvar, msg = case
    rc, _, got = check(shim, prefix, loss, thr, nvar)
    assert rc == EINVAL
    assert got == f"{prefix} {msg}"


@pytest.mark.parametrize('prefix', PREFIXES)
def test_null_threshold_is_refused_before_any_factor(shim, prefix):
    rc, any_, got = check(shim, prefix, [7, HUBER], None, None)
    assert rc == EINVAL and got == "threshold is NULL" and any_ == 0
    rc, _, got = check(shim, prefix, [], None, None)       # an empty list as well: the rule is the caller's argument, not a factor's
    assert rc == EINVAL and got == "threshold is NULL"


@pytest.mark.parametrize('prefix', PREFIXES)
def test_all_none_list_passes_and_leaves_any_false(shim, prefix):
    """Thresholds and variances of factors at NONE are not looked at, and noise_var may be NULL."""
    rc, any_, got = check(shim, prefix, [NONE] * 5, [0.0, -1.0, np.nan, np.inf, 2.0], None)
    assert (rc, any_, got) == (0, 0, "")
    rc, any_, got = check(shim, prefix, [], [1.0], None)
    assert (rc, any_, got) == (0, 0, "")


@pytest.mark.parametrize('prefix', PREFIXES)
def test_valid_list_passes_and_sets_any(shim, prefix):
    rc, any_, got = check(shim, prefix, [NONE, HUBER, CONSTANT], [-1.0, 2.0, 1e-300], [0.0, -1.0, 1e-300])   # huber does not read noise_var
    assert (rc, any_, got) == (0, 1, "")
    rc, any_, got = check(shim, prefix, [NONE, NONE, HUBER], [0.0, 0.0, 3.0], None)
    assert (rc, any_, got) == (0, 1, "")


# ---- measurements of the nonlinear factors: gbp_lin_set_nonlinear ("factor") and gbp_lin_extend_nonlinear ("new factor") ----
MEAS_PREFIXES = ('factor', 'new factor')
BAD_SINFO = [0.0, -2.0, np.nan, np.inf]
BAD_MEAS = [np.nan, np.inf, -np.inf]


def check_meas(so, prefix, z, s):
    z, s = np.ascontiguousarray(z, dtype=np.float64), np.ascontiguousarray(s, dtype=np.float64)
    rc = so.lin_check_measurements_host(dptr(z), dptr(s), z.shape[0], prefix.encode())
    return rc, so.lin_pack_last_error().decode()


def entries(count):
    """the first, a middle and the last of the count * 3 entries"""
    n = 3 * count
    return sorted({0, n // 2, n - 1}) if n else []


@pytest.mark.parametrize('count', [0, 1, 3])
def test_measurements_are_packed_as_soa_rows(shim, count):
    """out_meas and out_sinfo [3][count] are the transposes of the two [count][3] lists; the outputs start as NaN, so an entry not
    written shows."""
    rs = np.random.RandomState(200 + count)
    z, s = rs.randn(count, 3), rs.rand(count, 3) + 0.5
    oz, os_ = np.full((3, count), np.nan), np.full((3, count), np.nan)
    shim.lin_pack_measurements_host(count, dptr(z), dptr(s), dptr(oz), dptr(os_))
    assert np.array_equal(oz, z.T)
    assert np.array_equal(os_, s.T)


@pytest.mark.parametrize('prefix', MEAS_PREFIXES)
@pytest.mark.parametrize('count', [0, 1, 3])
def test_valid_measurements_pass(shim, count, prefix):
    rs = np.random.RandomState(300 + count)
    assert check_meas(shim, prefix, rs.randn(count, 3), rs.rand(count, 3) + 1e-300) == (0, "")


@pytest.mark.parametrize('prefix', MEAS_PREFIXES)
@pytest.mark.parametrize('count', [1, 3])
def test_measurement_refusals_name_the_factor_with_the_callers_prefix(shim, count, prefix):
    """A bad value in the first, a middle and the last entry: entry i belongs to factor i // 3.  (count = 0 has no entry to refuse: it
    is among the cases of test_valid_measurements_pass.)"""
    rs = np.random.RandomState(400 + count)
    for i in entries(count):
        for bad in BAD_SINFO:
            z, s = rs.randn(count, 3), rs.rand(count, 3) + 0.5
            s.reshape(-1)[i] = bad
            assert check_meas(shim, prefix, z, s) == (EINVAL, f"{prefix} {i // 3}: sqrt_info must be positive and finite")
        for bad in BAD_MEAS:
            z, s = rs.randn(count, 3), rs.rand(count, 3) + 0.5
            z.reshape(-1)[i] = bad
            assert check_meas(shim, prefix, z, s) == (EINVAL, f"{prefix} {i // 3}: the measurement must be finite")


@pytest.mark.parametrize('prefix', MEAS_PREFIXES)
def test_measurement_refusals_go_entry_by_entry(shim, prefix):
    """Within one entry sqrt_info is looked at before the measurement; across entries the earlier one is refused, whichever list it is in."""
    z, s = np.zeros((3, 3)), np.ones((3, 3))
    z[1, 1], s[1, 1] = np.nan, 0.0
    assert check_meas(shim, prefix, z, s) == (EINVAL, f"{prefix} 1: sqrt_info must be positive and finite")
    z, s = np.zeros((3, 3)), np.ones((3, 3))
    z[0, 2], s[2, 0] = np.inf, -1.0
    assert check_meas(shim, prefix, z, s) == (EINVAL, f"{prefix} 0: the measurement must be finite")
