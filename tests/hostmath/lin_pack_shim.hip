// lin_pack_shim.hip -- TEST INFRASTRUCTURE: the host routines that gbp_lin_create, gbp_lin_extend, gbp_lin_set_robust,
// gbp_lin_set_nonlinear and gbp_lin_extend_nonlinear share (gbp_amd/csrc/gbp_lin_generation.hpp: packing factors, priors and
// measurements for upload, the rules for a list of losses and for a list of measurements) compiled for the host,
// so that tests/test_linear_pack_cpu.py can run them on a CPU against numpy.  They make no HIP call.  The library's set_error
// (gbp_capi.hip) is replaced by one that keeps the message where the test can read it.  Built host-only by that test with hipcc;
// nothing in the product links or loads it.
#include "../../gbp_amd/csrc/gbp_lin_generation.hpp"

#include <cstdarg>
#include <cstdio>

namespace {
char g_msg[512];
}

namespace gbp {
int set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return code;
}
}  // namespace gbp

extern "C" {

void lin_pack_factors_host(int D, int count, const double *eta, const double *lam, double *out_eta, double *out_lam)
{
    lin_pack_factors(D, count, eta, lam, out_eta, out_lam);
}

void lin_pack_priors_host(int D, int count, const double *eta, const double *lam, double *out) { lin_pack_priors(D, count, eta, lam, out); }

// the return code; *any as the routine left it; the message of a refusal in lin_pack_last_error()
int lin_check_losses_host(const int32_t *loss, const double *thr, const double *nvar, int count, const char *prefix, int *any)
{
    bool a = false;
    g_msg[0] = 0;
    const int rc = lin_check_losses(loss, thr, nvar, count, prefix, &a);
    *any = a ? 1 : 0;
    return rc;
}

// measurements and square-root informations [count][3]: the return code, the message of a refusal in lin_pack_last_error()
int lin_check_measurements_host(const double *meas, const double *sinfo, int count, const char *prefix)
{
    g_msg[0] = 0;
    return lin_check_measurements(meas, sinfo, count, prefix);
}

void lin_pack_measurements_host(int count, const double *meas, const double *sinfo, double *out_meas, double *out_sinfo)
{
    lin_pack_measurements(count, meas, sinfo, out_meas, out_sinfo);
}

const char *lin_pack_last_error() { return g_msg; }

}  // extern "C"
