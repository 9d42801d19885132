// gbp_lin_capi_nonlin.hip -- the nonlinear entry points of include/gbp_lin.h: FactorGraph(nonlinear_factors=True) (gbp.py:30-34),
// relinearise_factors (gbp.py:64-80), the per-factor damping of compute_all_messages (gbp.py:46-54) and
// synchronous_iteration(local_relin=True) (gbp.py:86-92) for the SE(2) and SE(3) relative-pose factors (kernels and models:
// gbp_lin_nonlin.hpp).  The handle's model is a value; lin_model_dispatch (below the includes) turns it into the template argument.
//
// A nonlinear handle keeps (eta_f, Lambda_f) where a linear one does -- LinParams::feta / flam -- so the plain sweep, the joint behind the
// batch MAP and the marginals read the factor "at the current linearisation point" (gbp.py:96-97) without knowing.  What is added per
// factor: measurement and square-root information, the linearisation point, iters_since_relin and the factor's damping.  A sweep is
// three kernels queued on the handle's stream (k_lin_relin, k_lin_factor<D, false, LinRelin>, k_lin_belief; D = 3 or 6): no host round trip; the
// only atomics are integer adds of the per-sweep counts.  With losses set (gbp_lin_capi_nonlin_robust.hip) the factor stage is
// k_lin_factor<D, true, LinRelin>, at the weights as they stand.  Every call that may relinearise clears map_ready, as a change of robust
// weights does.  The five per-factor arrays are the nonlinear columns of a generation (lin_gen_columns, gbp_lin_generation.hpp):
// gbp_lin_set_nonlinear allocates them through that list, and extend / shrink rebuild them with the graph's.
#include "gbp_lin_generation.hpp"
#include "gbp_lin_nonlin.hpp"
#include "gbp_lin_sweep.hpp"

using namespace gbp;

namespace {

int nl_check_state(gbp_lin *h)
{
    if (!h->nonlinear) return set_error(GBP_ESTATE, "the handle has no nonlinear factors: call gbp_lin_set_nonlinear first");
    return GBP_OK;
}

// the buffer of the relinearisation counts, of at least n slots
int nl_counts(gbp_lin *h, int n) { return lin_nonlin_grow_counts(h, h->nl.counts, h->nl.cap, n); }

// the relinearise stage (mode: gbp_lin_nonlin.hpp), counted into `count` (nullptr: not counted)
void nl_relin(gbp_lin *h, int mode, int *count)
{
    if (!h->p.F) return;
    lin_model_dispatch(h->nl.model, [&](auto m) {
        hipLaunchKernelGGL((k_lin_relin<decltype(m)::value>), dim3((h->p.F + 255) / 256), dim3(256), 0, h->stream, h->p, h->nl, mode, count, LinRobust{},
                           (int *)nullptr);
    });
}

}  // namespace

namespace gbp {
// a per-sweep counts buffer of at least n slots: grown by replacement, so the handle's allocation count stays
int lin_nonlin_grow_counts(gbp_lin *h, int *&buf, int &cap, int n)
{
    if (n > cap) {
        int *c = nullptr;
        LCHK(lin_alloc(h, &c, (size_t)n));
        lin_free(h, buf);                                   // no call is in flight: every call that counts ends in a synchronisation
        buf = c;
        cap = n;
    }
    return GBP_OK;
}

// the factor stage of a relinearising sweep: every factor with ITS damping (gbp.py:52), and with losses set times its weight as it stands
void lin_nonlin_factor_stage(gbp_lin *h)
{
    if (!h->p.F) return;
    const LinRelin r{h->p, h->nl.fdamp};
    lin_model_dispatch(h->nl.model, [&](auto m) {
        constexpr int D = NonlinModel<decltype(m)::value>::D;
        if (h->p.w) hipLaunchKernelGGL((k_lin_factor<D, true, LinRelin>), dim3((h->p.F + 63) / 64), dim3(64), 0, h->stream, r);
        else hipLaunchKernelGGL((k_lin_factor<D, false, LinRelin>), dim3((h->p.F + 63) / 64), dim3(64), 0, h->stream, r);
    });
}

int lin_nonlin_energy(gbp_lin *h, double *out)
{
    // over red_blocks blocks, as k_lin_energy: the caller adds up red_blocks partials, and after a shrink that is more than
    // ceil(F / 256) (d_red stays with the handle) -- a block past F writes 0 over what an energy at the larger F left there
    lin_model_dispatch(h->nl.model, [&](auto m) {
        hipLaunchKernelGGL((k_lin_energy_nl<decltype(m)::value>), dim3(h->red_blocks), dim3(256), 0, h->stream, h->p, h->nl, out);
    });
    return GBP_OK;
}

// compute_factor (gbp.py:267-294) on the factors [f0, f1) alone, at their adjacent belief means as the handle holds them: eta_f,
// Lambda_f, linpoint, iters = 1, damping = 0 -- the lane code of compute_all_factors, over a launch sized by the range
int lin_nonlin_linearise(gbp_lin *h, int f0, int f1)
{
    if (f1 <= f0) return GBP_OK;
    lin_model_dispatch(h->nl.model, [&](auto m) {
        hipLaunchKernelGGL((k_lin_relin_range<decltype(m)::value>), dim3((f1 - f0 + 255) / 256), dim3(256), 0, h->stream, h->p, h->nl, NL_INIT, f0, f1);
    });
    LHIPCHK(hipGetLastError());
    return GBP_OK;
}
}  // namespace gbp

extern "C" {

int gbp_lin_set_nonlinear(gbp_lin_t *h, const gbp_lin_nonlinear_desc_t *d)
{
    LENTER(h);
    if (!d) return set_error(GBP_EINVAL, "NULL descriptor");
    const int F = h->p.F;
    const int M = lin_model_rows(d->model);
    if (!M) return set_error(GBP_EINVAL, "unknown model %d", d->model);
    if (h->D != lin_model_dofs(d->model))
        return set_error(GBP_EINVAL, "the %s relative-pose factor needs dofs == %d, the handle has %d", d->model == GBP_LIN_MODEL_SE2_BETWEEN ? "SE(2)" : "SE(3)",
                         lin_model_dofs(d->model), h->D);
    if (d->num_undamped_iters < 0 || d->min_linear_iters < 0) return set_error(GBP_EINVAL, "num_undamped_iters and min_linear_iters must not be negative");
    if (!(d->beta >= 0.0)) return set_error(GBP_EINVAL, "beta must not be negative (+inf: never relinearise)");
    if (F && (!d->measurement || !d->sqrt_info)) return set_error(GBP_EINVAL, "NULL array in the descriptor");
    LCHK(lin_check_measurements(d->model, d->measurement, d->sqrt_info, F, "factor"));
    if (h->p.w) return set_error(GBP_ESTATE, "losses of gbp_lin_set_robust are set: a nonlinear handle takes its losses afterwards, from gbp_lin_set_robust_nonlinear");
    if (h->nonlinear) return set_error(GBP_ESTATE, "the handle already has nonlinear factors");

    std::vector<double> z((size_t)M * F), s((size_t)M * F);           // SoA, stride F
    lin_pack_measurements(M, F, d->measurement, d->sqrt_info, z.data(), s.data());
    LinGen g;                                               // the nonlinear columns of the generation the handle holds
    int rc = GBP_OK;
    lin_gen_columns(h, g, [&](auto c) { if (rc == GBP_OK && c.group == LIN_NONLIN) rc = lin_alloc(h, &c.neu, (size_t)c.rows * F); }, d->model);
    LCHK(rc);
    LinNonlin &nl = g.nl;
    LCHK(lin_alloc(h, &nl.counts, 1));
    nl.cap = 1;
    nl.rcounts = nullptr; nl.rcap = 0;                      // allocated with the robust arrays (gbp_lin_set_robust_nonlinear)
    nl.beta = d->beta; nl.num_undamped = d->num_undamped_iters; nl.min_linear = d->min_linear_iters; nl.model = d->model;
    if (F) {
        LHIPCHK(hipMemcpyAsync(lin_mut(nl.meas), z.data(), z.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
        LHIPCHK(hipMemcpyAsync(lin_mut(nl.sinfo), s.data(), s.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    h->nl = nl;
    lin_nl_point(h);
    if (!h->has_beliefs) LCHK(gbp_lin_update_beliefs(h));  // belief = prior (+ whatever messages the handle holds)
    nl_relin(h, NL_INIT, nullptr);                         // compute_all_factors gbp.py:60-62
    LHIPCHK(hipGetLastError());
    LHIPCHK(hipStreamSynchronize(h->stream));              // z and s are temporaries
    h->nonlinear = true;
    h->map_ready = false;
    return GBP_OK;
}

int gbp_lin_relinearise(gbp_lin_t *h, int32_t *n_relinearised)
{
    LENTER(h);
    LCHK(nl_check_state(h));
    LHIPCHK(hipMemsetAsync(h->nl.counts, 0, sizeof(int), h->stream));
    nl_relin(h, NL_ALONE, h->nl.counts);
    LHIPCHK(hipGetLastError());
    h->map_ready = false;                                   // the joint is that of the new linearisation point
    if (n_relinearised) {
        LHIPCHK(hipMemcpyAsync(n_relinearised, h->nl.counts, sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        LHIPCHK(hipStreamSynchronize(h->stream));
    }
    return GBP_OK;
}

int gbp_lin_iterate_nonlinear(gbp_lin_t *h, int32_t n_iters, int32_t *relin_counts)
{
    LENTER(h);
    if (n_iters < 0) return set_error(GBP_EINVAL, "negative iteration count");
    LCHK(nl_check_state(h));
    if (!n_iters) return GBP_OK;
    LCHK(nl_counts(h, n_iters));
    const LinNonlin &nl = h->nl;
    LHIPCHK(hipMemsetAsync(nl.counts, 0, (size_t)n_iters * sizeof(int), h->stream));
    h->map_ready = false;                                   // the joint is that of the new linearisation point
    for (int it = 0; it < n_iters; ++it) {
        nl_relin(h, NL_SWEEP, nl.counts + it);
        lin_nonlin_factor_stage(h);                         // with losses set: at the weights as they stand (robustify=False)
        LCHK(gbp_lin_update_beliefs(h));
    }
    LHIPCHK(hipGetLastError());
    if (relin_counts) {
        LHIPCHK(hipMemcpyAsync(relin_counts, nl.counts, (size_t)n_iters * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        LHIPCHK(hipStreamSynchronize(h->stream));
    }
    return GBP_OK;
}

int gbp_lin_get_linearisation(gbp_lin_t *h, double *linpoint, int32_t *iters_since_relin, double *eta_damping)
{
    LENTER(h);
    LCHK(nl_check_state(h));
    const size_t F = (size_t)h->p.F, W = 2 * (size_t)h->D;    // a linpoint is [xa; xb]
    std::vector<double> lp;
    if (F) {
        if (linpoint) {
            lp.resize(W * F);
            LHIPCHK(hipMemcpyAsync(lp.data(), h->nl.linpoint, lp.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        }
        if (iters_since_relin) LHIPCHK(hipMemcpyAsync(iters_since_relin, h->nl.iters, F * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        if (eta_damping) LHIPCHK(hipMemcpyAsync(eta_damping, h->nl.fdamp, F * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    LHIPCHK(hipStreamSynchronize(h->stream));
    if (linpoint) for (size_t f = 0; f < F; ++f) for (size_t k = 0; k < W; ++k) linpoint[f * W + k] = lp[k * F + f];
    return GBP_OK;
}

}  // extern "C"
