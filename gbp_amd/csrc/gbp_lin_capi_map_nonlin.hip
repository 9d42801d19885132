// gbp_lin_capi_map_nonlin.hip -- gbp_lin_solve_map_nonlinear of include/gbp_lin.h: the minimiser of the nonlinear least-squares problem
// of a handle with SE(2) / SE(3) factors (what joint_distribution_cov's mu, gbp.py:128-144, becomes when it is iterated to a fixed
// point), by Levenberg-Marquardt on the device.  Kernels and method: gbp_lin_gn.hpp; the inner solves are the conjugate gradients of
// gbp_lin_capi_map.hip on a LinParams copy whose feta / flam / prior point at the solver's own linearisation and damped priors.
//
// Nothing of the sweep is written: the handle's eta_f / Lambda_f, linpoint, iters, damping, weights, messages and beliefs are read at
// most (the means as a starting point, the weights as they stand).  The call works in LinMap's workspace and leaves map_ready false --
// the LDL^T and joint eta in it are those of the last damped system --, so the next gbp_lin_solve_map re-makes them; the final x lands
// in LinMap::x with map_solved set.  The host decides each step from four downloaded doubles.
#include "gbp_lin_generation.hpp"
#include "gbp_lin_gn.hpp"

#include <cmath>

using namespace gbp;

// What gbp_lin_solve_map_nonlinear and gbp_lin_solve_map_nonlinear_robust (gbp_lin_capi_map_irls.hip) share, declared in gbp_lin_gn.hpp:
// the options' defaults and rules, the workspace, the start and the Levenberg-Marquardt loop itself.
namespace gbp {

gbp_lin_nlmap_opts_t gn_nlmap_defaults() { return {50, GBP_LIN_NLMAP_FROM_MEANS, 1e-4, 10.0, 0.1, 1e-12, 1e8, 1e-10, 1e-8, {1e-12, 10000, 8, 0}}; }

int gn_check_opts(const gbp_lin_nlmap_opts_t &o)
{
    if (o.max_outer < 0) return set_error(GBP_EINVAL, "negative max_outer");
    if (o.init != GBP_LIN_NLMAP_FROM_MEANS && o.init != GBP_LIN_NLMAP_FROM_MAP) return set_error(GBP_EINVAL, "unknown init %d", o.init);
    for (double v : {o.lambda0, o.lambda_up, o.lambda_down, o.lambda_min, o.lambda_max})
        if (!(v > 0.0) || !std::isfinite(v)) return set_error(GBP_EINVAL, "lambda0, lambda_up, lambda_down, lambda_min and lambda_max must be positive and finite");
    if (!(o.lambda_up > 1.0)) return set_error(GBP_EINVAL, "lambda_up must be above 1");
    if (!(o.lambda_down < 1.0)) return set_error(GBP_EINVAL, "lambda_down must be below 1");
    if (!(o.lambda_min <= o.lambda0 && o.lambda0 <= o.lambda_max)) return set_error(GBP_EINVAL, "lambda_min <= lambda0 <= lambda_max does not hold");
    if (!(o.tol_step >= 0.0) || !std::isfinite(o.tol_step) || !(o.tol_grad >= 0.0) || !std::isfinite(o.tol_grad))
        return set_error(GBP_EINVAL, "a tolerance is negative or not finite");
    if (!(o.cg.rel_tol > 0.0)) return set_error(GBP_EINVAL, "cg.rel_tol must be positive");
    if (o.cg.max_iters < 0) return set_error(GBP_EINVAL, "negative cg.max_iters");
    if (o.cg.check_every < 1) return set_error(GBP_EINVAL, "cg.check_every must be at least 1");
    if (o.cg.warm_start) return set_error(GBP_EINVAL, "cg.warm_start must be 0: the inner solves always start at x");
    return GBP_OK;
}

// the solver's own arrays, once per generation.  All or nothing: a failed allocation (or memset) gives back what was made before it and
// leaves h->gn as it was -- `alloc` false, every pointer null --, so the call returns its error and a later one starts clean
int gn_workspace(gbp_lin *h)
{
    if (h->gn.alloc) return GBP_OK;
    const int D = h->D, P = D * (D + 1) / 2, P2 = D * (2 * D + 1);
    const size_t N = (size_t)h->p.N, F = (size_t)h->p.F;
    LinGn g{};
    g.nen = std::max(1, (h->p.F + 255) / 256);
    g.nb = h->map.nb;
    const int rc = [&]() -> int {
        LCHK(lin_alloc(h, &g.feta, 2 * D * F)); LCHK(lin_alloc(h, &g.flam, P2 * F));
        LCHK(lin_alloc(h, &g.prior, N * (D + P))); LCHK(lin_alloc(h, &g.x, N * D));
        LCHK(lin_alloc(h, &g.e_part, (size_t)2 * g.nen)); LCHK(lin_alloc(h, &g.v_part, (size_t)2 * g.nb)); LCHK(lin_alloc(h, &g.out, (size_t)GN_OUT));
        LHIPCHK(hipMemsetAsync(g.e_part, 0, (size_t)2 * g.nen * sizeof(double), h->stream));
        LHIPCHK(hipMemsetAsync(g.v_part, 0, (size_t)2 * g.nb * sizeof(double), h->stream));
        return GBP_OK;
    }();
    if (rc != GBP_OK) {
        for (const void *q : {(const void *)g.feta, (const void *)g.flam, (const void *)g.prior, (const void *)g.x, (const void *)g.e_part, (const void *)g.v_part,
                              (const void *)g.out})
            lin_free(h, q);                                 // nullptr: nothing to free
        return rc;
    }
    g.alloc = true;
    h->gn = g;
    return GBP_OK;
}

}  // namespace gbp

namespace {

// the factors at `x`: LIN: the linearisation into the solver's arrays and the energy partials of slot 0; else the energy partials of slot 1
template <bool LIN>
int gn_factors(gbp_lin *h, const LinParams &p, const double *x)
{
    const LinGn &g = h->gn;
    if (!p.F) return GBP_OK;                             // the partials stay at the zeros of gn_workspace
    lin_model_dispatch(h->nl.model, [&](auto m) {
        hipLaunchKernelGGL((k_gn_factor<decltype(m)::value, LIN>), dim3(g.nen), dim3(256), 0, h->stream, p, h->nl, x, g.feta, g.flam, g.e_part + (LIN ? 0 : g.nen));
    });
    LHIPCHK(hipGetLastError());
    return GBP_OK;
}

// out = (E(x), E(x_c), the prior difference, max |x_c - x|) on the host
int gn_read(gbp_lin *h, double (&out)[GN_OUT])
{
    const LinGn &g = h->gn;
    hipLaunchKernelGGL((k_gn_finish<GN_OUT>), dim3(1), dim3(MAP_BLOCK), 0, h->stream, (const double *)g.e_part, (const double *)(g.e_part + g.nen), g.nen, (const double *)g.v_part, g.nb, g.out);
    LHIPCHK(hipGetLastError());
    LHIPCHK(hipMemcpyAsync(out, g.out, sizeof(out), hipMemcpyDeviceToHost, h->stream));
    LHIPCHK(hipStreamSynchronize(h->stream));
    return GBP_OK;
}

}  // namespace

namespace gbp {

// x0 -> g.x.  From the means: gathered into m.x by the solver's own kernel.  The iterate of the last solve stays valid (map_solved)
// until the first inner solve overwrites it; from then on it is invalid until the call has put its final x there.
int gn_start(gbp_lin *h, int init)
{
    const LinMap &m = h->map;
    if (init == GBP_LIN_NLMAP_FROM_MEANS) {
        lin_dispatch(h->D, [&](auto d) {
            hipLaunchKernelGGL((k_map_load_means<decltype(d)::value>), dim3(m.nb), dim3(MAP_BLOCK), 0, h->stream, h->p, m);
        });
        LHIPCHK(hipGetLastError());
    }
    h->map_solved = false;
    LHIPCHK(hipMemcpyAsync(h->gn.x, m.x, (size_t)h->p.N * h->D * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return GBP_OK;
}

// The Levenberg-Marquardt loop from LinGn::x, which it leaves at the final point.  `base`: the handle's LinParams with the weights the
// loop minimises at (`w`: the handle's as they stand, or the robust solver's own).  `linearised`: the linearisation at x and the
// partials of E(x) in slot 0 of e_part are already made (by k_gn_reweight) -- the first iteration then does not linearise again.
// N > 0.  trace: max_outer x 5 or NULL.
int gn_lm(gbp_lin *h, const LinParams &base, bool linearised, const gbp_lin_nlmap_opts_t &o, double *trace, gbp_lin_nlmap_info_t *info)
{
    gbp_lin_nlmap_info_t out{};
    out.lambda = o.lambda0;
    const int N = base.N, D = h->D;
    const size_t bytes = (size_t)N * D * sizeof(double);
    const LinMap &m = h->map;
    const LinGn &g = h->gn;

    LinParams pd = base;                                    // the joint the inner solves see: this linearisation, these priors, these weights
    pd.feta = g.feta; pd.flam = g.flam; pd.prior = g.prior;
    LinParams pl = base;                                    // the damping lane: this linearisation, the handle's priors
    pl.feta = g.feta; pl.flam = g.flam;

    double res[GN_OUT];
    double lambda = o.lambda0, E = 0.0;
    bool fresh = true;                                      // x has moved since the last linearisation
    bool made = linearised;                                 // ... which the caller made for the first x
    const bool linear = base.F == 0;                        // no factors: Phi is the priors' quadratic, one undamped step is exact
    for (int it = 0; it < o.max_outer; ++it) {
        if (fresh && !made) LCHK(gn_factors<true>(h, base, g.x));
        made = false;
        const double lam = linear ? 0.0 : lambda;
        lin_dispatch(D, [&](auto d) {
            hipLaunchKernelGGL((k_gn_damp<decltype(d)::value>), dim3(m.nb), dim3(MAP_BLOCK), 0, h->stream, pl, (const double *)g.x, lam, g.prior);
        });
        LHIPCHK(hipGetLastError());
        double eta_norm = 0.0, rn = 0.0;
        LCHK(lin_map_setup(h, pd, m, &eta_norm));
        LHIPCHK(hipMemcpyAsync(m.x, g.x, bytes, hipMemcpyDeviceToDevice, h->stream));
        if (fresh && o.tol_grad > 0.0) {                    // the first true residual is -grad Phi(x): tested before any CG iteration
            LCHK(lin_map_matvec(h, pd, m, m.x, m.q));
            LCHK(lin_map_restart(h, pd, m, 1, 0, &rn));
            out.grad_norm = rn;
            if (rn <= o.tol_grad) {
                LCHK(gn_read(h, res));
                E = res[0];
                if (it == 0) out.energy0 = E;
                out.converged = 1; out.reason = GBP_LIN_NLMAP_GRAD;
                fresh = false;
                break;
            }
        }
        gbp_lin_map_info_t ci{};
        LCHK(lin_map_solve(h, pd, m, eta_norm, o.cg, LIN_MAP_FROM_X, &ci, &rn));
        if (fresh) out.grad_norm = rn;
        out.cg_iters += ci.iters;
        LCHK(gn_factors<false>(h, base, m.x));
        lin_dispatch(D, [&](auto d) {
            hipLaunchKernelGGL((k_gn_diff<decltype(d)::value>), dim3(m.nb), dim3(MAP_BLOCK), 0, h->stream, base.prior, N, (const double *)g.x, (const double *)m.x, g.v_part, g.nb);
        });
        LHIPCHK(hipGetLastError());
        LCHK(gn_read(h, res));
        if (fresh) E = res[0];
        if (it == 0) out.energy0 = E;
        fresh = false;
        const double dphi = (res[1] - E) + res[2], step = res[3];
        bool take, stop = false;
        if (o.tol_step > 0.0 && step <= o.tol_step) { take = dphi <= 0.0; stop = true; }
        else take = linear ? dphi <= 0.0 : dphi < 0.0;      // a NaN compares false: rejected
        if (trace) { double *row = trace + (size_t)it * 5; row[0] = E; row[1] = lam; row[2] = step; row[3] = dphi; row[4] = take ? 1.0 : 0.0; }
        ++out.outer;
        if (take) {
            LHIPCHK(hipMemcpyAsync(g.x, m.x, bytes, hipMemcpyDeviceToDevice, h->stream));
            E = res[1];
            fresh = true;
            ++out.accepted;
        } else ++out.rejected;
        if (stop) { out.converged = 1; out.reason = GBP_LIN_NLMAP_STEP; break; }
        if (linear) {                                       // solved: one step of an exact method
            if (take) { out.converged = 1; out.reason = GBP_LIN_NLMAP_GRAD; out.grad_norm = ci.rel_residual * eta_norm; }
            break;
        }
        if (take) lambda = std::max(lambda * o.lambda_down, o.lambda_min);
        else {
            if (lambda > o.lambda_max) { out.reason = GBP_LIN_NLMAP_STALL; break; }
            lambda *= o.lambda_up;
        }
    }
    if (o.max_outer == 0) {                                 // no iteration ran: the energy at x0 still has to be made
        if (!linearised) LCHK(gn_factors<true>(h, base, g.x));
        LCHK(gn_read(h, res));
        E = res[0];
        out.energy0 = E;
    }
    out.energy = E; out.lambda = lambda;
    if (info) *info = out;
    return GBP_OK;
}

}  // namespace gbp

extern "C" {

int gbp_lin_solve_map_nonlinear(gbp_lin_t *h, const gbp_lin_nlmap_opts_t *opts, double *trace, gbp_lin_nlmap_info_t *info)
{
    LENTER(h);
    if (!h->nonlinear) return set_error(GBP_ESTATE, "the handle has no nonlinear factors: call gbp_lin_set_nonlinear first");
    const gbp_lin_nlmap_opts_t o = opts ? *opts : gn_nlmap_defaults();
    LCHK(gn_check_opts(o));
    if (o.init == GBP_LIN_NLMAP_FROM_MEANS && !h->has_beliefs) return set_error(GBP_ESTATE, "init from the means needs beliefs");
    if (o.init == GBP_LIN_NLMAP_FROM_MAP && !h->map_solved) return set_error(GBP_ESTATE, "init from the MAP iterate needs a solve: call gbp_lin_solve_map first");

    LCHK(lin_map_workspace(h));
    LCHK(gn_workspace(h));
    h->map_ready = false;                                   // the workspace is about to hold the LDL^T and eta of damped systems
    if (!h->p.N) {                                          // nothing to solve: the gradient of the empty problem is 0
        gbp_lin_nlmap_info_t out{};
        out.lambda = o.lambda0;
        h->map_solved = true;
        out.converged = 1; out.reason = GBP_LIN_NLMAP_GRAD;
        if (info) *info = out;
        return GBP_OK;
    }
    LCHK(gn_start(h, o.init));
    LCHK(gn_lm(h, h->p, false, o, trace, info));            // at the weights as they stand
    LHIPCHK(hipMemcpyAsync(h->map.x, h->gn.x, (size_t)h->p.N * h->D * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    LHIPCHK(hipStreamSynchronize(h->stream));
    h->map_solved = true;
    return GBP_OK;
}

}  // extern "C"
