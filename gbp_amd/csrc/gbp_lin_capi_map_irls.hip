// gbp_lin_capi_map_irls.hip -- gbp_lin_solve_map_nonlinear_robust of include/gbp_lin.h: the robust nonlinear batch MAP of a handle with
// SE(2) / SE(3) factors, the fixed point of synchronous_iteration(local_relin=True, robustify=True) (gbp.py:86-92): linpoints equal to the
// means, weights those of Factor.robustify_loss at them (gbp.py:296-332), means solving the joint at that linearisation and those
// weights (gbp.py:94-144).  It is reached by iteratively reweighted least squares with the reference's own, energy-matched weights:
//   reweight r   k_gn_reweight<MODEL> (gbp_lin_gn.hpp): w_f and the flag of every factor from M_f at the SOLVER's x, into arrays of the
//                solver's own (LinGn::w / flag, never LinRobust's), with the linearisation at x, the weighted energy, max |w_new - w_old|
//                and the flagged count in the same lane; k_gn_reweight_finish: four doubles reach the host;
//   round r      the Levenberg-Marquardt loop of gbp_lin_solve_map_nonlinear (gn_lm, gbp_lin_capi_map_nonlin.hip) on a LinParams whose
//                `w` points at those weights, from x, its first linearisation being the one the reweight just made.
// Nothing of the sweep is written, the handle's weights and flags included; the final x lands in LinMap::x with map_solved set.
#include "gbp_lin_generation.hpp"
#include "gbp_lin_gn.hpp"

#include <cmath>

using namespace gbp;

namespace {

// the arrays this call adds to LinGn, once per generation, all or nothing like gn_workspace's
int irls_workspace(gbp_lin *h)
{
    if (h->gn.irls) return GBP_OK;
    const size_t N = (size_t)h->p.N, F = (size_t)h->p.F;
    LinGn g = h->gn;
    const int rc = [&]() -> int {
        LCHK(lin_alloc(h, &g.w, F)); LCHK(lin_alloc(h, &g.flag, F)); LCHK(lin_alloc(h, &g.xs, N * h->D));
        LCHK(lin_alloc(h, &g.w_part, (size_t)g.nen)); LCHK(lin_alloc(h, &g.count, (size_t)1)); LCHK(lin_alloc(h, &g.rout, (size_t)GN_RW_OUT));
        LHIPCHK(hipMemsetAsync(g.w_part, 0, (size_t)g.nen * sizeof(double), h->stream));
        return GBP_OK;
    }();
    if (rc != GBP_OK) {
        for (const void *q : {(const void *)g.w, (const void *)g.flag, (const void *)g.xs, (const void *)g.w_part, (const void *)g.count, (const void *)g.rout})
            lin_free(h, q);                                 // nullptr: nothing to free
        return rc;
    }
    g.irls = true;
    h->gn = g;
    return GBP_OK;
}

// One reweight at LinGn::x: out = (the weighted energy, max |w_new - w_old|, the flagged count, the last round's max |x_end - x_start|)
// on the host.  Without factors nothing is launched but the finish: the partials stay at the zeros of the workspaces.
int irls_reweight(gbp_lin *h, bool first, double (&out)[GN_RW_OUT])
{
    const LinGn &g = h->gn;
    LHIPCHK(hipMemsetAsync(g.count, 0, sizeof(int), h->stream));
    if (h->p.F) {
        const int *loss = h->p.w ? h->rob.loss : nullptr;   // losses are set while LinParams::w points at the handle's weights
        const double *thr = h->p.w ? h->rob.thr : nullptr;
        lin_model_dispatch(h->nl.model, [&](auto m) {
            hipLaunchKernelGGL((k_gn_reweight<decltype(m)::value>), dim3(g.nen), dim3(256), 0, h->stream, h->p, h->nl, loss, thr, (const double *)g.x, first ? 1 : 0,
                               g.feta, g.flam, g.w, g.flag, g.e_part, g.w_part, g.count);
        });
        LHIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL((k_gn_reweight_finish<GN_RW_OUT>), dim3(1), dim3(MAP_BLOCK), 0, h->stream, (const double *)g.e_part, (const double *)g.w_part, g.nen,
                       (const int *)g.count, (const double *)g.v_part, g.nb, g.rout);
    LHIPCHK(hipGetLastError());
    LHIPCHK(hipMemcpyAsync(out, g.rout, sizeof(out), hipMemcpyDeviceToHost, h->stream));
    LHIPCHK(hipStreamSynchronize(h->stream));
    return GBP_OK;
}

}  // namespace

extern "C" {

int gbp_lin_solve_map_nonlinear_robust(gbp_lin_t *h, const gbp_lin_irls_opts_t *opts, double *round_trace, double *lm_trace, double *weights, int32_t *robust_flag,
                                       gbp_lin_irls_info_t *info)
{
    LENTER(h);
    if (!h->nonlinear) return set_error(GBP_ESTATE, "the handle has no nonlinear factors: call gbp_lin_set_nonlinear first");
    const gbp_lin_irls_opts_t o = opts ? *opts : gbp_lin_irls_opts_t{20, 0, 1e-9, 1e-10, gn_nlmap_defaults()};
    if (o.max_rounds < 0) return set_error(GBP_EINVAL, "negative max_rounds");
    if (!(o.tol_weight >= 0.0) || !std::isfinite(o.tol_weight) || !(o.tol_move >= 0.0) || !std::isfinite(o.tol_move))
        return set_error(GBP_EINVAL, "tol_weight or tol_move is negative or not finite");
    LCHK(gn_check_opts(o.lm));
    if (o.lm.init == GBP_LIN_NLMAP_FROM_MEANS && !h->has_beliefs) return set_error(GBP_ESTATE, "init from the means needs beliefs");
    if (o.lm.init == GBP_LIN_NLMAP_FROM_MAP && !h->map_solved) return set_error(GBP_ESTATE, "init from the MAP iterate needs a solve: call gbp_lin_solve_map first");

    gbp_lin_irls_info_t out{};
    LCHK(lin_map_workspace(h));
    LCHK(gn_workspace(h));
    LCHK(irls_workspace(h));
    const int N = h->p.N, F = h->p.F, D = h->D;
    const size_t bytes = (size_t)N * D * sizeof(double);
    const LinMap &m = h->map;
    const LinGn &g = h->gn;
    h->map_ready = false;                                   // the workspace is about to hold the LDL^T and eta of damped systems
    if (!N) {                                               // nothing to solve, no factor to weigh
        h->map_solved = true;
        out.converged = 1; out.reason = GBP_LIN_IRLS_WEIGHTS;
        if (round_trace) for (int k = 0; k < 6; ++k) round_trace[k] = 0.0;
        if (info) *info = out;
        return GBP_OK;
    }
    LCHK(gn_start(h, o.lm.init));
    LinParams base = h->p;                                  // what every round minimises at: the solver's weights, not the handle's
    base.w = g.w;

    double rw[GN_RW_OUT];
    for (int r = 0;; ++r) {
        LCHK(irls_reweight(h, r == 0, rw));
        const double wchange = r ? rw[1] : 0.0, move = r ? rw[3] : 0.0;
        double *row = round_trace ? round_trace + (size_t)r * 6 : nullptr;
        if (row) { row[0] = rw[0]; row[1] = rw[2]; row[2] = wchange; row[3] = move; row[4] = 0.0; row[5] = 0.0; }
        if (r == 0) out.energy0 = rw[0];
        out.energy = rw[0]; out.flagged = (int32_t)rw[2]; out.weight_change = wchange; out.move = move;
        if (r >= 1) {                                       // the stop test, in this order; a NaN compares false
            if (o.tol_weight > 0.0 && wchange <= o.tol_weight) { out.converged = 1; out.reason = GBP_LIN_IRLS_WEIGHTS; break; }
            if (o.tol_move > 0.0 && move <= o.tol_move) { out.converged = 1; out.reason = GBP_LIN_IRLS_MOVE; break; }
        }
        if (r == o.max_rounds) break;                       // reason NONE: the weights are still those made at the final x
        LHIPCHK(hipMemcpyAsync(g.xs, g.x, bytes, hipMemcpyDeviceToDevice, h->stream));
        gbp_lin_nlmap_info_t li{};
        LCHK(gn_lm(h, base, true, o.lm, lm_trace ? lm_trace + (size_t)out.outer * 5 : nullptr, &li));   // STALL or NONE: the loop goes on
        if (row) { row[4] = (double)li.outer; row[5] = (double)li.reason; }
        out.outer += li.outer; out.accepted += li.accepted; out.rejected += li.rejected; out.cg_iters += li.cg_iters;
        out.grad_norm = li.grad_norm;
        ++out.rounds;
        // max |x_end - x_start| of the round into the second half of v_part, which the next reweight's finish reads
        lin_dispatch(D, [&](auto d) {
            hipLaunchKernelGGL((k_gn_diff<decltype(d)::value>), dim3(m.nb), dim3(MAP_BLOCK), 0, h->stream, base.prior, N, (const double *)g.xs, (const double *)g.x, g.v_part, g.nb);
        });
        LHIPCHK(hipGetLastError());
    }
    if (weights && F) LHIPCHK(hipMemcpyAsync(weights, g.w, (size_t)F * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (robust_flag && F) LHIPCHK(hipMemcpyAsync(robust_flag, g.flag, (size_t)F * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    LHIPCHK(hipMemcpyAsync(m.x, g.x, bytes, hipMemcpyDeviceToDevice, h->stream));
    LHIPCHK(hipStreamSynchronize(h->stream));
    h->map_solved = true;
    if (info) *info = out;
    return GBP_OK;
}

}  // extern "C"
