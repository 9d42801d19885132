// gbp_lin_capi_robust.hip -- the robust-loss entry points of include/gbp_lin.h: Factor(loss=, mahalanobis_threshold=),
// Factor.robustify_loss (gbp.py:296-332), FactorGraph.robustify_all_factors (gbp.py:82-84) and synchronous_iteration(robustify=True)
// (gbp.py:86-92) for the linear engine (kernels and semantics: gbp_lin_robust.hpp).
//
// The handle keeps its nominal factors; what a loss changes is one weight per factor, LinParams::w, which every user of
// (eta_f, Lambda_f) multiplies in: the sweep (k_lin_factor<D, true>), the energy, and the joint behind the batch MAP and the marginals.
// LinParams::w is nullptr until losses are set and again after they are cleared: such a handle runs the plain kernels only.  Every call
// that changes the weights clears map_ready, so the next solve re-makes the LDL^T of the diagonal blocks and the joint eta in the same
// workspace; the iterate of the last solve stays where it is (gbp_lin_get_map).  A robust sweep is three kernels queued on the handle's
// stream (k_lin_robustify, k_lin_factor<D, true>, k_lin_belief): no host round trip, no floating-point atomics.  The five arrays of
// LinRobust are the robust columns of a generation (lin_gen_columns, gbp_lin_generation.hpp): the first gbp_lin_set_robust allocates
// them through that list, and the values it starts from are the list's fills.
#include "gbp_lin_robust.hpp"
#include "gbp_lin_generation.hpp"

using namespace gbp;

namespace {

template <typename T>
int rob_upload(gbp_lin *h, const T *dst, const std::vector<T> &v)
{
    if (!v.empty()) LHIPCHK(hipMemcpyAsync(const_cast<T *>(dst), v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return GBP_OK;
}

// every weight and every flag as a new factor has them: 1 and 0
int rob_reset(gbp_lin *h)
{
    const size_t F = (size_t)h->p.F;
    static_assert(LIN_NEW_FLAG == 0, "the flags are reset by a memset");
    LCHK(rob_upload(h, h->rob.w, std::vector<double>(F, LIN_NEW_W)));
    if (F) LHIPCHK(hipMemsetAsync(h->rob.flag, 0, F * sizeof(int), h->stream));
    LHIPCHK(hipStreamSynchronize(h->stream));              // the host vectors above are temporaries
    return GBP_OK;
}

int rob_robustify(gbp_lin *h)
{
    if (h->p.F) {
        lin_dispatch(h->D, [&](auto d) {
            hipLaunchKernelGGL((k_lin_robustify<decltype(d)::value>), dim3((h->p.F + 255) / 256), dim3(256), 0, h->stream, h->p, h->rob);
        });
        LHIPCHK(hipGetLastError());
    }
    h->map_ready = false;                                   // the joint is that of the new weights
    return GBP_OK;
}

int rob_check_state(gbp_lin *h)
{
    if (!h->p.w) return set_error(GBP_ESTATE, "no losses set: call gbp_lin_set_robust first");
    if (!h->has_beliefs) return set_error(GBP_ESTATE, "call gbp_lin_update_beliefs first: the weights are taken at the belief means");
    return GBP_OK;
}

}  // namespace

extern "C" {

int gbp_lin_set_robust(gbp_lin_t *h, const int32_t *loss, const double *threshold, const double *noise_var)
{
    LENTER(h);
    LIN_REFUSE_NONLINEAR(h, "gbp_lin_set_robust");
    const int F = h->p.F;
    if (!loss) {                                            // clear: back to the plain path
        LHIPCHK(hipStreamSynchronize(h->stream));
        if (h->p.w) { h->p.w = nullptr; h->map_ready = false; }
        if (h->rob_alloc) LCHK(rob_reset(h));
        return GBP_OK;
    }
    bool any = false;
    LCHK(lin_check_losses(loss, threshold, noise_var, F, "factor", &any));
    if (any && !h->has_const)
        return set_error(GBP_EINVAL, "a loss needs the factors' constants: the handle was created with factor_const == NULL");
    if (!h->rob_alloc) {                                    // the robust columns of the generation the handle holds
        LinGen g;
        int rc = GBP_OK;
        lin_gen_columns(h, g, [&](auto c) { if (rc == GBP_OK && c.group == LIN_ROBUST) rc = lin_alloc(h, &c.neu, (size_t)c.rows * F); });
        LCHK(rc);
        h->rob = g.rob;
        h->rob_alloc = true;
    }
    std::vector<int> hl(loss, loss + F);
    std::vector<double> ht((size_t)F, LIN_NEW_THR), hn((size_t)F, LIN_NEW_NVAR);
    for (int f = 0; f < F; ++f) {
        if (loss[f] != GBP_LIN_LOSS_NONE) ht[f] = threshold[f];
        if (loss[f] == GBP_LIN_LOSS_CONSTANT) hn[f] = noise_var[f];
    }
    LHIPCHK(hipStreamSynchronize(h->stream));              // no sweep in flight reads the arrays about to change
    LCHK(rob_upload(h, h->rob.loss, hl)); LCHK(rob_upload(h, h->rob.thr, ht)); LCHK(rob_upload(h, h->rob.nvar, hn));
    LCHK(rob_reset(h));
    h->p.w = h->rob.w;
    h->map_ready = false;
    return GBP_OK;
}

int gbp_lin_robustify(gbp_lin_t *h)
{
    LENTER(h);
    LIN_REFUSE_NONLINEAR(h, "gbp_lin_robustify");
    LCHK(rob_check_state(h));
    return rob_robustify(h);
}

int gbp_lin_iterate_robust(gbp_lin_t *h, int32_t n_iters)
{
    LENTER(h);
    LIN_REFUSE_NONLINEAR(h, "gbp_lin_iterate_robust");
    if (n_iters < 0) return set_error(GBP_EINVAL, "negative iteration count");
    LCHK(rob_check_state(h));
    for (int it = 0; it < n_iters; ++it) {
        LCHK(rob_robustify(h));
        LCHK(lin_sweep(h));
    }
    LHIPCHK(hipGetLastError());
    return GBP_OK;
}

int gbp_lin_get_weights(gbp_lin_t *h, double *w, int32_t *robust_flag)
{
    LENTER(h);
    if (!w) return set_error(GBP_EINVAL, "w is NULL");
    const size_t F = (size_t)h->p.F;
    LHIPCHK(hipStreamSynchronize(h->stream));
    if (!h->p.w) {                                          // no losses set: every factor is Gaussian
        for (size_t f = 0; f < F; ++f) { w[f] = 1.0; if (robust_flag) robust_flag[f] = 0; }
        return GBP_OK;
    }
    if (F) {
        LHIPCHK(hipMemcpyAsync(w, h->rob.w, F * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        if (robust_flag) LHIPCHK(hipMemcpyAsync(robust_flag, h->rob.flag, F * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    }
    LHIPCHK(hipStreamSynchronize(h->stream));
    return GBP_OK;
}

}  // extern "C"
