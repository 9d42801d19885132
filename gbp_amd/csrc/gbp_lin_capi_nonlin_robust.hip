// gbp_lin_capi_nonlin_robust.hip -- robust losses on a nonlinear handle (include/gbp_lin.h): Factor(loss=, mahalanobis_threshold=) on
// FactorGraph(nonlinear_factors=True), Factor.robustify_loss (gbp.py:296-332), robustify_all_factors (gbp.py:82-84) and
// synchronous_iteration(local_relin=True, robustify=True) (gbp.py:86-92) for the SE(2) and SE(3) relative-pose factors.
//
// The weight is made from M_f = |diag(s) z - h(linpoint_f)| -- at the LINPOINT, the reference's reading (gbp.py:309), which here moves
// with every relinearisation -- by the relinearise lane itself: k_lin_relin<MODEL, true> (gbp_lin_nonlin.hpp) robustifies a factor at
// its linpoint as it stands and then runs the relinearisation test and re-make unchanged, so a robust relinearising sweep is still three
// kernels (that, k_lin_factor<D, true, LinRelin>, k_lin_belief), with no host round trip and no floating-point atomics.  The weight
// multiplies the factor as linearised wherever it is used, exactly as on a linear handle: LinParams::w is what the factor stage, the
// energy and the joint read, and nullptr -- the plain nonlinear path -- until losses are set and again after they are cleared.  The
// arrays are the robust columns of a generation (lin_gen_columns): the first gbp_lin_set_robust_nonlinear allocates them through that
// list, with the buffer of the per-sweep flag counts, and extend / shrink carry them with the graph's.  The noise variance column is
// kept at its fill: the whitened model has variance 1.
#include "gbp_lin_generation.hpp"
#include "gbp_lin_nonlin.hpp"

using namespace gbp;

namespace {

int nlr_check_state(gbp_lin *h)
{
    if (!h->nonlinear) return set_error(GBP_ESTATE, "the handle has no nonlinear factors: call gbp_lin_set_nonlinear first");
    if (!h->p.w) return set_error(GBP_ESTATE, "no losses set: call gbp_lin_set_robust_nonlinear first");
    return GBP_OK;
}

// the fused lane over every factor (mode: gbp_lin_nonlin.hpp), counted into `count` / `rcount` (nullptr: not counted)
void nlr_relin(gbp_lin *h, int mode, int *count, int *rcount)
{
    if (!h->p.F) return;
    lin_model_dispatch(h->nl.model, [&](auto m) {
        hipLaunchKernelGGL((k_lin_relin<decltype(m)::value, true>), dim3((h->p.F + 255) / 256), dim3(256), 0, h->stream, h->p, h->nl, mode, count, h->rob,
                           rcount);
    });
}

template <typename T>
int nlr_upload(gbp_lin *h, const T *dst, size_t at, const std::vector<T> &v)
{
    if (!v.empty()) LHIPCHK(hipMemcpyAsync(const_cast<T *>(dst) + at, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return GBP_OK;
}

// loss, threshold, weight and flag of the factors [first, first + count): the caller's where `loss` is given, else what a new factor has
int nlr_write(gbp_lin *h, int first, int count, const int32_t *loss, const double *thr)
{
    std::vector<int> hl((size_t)count, LIN_NEW_LOSS), hf((size_t)count, LIN_NEW_FLAG);
    std::vector<double> ht((size_t)count, LIN_NEW_THR), hw((size_t)count, LIN_NEW_W);
    if (loss)
        for (int f = 0; f < count; ++f) {
            hl[f] = loss[f];
            if (loss[f] != GBP_LIN_LOSS_NONE) ht[f] = thr[f];
        }
    LCHK(nlr_upload(h, h->rob.loss, (size_t)first, hl)); LCHK(nlr_upload(h, h->rob.thr, (size_t)first, ht));
    LCHK(nlr_upload(h, (const double *)h->rob.w, (size_t)first, hw)); LCHK(nlr_upload(h, (const int *)h->rob.flag, (size_t)first, hf));
    if (!loss) LCHK(nlr_upload(h, h->rob.nvar, (size_t)first, std::vector<double>((size_t)count, LIN_NEW_NVAR)));
    LHIPCHK(hipStreamSynchronize(h->stream));              // the host vectors above are temporaries
    return GBP_OK;
}

}  // namespace

extern "C" {

int gbp_lin_set_robust_nonlinear(gbp_lin_t *h, int32_t first, int32_t count, const int32_t *loss, const double *threshold)
{
    LENTER(h);
    if (!h->nonlinear) return set_error(GBP_ESTATE, "the handle has no nonlinear factors: call gbp_lin_set_nonlinear first, or gbp_lin_set_robust");
    const int F = h->p.F;
    if (first < 0 || count < 0 || (long long)first + count > F)
        return set_error(GBP_EINVAL, "factors [%d, %d + %d) are not a range of the handle's %d", first, first, count, F);
    if (!loss && !(first == 0 && count == F)) return set_error(GBP_EINVAL, "loss is NULL: clearing is for the whole graph (first == 0, count == F)");
    if (!count) return GBP_OK;
    if (!loss) {                                            // clear: back to the plain nonlinear path
        LHIPCHK(hipStreamSynchronize(h->stream));
        if (h->p.w) { h->p.w = nullptr; h->map_ready = false; }
        if (h->rob_alloc) LCHK(nlr_write(h, 0, F, nullptr, nullptr));
        return GBP_OK;
    }
    bool any = false;
    const std::vector<double> one((size_t)count, 1.0);      // the whitened model: the constant loss needs no noise_var
    LCHK(lin_check_losses(loss, threshold, one.data(), count, "factor first +", &any));
    if (!h->rob_alloc) {                                    // the robust columns of the generation the handle holds
        LinGen g;
        int rc = GBP_OK;
        lin_gen_columns(h, g, [&](auto c) { if (rc == GBP_OK && c.group == LIN_ROBUST) rc = lin_alloc(h, &c.neu, (size_t)c.rows * F); });
        LCHK(rc);
        h->rob = g.rob;
        h->rob_alloc = true;
    }
    if (!h->nl.rcounts) LCHK(lin_nonlin_grow_counts(h, h->nl.rcounts, h->nl.rcap, 1));
    LHIPCHK(hipStreamSynchronize(h->stream));              // no sweep in flight reads the arrays about to change
    if (!h->p.w) LCHK(nlr_write(h, 0, F, nullptr, nullptr));   // losses were not set: every factor outside the range is a new one's
    LCHK(nlr_write(h, first, count, loss, threshold));
    h->p.w = h->rob.w;
    h->map_ready = false;
    return GBP_OK;
}

int gbp_lin_robustify_nonlinear(gbp_lin_t *h)
{
    LENTER(h);
    LCHK(nlr_check_state(h));
    nlr_relin(h, NL_ROBUSTIFY, nullptr, nullptr);
    LHIPCHK(hipGetLastError());
    h->map_ready = false;                                   // the joint is that of the new weights
    return GBP_OK;
}

int gbp_lin_iterate_nonlinear_robust(gbp_lin_t *h, int32_t n_iters, int32_t *relin_counts, int32_t *robust_counts)
{
    LENTER(h);
    if (n_iters < 0) return set_error(GBP_EINVAL, "negative iteration count");
    LCHK(nlr_check_state(h));
    if (!n_iters) return GBP_OK;
    LCHK(lin_nonlin_grow_counts(h, h->nl.counts, h->nl.cap, n_iters));
    LCHK(lin_nonlin_grow_counts(h, h->nl.rcounts, h->nl.rcap, n_iters));
    const LinNonlin &nl = h->nl;
    LHIPCHK(hipMemsetAsync(nl.counts, 0, (size_t)n_iters * sizeof(int), h->stream));
    LHIPCHK(hipMemsetAsync(nl.rcounts, 0, (size_t)n_iters * sizeof(int), h->stream));
    h->map_ready = false;                                   // the joint is that of the new weights and linearisation point
    for (int it = 0; it < n_iters; ++it) {
        nlr_relin(h, NL_SWEEP, nl.counts + it, nl.rcounts + it);   // gbp.py:87-90: robustify at the old linpoint, then relinearise
        lin_nonlin_factor_stage(h);                         // gbp.py:91: each factor's own damping, times its weight
        LCHK(gbp_lin_update_beliefs(h));                    // gbp.py:92
    }
    LHIPCHK(hipGetLastError());
    if (relin_counts) LHIPCHK(hipMemcpyAsync(relin_counts, nl.counts, (size_t)n_iters * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (robust_counts) LHIPCHK(hipMemcpyAsync(robust_counts, nl.rcounts, (size_t)n_iters * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (relin_counts || robust_counts) LHIPCHK(hipStreamSynchronize(h->stream));
    return GBP_OK;
}

}  // extern "C"
