// gbp_lin_capi_until.hip -- gbp_lin_iterate_until of include/gbp_lin.h: the loop of ndim_posegraph.py:104-108 (synchronous_iteration
// gbp.py:86-92, energy gbp.py:36-44, get_means gbp.py:146-153 against the MAP) in one call, the decision to stop taken on the device
// (method: gbp_lin_until.hpp; the stages are the kernels of gbp_lin_sweep.hpp and gbp_lin_robust.hpp in their gated and traced forms).
//
// The pattern is gbp_lin_solve_map's: sweeps are queued check_every at a time on the handle's stream, each followed by a one-block
// finishing kernel that writes a trace row and, when a tolerance is met, a stop word in device memory; the host reads that word (8
// bytes) only after each batch.  What was queued behind the deciding sweep returns at its head, so the state the call leaves is that of
// gbp_lin_iterate(h, iters), whatever check_every was.  The rows are copied out once, at the end, and only the `iters` that were written.
#include "gbp_lin_sweep.hpp"

#include <cmath>
#include <cstring>

using namespace gbp;

namespace {

constexpr int KNOWN_WANT = GBP_LIN_TRACE_ENERGY | GBP_LIN_TRACE_MAP;

bool tol_ok(double t) { return t >= 0.0 && std::isfinite(t); }

}  // namespace

namespace gbp {
// a trace buffer of at least max_iters rows, the stop word, and the partials of this generation: whatever is missing.  The trace buffer
// (24 bytes per sweep of max_iters) is the one piece a caller can make too large, so it is asked for first: GBP_ENOMEM for it leaves
// the handle holding exactly what it held.  gbp_lin_iterate_until_nonlinear (gbp_lin_capi_until_nonlin.hip) uses the same workspace.
int lin_until_workspace(gbp_lin *h, int max_iters)
{
    LinUntil &u = h->until;
    if (max_iters > u.cap) {
        double *t = nullptr;
        LCHK(lin_alloc(h, &t, (size_t)3 * max_iters));
        lin_free(h, u.trace);                               // no call is in flight: every call ends in a synchronisation
        u.trace = t;
        u.cap = max_iters;
    }
    if (!u.stop) LCHK(lin_alloc(h, &u.stop, 2));
    if (!u.bel_part || !u.en_part) {
        const int R = h->D + h->D * (h->D + 1) / 2, VPW = 64 / R;
        u.nbel = (h->p.N + VPW - 1) / VPW;
        u.nen = (h->p.F + 255) / 256;
        if (!u.bel_part) LCHK(lin_alloc(h, &u.bel_part, (size_t)2 * u.nbel));
        if (!u.en_part) LCHK(lin_alloc(h, &u.en_part, (size_t)u.nen));
    }
    return GBP_OK;
}
}  // namespace gbp

namespace {

// sweep `it` + 1 of the call: every kernel gated on the stop word
int until_sweep(gbp_lin *h, const gbp_lin_until_opts_t &o, const UntilRule &rule, int it)
{
    const LinUntil &u = h->until;
    const LinGated g{h->p, u.stop};
    const LinTraced t{h->p, u, (o.want & GBP_LIN_TRACE_MAP) ? h->map.x : nullptr};
    lin_dispatch(h->D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        if (h->p.F) {
            if (o.robustify) hipLaunchKernelGGL((k_lin_robustify<DD, LinGated>), dim3((h->p.F + 255) / 256), dim3(256), 0, h->stream, g, h->rob);
            if (h->p.w) hipLaunchKernelGGL((k_lin_factor<DD, true, LinGated>), dim3((h->p.F + 63) / 64), dim3(64), 0, h->stream, g);
            else hipLaunchKernelGGL((k_lin_factor<DD, false, LinGated>), dim3((h->p.F + 63) / 64), dim3(64), 0, h->stream, g);
        }
        if (h->p.N) hipLaunchKernelGGL((k_lin_belief<DD, LinTraced>), dim3(u.nbel), dim3(64), 0, h->stream, t);
        if (h->p.F && (o.want & GBP_LIN_TRACE_ENERGY)) hipLaunchKernelGGL((k_lin_energy<DD, LinGated>), dim3(u.nen), dim3(256), 0, h->stream, g, u.en_part);
    });
    hipLaunchKernelGGL((k_until_finish<UNTIL_FIN>), dim3(1), dim3(UNTIL_FIN), 0, h->stream, u, rule, it);
    LHIPCHK(hipGetLastError());
    return GBP_OK;
}

}  // namespace

extern "C" {

int gbp_lin_iterate_until(gbp_lin_t *h, const gbp_lin_until_opts_t *opts, double *trace, gbp_lin_until_info_t *info)
{
    LENTER(h);
    LIN_REFUSE_NONLINEAR(h, "gbp_lin_iterate_until");
    if (!opts) return set_error(GBP_EINVAL, "opts is NULL");
    const gbp_lin_until_opts_t o = *opts;
    if (o.max_iters < 0) return set_error(GBP_EINVAL, "negative max_iters");
    if (o.check_every < 1) return set_error(GBP_EINVAL, "check_every must be at least 1");
    if (o.robustify != 0 && o.robustify != 1) return set_error(GBP_EINVAL, "robustify must be 0 or 1");
    if (o.want & ~KNOWN_WANT) return set_error(GBP_EINVAL, "unknown bits in want: 0x%x", (unsigned)(o.want & ~KNOWN_WANT));
    if (!tol_ok(o.tol_step) || !tol_ok(o.tol_map)) return set_error(GBP_EINVAL, "a tolerance must be finite and not negative (0: off)");
    if (o.tol_map > 0.0 && !(o.want & GBP_LIN_TRACE_MAP)) return set_error(GBP_EINVAL, "tol_map needs GBP_LIN_TRACE_MAP in want");
    if (!h->has_beliefs) return set_error(GBP_ESTATE, "call gbp_lin_update_beliefs first (ndim_posegraph.py:90)");
    if (o.robustify && !h->p.w) return set_error(GBP_ESTATE, "no losses set: call gbp_lin_set_robust first");
    if ((o.want & GBP_LIN_TRACE_MAP) && !h->map_solved) return set_error(GBP_ESTATE, "GBP_LIN_TRACE_MAP: call gbp_lin_solve_map first");
    gbp_lin_until_info_t out{0, 0, GBP_LIN_STOP_NONE, 0};
    if (o.max_iters == 0) {
        if (info) *info = out;
        return GBP_OK;
    }
    LCHK(lin_until_workspace(h, o.max_iters));
    const LinUntil &u = h->until;
    const UntilRule rule{o.want, o.tol_step, o.tol_map};
    LHIPCHK(hipMemsetAsync(u.stop, 0, 2 * sizeof(int), h->stream));
    if (o.robustify) h->map_ready = false;                 // the joint is that of the new weights (as gbp_lin_robustify)
    int it = 0, stop[2] = {0, 0};
    while (it < o.max_iters && !stop[0]) {
        const int n = std::min(o.check_every, o.max_iters - it);
        for (int j = 0; j < n; ++j, ++it) LCHK(until_sweep(h, o, rule, it));
        LHIPCHK(hipMemcpyAsync(stop, u.stop, sizeof(stop), hipMemcpyDeviceToHost, h->stream));
        LHIPCHK(hipStreamSynchronize(h->stream));
    }
    out.iters = stop[0] ? stop[1] : it;
    out.converged = stop[0] ? 1 : 0;
    out.reason = stop[0];
    if (trace) {
        LHIPCHK(hipMemcpyAsync(trace, u.trace, (size_t)out.iters * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        LHIPCHK(hipStreamSynchronize(h->stream));
    }
    if (info) *info = out;
    return GBP_OK;
}

int gbp_lin_get_alloc_count(gbp_lin_t *h, int32_t *count)
{
    LENTER(h);
    if (!count) return set_error(GBP_EINVAL, "count is NULL");
    *count = (int32_t)h->allocs.size();
    return GBP_OK;
}

}  // extern "C"
