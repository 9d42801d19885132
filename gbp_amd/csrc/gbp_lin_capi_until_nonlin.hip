// gbp_lin_capi_until_nonlin.hip -- gbp_lin_iterate_until_nonlinear of include/gbp_lin.h: the loop
//   for i in range(n): graph.synchronous_iteration(local_relin=True[, robustify=True]); graph.energy(); norm(graph.get_means() - mu)
// (gbp.py:86-92, 36-44, 146-153) on a handle with nonlinear factors, in one call, the decision to stop taken on the device.
//
// The pattern is gbp_lin_iterate_until's (gbp_lin_capi_until.hip), with the sweep of gbp_lin_iterate_nonlinear[_robust]: every stage is
// the kernel text that call launches, instantiated with the parameter block that gates it --
//   k_lin_relin<MODEL, ROBUST, LinGated>      relinearise (with losses and robustify: the fused robustify + relinearise lane), counted into
//                                             the handle's own count buffers; a gated launch writes nothing and adds to no count;
//   k_lin_factor<D, ROBUST, LinRelinGated>    per-factor damping and the stop word in one block;
//   k_lin_belief<D, LinTraced>                gated, with the step and the squared MAP distance of its block;
//   k_lin_energy_nl<MODEL, LinGated>          when the energy is traced, into the call's own partials;
//   k_until_finish<UNTIL_FIN, UntilSettled>   the row, and the decision, which under GBP_LIN_UNTIL_SETTLED reads the sweep's count slot.
// Sweeps are queued check_every at a time; the host reads the stop word (8 bytes) after each batch; trace and counts are copied out once,
// and only the `iters` entries that were written.  The workspace is LinUntil, shared with the linear call.
#include "gbp_lin_nonlin.hpp"
#include "gbp_lin_sweep.hpp"

#include <cmath>

using namespace gbp;

namespace {

constexpr int KNOWN_WANT = GBP_LIN_TRACE_ENERGY | GBP_LIN_TRACE_MAP | GBP_LIN_UNTIL_SETTLED;

bool tol_ok(double t) { return t >= 0.0 && std::isfinite(t); }

// sweep `it` + 1 of the call: every kernel gated on the stop word
template <int MODEL>
int until_nl_sweep(gbp_lin *h, const gbp_lin_until_opts_t &o, const UntilSettled &rule, int it)
{
    constexpr int D = NonlinModel<MODEL>::D;
    const LinUntil &u = h->until;
    const LinNonlin &nl = h->nl;
    const LinGated g{h->p, u.stop};
    const LinTraced t{h->p, u, (o.want & GBP_LIN_TRACE_MAP) ? h->map.x : nullptr};
    if (h->p.F) {
        const dim3 lanes((h->p.F + 255) / 256), waves((h->p.F + 63) / 64);
        if (o.robustify) hipLaunchKernelGGL((k_lin_relin<MODEL, true, LinGated>), lanes, dim3(256), 0, h->stream, g, nl, NL_SWEEP, nl.counts + it, h->rob, nl.rcounts + it);
        else hipLaunchKernelGGL((k_lin_relin<MODEL, false, LinGated>), lanes, dim3(256), 0, h->stream, g, nl, NL_SWEEP, nl.counts + it, LinRobust{}, (int *)nullptr);
        const LinRelinGated r{{h->p, nl.fdamp}, u.stop};
        if (h->p.w) hipLaunchKernelGGL((k_lin_factor<D, true, LinRelinGated>), waves, dim3(64), 0, h->stream, r);
        else hipLaunchKernelGGL((k_lin_factor<D, false, LinRelinGated>), waves, dim3(64), 0, h->stream, r);
    }
    if (h->p.N) hipLaunchKernelGGL((k_lin_belief<D, LinTraced>), dim3(u.nbel), dim3(64), 0, h->stream, t);
    if (h->p.F && (o.want & GBP_LIN_TRACE_ENERGY)) hipLaunchKernelGGL((k_lin_energy_nl<MODEL, LinGated>), dim3(u.nen), dim3(256), 0, h->stream, g, nl, u.en_part);
    UntilSettled r = rule;
    r.count = nl.counts + it;
    hipLaunchKernelGGL((k_until_finish<UNTIL_FIN, UntilSettled>), dim3(1), dim3(UNTIL_FIN), 0, h->stream, u, r, it);
    LHIPCHK(hipGetLastError());
    return GBP_OK;
}

}  // namespace

extern "C" {

int gbp_lin_iterate_until_nonlinear(gbp_lin_t *h, const gbp_lin_until_opts_t *opts, double *trace, int32_t *relin_counts, int32_t *robust_counts,
                                    gbp_lin_until_info_t *info)
{
    LENTER(h);
    if (!h->nonlinear) return set_error(GBP_ESTATE, "the handle has no nonlinear factors: call gbp_lin_set_nonlinear first, or gbp_lin_iterate_until");
    if (!opts) return set_error(GBP_EINVAL, "opts is NULL");
    const gbp_lin_until_opts_t o = *opts;
    if (o.max_iters < 0) return set_error(GBP_EINVAL, "negative max_iters");
    if (o.check_every < 1) return set_error(GBP_EINVAL, "check_every must be at least 1");
    if (o.robustify != 0 && o.robustify != 1) return set_error(GBP_EINVAL, "robustify must be 0 or 1");
    if (o.want & ~KNOWN_WANT) return set_error(GBP_EINVAL, "unknown bits in want: 0x%x", (unsigned)(o.want & ~KNOWN_WANT));
    if (!tol_ok(o.tol_step) || !tol_ok(o.tol_map)) return set_error(GBP_EINVAL, "a tolerance must be finite and not negative (0: off)");
    if (o.tol_map > 0.0 && !(o.want & GBP_LIN_TRACE_MAP)) return set_error(GBP_EINVAL, "tol_map needs GBP_LIN_TRACE_MAP in want");
    if (robust_counts && !o.robustify) return set_error(GBP_EINVAL, "robust_counts must be NULL when robustify is 0");
    if (o.robustify && !h->p.w) return set_error(GBP_ESTATE, "no losses set: call gbp_lin_set_robust_nonlinear first");
    if ((o.want & GBP_LIN_TRACE_MAP) && !h->map_solved) return set_error(GBP_ESTATE, "GBP_LIN_TRACE_MAP: call gbp_lin_solve_map first");
    gbp_lin_until_info_t out{0, 0, GBP_LIN_STOP_NONE, 0};
    if (o.max_iters == 0) {
        if (info) *info = out;
        return GBP_OK;
    }
    LCHK(lin_until_workspace(h, o.max_iters));
    LCHK(lin_nonlin_grow_counts(h, h->nl.counts, h->nl.cap, o.max_iters));
    if (o.robustify) LCHK(lin_nonlin_grow_counts(h, h->nl.rcounts, h->nl.rcap, o.max_iters));
    const LinUntil &u = h->until;
    const LinNonlin &nl = h->nl;
    UntilSettled rule;
    rule.want = o.want; rule.tol_step = o.tol_step; rule.tol_map = o.tol_map; rule.count = nullptr;
    LHIPCHK(hipMemsetAsync(u.stop, 0, 2 * sizeof(int), h->stream));
    LHIPCHK(hipMemsetAsync(nl.counts, 0, (size_t)o.max_iters * sizeof(int), h->stream));
    if (o.robustify) LHIPCHK(hipMemsetAsync(nl.rcounts, 0, (size_t)o.max_iters * sizeof(int), h->stream));
    h->map_ready = false;                                   // the joint is that of the new linearisation point (and weights)
    int it = 0, stop[2] = {0, 0};
    while (it < o.max_iters && !stop[0]) {
        const int n = std::min(o.check_every, o.max_iters - it);
        for (int j = 0; j < n; ++j, ++it) {
            int rc = GBP_OK;
            lin_model_dispatch(nl.model, [&](auto m) { rc = until_nl_sweep<decltype(m)::value>(h, o, rule, it); });
            LCHK(rc);
        }
        LHIPCHK(hipMemcpyAsync(stop, u.stop, sizeof(stop), hipMemcpyDeviceToHost, h->stream));
        LHIPCHK(hipStreamSynchronize(h->stream));
    }
    out.iters = stop[0] ? stop[1] : it;
    out.converged = stop[0] ? 1 : 0;
    out.reason = stop[0];
    if (trace) LHIPCHK(hipMemcpyAsync(trace, u.trace, (size_t)out.iters * 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (relin_counts) LHIPCHK(hipMemcpyAsync(relin_counts, nl.counts, (size_t)out.iters * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (robust_counts) LHIPCHK(hipMemcpyAsync(robust_counts, nl.rcounts, (size_t)out.iters * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (trace || relin_counts || robust_counts) LHIPCHK(hipStreamSynchronize(h->stream));
    if (info) *info = out;
    return GBP_OK;
}

}  // extern "C"
