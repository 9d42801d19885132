// gbp_lin_until.hpp -- what belongs to gbp_lin_iterate_until alone on gfx950: the loop of ndim_posegraph.py:104-108 (synchronous_iteration
// gbp.py:86-92, then energy() gbp.py:36-44 and |get_means() - mu| gbp.py:146-153) with the decision "stop" taken on the device.
//
// A sweep of the call is the sweep of gbp_lin_iterate (or gbp_lin_iterate_robust): the SAME stage kernels (gbp_lin_sweep.hpp,
// gbp_lin_robust.hpp), instantiated with the parameter blocks of gbp_lin_handle.hpp that gate them -- each reads the call's stop word at
// its head and returns once it is set, so the sweeps queued behind the deciding one change nothing -- and, for the belief stage, trace
// it, so that no second pass over the beliefs is needed.  There is one text of the belief, factor, energy and robustify arithmetic: the
// state after the deciding sweep s is bit for bit that of gbp_lin_iterate(h, s) by construction.  What is here:
//   until_var, until_max     what the traced belief stage adds per variable: max_k |mu_new - mu_old| and, when asked, sum_k (mu_new - x)^2
//                            against the iterate of the last gbp_lin_solve_map;
//   k_until_finish           one block: max of the step partials, fixed-order sums of the others (strided per thread, then a fixed
//                            tree), row i of the device trace, and the stop word when an enabled tolerance is met;
//   until_row_settled        the decision of gbp_lin_iterate_until_nonlinear (gbp_lin_capi_until_nonlin.hip), whose sweeps are those of
//                            gbp_lin_iterate_nonlinear[_robust] in gated forms: a sweep that relinearised anything may be made to decide nothing.
// A maximum does not depend on the order it is taken in, so the step is exact; the two sums are added in a fixed order.  No
// floating-point atomics.
// The per-variable and finishing arithmetic are host/device routines (tests/hostmath/lin_until_shim.hip runs them on a CPU).
#pragma once
#include "gbp_lin_handle.hpp"

namespace gbp {

constexpr int UNTIL_FIN = 1024;      // threads of the finishing block

// what the finishing kernel needs of gbp_lin_until_opts_t
struct UntilRule {
    int want;                        // GBP_LIN_TRACE_*
    double tol_step, tol_map;        // 0: off
};

// ---- per-variable and finishing routines (host and device) -------------------------------------------------------------------------

// max(a, b) of two magnitudes; a NaN on either side stays (fmax would drop it, numpy's max keeps it)
GBP_HD double until_max(double a, double b) { return (b > a || b != b) ? b : a; }

// step = max_k |mu_new[k] - mu_old[k]|; sq = sum_k (mu_new[k] - x[k])^2, 0 for x == nullptr
template <int D>
GBP_HD void until_var(const double (&mu)[D], const double *old, const double *x, double &step, double &sq)
{
    step = 0.0; sq = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) step = until_max(step, fabs(mu[k] - old[k]));
    if (x) {
#pragma unroll
        for (int k = 0; k < D; ++k) { const double d = mu[k] - x[k]; sq += d * d; }
    }
}

// thread t of T: its share of n partials, in index order.  One block reads all of them, so the loop is bound by load latency: eight
// loads are issued before the first is used; the values are still combined one after the other in index order.
GBP_HD double until_strided_max(const double *part, int n, int t, int T)
{
    double a = 0.0;
    int i = t;
    for (; (long long)i + 7LL * T < n; i += 8 * T) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = part[i + j * T];
#pragma unroll
        for (int j = 0; j < 8; ++j) a = until_max(a, v[j]);
    }
    for (; i < n; i += T) a = until_max(a, part[i]);
    return a;
}
GBP_HD double until_strided_sum(const double *part, int n, int t, int T)
{
    double a = 0.0;
    int i = t;
    for (; (long long)i + 7LL * T < n; i += 8 * T) {
        double v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = part[i + j * T];
#pragma unroll
        for (int j = 0; j < 8; ++j) a += v[j];
    }
    for (; i < n; i += T) a += part[i];
    return a;
}

// one level of the fixed tree over the three columns of per-thread values: slot t takes in slot t + s (for every t < s, then s halves)
GBP_HD void until_fold(double *step, double *sq, double *en, int t, int s)
{
    step[t] = until_max(step[t], step[t + s]);
    sq[t] += sq[t + s];
    en[t] += en[t + s];
}

// row (step, energy, MAP distance) from the three reduced values -- NaN where a column was not asked for -- and the decision:
// STEP is tested before MAP
GBP_HD int until_row(const UntilRule &r, double step, double sq, double en, double *row)
{
    const double dist = sqrt(sq);
    row[0] = step;
    row[1] = (r.want & GBP_LIN_TRACE_ENERGY) ? en : __builtin_nan("");
    row[2] = (r.want & GBP_LIN_TRACE_MAP) ? dist : __builtin_nan("");
    if (r.tol_step > 0.0 && step <= r.tol_step) return GBP_LIN_STOP_STEP;
    if (r.tol_map > 0.0 && (r.want & GBP_LIN_TRACE_MAP) && dist <= r.tol_map) return GBP_LIN_STOP_MAP;
    return GBP_LIN_STOP_NONE;
}

// the same row, and the decision of gbp_lin_iterate_until_nonlinear: with GBP_LIN_UNTIL_SETTLED in r.want a sweep in which any factor
// relinearised (*count != 0, the sweep's slot of the relinearisation counts) decides nothing -- neither STEP nor MAP.  count == nullptr
// or the bit clear: row and decision are until_row's.
GBP_HD int until_row_settled(const UntilRule &r, const int *count, double step, double sq, double en, double *row)
{
    const int reason = until_row(r, step, sq, en, row);
    if ((r.want & GBP_LIN_UNTIL_SETTLED) && count && *count != 0) return GBP_LIN_STOP_NONE;
    return reason;
}

// the rule of gbp_lin_iterate_until_nonlinear: UntilRule and where the finishing kernel finds the sweep's relinearisation count
struct UntilSettled : UntilRule {
    const int *count;                // device: the slot of sweep `it` (LinNonlin::counts + it); complete when the finishing kernel runs,
                                     // which the stream orders behind the relinearise kernel that adds to it
};
GBP_HD int until_decide(const UntilRule &r, double step, double sq, double en, double *row) { return until_row(r, step, sq, en, row); }
GBP_HD int until_decide(const UntilSettled &r, double step, double sq, double en, double *row) { return until_row_settled(r, r.count, step, sq, en, row); }

// ---- the finishing kernel --------------------------------------------------------------------------------------------------------

// one block after sweep `it` + 1 of the call: row `it` of the trace, and the stop word.  Without variables (factors) there are no
// partials: the step (the energy) is 0.  T = UNTIL_FIN threads (a template, so that a host-only build of this header has no kernel).
// RT = UntilRule: the linear call's; RT = UntilSettled: the decision also reads the sweep's relinearisation count.
template <int T, typename RT = UntilRule>
__global__ __launch_bounds__(T) void k_until_finish(LinUntil u, RT r, int it)
{
    __shared__ double red[3][T];
    if (u.stop[0]) return;
    const int t = threadIdx.x;
    red[0][t] = until_strided_max(u.bel_part, u.nbel, t, T);
    red[1][t] = (r.want & GBP_LIN_TRACE_MAP) ? until_strided_sum(u.bel_part + u.nbel, u.nbel, t, T) : 0.0;
    red[2][t] = (r.want & GBP_LIN_TRACE_ENERGY) ? until_strided_sum(u.en_part, u.nen, t, T) : 0.0;
    __syncthreads();
    for (int s = T / 2; s > 0; s >>= 1) {
        if (t < s) until_fold(red[0], red[1], red[2], t, s);
        __syncthreads();
    }
    if (t == 0) {
        const int reason = until_decide(r, red[0][0], red[1][0], red[2][0], u.trace + (size_t)it * 3);
        if (reason != GBP_LIN_STOP_NONE) { u.stop[1] = it + 1; u.stop[0] = reason; }
    }
}

}  // namespace gbp
