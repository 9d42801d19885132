// gbp_lin_robust.hpp -- robust (Huber / constant) losses of the linear engine on gfx950: Factor.robustify_loss (gbp.py:296-332) and
// FactorGraph.robustify_all_factors / synchronous_iteration(robustify=True) (gbp.py:82-92) for linear pairwise factors.
//
// A robust factor is the NOMINAL factor (eta_f, Lambda_f, const_f) times one scalar weight w_f = sigma_f^2 / adaptive_gauss_noise_var,
// re-made from the current belief means:
//   M_f^2 = 2 (0.5 x^T Lambda_f x - eta_f^T x + const_f) = |h(x) - z|^2 / sigma_f^2                 (gbp.py:312, 322)
//   huber    : w_f = (2 t M - t^2) / M^2 if M > t, else 1                                              (gbp.py:313-319)
//   constant : w_f = sigma_f^2 / M^2     if M > t, else 1    (the reference sets the adaptive variance to M^2, gbp.py:323-328)
// The weight multiplies the stored nominal factor wherever (eta_f, Lambda_f) is used -- the sweep (k_lin_factor<D, true>), the energy
// (sum w_f e_f, gbp.py:43) and the joint of the batch MAP and of the marginals -- where the reference rescales the factor in place by
// old / new (gbp.py:331-332); the two differ by rounding only.
// DEPARTURE: the reference evaluates h at Factor.linpoint (gbp.py:309), which a linear factor never moves after compute_all_factors();
// here M is taken at the current belief means, which is the reference's own arithmetic with linpoint set to the adjacent belief means
// before each robustify.
//   lin_factor_energy<D>  the per-factor energy e_f in the cancellation-free residual form (a pivoted LDL^T of Lambda_f), shared by
//                         k_lin_energy, k_lin_robustify and the host shim (tests/hostmath/lin_robust_shim.hip);
//   k_lin_robustify<D, PT>  one lane per factor: M^2 = 2 e_f, then w_f and the flag, plain vector stores; PT = LinGated
//                         (gbp_lin_handle.hpp): gated on the stop word of gbp_lin_iterate_until.
#pragma once
#include "gbp_lin_handle.hpp"
#include "gbp_math.hpp"

namespace gbp {

// 0.5 |h(mu) - z|^2 / sigma^2 of factor f for linear h (gbp.py:36-44, 251-265), from (Lambda_f, eta_f, const) and the belief means of
// its two variables, without the cancellation of the expanded 0.5 x^T Lambda_f x - eta_f^T x + const (terms of |x|^2 / sigma^2 that
// cancel to the residual: map coordinates with centimetre noise lose every digit).  A pivoted LDL^T of Lambda_f, stopped at a relative
// pivot tolerance (a factor has rank m <= 2d), writes Lambda_f = sum_k d_k l_k l_k^T and eta_f = sum_k d_k y_k l_k, so the energy is
//   0.5 sum_k d_k (l_k^T x - y_k)^2 + (const - 0.5 sum_k d_k y_k^2)
// whose squares are of residuals.  For linear_displacement (Lambda_f = [I -I; -I I] / sigma^2) l_k^T x = x_a - x_b exactly.
template <int D>
GBP_HD double lin_factor_energy(const LinParams &p, int f)
{
    constexpr int P = LinDims<D>::P, REC = LinDims<D>::REC, N2 = 2 * D;
    const size_t F = (size_t)p.F;
    double x[N2], eta[N2], a[Sym<N2>::size];
    const double *ra = p.bel + (size_t)p.va[f] * REC + D + P, *rb = p.bel + (size_t)p.vb[f] * REC + D + P;
#pragma unroll
    for (int k = 0; k < D; ++k) { x[k] = ra[k]; x[D + k] = rb[k]; }
#pragma unroll
    for (int i = 0; i < N2; ++i) eta[i] = p.feta[i * F + f];
#pragma unroll
    for (int i = 0; i < Sym<N2>::size; ++i) a[i] = p.flam[(size_t)i * F + f];
    double amax = 0.0;
#pragma unroll
    for (int i = 0; i < N2; ++i) amax = fmax(amax, a[Sym<N2>::at(i, i)]);
    const double tol = N2 * 64 * __DBL_EPSILON__ * amax;
    double cst = p.fconst ? p.fconst[f] : 0.0, sq = 0.0;
    int done = 0;                                         // bit i: index i already eliminated
#pragma unroll 1
    for (int step = 0; step < N2; ++step) {
        int piv = -1;
        double dk = tol;
#pragma unroll
        for (int i = 0; i < N2; ++i)
            if (!((done >> i) & 1) && a[Sym<N2>::at(i, i)] > dk) { dk = a[Sym<N2>::at(i, i)]; piv = i; }
        if (piv < 0) break;                               // the rest of Lambda_f is rounding: rank reached
        // column piv over the live indices (register arrays: selected, never indexed by piv)
        double col[N2], raw[N2], zk = 0.0, lx = 0.0;
#pragma unroll
        for (int i = 0; i < N2; ++i) {
            double c = 0.0;
#pragma unroll
            for (int j = 0; j < N2; ++j)
                if (j == piv) c = a[Sym<N2>::at(i < j ? i : j, i < j ? j : i)];
            const bool live = !((done >> i) & 1) && i != piv;
            raw[i] = live ? c : 0.0;
            col[i] = live ? c / dk : 0.0;                 // l_k (exactly -1 / 0 for a displacement factor)
            if (i == piv) { zk = eta[i]; lx = x[i]; }
        }
#pragma unroll
        for (int i = 0; i < N2; ++i) lx += col[i] * x[i];
        const double yk = zk / dk, t = lx - yk;
        sq += 0.5 * dk * t * t;
        cst -= 0.5 * zk * yk;
#pragma unroll
        for (int i = 0; i < N2; ++i) {
            eta[i] -= col[i] * zk;
#pragma unroll
            for (int j = i; j < N2; ++j) a[Sym<N2>::at(i, j)] -= col[i] * raw[j];
        }
        done |= 1 << piv;
    }
    return cst + sq;
}

// w_f and robust_flag_f from M^2 = 2 e_f (gbp.py:311-328); nvar is read for the constant loss only.  M^2 <= 0 (rounding at a
// residual of zero) is M = 0: never above a positive threshold.
GBP_HD double lin_robust_weight(int loss, double thr, double nvar, double e, int &flag)
{
    const double m2 = e > 0.0 ? 2.0 * e : 0.0, m = sqrt(m2);
    flag = (loss != GBP_LIN_LOSS_NONE && m > thr) ? 1 : 0;
    if (!flag) return 1.0;
    return loss == GBP_LIN_LOSS_HUBER ? (2.0 * thr * m - thr * thr) / m2 : nvar / m2;
}

// Factor.robustify_loss (gbp.py:296-332) of factor f at the current belief means
template <int D>
GBP_HD void lin_robustify_one(const LinParams &p, const LinRobust &r, int f)
{
    int flag = 0;
    const int loss = r.loss[f];
    double w = 1.0;
    if (loss != GBP_LIN_LOSS_NONE) w = lin_robust_weight(loss, r.thr[f], r.nvar[f], lin_factor_energy<D>(p, f), flag);
    r.w[f] = w;
    r.flag[f] = flag;
}

template <int D, typename PT = LinParams>
__global__ __launch_bounds__(256) void k_lin_robustify(PT p, LinRobust r)
{
    if (lin_stopped(p)) return;                           // PT = LinParams: never
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < p.F) lin_robustify_one<D>(p, r, f);
}

}  // namespace gbp
