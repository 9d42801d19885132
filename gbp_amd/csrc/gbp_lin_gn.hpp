// gbp_lin_gn.hpp -- what gbp_lin_solve_map_nonlinear (include/gbp_lin.h) adds around the conjugate gradients of gbp_lin_map.hpp: the
// nonlinear batch MAP of a handle with SE(2) / SE(3) factors by Levenberg-Marquardt, every array on the device.
//
// One outer iteration at (x, lambda) -- x is a point [N][D] of the solver's own, not the belief means:
//   k_gn_factor<MODEL, true>    one lane per factor: eta_f, Lambda_f at [x_a; x_b] into the SOLVER's [2D][F] / [P2][F] arrays, with the
//                               model code the relinearise lane runs (nonlin_factor; SE(3): factor_store at stride F), and the block's
//                               partial of sum_f w_f 0.5 |h(x) - diag(s) z|^2 (h(x) is computed anyway);
//   k_gn_damp<D>                one lane per variable: the damped copy of the prior, Lambda0_v + lambda diag(D_v) and
//                               eta0_v + lambda diag(D_v) x_v, D_v the joint's diagonal block at x in the order of map_var_setup, each
//                               diagonal entry floored at GN_DIAG_FLOOR;
//   the kernels of gbp_lin_map.hpp, unchanged, on a LinParams whose feta / flam / prior point at those three arrays, started at x: the
//   first true residual is eta - Lambda x = -grad Phi(x) whatever lambda is;
//   k_gn_factor<MODEL, false>   the energy-only instantiation at the candidate x_c;
//   k_gn_diff<D>                one lane per variable: the prior's part of Phi(x_c) - Phi(x) in difference form,
//                               (x_c - x)_v^T (Lambda0_v (x_c + x)_v / 2 - eta0_v), which does not cancel far from the origin, and
//                               max |x_c - x|; per-block partials;
//   k_gn_finish                 ONE block: the partials added in a fixed order (strided per thread, then the tree of map_block_sum) into
//                               four doubles, which is all the host downloads to decide.
// gbp_lin_solve_map_nonlinear_robust (gbp_lin_capi_map_irls.hip) runs that loop (gn_lm) inside rounds of re-made weights:
//   k_gn_reweight<MODEL>        one lane per factor: k_gn_factor<MODEL, true>'s linearisation and energy at x, and from the same M_f the
//                               weight and flag of Factor.robustify_loss into the SOLVER's w / flag arrays; per-block partials of the
//                               weighted energy and of max |w_new - w_old|, the flagged factors counted by one integer add per wave;
//   k_gn_reweight_finish        ONE block: those partials, the count and the last round's max |x_end - x_start| into four doubles.
// No floating-point atomics anywhere: two identical call sequences on two handles are bit-identical.
// The per-factor and per-variable routines are host/device functions, so that the same code runs in plain loops on a CPU
// (tests/hostmath/lin_gn_shim.hip); the kernels are thin wrappers.
#pragma once
#include "gbp_lin_map.hpp"
#include "gbp_lin_nonlin.hpp"

namespace gbp {

constexpr double GN_DIAG_FLOOR = 1e-12;                    // the least a diagonal entry of D_v counts for in the damping
constexpr int GN_OUT = 4;                                  // what k_gn_finish leaves: E(x), E(x_c), the prior difference, max |x_c - x|
constexpr int GN_RW_OUT = 4;                               // what k_gn_reweight_finish leaves: E_w(x), max |w_new - w_old|, flagged, max |x_end - x_start|

// ---- per-factor / per-variable routines (host and device) --------------------------------------------------------------------------

// eta_f and Lambda_f (packed upper) of factor f at the point pt = [x_a; x_b] into feta [2D][F] / flam [P2][F]: the entries and the stores
// of the relinearise lane (lin_relin_one, gbp_lin_nonlin.hpp)
template <int MODEL>
GBP_HD void gn_linearise(const double (&pt)[2 * NonlinModel<MODEL>::D], const double (&z)[NonlinModel<MODEL>::M], const double (&s)[NonlinModel<MODEL>::M], int f, size_t F,
                         double *feta, double *flam)
{
    if constexpr (NonlinModel<MODEL>::dense) {
        double eta[6], lam[Sym<6>::size];
        nonlin_factor<MODEL>(pt, z, s, eta, lam);
#pragma unroll
        for (int k = 0; k < 6; ++k) feta[k * F + f] = eta[k];
#pragma unroll
        for (int k = 0; k < Sym<6>::size; ++k) flam[(size_t)k * F + f] = lam[k];
    } else {
        NonlinModel<MODEL>::factor_store(pt, z, s, feta + f, flam + f, F);
    }
}

// Factor f at the point x [N][D]: with LIN, eta_f and Lambda_f (packed upper) at [x_a; x_b] into feta [2D][F] / flam [P2][F] -- the
// entries and the stores of the relinearise lane (lin_relin_one, gbp_lin_nonlin.hpp) --; returns w_f 0.5 |h(x) - diag(s) z|^2.
template <int MODEL, bool LIN>
GBP_HD double gn_factor_at(const LinParams &p, const LinNonlin &n, int f, const double *x, double *feta, double *flam)
{
    constexpr int D = NonlinModel<MODEL>::D, M = NonlinModel<MODEL>::M;
    const size_t F = (size_t)p.F;
    const double *xa = x + (size_t)p.va[f] * D, *xb = x + (size_t)p.vb[f] * D;
    double pt[2 * D], z[M], s[M];
#pragma unroll
    for (int k = 0; k < D; ++k) { pt[k] = xa[k]; pt[D + k] = xb[k]; }
#pragma unroll
    for (int k = 0; k < M; ++k) { z[k] = n.meas[k * F + f]; s[k] = n.sinfo[k * F + f]; }
    if constexpr (LIN) gn_linearise<MODEL>(pt, z, s, f, F, feta, flam);
    double e = nonlin_energy<MODEL>(pt, z, s);
    if (p.w) e *= p.w[f];                                   // the weights as they stand (gbp.py:43)
    return e;
}

// The reweight lane of gbp_lin_solve_map_nonlinear_robust for factor f at the solver's x: x_a, x_b, z, s loaded once; h(x) evaluated ONCE
// for M_f^2 = |diag(s) z - h(x)|^2, which gives the weight and the flag (lin_robust_weight at noise variance 1, Factor.robustify_loss
// gbp.py:296-332 with the linpoint at x) and the weighted energy; w[f] and flag[f] stored -- arrays of the SOLVER's, never LinRobust's --;
// then the linearisation at x with the stores of gn_factor_at<MODEL, true>.  loss == nullptr (no losses set) or a factor at NONE: weight
// 1, flag 0, threshold not loaded.  Returns w_f 0.5 M_f^2; change = |w_f - the weight w[f] held| (0 when `first`: nothing is loaded),
// flagged = the flag.
template <int MODEL>
GBP_HD double gn_reweight_at(const LinParams &p, const LinNonlin &n, const int *loss, const double *thr, int f, const double *x, bool first, double *feta, double *flam,
                             double *w, int *flag, double &change, int &flagged)
{
    constexpr int D = NonlinModel<MODEL>::D, M = NonlinModel<MODEL>::M;
    const size_t F = (size_t)p.F;
    const double *xa = x + (size_t)p.va[f] * D, *xb = x + (size_t)p.vb[f] * D;
    double pt[2 * D], z[M], s[M];
#pragma unroll
    for (int k = 0; k < D; ++k) { pt[k] = xa[k]; pt[D + k] = xb[k]; }
#pragma unroll
    for (int k = 0; k < M; ++k) { z[k] = n.meas[k * F + f]; s[k] = n.sinfo[k * F + f]; }
    // the linearisation and then the energy, in the order and with the calls of gn_factor_at<MODEL, true>: the compiler fuses
    // multiply-adds by context, and only the same context gives that kernel's bits (a handle without losses must reproduce
    // gbp_lin_solve_map_nonlinear bit for bit)
    gn_linearise<MODEL>(pt, z, s, f, F, feta, flam);
    const double e = nonlin_energy<MODEL>(pt, z, s);       // 0.5 M^2: the one evaluation of h beside the linearisation's
    const int ls = loss ? loss[f] : GBP_LIN_LOSS_NONE;
    double wf = 1.0;
    flagged = 0;
    if (ls != GBP_LIN_LOSS_NONE) wf = lin_robust_weight(ls, thr[f], 1.0, e, flagged);
    change = first ? 0.0 : fabs(wf - w[f]);
    w[f] = wf;
    flag[f] = flagged;
    return e * wf;
}

// The damped prior of variable v: D_v's diagonal = prior Lambda_v's + the own diagonal entries of the factors of its adjacency run
// (times their weights), added in the order of map_var_setup; each entry floored; dprior[v] = (eta0 + lambda d x_v | Lambda0 with
// lambda d added to its diagonal).  p.flam is the linearisation at x, p.prior the handle's prior.
template <int D>
GBP_HD void gn_var_damp(const LinParams &p, int v, const double *x, double lambda, double *dprior)
{
    constexpr int P = LinDims<D>::P, R = D + P;
    const size_t F = (size_t)p.F;
    double d[D];
#pragma unroll
    for (int k = 0; k < D; ++k) d[k] = p.prior[(size_t)v * R + D + Sym<D>::at(k, k)];
    for (int ed = p.vptr[v]; ed < p.vptr[v + 1]; ++ed) {
        const int f = p.vadj[ed] >> 1, o = (p.vadj[ed] & 1) * D;
        const double w = p.w ? p.w[f] : 1.0;
#pragma unroll
        for (int k = 0; k < D; ++k) d[k] += w * p.flam[(size_t)Sym<2 * D>::at(o + k, o + k) * F + f];
    }
#pragma unroll
    for (int k = 0; k < P; ++k) dprior[(size_t)v * R + D + k] = p.prior[(size_t)v * R + D + k];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double ld = lambda * (d[k] > GN_DIAG_FLOOR ? d[k] : GN_DIAG_FLOOR);
        dprior[(size_t)v * R + k] = p.prior[(size_t)v * R + k] + ld * x[(size_t)v * D + k];
        dprior[(size_t)v * R + D + Sym<D>::at(k, k)] = p.prior[(size_t)v * R + D + Sym<D>::at(k, k)] + ld;
    }
}

// The prior's part of Phi(xc) - Phi(x) for variable v, (xc - x)^T (Lambda0 (xc + x) / 2 - eta0); mx takes max |xc - x| (a NaN
// difference makes it NaN: the host then rejects)
template <int D>
GBP_HD double gn_var_diff(const double *prior, int v, const double *x, const double *xc, double &mx)
{
    constexpr int P = LinDims<D>::P, R = D + P;
    double d[D], m[D], y[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double a = x[(size_t)v * D + k], c = xc[(size_t)v * D + k];
        d[k] = c - a; m[k] = 0.5 * (c + a); y[k] = -prior[(size_t)v * R + k];
        const double ad = fabs(d[k]);
        mx = (ad > mx || ad != ad) ? ad : mx;
    }
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
        for (int j = i; j < D; ++j) {
            const double a = prior[(size_t)v * R + D + Sym<D>::at(i, j)];
            y[i] += a * m[j];
            if (j != i) y[j] += a * m[i];
        }
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) s += d[k] * y[k];
    return s;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------

// One lane per factor, in the block / partials shape of k_lin_energy_nl.  Lanes past F neither load nor store.
template <int MODEL, bool LIN>
__global__ __launch_bounds__(256) void k_gn_factor(LinParams p, LinNonlin n, const double *x, double *feta, double *flam, double *e_part)
{
    __shared__ double red[256 / 64];
    const int f = blockIdx.x * 256 + threadIdx.x;
    double e = 0.0;
    if (f < p.F) e = gn_factor_at<MODEL, LIN>(p, n, f, x, feta, flam);
    e = map_block_sum(e, red);
    if (threadIdx.x == 0) e_part[blockIdx.x] = e;
}

template <int D>
__global__ __launch_bounds__(MAP_BLOCK) void k_gn_damp(LinParams p, const double *x, double lambda, double *dprior)
{
    for (long long v = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; v < p.N; v += (long long)gridDim.x * MAP_BLOCK)
        gn_var_damp<D>(p, (int)v, x, lambda, dprior);
}

// part[0 .. nb): the prior differences, part[nb .. 2 nb): the maxima
template <int D>
__global__ __launch_bounds__(MAP_BLOCK) void k_gn_diff(const double *prior, int N, const double *x, const double *xc, double *part, int nb)
{
    __shared__ double red[MAP_BLOCK / 64];
    double acc = 0.0, mx = 0.0;
    for (long long v = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; v < N; v += (long long)gridDim.x * MAP_BLOCK)
        acc += gn_var_diff<D>(prior, (int)v, x, xc, mx);
    acc = map_block_sum(acc, red);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_down(mx, off, 64); mx = (o > mx || o != o) ? o : mx; }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < MAP_BLOCK / 64; ++k) mx = (red[k] > mx || red[k] != red[k]) ? red[k] : mx;
        part[blockIdx.x] = acc;
        part[nb + blockIdx.x] = mx;
    }
}

// ONE block of MAP_BLOCK threads: out = (sum e_x[0 .. nen), sum e_c[0 .. nen), sum part[0 .. nb), max part[nb .. 2 nb)).  A template like
// every kernel a header of the engine holds, so that a host-only build of the header (the shim) instantiates none.
template <int OUT>
__global__ __launch_bounds__(MAP_BLOCK) void k_gn_finish(const double *e_x, const double *e_c, int nen, const double *part, int nb, double *out)
{
    __shared__ double red[MAP_BLOCK / 64];
    const double ex = map_sum_partials(e_x, nen, red), ec = map_sum_partials(e_c, nen, red), dp = map_sum_partials(part, nb, red);
    double mx = 0.0;
    for (int i = threadIdx.x; i < nb; i += MAP_BLOCK) { const double o = part[nb + i]; mx = (o > mx || o != o) ? o : mx; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_down(mx, off, 64); mx = (o > mx || o != o) ? o : mx; }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < MAP_BLOCK / 64; ++k) mx = (red[k] > mx || red[k] != red[k]) ? red[k] : mx;
        static_assert(OUT == 4, "E(x), E(x_c), the prior difference, max |x_c - x|");
        out[0] = ex; out[1] = ec; out[2] = dp; out[3] = mx;
    }
}

// The reweight lane over every factor: 256 lanes, one per factor; lanes past F neither load nor store.  Per block: the partial of the
// weighted energy (the sum of k_gn_factor, so that a round's first E(x) is the one that kernel would have left) and of
// max_f |w_new - w_old| (NaN-propagating like k_gn_diff's maximum); the flagged factors of a wave are counted by one ballot, one
// popcount and ONE integer atomic add, as k_lin_relin counts.
template <int MODEL>
__global__ __launch_bounds__(256) void k_gn_reweight(LinParams p, LinNonlin n, const int *loss, const double *thr, const double *x, int first, double *feta, double *flam,
                                                     double *w, int *flag, double *e_part, double *w_part, int *count)
{
    __shared__ double red[256 / 64];
    const int f = blockIdx.x * 256 + threadIdx.x;
    double e = 0.0, mx = 0.0;
    int fl = 0;
    if (f < p.F) e = gn_reweight_at<MODEL>(p, n, loss, thr, f, x, first != 0, feta, flam, w, flag, mx, fl);
    const unsigned long long who = __ballot(fl != 0);
    if ((threadIdx.x & 63) == 0 && who) atomicAdd(count, __popcll(who));
    e = map_block_sum(e, red);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_down(mx, off, 64); mx = (o > mx || o != o) ? o : mx; }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 256 / 64; ++k) mx = (red[k] > mx || red[k] != red[k]) ? red[k] : mx;
        e_part[blockIdx.x] = e;
        w_part[blockIdx.x] = mx;
    }
}

// k_gn_finish's sibling for a reweight, ONE block of MAP_BLOCK threads, in a fixed order:
// out = (sum e_x[0 .. nen), max w_part[0 .. nen), the flagged count, max part[nb .. 2 nb) = the last round's max |x_end - x_start|)
template <int OUT>
__global__ __launch_bounds__(MAP_BLOCK) void k_gn_reweight_finish(const double *e_x, const double *w_part, int nen, const int *count, const double *part, int nb, double *out)
{
    __shared__ double red[MAP_BLOCK / 64];
    const double ex = map_sum_partials(e_x, nen, red);
    double r[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const double *src = q ? part + nb : w_part;
        const int cnt = q ? nb : nen;
        double mx = 0.0;
        for (int i = threadIdx.x; i < cnt; i += MAP_BLOCK) { const double o = src[i]; mx = (o > mx || o != o) ? o : mx; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_down(mx, off, 64); mx = (o > mx || o != o) ? o : mx; }
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
        __syncthreads();
        for (int k = 1; k < MAP_BLOCK / 64; ++k) mx = (red[k] > mx || red[k] != red[k]) ? red[k] : mx;   // thread 0's is the block's
        r[q] = mx;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        static_assert(OUT == 4, "the weighted energy, max |w_new - w_old|, the flagged count, max |x_end - x_start|");
        out[0] = ex; out[1] = r[0]; out[2] = (double)count[0]; out[3] = r[1];
    }
}

// ---- the host side both entry points share (defined in gbp_lin_capi_map_nonlin.hip) --------------------------------------------------

gbp_lin_nlmap_opts_t gn_nlmap_defaults();                  // what NULL opts of gbp_lin_solve_map_nonlinear mean
int gn_check_opts(const gbp_lin_nlmap_opts_t &o);          // every GBP_EINVAL rule of gbp_lin_nlmap_opts_t
int gn_workspace(gbp_lin *h);                              // LinGn's arrays of the Levenberg-Marquardt loop, once per generation, all or nothing
int gn_start(gbp_lin *h, int init);                        // x0 (GBP_LIN_NLMAP_FROM_*) -> LinGn::x; map_solved cleared
// the loop itself, from LinGn::x: `base` names the weights (LinParams::w), `linearised` says that the linearisation and the energy
// partials at x are already made
int gn_lm(gbp_lin *h, const LinParams &base, bool linearised, const gbp_lin_nlmap_opts_t &o, double *trace, gbp_lin_nlmap_info_t *info);

}  // namespace gbp
