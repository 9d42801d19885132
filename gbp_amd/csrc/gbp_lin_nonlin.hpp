// gbp_lin_nonlin.hpp -- nonlinear pairwise factors of the linear engine on gfx950, relinearised on the device: FactorGraph(
// nonlinear_factors=True) with relinearise_factors (gbp.py:64-80), the per-factor damping of compute_all_messages (gbp.py:46-54) and
// Factor.compute_factor at a moving linearisation point (gbp.py:267-294).  include/gbp_lin.h states the semantics.
//
// The model is a template parameter of what evaluates it; there is one so far, GBP_LIN_MODEL_SE2_BETWEEN: x = (tx, ty, theta), and with
// c = cos theta_a, s_ = sin theta_a, dx = xb - xa, dy = yb - ya
//   h = diag(s) [ c dx + s_ dy ;  -s_ dx + c dy ;  theta_b - theta_a ]
//   J = diag(s) [ -c  -s_  (-s_ dx + c dy) |  c   s_  0 ;   s_ -c  (-c dx - s_ dy) | -s_  c  0 ;   0  0  -1 | 0  0  1 ]
//   Lambda_f = J^T J,  eta_f = J^T (J x0 + diag(s) z - h(x0))                                      (gbp.py:280-289, noise variance 1)
// Angles are never wrapped: the reference does not wrap, and the caller keeps theta continuous.
//   nonlin_h<MODEL>, nonlin_factor<MODEL>   the model: h at a point; eta_f and packed-upper Lambda_f at a linearisation point
//   lin_relin_one<MODEL>   one lane, one factor: the test of gbp.py:75, the factor re-made where it passes, iters, and the damping
//                          switch of gbp.py:50-51
//   k_lin_relin<MODEL>     that over every factor; the relinearised factors of a wave are counted by a popcount and ONE integer atomic add
//   k_lin_relin_range<MODEL>  that over a range of factors (the ones gbp_lin_extend_nonlinear appended), uncounted
//   k_lin_energy_nl<MODEL> sum_f w_f 0.5 |h(mu) - diag(s) z|^2 at the belief means (w_f = 1 without losses), in the block / partials
//                          shape of k_lin_energy
// k_lin_relin and k_lin_energy_nl take the parameter block as a template argument like the stages of gbp_lin_sweep.hpp: LinParams is
// the plain form, LinGated the one gbp_lin_iterate_until_nonlinear queues (gbp_lin_capi_until_nonlin.hip).
// Robust losses on such factors (include/gbp_lin.h, gbp_lin_set_robust_nonlinear):
//   nonlin_mahalanobis2<MODEL>   |diag(s) z - h(x)|^2 at a point;
//   nonlin_robustify_one<MODEL>  w_f and the flag of one factor from M at its LINPOINT (gbp.py:309), through lin_robust_weight;
//   lin_relin_one / k_lin_relin <MODEL, true>   the same lane with that in front: robustify and relinearise are both one lane per
//                          factor on the same linpoint, z and s, so the robust sweep stays at three launches.
// The factor stage of such a sweep is k_lin_factor<3, false, LinRelin>, with losses set k_lin_factor<3, true, LinRelin> (gbp_lin_sweep.hpp),
// both instantiated in gbp_lin_capi_nonlin.hip.
// The model routines are host/device, so a host program can run them.
#pragma once
#include "gbp_lin_handle.hpp"
#include "gbp_lin_robust.hpp"
#include "gbp_math.hpp"

namespace gbp {

// how k_lin_relin is run
constexpr int NL_SWEEP = 0;                               // the stage of a sweep: test, iters, damping switch
constexpr int NL_ALONE = 1;                               // relinearise_factors alone (gbp.py:64-80): no damping switch
constexpr int NL_INIT = 2;                                // compute_all_factors (gbp.py:60-62): every factor, iters = 1, damping = 0
constexpr int NL_ROBUSTIFY = 3;                           // robustify_all_factors alone (gbp.py:82-84): k_lin_relin<MODEL, true> only

template <int MODEL> struct NonlinModel;

template <> struct NonlinModel<GBP_LIN_MODEL_SE2_BETWEEN> {
    // h(x) whitened, and the two entries of J that depend on the translation; c, sn = cos, sin of theta_a
    static GBP_HD void h(const double (&x)[6], const double (&s)[3], double c, double sn, double (&out)[3])
    {
        const double dx = x[3] - x[0], dy = x[4] - x[1];
        out[0] = s[0] * (c * dx + sn * dy);
        out[1] = s[1] * (-sn * dx + c * dy);
        out[2] = s[2] * (x[5] - x[2]);
    }
    static GBP_HD void jac(const double (&x)[6], const double (&s)[3], double c, double sn, double (&J)[3][6])
    {
        const double dx = x[3] - x[0], dy = x[4] - x[1];
        J[0][0] = -s[0] * c;  J[0][1] = -s[0] * sn; J[0][2] = s[0] * (-sn * dx + c * dy); J[0][3] = s[0] * c;   J[0][4] = s[0] * sn; J[0][5] = 0.0;
        J[1][0] = s[1] * sn;  J[1][1] = -s[1] * c;  J[1][2] = s[1] * (-c * dx - sn * dy); J[1][3] = -s[1] * sn; J[1][4] = s[1] * c;  J[1][5] = 0.0;
        J[2][0] = 0.0;        J[2][1] = 0.0;        J[2][2] = -s[2];                      J[2][3] = 0.0;        J[2][4] = 0.0;       J[2][5] = s[2];
    }
};

// 0.5 |h(x) - diag(s) z|^2 (Factor.energy gbp.py:261-265 with noise variance 1)
template <int MODEL>
GBP_HD double nonlin_energy(const double (&x)[6], const double (&z)[3], const double (&s)[3])
{
    double sn, c, h[3], e = 0.0;
    sincos(x[2], &sn, &c);
    NonlinModel<MODEL>::h(x, s, c, sn, h);
#pragma unroll
    for (int k = 0; k < NL_M; ++k) { const double r = h[k] - s[k] * z[k]; e += r * r; }
    return 0.5 * e;
}

// Factor.compute_factor at linpoint x (gbp.py:280-289): eta_f [6], Lambda_f packed upper [21] (the layout k_lin_factor reads)
template <int MODEL>
GBP_HD void nonlin_factor(const double (&x)[6], const double (&z)[3], const double (&s)[3], double (&eta)[6], double (&lam)[Sym<6>::size])
{
    double sn, c, h[3], J[3][6], b[3];
    sincos(x[2], &sn, &c);                                  // once: h and J share it
    NonlinModel<MODEL>::h(x, s, c, sn, h);
    NonlinModel<MODEL>::jac(x, s, c, sn, J);
#pragma unroll
    for (int k = 0; k < NL_M; ++k) {                        // J x0 + diag(s) z - h(x0)
        double v = s[k] * z[k] - h[k];
#pragma unroll
        for (int i = 0; i < 6; ++i) v += J[k][i] * x[i];
        b[k] = v;
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double e = 0.0;
#pragma unroll
        for (int k = 0; k < NL_M; ++k) e += J[k][i] * b[k];
        eta[i] = e;
#pragma unroll
        for (int j = i; j < 6; ++j) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < NL_M; ++k) v += J[k][i] * J[k][j];
            lam[Sym<6>::at(i, j)] = v;
        }
    }
}

// |diag(s) z - h(x)|^2 at a point: the squared Mahalanobis distance of Factor.robustify_loss (gbp.py:312, 322) with noise variance 1
template <int MODEL>
GBP_HD double nonlin_mahalanobis2(const double (&x)[6], const double (&z)[3], const double (&s)[3])
{
    double sn, c, h[3], m2 = 0.0;
    sincos(x[2], &sn, &c);
    NonlinModel<MODEL>::h(x, s, c, sn, h);
#pragma unroll
    for (int k = 0; k < NL_M; ++k) { const double r = s[k] * z[k] - h[k]; m2 += r * r; }
    return m2;
}

// Factor.robustify_loss (gbp.py:296-332) of nonlinear factor f, one lane: h is evaluated at Factor.linpoint (gbp.py:309) AS IT STANDS,
// which is the reference's reading -- here the linpoint moves with every relinearisation.  Writes w_f and the flag with plain vector
// stores; a factor without a loss loads nothing but its loss.  Returns the flag.
template <int MODEL>
GBP_DEV bool nonlin_robustify_one(const LinParams &p, const LinNonlin &n, const LinRobust &r, int f)
{
    const size_t F = (size_t)p.F;
    const int loss = r.loss[f];
    int flag = 0;
    double w = 1.0;
    if (loss != GBP_LIN_LOSS_NONE) {
        double x[6], z[3], s[3];
#pragma unroll
        for (int k = 0; k < 6; ++k) x[k] = n.linpoint[k * F + f];
#pragma unroll
        for (int k = 0; k < NL_M; ++k) { z[k] = n.meas[k * F + f]; s[k] = n.sinfo[k * F + f]; }
        w = lin_robust_weight(loss, r.thr[f], 1.0, 0.5 * nonlin_mahalanobis2<MODEL>(x, z, s), flag);
    }
    r.w[f] = w;
    r.flag[f] = flag;
    return flag != 0;
}

// The relinearise stage for factor f, one lane: shared by the two kernels below so that a factor linearised over a range comes out bit
// for bit as one linearised with the whole graph.  A lane that does not relinearise writes iters only (and its damping in the sweep in
// which that switches); a relinearising lane writes the 6 + 21 doubles of the factor, the 6 of the linpoint, iters and its damping.  A
// lane that is not `live` neither loads nor stores.  Returns whether the factor was relinearised.
// ROBUST (losses are set): the lane FIRST makes w_f and the flag from the linpoint as it stands (robustify_all_factors comes before
// relinearise_factors in synchronous_iteration, gbp.py:87-90), then runs the test and the re-make below unchanged -- the re-made factor
// is the nominal one, and the weight stays.  In mode NL_ROBUSTIFY that is all it does.  `flagged`: whether the factor was flagged.
// The `false` instantiation reads nothing of `r` and is the code of a handle without losses.
template <int MODEL, bool ROBUST = false>
GBP_DEV bool lin_relin_one(const LinParams &p, const LinNonlin &n, const LinRobust &r, int mode, int f, bool live, bool &flagged)
{
    constexpr int D = NL_D, P = LinDims<D>::P, REC = LinDims<D>::REC;
    const size_t F = (size_t)p.F;
    bool relin = false;
    flagged = false;
    if constexpr (ROBUST) {
        if (live) flagged = nonlin_robustify_one<MODEL>(p, n, r, f);
        if (mode == NL_ROBUSTIFY) return false;
    }
    if (live) {
        const double *ma = p.bel + (size_t)p.va[f] * REC + D + P, *mb = p.bel + (size_t)p.vb[f] * REC + D + P;
        double x[6];
#pragma unroll
        for (int k = 0; k < D; ++k) { x[k] = ma[k]; x[D + k] = mb[k]; }
        int it = 1;
        if (mode == NL_INIT) relin = true;
        else {
            it = n.iters[f];
            double d2 = 0.0;
#pragma unroll
            for (int k = 0; k < 6; ++k) { const double d = n.linpoint[k * F + f] - x[k]; d2 += d * d; }
            relin = sqrt(d2) > n.beta && it >= n.min_linear;                      // gbp.py:75
            it = relin ? 0 : it + 1;                                               // gbp.py:77, 80
        }
        n.iters[f] = it;
        if (relin) {
            double z[3], s[3], eta[6], lam[Sym<6>::size];
#pragma unroll
            for (int k = 0; k < NL_M; ++k) { z[k] = n.meas[k * F + f]; s[k] = n.sinfo[k * F + f]; }
            nonlin_factor<MODEL>(x, z, s, eta, lam);
#pragma unroll
            for (int k = 0; k < 6; ++k) { n.feta[k * F + f] = eta[k]; n.linpoint[k * F + f] = x[k]; }
#pragma unroll
            for (int k = 0; k < Sym<6>::size; ++k) n.flam[(size_t)k * F + f] = lam[k];
        }
        // gbp.py:78, then the switch of gbp.py:50-51 on the iters just written (0 after a relinearisation: fires when num_undamped == 0)
        if (mode == NL_SWEEP && it == n.num_undamped) n.fdamp[f] = p.damping;
        else if (relin) n.fdamp[f] = 0.0;
    }
    return relin;
}

// One lane per factor of the graph.  Lanes past F neither load nor store.  `count`: the slot of this sweep (nullptr for NL_INIT): one
// integer atomic add per wave that relinearised anything.
// ROBUST: the fused robustify + relinearise lane; `r` is read and `rcount` counted (the same way: one ballot, one popcount, one integer
// atomic add per wave that flagged anything) under it only.
// PT = LinGated (a sweep queued by gbp_lin_iterate_until_nonlinear): the whole kernel -- the lane and both counts -- returns at its head
// once the call's stop word is set; for PT = LinParams lin_stopped() is the constant false and the gate compiles away.
template <int MODEL, bool ROBUST = false, typename PT = LinParams>
__global__ __launch_bounds__(256) void k_lin_relin(PT p, LinNonlin n, int mode, int *count, LinRobust r, int *rcount)
{
    if (lin_stopped(p)) return;                             // PT = LinParams: never
    const int f = blockIdx.x * 256 + threadIdx.x;
    bool flagged;
    const bool relin = lin_relin_one<MODEL, ROBUST>(p, n, r, mode, f, f < p.F, flagged);
    if (count) {
        const unsigned long long who = __ballot(relin);
        if ((threadIdx.x & 63) == 0 && who) atomicAdd(count, __popcll(who));
    }
    if constexpr (ROBUST) {
        if (rcount) {
            const unsigned long long who = __ballot(flagged);
            if ((threadIdx.x & 63) == 0 && who) atomicAdd(rcount, __popcll(who));
        }
    }
}

// The same stage over the factors [f0, f1) only, one lane per factor of the RANGE: what gbp_lin_extend_nonlinear runs in mode NL_INIT
// on the factors it appended (compute_factor on the new factors, gbp.py:267-294).  Work and traffic go by f1 - f0, not by F; lanes
// outside the range neither load nor store; no atomics.  `mode` stays a run-time argument so that the lane's code is k_lin_relin's.
template <int MODEL>
__global__ __launch_bounds__(256) void k_lin_relin_range(LinParams p, LinNonlin n, int mode, int f0, int f1)
{
    const int f = f0 + blockIdx.x * 256 + threadIdx.x;
    bool flagged;
    (void)lin_relin_one<MODEL>(p, n, LinRobust{}, mode, f, f < f1, flagged);
}

// sum_f 0.5 |h(mu) - diag(s) z|^2 at the current belief means (gbp.py:36-44, 251-265): one partial per block, the lanes of a wave and
// the four waves of a block added in a fixed order, exactly the shape of k_lin_energy (gbp_lin_sweep.hpp).  PT = LinGated: the energy
// pass of a sweep of gbp_lin_iterate_until_nonlinear, gated like the stage above, into the call's own partials.
template <int MODEL, typename PT = LinParams>
__global__ __launch_bounds__(256) void k_lin_energy_nl(PT p, LinNonlin n, double *out)
{
    if (lin_stopped(p)) return;                             // PT = LinParams: never
    constexpr int D = NL_D, P = LinDims<D>::P, REC = LinDims<D>::REC;
    __shared__ double red[256 / 64];
    const int f = blockIdx.x * 256 + threadIdx.x;
    const size_t F = (size_t)p.F;
    double e = 0.0;
    if (f < p.F) {
        const double *ma = p.bel + (size_t)p.va[f] * REC + D + P, *mb = p.bel + (size_t)p.vb[f] * REC + D + P;
        double x[6], z[3], s[3];
#pragma unroll
        for (int k = 0; k < D; ++k) { x[k] = ma[k]; x[D + k] = mb[k]; }
#pragma unroll
        for (int k = 0; k < NL_M; ++k) { z[k] = n.meas[k * F + f]; s[k] = n.sinfo[k * F + f]; }
        e = nonlin_energy<MODEL>(x, z, s);
        if (p.w) e *= p.w[f];                               // the weighted form (gbp.py:43): sigma^2 / adaptive_gauss_noise_var, as k_lin_energy
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) e += __shfl_down(e, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

}  // namespace gbp
