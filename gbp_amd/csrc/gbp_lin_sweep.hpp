// gbp_lin_sweep.hpp -- the stages of a sweep of the linear engine, one source body each (the robustify stage is gbp_lin_robust.hpp):
//   k_lin_factor<D, ROBUST, PT>   one lane per factor: both outgoing messages from the OLD incoming ones, with its Schur step;
//   k_lin_belief<D, PT>           64/(d+P) variables per wave: prior + messages in adj_factors order, mean by a d x d solve;
//   k_lin_energy<D, PT>           the energy of the graph at the belief means, one partial per block.
// The parameter block PT (gbp_lin_handle.hpp) selects the form, and two translation units instantiate them: gbp_lin_capi.hip launches the
// plain forms (PT = LinParams), gbp_lin_capi_until.hip the gated ones (PT = LinGated; for the belief stage LinTraced, gated and traced),
// which return at their head once gbp_lin_iterate_until's stop word is set.  For PT = LinParams lin_stopped() is the constant false and
// the gate -- and with `if constexpr` the trace -- compiles away.  gbp_lin_capi_nonlin.hip instantiates the factor stage once more with
// PT = LinRelin, where lin_damping() reads the factor's own damping instead of the graph's.
// gbp_lin_capi_until_nonlin.hip instantiates it with PT = LinRelinGated (that damping and the gate) for gbp_lin_iterate_until_nonlinear.
#pragma once
#include "gbp_lin_robust.hpp"
#include "gbp_lin_until.hpp"

#include <hip/hip_runtime.h>

namespace gbp {

// Message to the KEPT variable from  [ A_kk  A_kn ; A_nk  A_nn ] , with the eliminated block S = A_nn + cavity already
// formed (consumed):  Lambda = A_kk - A_kn S^-1 A_nk,  eta = e_k - A_kn S^-1 e_n   (gbp.py:353-367).
// akn(i, j) = A[k_i][n_j] is supplied by the caller as a dense D x D array.
template <int D>
GBP_DEV void lin_schur(const double (&akk)[Sym<D>::size], const double (&akn)[D][D], double (&S)[Sym<D>::size],
                       const double (&ek)[D], double (&en)[D], double (&lam)[Sym<D>::size], double (&eta)[D])
{
    double invd[D];
    ldl_factor<D>(S, invd);
    ldl_forward<D>(S, en);                            // L^-1 e_n
    double y[D][D];                                   // y[i] = L^-1 (A_nk column i) = L^-1 akn[i][:]
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
        for (int j = 0; j < D; ++j) y[i][j] = akn[i][j];
        ldl_forward<D>(S, y[i]);
    }
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double e = ek[i];
#pragma unroll
        for (int k = 0; k < D; ++k) e -= y[i][k] * invd[k] * en[k];
        eta[i] = e;
#pragma unroll
        for (int j = i; j < D; ++j) {
            double v = akk[Sym<D>::at(i, j)];
#pragma unroll
            for (int k = 0; k < D; ++k) v -= y[i][k] * invd[k] * y[j][k];
            lam[Sym<D>::at(i, j)] = v;
        }
    }
}

// ROBUST: the factor is the stored nominal one times its weight p.w[f] (gbp_lin_robust.hpp; gbp.py:331-332), applied on load.  A handle
// without losses launches only the `false` instantiation, which reads no weight.
template <int D, bool ROBUST, typename PT = LinParams>
__global__ __launch_bounds__(64) void k_lin_factor(PT p)
{
    if (lin_stopped(p)) return;                             // PT = LinParams: never
    constexpr int P = LinDims<D>::P, REC = LinDims<D>::REC, R = D + P;
    __shared__ double tr[64 * R];                           // transposes a wave's messages for the variable-major copy
    __shared__ int tp[64];
    const int lane = threadIdx.x;
    const int nlive = min(64, p.F - (int)blockIdx.x * 64);  // factors of this wave (> 0 by the launch grid)
    const int f = blockIdx.x * 64 + min(lane, nlive - 1);   // lanes past the end redo the last factor and store nothing
    const bool live = lane < nlive;
    const size_t F = (size_t)p.F;
    // the belief stage reads messages in CSR edge order: stage this wave's 64 records in LDS and write them out as
    // contiguous (D+P)-double runs, 64/(D+P) records per store instruction (a lane-per-record store would touch 64 lines)
    auto stage_out = [&](const double (&eta)[D], const double (&lam)[P], const int *epos) {
#pragma unroll
        for (int k = 0; k < D; ++k) tr[lane * R + k] = eta[k];
#pragma unroll
        for (int k = 0; k < P; ++k) tr[lane * R + D + k] = lam[k];
        tp[lane] = epos[f];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // one wave per block
        constexpr int G = 64 / R;
        const int g = lane / R, k = lane - g * R;
        if (g < G) {
            if (nlive == 64) {                              // full wave: fixed trip count, LDS reads batched ahead of the stores
#pragma unroll
                for (int j0 = 0; j0 < 64; j0 += G) {
                    const int j = j0 + g;
                    if (j < 64) p.vmsg[(size_t)tp[j] * R + k] = tr[j * R + k];
                }
            } else {
                for (int j = g; j < nlive; j += G) p.vmsg[(size_t)tp[j] * R + k] = tr[j * R + k];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    const double *ra = p.bel + (size_t)p.va[f] * REC, *rb = p.bel + (size_t)p.vb[f] * REC;
    // cavities: belief minus this factor's old message (gbp.py:341-350)
    double cea[D], cla[P], ceb[D], clb[P], oea[D], oeb[D];
#pragma unroll
    for (int k = 0; k < D; ++k) { oea[k] = p.msg_a[k * F + f]; oeb[k] = p.msg_b[k * F + f]; cea[k] = ra[k] - oea[k]; ceb[k] = rb[k] - oeb[k]; }
#pragma unroll
    for (int k = 0; k < P; ++k) { cla[k] = ra[D + k] - p.msg_a[(D + k) * F + f]; clb[k] = rb[D + k] - p.msg_b[(D + k) * F + f]; }
    // the factor: packed upper 2D x 2D = [ A_aa A_ab ; . A_bb ]
    double aaa[P], abb[P], aab[D][D], aba[D][D], fa[D], fb[D];
#pragma unroll
    for (int k = 0; k < D; ++k) { fa[k] = p.feta[k * F + f]; fb[k] = p.feta[(D + k) * F + f]; }
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
        for (int j = i; j < D; ++j) {
            aaa[Sym<D>::at(i, j)] = p.flam[(size_t)Sym<2 * D>::at(i, j) * F + f];
            abb[Sym<D>::at(i, j)] = p.flam[(size_t)Sym<2 * D>::at(D + i, D + j) * F + f];
        }
#pragma unroll
        for (int j = 0; j < D; ++j) { const double v = p.flam[(size_t)Sym<2 * D>::at(i, D + j) * F + f]; aab[i][j] = v; aba[j][i] = v; }
    }
    if constexpr (ROBUST) {
        const double w = p.w[f];
#pragma unroll
        for (int k = 0; k < D; ++k) { fa[k] *= w; fb[k] *= w; }
#pragma unroll
        for (int k = 0; k < P; ++k) { aaa[k] *= w; abb[k] *= w; }
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) { aab[i][j] *= w; aba[j][i] = aab[i][j]; }
    }
    const double d = lin_damping(p, f);                     // PT = LinRelin: the factor's own (gbp.py:52), else the graph's (gbp.py:54)
    double lam[P], eta[D], S[P], en[D];
    // to a: eliminate b
#pragma unroll
    for (int k = 0; k < P; ++k) S[k] = abb[k] + clb[k];
#pragma unroll
    for (int k = 0; k < D; ++k) en[k] = fb[k] + ceb[k];
    lin_schur<D>(aaa, aab, S, fa, en, lam, eta);
#pragma unroll
    for (int k = 0; k < D; ++k) eta[k] = (1.0 - d) * eta[k] + d * oea[k];                   // gbp.py:368
    if (live) {
#pragma unroll
        for (int k = 0; k < D; ++k) p.msg_a[k * F + f] = eta[k];
#pragma unroll
        for (int k = 0; k < P; ++k) p.msg_a[(D + k) * F + f] = lam[k];
    }
    stage_out(eta, lam, p.epos_a);
    // to b: eliminate a (from the OLD message of b: both are committed together, gbp.py:371-373 -- cea / cla were
    // formed before the store above)
#pragma unroll
    for (int k = 0; k < P; ++k) S[k] = aaa[k] + cla[k];
#pragma unroll
    for (int k = 0; k < D; ++k) en[k] = fa[k] + cea[k];
    lin_schur<D>(abb, aba, S, fb, en, lam, eta);
#pragma unroll
    for (int k = 0; k < D; ++k) eta[k] = (1.0 - d) * eta[k] + d * oeb[k];
    if (live) {
#pragma unroll
        for (int k = 0; k < D; ++k) p.msg_b[k * F + f] = eta[k];
#pragma unroll
        for (int k = 0; k < P; ++k) p.msg_b[(D + k) * F + f] = lam[k];
    }
    stage_out(eta, lam, p.epos_b);
}

// 64/(D+P) variables per wave, one lane per (variable, belief entry): the variable's messages are one contiguous run of
// vmsg (CSR edge order = adj_factors order), so the wave streams whole lines; the d x d solve is done by the entry-0 lane.
// PT = LinTraced adds the gate and the trace of the block: the entry-0 lane, which holds the new mean in registers, reads the old mean
// from the record before it writes the new one, and the wave (one per block) reduces step and squared distance to one partial each.
template <int D, typename PT = LinParams>
__global__ __launch_bounds__(64) void k_lin_belief(PT p)
{
    constexpr bool TRACED = std::is_same<PT, LinTraced>::value;
    if (lin_stopped(p)) return;                             // PT = LinParams: never
    constexpr int P = LinDims<D>::P, REC = LinDims<D>::REC, R = D + P, VPW = 64 / R;
    __shared__ double sh[VPW * R];
    const int lane = threadIdx.x, j = lane / R, k = lane - j * R;
    const int v = blockIdx.x * VPW + j;
    const bool on = j < VPW && v < p.N;
    if (on) {
        double acc = p.prior[(size_t)v * R + k];
        const int e1 = p.vptr[v + 1];
        int e = p.vptr[v];
        for (; e + 3 < e1; e += 4) {                              // four loads in flight, added in adj_factors order (gbp.py:182-188)
            const double m0 = p.vmsg[(size_t)e * R + k], m1 = p.vmsg[(size_t)(e + 1) * R + k], m2 = p.vmsg[(size_t)(e + 2) * R + k],
                         m3 = p.vmsg[(size_t)(e + 3) * R + k];
            acc += m0; acc += m1; acc += m2; acc += m3;
        }
        for (; e < e1; ++e) acc += p.vmsg[(size_t)e * R + k];
        p.bel[(size_t)v * REC + k] = acc;
        sh[j * R + k] = acc;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // one wave per block
    [[maybe_unused]] double step = 0.0, sq = 0.0;
    if (on && k == 0) {
        double eta[D], lam[P], mu[D];
#pragma unroll
        for (int i = 0; i < D; ++i) eta[i] = sh[j * R + i];
#pragma unroll
        for (int i = 0; i < P; ++i) lam[i] = sh[j * R + D + i];
        spd_solve<D>(lam, eta, mu);                               // gbp.py:192-193
        // The old mean, before the store.  The step is bit-equal to numpy's only while mu_new - mu_old is a subtraction of the ROUNDED
        // mean that is stored below: were the last multiply of spd_solve fused into it (-ffp-contract=fast allows an fma), the step
        // would be that of an unrounded mean.  The twin tests (tests/test_linear_until_gpu.py) compare it bit for bit for d = 1 .. 6.
        if constexpr (TRACED) until_var<D>(mu, p.bel + (size_t)v * REC + R, p.x ? p.x + (size_t)v * D : nullptr, step, sq);
#pragma unroll
        for (int i = 0; i < D; ++i) p.bel[(size_t)v * REC + R + i] = mu[i];
    }
    if constexpr (TRACED) {
        // the wave's partials: every other lane holds 0; lane 0 ends with the lanes combined in a fixed order
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            step = until_max(step, __shfl_down(step, off, 64));
            sq += __shfl_down(sq, off, 64);
        }
        if (lane == 0) {
            p.u.bel_part[blockIdx.x] = step;
            if (p.x) p.u.bel_part[(size_t)p.u.nbel + blockIdx.x] = sq;
        }
    }
}

// sum over factors of w_f 0.5 |h(mu) - z|^2 / sigma^2 for linear h (gbp.py:36-44, 251-265; w_f = sigma^2 / adaptive_gauss_noise_var, 1 on a
// handle without losses): the per-factor term is lin_factor_energy (gbp_lin_robust.hpp), the residual form without cancellation.
// out: one partial per block -- the handle's for gbp_lin_energy, the call's own for the trace of gbp_lin_iterate_until.
template <int D, typename PT = LinParams>
__global__ __launch_bounds__(256) void k_lin_energy(PT p, double *out)
{
    if (lin_stopped(p)) return;                             // PT = LinParams: never
    __shared__ double red[256 / 64];
    const int f = blockIdx.x * 256 + threadIdx.x;
    double e = 0.0;
    if (f < p.F) {
        e = lin_factor_energy<D>(p, f);
        if (p.w) e *= p.w[f];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) e += __shfl_down(e, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

}  // namespace gbp
