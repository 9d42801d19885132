// gbp_lin_capi.hip -- linear pairwise GBP on gfx950 behind include/gbp_lin.h.
//
// The reference's generic path (gbp/gbp.py FactorGraph with nonlinear_factors=False, ndim_posegraph.py) for graphs
// of two-variable factors over d-dimensional variables.  Two kernels per sweep, like the general BA sweep, both in gbp_lin_sweep.hpp
// (one source body per stage; this file launches the plain forms, gbp_lin_capi_until.hip the gated and traced ones):
//   k_lin_factor<D>   one lane per factor: both outgoing messages from the OLD incoming ones
//                     (Factor.compute_messages gbp.py:334-373): cavity of the other variable folded into its block,
//                     that block eliminated by an unpivoted LDL^T (SPD: factor block + prior-backed cavity);
//   k_lin_belief<D>   64/(d+P) variables per wave, one lane per belief entry: prior + messages in adj_factors order from
//                     the variable-major copy of the messages (one contiguous run per variable), mean by a d x d solve
//                     (VariableNode.update_belief gbp.py:176-198).
// Layout: everything factor-indexed is SoA [row][F] (coalesced across lanes); the new messages are ALSO written in CSR
// edge order (vmsg, through an LDS transpose) for the belief stage; beliefs are records [N][d + d(d+1)/2 + d]
// (eta | packed Lambda | mu) gathered per factor.  Lambda_f is constant: packed upper 2d x 2d, read every sweep.
// HBM-bound like the BA sweep; d <= 6 keeps a factor's working set in registers (one wave per SIMD for d = 6).
#include "gbp_lin_generation.hpp"
#include "gbp_lin_robust.hpp"
#include "gbp_lin_sweep.hpp"
#include "gbp_math.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

static int lin_beliefs(gbp_lin *h)
{
    if (h->p.N) lin_dispatch(h->D, [&](auto d) {
        constexpr int DD = decltype(d)::value, VPW = 64 / (DD + DD * (DD + 1) / 2);
        hipLaunchKernelGGL((k_lin_belief<DD>), dim3((h->p.N + VPW - 1) / VPW), dim3(64), 0, h->stream, h->p);
    });
    LHIPCHK(hipGetLastError());
    h->has_beliefs = true;
    return GBP_OK;
}

namespace gbp {
int lin_sweep(gbp_lin *h)
{
    if (h->p.F) lin_dispatch(h->D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        if (h->p.w) hipLaunchKernelGGL((k_lin_factor<DD, true>), dim3((h->p.F + 63) / 64), dim3(64), 0, h->stream, h->p);
        else hipLaunchKernelGGL((k_lin_factor<DD, false>), dim3((h->p.F + 63) / 64), dim3(64), 0, h->stream, h->p);
    });
    return lin_beliefs(h);
}
}  // namespace gbp

static int lin_create_impl(gbp_lin *h, const gbp_lin_desc_t *d)
{
    const int N = d->n_vars, F = d->n_factors, D = d->dofs;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return set_error(GBP_ENODEV, "no HIP device visible: libgbp_hip.so has no CPU path");
    if (d->device < 0 || d->device >= ndev) return set_error(GBP_EINVAL, "device %d out of range (%d visible)", d->device, ndev);
    h->device = d->device;
    LHIPCHK(hipSetDevice(h->device));
    hipDeviceProp_t prop;
    LHIPCHK(hipGetDeviceProperties(&prop, h->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_error(GBP_ENODEV, "device %d is %s; this library is built for gfx950 (MI355X) only", h->device, prop.gcnArchName);
    LHIPCHK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->D = D;
    h->has_const = d->factor_const != nullptr;
    const LinRows r = lin_rows(D);
    h->p.damping = d->eta_damping;

    // factor data -> SoA, packed upper; adjacency CSR in ascending factor id (= append order, ndim_posegraph.py:86-88)
    std::vector<int32_t> va(d->var_a, d->var_a + F), vb(d->var_b, d->var_b + F), vptr((size_t)N + 1, 0), vadj((size_t)2 * F);
    std::vector<double> feta((size_t)r.eta2 * F), flam((size_t)r.lam2 * F), fconst((size_t)F, 0.0), prior((size_t)N * r.msg);
    for (int f = 0; f < F; ++f) {
        if (va[f] < 0 || va[f] >= N || vb[f] < 0 || vb[f] >= N || va[f] == vb[f])
            return set_error(GBP_EINVAL, "factor %d joins variables (%d, %d): need two different ids in [0, %d)", f, va[f], vb[f], N);
        ++vptr[va[f] + 1]; ++vptr[vb[f] + 1];
    }
    lin_pack_factors(D, F, d->factor_eta, d->factor_lam, feta.data(), flam.data());
    if (d->factor_const) fconst.assign(d->factor_const, d->factor_const + F);
    lin_pack_priors(D, N, d->prior_eta, d->prior_lam, prior.data());
    for (int v = 0; v < N; ++v) vptr[v + 1] += vptr[v];
    std::vector<int32_t> epos_a((size_t)F), epos_b((size_t)F);
    {
        std::vector<int32_t> fill(vptr.begin(), vptr.end() - 1);
        for (int f = 0; f < F; ++f) {
            epos_a[f] = fill[va[f]]; vadj[fill[va[f]]++] = f << 1;
            epos_b[f] = fill[vb[f]]; vadj[fill[vb[f]]++] = (f << 1) | 1;
        }
    }

    // the first generation: allocated, filled and committed like every later one (gbp_lin_generation.hpp), with nothing to replace.
    // The host vectors above are the sources of the copies and outlive the one synchronisation, on the failure path too.
    LinScratch mem;
    LinGen g;
    LinParams &n = g.p;
    auto copy = [&](const auto *dst, const auto &v) { return v.empty() ? hipSuccess : hipMemcpyAsync(lin_mut(dst), v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice, h->stream); };
    auto zero = [&](double *dst, size_t cnt) { return cnt ? hipMemsetAsync(dst, 0, cnt * sizeof(double), h->stream) : hipSuccess; };
    const int rc = [&]() -> int {
        LCHK(lin_gen_alloc(h, mem, g, N, F));
        LHIPCHK(copy(n.va, va)); LHIPCHK(copy(n.vb, vb)); LHIPCHK(copy(n.vptr, vptr)); LHIPCHK(copy(n.vadj, vadj));
        LHIPCHK(copy(n.feta, feta)); LHIPCHK(copy(n.flam, flam)); LHIPCHK(copy(n.fconst, fconst)); LHIPCHK(copy(n.prior, prior));
        LHIPCHK(copy(n.epos_a, epos_a)); LHIPCHK(copy(n.epos_b, epos_b));
        LHIPCHK(zero(n.msg_a, (size_t)r.msg * F)); LHIPCHK(zero(n.msg_b, (size_t)r.msg * F)); LHIPCHK(zero(n.vmsg, (size_t)2 * F * r.msg));
        LHIPCHK(zero(n.bel, (size_t)N * r.rec)); LHIPCHK(zero(g.d_red, (size_t)g.red_blocks));
        LHIPCHK(hipStreamSynchronize(h->stream));
        return GBP_OK;
    }();
    if (rc != GBP_OK) {
        (void)hipStreamSynchronize(h->stream);              // before `mem` frees what the stream may still be writing
        return rc;
    }
    lin_gen_commit(h, mem, g);
    return GBP_OK;
}

extern "C" {

int gbp_lin_create(gbp_lin_t **out, const gbp_lin_desc_t *d)
{
    if (!out || !d) return set_error(GBP_EINVAL, "NULL argument");
    *out = nullptr;
    if (d->n_vars < 0 || d->n_factors < 0) return set_error(GBP_EINVAL, "negative size");
    if (d->dofs < 1 || d->dofs > GBP_LIN_MAX_DOFS) return set_error(GBP_EINVAL, "dofs %d not in 1..%d", d->dofs, GBP_LIN_MAX_DOFS);
    if ((d->n_factors && (!d->var_a || !d->var_b || !d->factor_eta || !d->factor_lam)) || (d->n_vars && (!d->prior_eta || !d->prior_lam)))
        return set_error(GBP_EINVAL, "NULL array in the descriptor");
    gbp_lin *h = new (std::nothrow) gbp_lin;
    if (!h) return set_error(GBP_ENOMEM, "out of host memory");
    const int rc = lin_create_impl(h, d);
    if (rc != GBP_OK) { gbp_lin_destroy(h); return rc; }
    *out = h;
    return GBP_OK;
}

void gbp_lin_destroy(gbp_lin_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void *q : h->allocs) (void)hipFree(q);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int gbp_lin_sync(gbp_lin_t *h)
{
    LENTER(h);
    LHIPCHK(hipStreamSynchronize(h->stream));
    return GBP_OK;
}

int gbp_lin_update_beliefs(gbp_lin_t *h)
{
    LENTER(h);
    return lin_beliefs(h);
}

int gbp_lin_iterate(gbp_lin_t *h, int32_t n_iters)
{
    LENTER(h);
    if (n_iters < 0) return set_error(GBP_EINVAL, "negative iteration count");
    if (!h->has_beliefs) return set_error(GBP_ESTATE, "call gbp_lin_update_beliefs first (ndim_posegraph.py:90)");
    for (int it = 0; it < n_iters; ++it) LCHK(lin_sweep(h));       // with losses set: at the weights as they stand (robustify=False)
    LHIPCHK(hipGetLastError());
    return GBP_OK;
}

int gbp_lin_energy(gbp_lin_t *h, double *out)
{
    LENTER(h);
    if (!out) return set_error(GBP_EINVAL, "out is NULL");
    if (!h->has_beliefs) return set_error(GBP_ESTATE, "beliefs have not been computed yet");
    double e = 0.0;
    if (h->p.F) {
        if (h->nonlinear) LCHK(lin_nonlin_energy(h, h->d_red));    // through the nonlinear h at the current means (gbp.py:251-265)
        else lin_dispatch(h->D, [&](auto d) {
            hipLaunchKernelGGL((k_lin_energy<decltype(d)::value>), dim3(h->red_blocks), dim3(256), 0, h->stream, h->p, h->d_red);
        });
        LHIPCHK(hipGetLastError());
        std::vector<double> r((size_t)h->red_blocks);
        LHIPCHK(hipMemcpyAsync(r.data(), h->d_red, r.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        LHIPCHK(hipStreamSynchronize(h->stream));
        for (double v : r) e += v;
    }
    *out = e;
    return GBP_OK;
}

static int lin_download(gbp_lin *h, std::vector<double> &dst, const double *src, size_t n)
{
    dst.resize(n);
    if (n) LHIPCHK(hipMemcpyAsync(dst.data(), src, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LHIPCHK(hipStreamSynchronize(h->stream));
    return GBP_OK;
}

static void unpack_sym(int D, const double *packed, size_t stride, double *dense)
{
    for (int i = 0; i < D; ++i)
        for (int j = i; j < D; ++j) {
            const double v = packed[(size_t)lin_packed_at(D, i, j) * stride];
            dense[i * D + j] = v; dense[j * D + i] = v;
        }
}

int gbp_lin_get_beliefs(gbp_lin_t *h, double *eta, double *lam)
{
    LENTER(h);
    const int D = h->D, P = D * (D + 1) / 2, REC = D + P + D;
    std::vector<double> b;
    LCHK(lin_download(h, b, h->p.bel, (size_t)h->p.N * REC));
    for (int v = 0; v < h->p.N; ++v) {
        if (eta) for (int k = 0; k < D; ++k) eta[(size_t)v * D + k] = b[(size_t)v * REC + k];
        if (lam) unpack_sym(D, &b[(size_t)v * REC + D], 1, lam + (size_t)v * D * D);
    }
    return GBP_OK;
}

int gbp_lin_get_means(gbp_lin_t *h, double *mu)
{
    LENTER(h);
    if (!mu) return set_error(GBP_EINVAL, "mu is NULL");
    const int D = h->D, P = D * (D + 1) / 2, REC = D + P + D;
    std::vector<double> b;
    LCHK(lin_download(h, b, h->p.bel, (size_t)h->p.N * REC));
    for (int v = 0; v < h->p.N; ++v) for (int k = 0; k < D; ++k) mu[(size_t)v * D + k] = b[(size_t)v * REC + D + P + k];
    return GBP_OK;
}

int gbp_lin_get_messages(gbp_lin_t *h, double *eta_a, double *lam_a, double *eta_b, double *lam_b)
{
    LENTER(h);
    const int D = h->D, P = D * (D + 1) / 2;
    const size_t F = (size_t)h->p.F;
    for (int side = 0; side < 2; ++side) {
        double *eta = side ? eta_b : eta_a, *lam = side ? lam_b : lam_a;
        if (!eta && !lam) continue;
        std::vector<double> m;
        LCHK(lin_download(h, m, side ? h->p.msg_b : h->p.msg_a, (size_t)(D + P) * F));
        for (size_t f = 0; f < F; ++f) {
            if (eta) for (int k = 0; k < D; ++k) eta[f * D + k] = m[(size_t)k * F + f];
            if (lam) unpack_sym(D, &m[(size_t)D * F + f], F, lam + f * D * D);
        }
    }
    return GBP_OK;
}

}  // extern "C"
