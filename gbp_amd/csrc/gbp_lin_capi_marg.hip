// gbp_lin_capi_marg.hip -- gbp_lin_solve_marginals of include/gbp_lin.h: blocks of Lambda_joint^-1 (the `sigma` of
// FactorGraph.joint_distribution_cov, gbp.py:128-144) for chosen variables, by the block-Jacobi conjugate gradients of the batch MAP run
// on GBP_LIN_MARG_COLS unit right-hand sides at a time (kernels and method: gbp_lin_marg.hpp).
//
// The LDL^T of the diagonal blocks is the MAP solver's (lin_map_prepare); everything else lives in a workspace of its own, made by the
// first call and freed with the handle through `allocs` (the staging of the outputs grows with the largest call seen), so the MAP solver's iterate and the sweep's state are never touched.  A batch
// queues four kernels per iteration and reads the per-column |r|^2 back every `check_every` iterations; the true residuals are formed
// with one more product when all columns claim convergence (or max_iters runs out).  The rows the caller asked for are gathered on the
// device into buffers of the outputs' shape and copied once, at the end of the call.
#include "gbp_lin_marg.hpp"

#include <cmath>
#include <cstdint>

using namespace gbp;

namespace {

constexpr int K = MARG_COLS;

// The staging of a call's outputs and ids: kept with the workspace and only ever grown, so that a call of a size seen before allocates
// nothing.  The old block is given back here, so the handle still holds one.
int marg_stage_reserve(gbp_lin *h, size_t bytes)
{
    LinMarg &m = h->marg;
    if (bytes <= m.stage_bytes) return GBP_OK;
    char *q = nullptr;
    LCHK(lin_alloc(h, &q, bytes));
    if (m.stage) {
        LHIPCHK(hipStreamSynchronize(h->stream));
        lin_free(h, m.stage);
    }
    m.stage = q;
    m.stage_bytes = bytes;
    return GBP_OK;
}

int marg_prepare(gbp_lin *h)
{
    LCHK(lin_map_prepare(h));
    if (h->marg_ready) return GBP_OK;
    LinMarg &m = h->marg;
    const size_t ndk = (size_t)h->p.N * h->D * K;
    m.nb = std::min(MAP_MAX_BLOCKS, std::max(1, (h->p.N + MAP_BLOCK / K - 1) / (MAP_BLOCK / K)));
    LCHK(lin_alloc(h, &m.x, ndk)); LCHK(lin_alloc(h, &m.r, ndk)); LCHK(lin_alloc(h, &m.z, ndk)); LCHK(lin_alloc(h, &m.p, ndk));
    LCHK(lin_alloc(h, &m.q, ndk));
    LCHK(lin_alloc(h, &m.ebuf, (size_t)2 * h->p.F * h->D * K));
    LCHK(lin_alloc(h, &m.pq_part, (size_t)m.nb * K)); LCHK(lin_alloc(h, &m.rz_part, (size_t)2 * m.nb * K));
    LCHK(lin_alloc(h, &m.rr_part, (size_t)m.nb * K));
    LHIPCHK(hipMemsetAsync(m.pq_part, 0, (size_t)m.nb * K * sizeof(double), h->stream));
    LHIPCHK(hipMemsetAsync(m.rz_part, 0, (size_t)2 * m.nb * K * sizeof(double), h->stream));
    LHIPCHK(hipMemsetAsync(m.rr_part, 0, (size_t)m.nb * K * sizeof(double), h->stream));
    h->marg_ready = true;
    return GBP_OK;
}

// dst = Lambda_joint src for all columns (both device [N][d][K]); leaves the per-column partials of src . dst in pq_part
int marg_matvec(gbp_lin *h, const double *src, double *dst)
{
    const LinMarg &m = h->marg;
    lin_dispatch(h->D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        if (h->p.F)
            hipLaunchKernelGGL((k_marg_factor<DD>), dim3((h->p.F + MARG_FACTORS_PER_BLOCK - 1) / MARG_FACTORS_PER_BLOCK), dim3(MAP_BLOCK), 0,
                               h->stream, h->p, src, m.ebuf);
        hipLaunchKernelGGL((k_marg_var<DD>), dim3(m.nb), dim3(MAP_BLOCK), 0, h->stream, h->p, src, (const double *)m.ebuf, dst, m.pq_part);
    });
    LHIPCHK(hipGetLastError());
    return GBP_OK;
}

// the worst column's |r| from the per-block partials, each column added in block order
int marg_read_worst(gbp_lin *h, double *worst)
{
    const LinMarg &m = h->marg;
    std::vector<double> v((size_t)m.nb * K);
    LHIPCHK(hipMemcpyAsync(v.data(), m.rr_part, v.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LHIPCHK(hipStreamSynchronize(h->stream));
    double w = 0.0;
    for (int c = 0; c < K; ++c) {
        double s = 0.0;
        for (int b = 0; b < m.nb; ++b) s += v[(size_t)b * K + c];
        s = std::sqrt(s);
        if (w == w && !(s <= w)) w = s;                   // a NaN is the worst, and stays
    }
    *worst = w;
    return GBP_OK;
}

// r = e - q (use_q) or e, z, p = z and the partials the iteration `next_it` reads as old; *rel = the worst column's |r| (|e| = 1)
int marg_restart(gbp_lin *h, const MargCols &cols, int use_q, int next_it, double *rel)
{
    const LinMarg &m = h->marg;
    lin_dispatch(h->D, [&](auto d) {
        hipLaunchKernelGGL((k_marg_restart<decltype(d)::value>), dim3(m.nb), dim3(MAP_BLOCK), 0, h->stream, m, (const double *)h->map.ldl, cols,
                           h->p.N, use_q, (next_it & 1) ^ 1);
    });
    LHIPCHK(hipGetLastError());
    return marg_read_worst(h, rel);
}

// one batch, from x = 0
int marg_solve_batch(gbp_lin *h, const gbp_lin_map_opts_t &o, const MargCols &cols, int *iters, bool *converged_out, double *rel_out)
{
    const LinMarg &m = h->marg;
    const int N = h->p.N, D = h->D;
    LHIPCHK(hipMemsetAsync(m.x, 0, (size_t)N * D * K * sizeof(double), h->stream));
    double rel = 0.0;
    LCHK(marg_restart(h, cols, 0, 0, &rel));
    const int every = h->p.F ? o.check_every : 1;         // without factors the preconditioner is the matrix: one iteration is exact
    int it = 0;
    bool converged = rel <= o.rel_tol;                    // r = e: already the true residual
    while (!converged && it < o.max_iters) {
        const int n = std::min(every, o.max_iters - it);
        for (int j = 0; j < n; ++j, ++it) {
            LCHK(marg_matvec(h, m.p, m.q));
            lin_dispatch(D, [&](auto d) {
                constexpr int DD = decltype(d)::value;
                hipLaunchKernelGGL((k_marg_step<DD>), dim3(m.nb), dim3(MAP_BLOCK), 0, h->stream, m, (const double *)h->map.ldl, N, it & 1);
                hipLaunchKernelGGL((k_marg_dir<DD>), dim3(m.nb), dim3(MAP_BLOCK), 0, h->stream, m, N, it & 1);
            });
            LHIPCHK(hipGetLastError());
        }
        double claim = 0.0;
        LCHK(marg_read_worst(h, &claim));
        if (claim <= o.rel_tol || it >= o.max_iters) {
            LCHK(marg_matvec(h, m.x, m.q));               // the true residuals; the recurrence goes on from them if a claim was wrong
            LCHK(marg_restart(h, cols, 1, it, &rel));
            converged = rel <= o.rel_tol;
        }
    }
    *iters = it; *converged_out = converged; *rel_out = rel;
    return GBP_OK;
}

int marg_solve(gbp_lin *h, const int32_t *ids, int n_ids, const gbp_lin_map_opts_t &o, double *sigma, double *sigma_joint, gbp_lin_marg_info_t *info)
{
    LCHK(marg_prepare(h));
    const LinMarg &m = h->marg;
    const int D = h->D;
    const long long ncols = (long long)n_ids * D;
    const size_t n_sigma = (size_t)n_ids * D * D, n_joint = sigma_joint ? (size_t)ncols * (size_t)ncols : 0;
    LCHK(marg_stage_reserve(h, (n_sigma + n_joint) * sizeof(double) + (size_t)n_ids * sizeof(int32_t)));
    double *d_sigma = static_cast<double *>(m.stage), *d_joint = sigma_joint ? d_sigma + n_sigma : nullptr;
    const int *d_ids = reinterpret_cast<const int *>(d_sigma + n_sigma + n_joint);
    LHIPCHK(hipMemcpyAsync(const_cast<int *>(d_ids), ids, (size_t)n_ids * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    gbp_lin_marg_info_t out{0, 1, (int32_t)((ncols + K - 1) / K), 0, 0.0};
    const long long n_gather = sigma_joint ? ncols * K : (long long)D * K;
    const int gather_blocks = (int)std::min<long long>(MAP_MAX_BLOCKS, (n_gather + MAP_BLOCK - 1) / MAP_BLOCK);
    for (long long c0 = 0; c0 < ncols; c0 += K) {
        MargCols cols;
        for (int c = 0; c < K; ++c) {
            const bool live = c0 + c < ncols;
            cols.var[c] = live ? ids[(c0 + c) / D] : -1;
            cols.k[c] = live ? (int)((c0 + c) % D) : 0;
        }
        int it = 0;
        bool conv = false;
        double rel = 0.0;
        LCHK(marg_solve_batch(h, o, cols, &it, &conv, &rel));
        out.iters += it;
        if (!conv) out.converged = 0;
        if (out.rel_residual == out.rel_residual && !(rel <= out.rel_residual)) out.rel_residual = rel;
        lin_dispatch(D, [&](auto d) {
            hipLaunchKernelGGL((k_marg_gather<decltype(d)::value>), dim3(gather_blocks), dim3(MAP_BLOCK), 0, h->stream, (const double *)m.x,
                               d_ids, n_ids, (int)c0, (int)ncols, n_gather, d_sigma, d_joint);
        });
        LHIPCHK(hipGetLastError());
    }
    LHIPCHK(hipMemcpyAsync(sigma, d_sigma, n_sigma * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (sigma_joint) LHIPCHK(hipMemcpyAsync(sigma_joint, d_joint, n_joint * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LHIPCHK(hipStreamSynchronize(h->stream));
    if (info) *info = out;
    return GBP_OK;
}

}  // namespace

extern "C" {

int gbp_lin_solve_marginals(gbp_lin_t *h, const int32_t *ids, int32_t n_ids, const gbp_lin_map_opts_t *opts, double *sigma, double *sigma_joint,
                            gbp_lin_marg_info_t *info)
{
    LENTER(h);
    gbp_lin_map_opts_t o{1e-12, 10000, 8, 0};
    if (opts) o = *opts;
    if (!(o.rel_tol > 0.0)) return set_error(GBP_EINVAL, "rel_tol must be positive");
    if (o.max_iters < 0) return set_error(GBP_EINVAL, "negative max_iters");
    if (o.check_every < 1) return set_error(GBP_EINVAL, "check_every must be at least 1");
    if (o.warm_start) return set_error(GBP_EINVAL, "warm_start has no meaning for marginals: it must be 0");
    if (n_ids < 0) return set_error(GBP_EINVAL, "negative n_ids");
    if (n_ids == 0) {
        if (info) *info = gbp_lin_marg_info_t{0, 1, 0, 0, 0.0};
        return GBP_OK;
    }
    if (!ids) return set_error(GBP_EINVAL, "ids is NULL");
    if (!sigma) return set_error(GBP_EINVAL, "sigma is NULL");
    if ((long long)n_ids * h->D > (long long)INT32_MAX - GBP_LIN_MARG_COLS) return set_error(GBP_EINVAL, "too many columns");
    std::vector<int32_t> sorted(ids, ids + n_ids);
    std::sort(sorted.begin(), sorted.end());
    if (sorted.front() < 0 || sorted.back() >= h->p.N) return set_error(GBP_EINVAL, "a variable id is out of range [0, %d)", h->p.N);
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return set_error(GBP_EINVAL, "a variable id is listed twice");
    return marg_solve(h, ids, n_ids, o, sigma, sigma_joint, info);
}

}  // extern "C"
