// gbp_lin_capi_map.hip -- the batch MAP entry points of include/gbp_lin.h: FactorGraph.joint_distribution_inf / _cov (gbp.py:94-144) on
// the device, by block-Jacobi conjugate gradients over the handle's own arrays (kernels and method: gbp_lin_map.hpp).
//
// The joint system of a handle changes only with its robust weights (gbp_lin_capi_robust.hip): the diagonal-block factors and the joint
// eta are made by the first call that needs them, and again after the weights changed; the workspace once (all of it freed with the
// handle through `allocs`).  A solve queues
// four kernels per iteration on the handle's stream and reads |r|^2 back only every `check_every` iterations; when the recurrence claims
// convergence (or max_iters runs out) the TRUE residual eta - Lambda x is formed with one more product, and the recurrence restarts from
// it if the claim was wrong.  Nothing here touches the sweep's state (messages, beliefs, has_beliefs).
#include "gbp_lin_map.hpp"

#include <cmath>
#include <cstring>

using namespace gbp;

namespace {

// sum of the first nb doubles of a partials array, in index order
int map_read_sum(gbp_lin *h, const LinMap &m, const double *part, double *out)
{
    std::vector<double> v((size_t)m.nb);
    LHIPCHK(hipMemcpyAsync(v.data(), part, v.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    LHIPCHK(hipStreamSynchronize(h->stream));
    double s = 0.0;
    for (double x : v) s += x;
    *out = s;
    return GBP_OK;
}

}  // namespace

// The host side of the iteration, over the joint that `p` names (factors, priors, weights) in the workspace `m`: the handle's own for
// gbp_lin_solve_map, a copy pointing at a linearisation and damped priors of its own for gbp_lin_solve_map_nonlinear
// (gbp_lin_capi_map_nonlin.hip).  None of them looks at map_ready, map_solved or map_eta_norm: those belong to the callers.
namespace gbp {

// the workspace: once per generation of the handle
int lin_map_workspace(gbp_lin *h)
{
    if (h->map_alloc) return GBP_OK;
    LinMap &m = h->map;
    const int D = h->D, P = D * (D + 1) / 2;
    const size_t nd = (size_t)h->p.N * D;
    m.nb = std::min(MAP_MAX_BLOCKS, std::max(1, (h->p.N + MAP_BLOCK - 1) / MAP_BLOCK));
    LCHK(lin_alloc(h, &m.ldl, (size_t)h->p.N * (P + D))); LCHK(lin_alloc(h, &m.jeta, nd));
    LCHK(lin_alloc(h, &m.x, nd)); LCHK(lin_alloc(h, &m.r, nd)); LCHK(lin_alloc(h, &m.z, nd)); LCHK(lin_alloc(h, &m.p, nd)); LCHK(lin_alloc(h, &m.q, nd));
    LCHK(lin_alloc(h, &m.ebuf, (size_t)2 * h->p.F * D));
    LCHK(lin_alloc(h, &m.pq_part, (size_t)m.nb)); LCHK(lin_alloc(h, &m.rz_part, (size_t)2 * m.nb)); LCHK(lin_alloc(h, &m.rr_part, (size_t)m.nb));
    LHIPCHK(hipMemsetAsync(m.pq_part, 0, (size_t)m.nb * sizeof(double), h->stream));
    LHIPCHK(hipMemsetAsync(m.rz_part, 0, (size_t)2 * m.nb * sizeof(double), h->stream));
    LHIPCHK(hipMemsetAsync(m.rr_part, 0, (size_t)m.nb * sizeof(double), h->stream));
    h->map_alloc = true;
    return GBP_OK;
}

// LDL^T of the diagonal blocks, joint eta and its norm
int lin_map_setup(gbp_lin *h, const LinParams &p, const LinMap &m, double *eta_norm)
{
    double ee = 0.0;
    if (p.N) {
        lin_dispatch(h->D, [&](auto d) {
            hipLaunchKernelGGL((k_map_setup<decltype(d)::value>), dim3(m.nb), dim3(MAP_BLOCK), 0, h->stream, p, m);
        });
        LHIPCHK(hipGetLastError());
        LCHK(map_read_sum(h, m, m.rr_part, &ee));
    }
    *eta_norm = std::sqrt(ee);
    return GBP_OK;
}

// dst = Lambda_joint src (both device [N][d]); leaves the partials of src . dst in pq_part
int lin_map_matvec(gbp_lin *h, const LinParams &p, const LinMap &m, const double *src, double *dst)
{
    if (!p.N) return GBP_OK;
    lin_dispatch(h->D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        if (p.F) hipLaunchKernelGGL((k_map_factor<DD>), dim3((p.F + 63) / 64), dim3(64), 0, h->stream, p, src, m.ebuf);
        hipLaunchKernelGGL((k_map_var<DD>), dim3(m.nb), dim3(MAP_BLOCK), 0, h->stream, p, src, (const double *)m.ebuf, dst, m.pq_part);
    });
    LHIPCHK(hipGetLastError());
    return GBP_OK;
}

// r = eta - q (use_q) or eta, z, p = z and the partials the iteration `next_it` reads as old; *rnorm = |r|
int lin_map_restart(gbp_lin *h, const LinParams &p, const LinMap &m, int use_q, int next_it, double *rnorm)
{
    lin_dispatch(h->D, [&](auto d) {
        hipLaunchKernelGGL((k_map_restart<decltype(d)::value>), dim3(m.nb), dim3(MAP_BLOCK), 0, h->stream, m, p.N, use_q, (next_it & 1) ^ 1);
    });
    LHIPCHK(hipGetLastError());
    double rr = 0.0;
    LCHK(map_read_sum(h, m, m.rr_part, &rr));
    *rnorm = std::sqrt(rr);
    return GBP_OK;
}

// The solve, x in m.x; `start`: LIN_MAP_FROM_ZERO, LIN_MAP_FROM_MEANS (the belief means), LIN_MAP_FROM_X (what m.x holds).  *rnorm0:
// |eta - Lambda x0|, the first true residual.
int lin_map_solve(gbp_lin *h, const LinParams &p, const LinMap &m, double eta_norm, const gbp_lin_map_opts_t &o, int start, gbp_lin_map_info_t *info, double *rnorm0)
{
    const int N = p.N, D = h->D;
    const size_t bytes = (size_t)N * D * sizeof(double);
    gbp_lin_map_info_t out{0, 1, 0.0, eta_norm};
    if (rnorm0) *rnorm0 = 0.0;
    if (!N || !(eta_norm > 0.0)) {                        // eta = 0 (or no variables): x = 0
        if (!N || eta_norm == 0.0) {
            if (bytes) LHIPCHK(hipMemsetAsync(m.x, 0, bytes, h->stream));
            LHIPCHK(hipStreamSynchronize(h->stream));
            if (info) *info = out;
            return GBP_OK;
        }
        return set_error(GBP_EINVAL, "the joint eta is not finite");
    }
    double rn = 0.0;
    if (start != LIN_MAP_FROM_ZERO) {
        if (start == LIN_MAP_FROM_MEANS) {
            lin_dispatch(D, [&](auto d) {
                hipLaunchKernelGGL((k_map_load_means<decltype(d)::value>), dim3(m.nb), dim3(MAP_BLOCK), 0, h->stream, p, m);
            });
            LHIPCHK(hipGetLastError());
        }
        LCHK(lin_map_matvec(h, p, m, m.x, m.q));
        LCHK(lin_map_restart(h, p, m, 1, 0, &rn));
    } else {
        LHIPCHK(hipMemsetAsync(m.x, 0, bytes, h->stream));
        LCHK(lin_map_restart(h, p, m, 0, 0, &rn));
    }
    if (rnorm0) *rnorm0 = rn;
    double rel = rn / eta_norm;
    // with no factors the preconditioner is the matrix: one iteration is exact, so it is tested after one
    const int every = p.F ? o.check_every : 1;
    int it = 0;
    bool converged = rel <= o.rel_tol;                    // r was formed from eta and x0 directly: already the true residual
    while (!converged && it < o.max_iters) {
        const int n = std::min(every, o.max_iters - it);
        for (int j = 0; j < n; ++j, ++it) {
            LCHK(lin_map_matvec(h, p, m, m.p, m.q));
            lin_dispatch(D, [&](auto d) {
                constexpr int DD = decltype(d)::value;
                hipLaunchKernelGGL((k_map_step<DD>), dim3(m.nb), dim3(MAP_BLOCK), 0, h->stream, m, N, it & 1);
                hipLaunchKernelGGL((k_map_dir<DD>), dim3(m.nb), dim3(MAP_BLOCK), 0, h->stream, m, N, it & 1);
            });
            LHIPCHK(hipGetLastError());
        }
        double rr = 0.0;
        LCHK(map_read_sum(h, m, m.rr_part, &rr));
        if (std::sqrt(rr) / eta_norm <= o.rel_tol || it >= o.max_iters) {
            LCHK(lin_map_matvec(h, p, m, m.x, m.q));      // the true residual; the recurrence goes on from it if the claim was wrong
            LCHK(lin_map_restart(h, p, m, 1, it, &rn));
            rel = rn / eta_norm;
            converged = rel <= o.rel_tol;
        }
    }
    LHIPCHK(hipStreamSynchronize(h->stream));
    out.iters = it; out.converged = converged ? 1 : 0; out.rel_residual = rel;
    if (info) *info = out;
    return GBP_OK;
}

// The handle's own joint.  LDL^T of the diagonal blocks, joint eta and its norm: by the first call that needs them, and again -- into
// the same workspace, nothing allocated -- by the first call after the robust weights or the linearisation changed (map_ready cleared).
// The iterate x of the last solve is not touched.
int lin_map_prepare(gbp_lin *h)
{
    if (h->map_ready) return GBP_OK;
    LCHK(lin_map_workspace(h));
    LCHK(lin_map_setup(h, h->p, h->map, &h->map_eta_norm));
    h->map_ready = true;
    return GBP_OK;
}

}  // namespace gbp

namespace {

int map_prepare(gbp_lin *h) { return lin_map_prepare(h); }
int map_matvec(gbp_lin *h, const double *src, double *dst) { return lin_map_matvec(h, h->p, h->map, src, dst); }

int map_solve(gbp_lin *h, const gbp_lin_map_opts_t &o, gbp_lin_map_info_t *info)
{
    LCHK(map_prepare(h));
    h->map_solved = false;
    LCHK(lin_map_solve(h, h->p, h->map, h->map_eta_norm, o, o.warm_start ? LIN_MAP_FROM_MEANS : LIN_MAP_FROM_ZERO, info, nullptr));
    h->map_solved = true;
    return GBP_OK;
}

int map_download(gbp_lin *h, const double *src, double *dst)
{
    const size_t bytes = (size_t)h->p.N * h->D * sizeof(double);
    if (bytes) LHIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    LHIPCHK(hipStreamSynchronize(h->stream));
    return GBP_OK;
}

}  // namespace

extern "C" {

int gbp_lin_joint_matvec(gbp_lin_t *h, const double *x, double *y)
{
    LENTER(h);
    if (!x || !y) return set_error(GBP_EINVAL, "x or y is NULL");
    LCHK(map_prepare(h));
    const size_t bytes = (size_t)h->p.N * h->D * sizeof(double);
    if (bytes) LHIPCHK(hipMemcpyAsync(h->map.p, x, bytes, hipMemcpyHostToDevice, h->stream));   // p / q are scratch between solves
    LCHK(map_matvec(h, h->map.p, h->map.q));
    return map_download(h, h->map.q, y);
}

int gbp_lin_joint_eta(gbp_lin_t *h, double *eta)
{
    LENTER(h);
    if (!eta) return set_error(GBP_EINVAL, "eta is NULL");
    LCHK(map_prepare(h));
    return map_download(h, h->map.jeta, eta);
}

int gbp_lin_solve_map(gbp_lin_t *h, const gbp_lin_map_opts_t *opts, gbp_lin_map_info_t *info)
{
    LENTER(h);
    gbp_lin_map_opts_t o{1e-12, 10000, 8, 0};
    if (opts) o = *opts;
    if (!(o.rel_tol > 0.0)) return set_error(GBP_EINVAL, "rel_tol must be positive");
    if (o.max_iters < 0) return set_error(GBP_EINVAL, "negative max_iters");
    if (o.check_every < 1) return set_error(GBP_EINVAL, "check_every must be at least 1");
    if (o.warm_start && !h->has_beliefs) return set_error(GBP_ESTATE, "warm_start needs beliefs: call gbp_lin_update_beliefs first");
    return map_solve(h, o, info);
}

int gbp_lin_get_map(gbp_lin_t *h, double *mu)
{
    LENTER(h);
    if (!mu) return set_error(GBP_EINVAL, "mu is NULL");
    if (!h->map_solved) return set_error(GBP_ESTATE, "call gbp_lin_solve_map first");
    return map_download(h, h->map.x, mu);
}

int gbp_lin_map_distance(gbp_lin_t *h, double *out)
{
    LENTER(h);
    if (!out) return set_error(GBP_EINVAL, "out is NULL");
    if (!h->has_beliefs) return set_error(GBP_ESTATE, "beliefs have not been computed yet");
    if (!h->map_solved) return set_error(GBP_ESTATE, "call gbp_lin_solve_map first");
    double s = 0.0;
    if (h->p.N) {
        lin_dispatch(h->D, [&](auto d) {
            hipLaunchKernelGGL((k_map_distance<decltype(d)::value>), dim3(h->map.nb), dim3(MAP_BLOCK), 0, h->stream, h->p, h->map);
        });
        LHIPCHK(hipGetLastError());
        LCHK(map_read_sum(h, h->map, h->map.pq_part, &s));
    }
    *out = std::sqrt(s);
    return GBP_OK;
}

}  // extern "C"
