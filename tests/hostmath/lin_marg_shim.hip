// lin_marg_shim.hip -- TEST INFRASTRUCTURE: the per-(item, column) routines of the linear engine's marginal-covariance solver
// (gbp_amd/csrc/gbp_lin_marg.hpp) compiled for the host and driven through whole multi-column block-Jacobi PCGs in plain loops, batch by
// batch as gbp_lin_solve_marginals does, so that tests/test_linear_marginals_cpu.py can compare them with np.linalg.inv on a CPU.  The
// arrays arrive in the engine's device layout, packed by the test (lin_map_cases.pack).  Built host-only by that test with hipcc; nothing
// in the product links or loads it.  With -DLIN_MARG_SHIM_MAIN it is a stand-alone program (rings of every d) for a sanitizer pass.
#include "../../gbp_amd/csrc/gbp_lin_marg.hpp"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace gbp;

namespace {

constexpr int K = MARG_COLS;

template <int D>
void matvec(const LinParams &p, const double *src, double *ebuf, double *dst, double *xy)
{
    for (int f = 0; f < p.F; ++f)
        for (int c = 0; c < K; ++c) marg_factor_store<D>(p, f, c, src, ebuf);
    for (int c = 0; c < K; ++c) xy[c] = 0.0;
    for (int v = 0; v < p.N; ++v)
        for (int c = 0; c < K; ++c) xy[c] += marg_var_gather<D>(p, v, c, src, ebuf, dst);
}

double worst(const double *rr)
{
    double w = 0.0;
    for (int c = 0; c < K; ++c) w = std::fmax(w, std::sqrt(rr[c]));
    return w;
}

// every batch from x = 0, the recurrence's residuals tested every iteration; the true residuals at the end of each batch
template <int D>
int marginals(const LinParams &p, const int *ids, int n_ids, double rel_tol, int max_iters, double *sigma, double *joint, double *rel_out)
{
    constexpr int P = LinDims<D>::P;
    const size_t nd = (size_t)p.N * D, ndk = nd * K;
    std::vector<double> ldl((size_t)p.N * (P + D) + 1), jeta(nd + 1), x(ndk + 1), r(ndk + 1), z(ndk + 1), pd(ndk + 1), q(ndk + 1),
        ebuf((size_t)2 * p.F * D * K + 1);
    for (int v = 0; v < p.N; ++v) map_var_setup<D>(p, v, ldl.data(), jeta.data());
    const int ncols = n_ids * D;
    int iters = 0;
    *rel_out = 0.0;
    for (int c0 = 0; c0 < ncols; c0 += K) {
        MargCols cols;
        for (int c = 0; c < K; ++c) {
            const bool live = c0 + c < ncols;
            cols.var[c] = live ? ids[(c0 + c) / D] : -1;
            cols.k[c] = live ? (c0 + c) % D : 0;
        }
        for (size_t i = 0; i < ndk; ++i) x[i] = 0.0;
        double rz[K] = {}, rr[K] = {}, pq[K];
        for (int v = 0; v < p.N; ++v)
            for (int c = 0; c < K; ++c) marg_var_restart<D>(v, c, cols, ldl.data(), nullptr, r.data(), z.data(), pd.data(), rz[c], rr[c]);
        int it = 0;
        while (worst(rr) > rel_tol && it < max_iters) {
            matvec<D>(p, pd.data(), ebuf.data(), q.data(), pq);
            double rz_new[K] = {};
            for (int c = 0; c < K; ++c) rr[c] = 0.0;
            for (int v = 0; v < p.N; ++v)
                for (int c = 0; c < K; ++c)
                    marg_var_step<D>(v, c, map_ratio(rz[c], pq[c]), ldl.data(), pd.data(), q.data(), x.data(), r.data(), z.data(), rz_new[c], rr[c]);
            for (int v = 0; v < p.N; ++v)
                for (int c = 0; c < K; ++c) marg_var_dir<D>(v, c, map_ratio(rz_new[c], rz[c]), z.data(), pd.data());
            for (int c = 0; c < K; ++c) rz[c] = rz_new[c];
            ++it;
        }
        iters += it;
        matvec<D>(p, x.data(), ebuf.data(), q.data(), pq);  // the true residuals
        double tz[K] = {}, tt[K] = {};
        for (int v = 0; v < p.N; ++v)
            for (int c = 0; c < K; ++c) marg_var_restart<D>(v, c, cols, ldl.data(), q.data(), r.data(), z.data(), pd.data(), tz[c], tt[c]);
        *rel_out = std::fmax(*rel_out, worst(tt));
        for (int c = 0; c < K; ++c)                         // a zero column stays exactly zero
            if (cols.var[c] < 0)
                for (size_t i = 0; i < nd; ++i)
                    if (x[i * K + c] != 0.0) return -1;
        const long long n_out = joint ? (long long)ncols * K : (long long)D * K;
        for (long long e = 0; e < n_out; ++e) marg_gather_one<D>(e, ids, n_ids, c0, ncols, x.data(), sigma, joint);
    }
    return iters;
}

LinParams params(int N, int F, const int *va, const int *vb, const double *feta, const double *flam, const double *prior, const int *vptr,
                 const int *vadj, const int *epos_a, const int *epos_b)
{
    LinParams p{};
    p.N = N; p.F = F; p.va = va; p.vb = vb; p.feta = feta; p.flam = flam; p.prior = prior; p.vptr = vptr; p.vadj = vadj; p.epos_a = epos_a; p.epos_b = epos_b;
    return p;
}

}  // namespace

extern "C" {

// sigma [n_ids][d][d] and (joint != NULL) joint [(n_ids d)][(n_ids d)] as gbp_lin_solve_marginals lays them out; returns the iterations
// summed over the batches (-1: a padded column did not stay zero), *rel = the worst column's true residual
int lin_marg_solve(int D, int N, int F, const int *va, const int *vb, const double *feta, const double *flam, const double *prior, const int *vptr,
                   const int *vadj, const int *epos_a, const int *epos_b, const int *ids, int n_ids, double rel_tol, int max_iters, double *sigma,
                   double *joint, double *rel)
{
    const LinParams p = params(N, F, va, vb, feta, flam, prior, vptr, vadj, epos_a, epos_b);
    int it = -1;
    lin_dispatch(D, [&](auto d) { it = marginals<decltype(d)::value>(p, ids, n_ids, rel_tol, max_iters, sigma, joint, rel); });
    return it;
}

}  // extern "C"

#ifdef LIN_MARG_SHIM_MAIN
// a ring of n variables, each joined to its next two neighbours by a displacement factor ([I -I; -I I]), priors I / 9; marginals of
// four variables in descending order with the joint block: symmetric, positive diagonal
int main()
{
    for (int D = 1; D <= GBP_LIN_MAX_DOFS; ++D) {
        const int N = 37, KN = 2, F = N * KN, D2 = 2 * D, P = D * (D + 1) / 2, P2 = D * (2 * D + 1);
        std::vector<int> va(F), vb(F), vptr(N + 1, 0), vadj(2 * F), ea(F), eb(F);
        std::vector<double> feta((size_t)D2 * F, 0.0), flam((size_t)P2 * F, 0.0), prior((size_t)N * (D + P), 0.0);
        auto at2 = [&](int i, int j) { return i * D2 - (i * (i - 1)) / 2 + (j - i); };     // packed upper 2d x 2d
        for (int f = 0; f < F; ++f) {
            va[f] = f / KN; vb[f] = (f / KN + 1 + f % KN) % N;
            ++vptr[va[f] + 1]; ++vptr[vb[f] + 1];
            for (int i = 0; i < D; ++i) {
                flam[(size_t)at2(i, i) * F + f] = 1.0; flam[(size_t)at2(i, D + i) * F + f] = -1.0; flam[(size_t)at2(D + i, D + i) * F + f] = 1.0;
            }
        }
        for (int v = 0; v < N; ++v) vptr[v + 1] += vptr[v];
        std::vector<int> fill(vptr.begin(), vptr.end() - 1);
        for (int f = 0; f < F; ++f) {
            ea[f] = fill[va[f]]; vadj[fill[va[f]]++] = f << 1;
            eb[f] = fill[vb[f]]; vadj[fill[vb[f]]++] = (f << 1) | 1;
        }
        for (int v = 0; v < N; ++v)
            for (int i = 0; i < D; ++i) prior[(size_t)v * (D + P) + D + i * D - (i * (i - 1)) / 2] = 1.0 / 9.0;
        const int ids[4] = {36, 20, 7, 0}, n = 4 * D;
        std::vector<double> sigma((size_t)4 * D * D, -1.0), joint((size_t)n * n, -1.0);
        double rel = 1.0;
        const int it = lin_marg_solve(D, N, F, va.data(), vb.data(), feta.data(), flam.data(), prior.data(), vptr.data(), vadj.data(), ea.data(), eb.data(),
                                      ids, 4, 1e-12, 200, sigma.data(), joint.data(), &rel);
        double asym = 0.0, dmin = 1e300;
        for (int i = 0; i < n; ++i) {
            dmin = std::fmin(dmin, joint[(size_t)i * n + i]);
            for (int j = 0; j < n; ++j) asym = std::fmax(asym, std::fabs(joint[(size_t)i * n + j] - joint[(size_t)j * n + i]));
        }
        std::printf("d=%d iters=%d rel=%.3e asym=%.3e min diag=%.3e\n", D, it, rel, asym, dmin);
        if (it < 1 || !(rel <= 2e-12) || !(asym <= 1e-10) || !(dmin > 0.0)) return 1;
    }
    std::printf("lin_marg_shim OK\n");
    return 0;
}
#endif
