// lin_map_shim.hip -- TEST INFRASTRUCTURE: the per-factor and per-variable routines of the linear engine's batch-MAP solver
// (gbp_amd/csrc/gbp_lin_map.hpp) compiled for the host and driven through a whole block-Jacobi PCG in plain loops, so that
// tests/test_linear_map_cpu.py can compare them with np.linalg.solve and a numpy PCG on a CPU.  The arrays arrive in the engine's device
// layout (SoA factor rows, packed upper triangles, CSR adjacency), packed by the test.  Built host-only by that test with hipcc; nothing
// in the product links or loads it.  With -DLIN_MAP_SHIM_MAIN it is a stand-alone program (rings of every d) for a sanitizer pass.
#include "../../gbp_amd/csrc/gbp_lin_map.hpp"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace gbp;

namespace {

template <int D>
void matvec(const LinParams &p, const double *src, double *ebuf, double *dst, double *xy)
{
    for (int f = 0; f < p.F; ++f) {
        double ya[D], yb[D];
        map_factor_apply<D>(p, f, src, ya, yb);
        for (int k = 0; k < D; ++k) { ebuf[(size_t)p.epos_a[f] * D + k] = ya[k]; ebuf[(size_t)p.epos_b[f] * D + k] = yb[k]; }
    }
    double s = 0.0;
    for (int v = 0; v < p.N; ++v) s += map_var_gather<D>(p, v, src, ebuf, dst);
    if (xy) *xy = s;
}

template <int D>
int pcg(const LinParams &p, double rel_tol, int max_iters, double *x, double *rel_out)
{
    constexpr int P = LinDims<D>::P;
    const size_t nd = (size_t)p.N * D;
    std::vector<double> ldl((size_t)p.N * (P + D) + 1), jeta(nd + 1), r(nd + 1), z(nd + 1), pd(nd + 1), q(nd + 1), ebuf((size_t)2 * p.F * D + 1);
    double ee = 0.0, rz = 0.0, rr = 0.0;
    for (int v = 0; v < p.N; ++v) ee += map_var_setup<D>(p, v, ldl.data(), jeta.data());
    for (size_t i = 0; i < nd; ++i) x[i] = 0.0;
    *rel_out = 0.0;
    if (ee == 0.0) return 0;
    for (int v = 0; v < p.N; ++v) map_var_restart<D>(v, ldl.data(), jeta.data(), nullptr, r.data(), z.data(), pd.data(), rz, rr);
    int it = 0;
    while (std::sqrt(rr / ee) > rel_tol && it < max_iters) {
        double pq = 0.0;
        matvec<D>(p, pd.data(), ebuf.data(), q.data(), &pq);
        const double alpha = map_ratio(rz, pq);
        double rz_new = 0.0;
        rr = 0.0;
        for (int v = 0; v < p.N; ++v) map_var_step<D>(v, alpha, ldl.data(), pd.data(), q.data(), x, r.data(), z.data(), rz_new, rr);
        const double beta = map_ratio(rz_new, rz);
        for (int v = 0; v < p.N; ++v) map_var_dir<D>(v, beta, z.data(), pd.data());
        rz = rz_new;
        ++it;
    }
    matvec<D>(p, x, ebuf.data(), q.data(), nullptr);       // the true residual
    double tt = 0.0;
    for (size_t i = 0; i < nd; ++i) tt += (jeta[i] - q[i]) * (jeta[i] - q[i]);
    *rel_out = std::sqrt(tt / ee);
    return it;
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

// block-Jacobi PCG from x = 0, the recurrence's residual tested every iteration; returns the iteration count, x [N][d], *rel = the true
// relative residual at the end
int lin_map_pcg(int D, int N, int F, const int *va, const int *vb, const double *feta, const double *flam, const double *prior, const int *vptr,
                const int *vadj, const int *epos_a, const int *epos_b, double rel_tol, int max_iters, double *x, double *rel)
{
    const LinParams p = params(N, F, va, vb, feta, flam, prior, vptr, vadj, epos_a, epos_b);
    int it = -1;
    lin_dispatch(D, [&](auto d) { it = pcg<decltype(d)::value>(p, rel_tol, max_iters, x, rel); });
    return it;
}

// y = Lambda_joint x and eta_joint, [N][d] each
void lin_map_joint(int D, int N, int F, const int *va, const int *vb, const double *feta, const double *flam, const double *prior, const int *vptr,
                   const int *vadj, const int *epos_a, const int *epos_b, const double *x, double *y, double *eta)
{
    const LinParams p = params(N, F, va, vb, feta, flam, prior, vptr, vadj, epos_a, epos_b);
    lin_dispatch(D, [&](auto d) {
        constexpr int DD = decltype(d)::value, P = LinDims<DD>::P;
        std::vector<double> ldl((size_t)N * (P + DD) + 1), ebuf((size_t)2 * F * DD + 1);
        for (int v = 0; v < N; ++v) map_var_setup<DD>(p, v, ldl.data(), eta);
        matvec<DD>(p, x, ebuf.data(), y, nullptr);
    });
}

}  // extern "C"

#ifdef LIN_MAP_SHIM_MAIN
// a ring of n variables, each joined to its next two neighbours by a displacement factor ([I -I; -I I] / sigma^2), priors I / 9
int main()
{
    for (int D = 1; D <= GBP_LIN_MAX_DOFS; ++D) {
        const int N = 37, K = 2, F = N * K, D2 = 2 * D, P = D * (D + 1) / 2, P2 = D * (2 * D + 1);
        std::vector<int> va(F), vb(F), vptr(N + 1, 0), vadj(2 * F), ea(F), eb(F);
        std::vector<double> feta((size_t)D2 * F), flam((size_t)P2 * F, 0.0), prior((size_t)N * (D + P), 0.0), x((size_t)N * D);
        unsigned s = 12345u + D;
        auto at2 = [&](int i, int j) { return i * D2 - (i * (i - 1)) / 2 + (j - i); };     // packed upper 2d x 2d
        auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (1 << 24); };
        for (int f = 0; f < F; ++f) {
            va[f] = f / K; vb[f] = (f / K + 1 + f % K) % N;
            ++vptr[va[f] + 1]; ++vptr[vb[f] + 1];
            for (int i = 0; i < D; ++i) {
                const double zi = rnd() - 0.5;
                feta[(size_t)i * F + f] = -zi; feta[(size_t)(D + i) * F + f] = zi;
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
            for (int i = 0; i < D; ++i) {
                prior[(size_t)v * (D + P) + i] = rnd();
                prior[(size_t)v * (D + P) + D + i * D - (i * (i - 1)) / 2] = 1.0 / 9.0;
            }
        double rel = 1.0;
        const int it = lin_map_pcg(D, N, F, va.data(), vb.data(), feta.data(), flam.data(), prior.data(), vptr.data(), vadj.data(), ea.data(), eb.data(),
                                   1e-12, 200, x.data(), &rel);
        std::printf("d=%d iters=%d rel=%.3e\n", D, it, rel);
        if (it < 1 || it >= 200 || !(rel <= 2e-12)) return 1;
    }
    std::printf("lin_map_shim OK\n");
    return 0;
}
#endif
