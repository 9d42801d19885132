// lin_robust_shim.hip -- TEST INFRASTRUCTURE: the per-factor routines of the linear engine's robust losses
// (gbp_amd/csrc/gbp_lin_robust.hpp: the residual-form energy, the weight and the flag) compiled for the host and run in plain loops, so
// that tests/test_linear_robust_cpu.py can compare them with a numpy oracle on a CPU.  The arrays arrive in the engine's device layout
// (SoA factor rows, packed upper triangles, belief records), packed by the test.  Built host-only by that test with hipcc; nothing in
// the product links or loads it.  With -DLIN_ROBUST_SHIM_MAIN it is a stand-alone program (displacement rings of every d with outliers)
// for a sanitizer pass.
#include "../../gbp_amd/csrc/gbp_lin_robust.hpp"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace gbp;

extern "C" {

// w [F], flag [F] at the means held in the belief records `bel` [N][d + P + d]; energy [F] (NULL ok): the per-factor e_f = M_f^2 / 2
void lin_robust_weights(int D, int N, int F, const int *va, const int *vb, const double *feta, const double *flam, const double *fconst,
                        const double *bel, const int *loss, const double *thr, const double *nvar, double *w, int *flag, double *energy)
{
    LinParams p{};
    p.N = N; p.F = F; p.va = va; p.vb = vb; p.feta = feta; p.flam = flam; p.fconst = fconst; p.bel = const_cast<double *>(bel);
    const LinRobust r{loss, thr, nvar, w, flag};
    lin_dispatch(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        for (int f = 0; f < F; ++f) {
            lin_robustify_one<DD>(p, r, f);
            if (energy) energy[f] = lin_factor_energy<DD>(p, f);
        }
    });
}

// the weight function alone: w and flag from a given e = M^2 / 2
double lin_robust_weight_of(int loss, double thr, double nvar, double e, int *flag) { return lin_robust_weight(loss, thr, nvar, e, *flag); }

}  // extern "C"

#ifdef LIN_ROBUST_SHIM_MAIN
// a ring of n variables joined to their next two neighbours by displacement factors ([I -I; -I I] / sigma^2); every fifth measurement
// is 30 sigma off; means = the true positions.  Checks every weight against |x_b - x_a - z| / sigma taken directly.
int main()
{
    for (int D = 1; D <= GBP_LIN_MAX_DOFS; ++D) {
        const int N = 37, K = 2, F = N * K, D2 = 2 * D, P = D * (D + 1) / 2, P2 = D * (2 * D + 1), REC = D + P + D;
        const double sigma = 0.1, s2 = sigma * sigma, t = 2.0;
        std::vector<int> va(F), vb(F), loss(F), flag(F);
        std::vector<double> feta((size_t)D2 * F), flam((size_t)P2 * F, 0.0), fconst(F, 0.0), bel((size_t)N * REC, 0.0), thr(F, t), nvar(F, s2), w(F), en(F), zz((size_t)F * D);
        unsigned s = 2200u + D;
        auto at2 = [&](int i, int j) { return i * D2 - (i * (i - 1)) / 2 + (j - i); };     // packed upper 2d x 2d
        auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (1 << 24); };
        for (int v = 0; v < N; ++v)
            for (int i = 0; i < D; ++i) bel[(size_t)v * REC + D + P + i] = 1000.0 + 10.0 * rnd();
        for (int f = 0; f < F; ++f) {
            va[f] = f / K; vb[f] = (f / K + 1 + f % K) % N;
            loss[f] = f % 3;
            for (int i = 0; i < D; ++i) {
                const double zi = bel[(size_t)vb[f] * REC + D + P + i] - bel[(size_t)va[f] * REC + D + P + i] + sigma * (rnd() - 0.5) + (f % 5 == 0 ? 30.0 * sigma : 0.0);
                zz[(size_t)f * D + i] = zi;
                feta[(size_t)i * F + f] = -zi / s2; feta[(size_t)(D + i) * F + f] = zi / s2;
                flam[(size_t)at2(i, i) * F + f] = 1.0 / s2; flam[(size_t)at2(i, D + i) * F + f] = -1.0 / s2; flam[(size_t)at2(D + i, D + i) * F + f] = 1.0 / s2;
                fconst[f] += 0.5 * zi * zi / s2;
            }
        }
        lin_robust_weights(D, N, F, va.data(), vb.data(), feta.data(), flam.data(), fconst.data(), bel.data(), loss.data(), thr.data(), nvar.data(),
                           w.data(), flag.data(), en.data());
        int n_robust = 0;
        for (int f = 0; f < F; ++f) {
            double m2 = 0.0;
            for (int i = 0; i < D; ++i) {
                const double r = bel[(size_t)vb[f] * REC + D + P + i] - bel[(size_t)va[f] * REC + D + P + i] - zz[(size_t)f * D + i];
                m2 += r * r / s2;
            }
            const double m = std::sqrt(m2);
            const bool rob = loss[f] != 0 && m > t;
            const double want = !rob ? 1.0 : loss[f] == 1 ? (2 * t * m - t * t) / m2 : s2 / m2;
            n_robust += rob;
            if (flag[f] != (int)rob || !(std::fabs(w[f] - want) <= 1e-6 * want)) {
                std::printf("d=%d factor %d: w %.12g want %.12g flag %d want %d\n", D, f, w[f], want, flag[f], (int)rob);
                return 1;
            }
        }
        std::printf("d=%d factors=%d robust=%d\n", D, F, n_robust);
        if (n_robust < 1) return 1;
    }
    std::printf("lin_robust_shim OK\n");
    return 0;
}
#endif
