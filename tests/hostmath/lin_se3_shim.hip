// lin_se3_shim.hip -- TEST INFRASTRUCTURE: the model routines of the nonlinear path (NonlinModel<MODEL>, nonlin_factor / factor_store,
// nonlin_energy, nonlin_mahalanobis2; gbp_amd/csrc/gbp_lin_nonlin.hpp) compiled for the host for both models, so that
// tests/test_linear_se3_cpu.py can compare them with the numpy twins of tests/lin_se3_cases.py and tests/lin_nonlin_cases.py on a CPU.
// Built host-only by that test with hipcc; nothing in the product links or loads it.
#include "../../gbp_amd/csrc/gbp_lin_nonlin.hpp"

using namespace gbp;

namespace {

constexpr int SE2 = GBP_LIN_MODEL_SE2_BETWEEN, SE3 = GBP_LIN_MODEL_SE3_BETWEEN;

template <int MODEL, typename FN>
void each_point(int n, const double *x, const double *z, const double *s, FN &&fn)
{
    constexpr int D = NonlinModel<MODEL>::D, M = NonlinModel<MODEL>::M;
    for (int p = 0; p < n; ++p) {
        double xx[2 * D], zz[M], ss[M];
        for (int k = 0; k < 2 * D; ++k) xx[k] = x[(size_t)p * 2 * D + k];
        for (int k = 0; k < M; ++k) { zz[k] = z[(size_t)p * M + k]; ss[k] = s[(size_t)p * M + k]; }
        fn(p, xx, zz, ss);
    }
}

}  // namespace

extern "C" {

int lin_se3_dims(int model, int which)
{
    if (model == SE2) return which ? NonlinModel<SE2>::M : NonlinModel<SE2>::D;
    if (model == SE3) return which ? NonlinModel<SE3>::M : NonlinModel<SE3>::D;
    return 0;
}

// n points x [n][12], z, s [n][6] -> h [n][6], eta [n][12], lam [n][78] packed upper, energy [n], m2 [n].  The factor is written at
// stride n into a scratch block first -- the way the relinearise lane stores it -- and read back per point.
void lin_se3_eval(int n, const double *x, const double *z, const double *s, double *h, double *eta, double *lam, double *energy, double *m2)
{
    std::vector<double> se((size_t)12 * n), sl((size_t)78 * n);
    each_point<SE3>(n, x, z, s, [&](int p, const double (&xx)[12], const double (&zz)[6], const double (&ss)[6]) {
        double hh[6];
        NonlinModel<SE3>::eval(xx, ss, hh);
        for (int k = 0; k < 6; ++k) h[(size_t)p * 6 + k] = hh[k];
        NonlinModel<SE3>::factor_store(xx, zz, ss, se.data() + p, sl.data() + p, (size_t)n);
        energy[p] = nonlin_energy<SE3>(xx, zz, ss);
        m2[p] = nonlin_mahalanobis2<SE3>(xx, zz, ss);
    });
    for (int p = 0; p < n; ++p) {
        for (int k = 0; k < 12; ++k) eta[(size_t)p * 12 + k] = se[(size_t)k * n + p];
        for (int k = 0; k < 78; ++k) lam[(size_t)p * 78 + k] = sl[(size_t)k * n + p];
    }
}

// the same for the SE(2) model: x [n][6], z, s [n][3] -> h [n][3], eta [n][6], lam [n][21]
void lin_se2_eval(int n, const double *x, const double *z, const double *s, double *h, double *eta, double *lam, double *energy, double *m2)
{
    each_point<SE2>(n, x, z, s, [&](int p, const double (&xx)[6], const double (&zz)[3], const double (&ss)[3]) {
        double hh[3], ee[6], ll[21];
        NonlinModel<SE2>::eval(xx, ss, hh);
        nonlin_factor<SE2>(xx, zz, ss, ee, ll);
        for (int k = 0; k < 3; ++k) h[(size_t)p * 3 + k] = hh[k];
        for (int k = 0; k < 6; ++k) eta[(size_t)p * 6 + k] = ee[k];
        for (int k = 0; k < 21; ++k) lam[(size_t)p * 21 + k] = ll[k];
        energy[p] = nonlin_energy<SE2>(xx, zz, ss);
        m2[p] = nonlin_mahalanobis2<SE2>(xx, zz, ss);
    });
}

}  // extern "C"
