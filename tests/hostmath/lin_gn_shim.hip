// lin_gn_shim.hip -- TEST INFRASTRUCTURE: the host side of the per-factor and per-variable routines of gbp_lin_solve_map_nonlinear
// (gn_factor_at, gn_var_damp, gn_var_diff; gbp_amd/csrc/gbp_lin_gn.hpp) run in plain loops over the engine's own array layouts, so that
// tests/test_linear_gn_cpu.py can compare them with the numpy twin of tests/lin_gn_cases.py on a CPU.
// Built host-only by that test with hipcc; nothing in the product links or loads it.
#include "../../gbp_amd/csrc/gbp_lin_gn.hpp"

using namespace gbp;

namespace {

template <typename K>
void by_model(int model, K &&k)
{
    if (model == GBP_LIN_MODEL_SE3_BETWEEN) k(std::integral_constant<int, GBP_LIN_MODEL_SE3_BETWEEN>{});
    else k(std::integral_constant<int, GBP_LIN_MODEL_SE2_BETWEEN>{});
}

}  // namespace

extern "C" {

double lin_gn_diag_floor() { return GN_DIAG_FLOOR; }

// Linearise-at-x with energy: x [N][D]; meas, sinfo [M][F] (SoA, stride F); w [F] or NULL -> feta [2D][F], flam [P2][F], and per factor
// the energy of the linearising instantiation (e_lin) and of the energy-only one (e_only)
void lin_gn_factors(int model, int N, int F, const int *va, const int *vb, const double *meas, const double *sinfo, const double *w, const double *x,
                    double *feta, double *flam, double *e_lin, double *e_only)
{
    LinParams p{};
    p.N = N; p.F = F; p.va = va; p.vb = vb; p.w = w;
    LinNonlin n{};
    n.meas = meas; n.sinfo = sinfo; n.model = model;
    by_model(model, [&](auto m) {
        constexpr int MODEL = decltype(m)::value;
        for (int f = 0; f < F; ++f) {
            e_lin[f] = gn_factor_at<MODEL, true>(p, n, f, x, feta, flam);
            e_only[f] = gn_factor_at<MODEL, false>(p, n, f, x, nullptr, nullptr);
        }
    });
}

// The damped prior: prior [N][D + P], flam [P2][F], CSR vptr / vadj (factor << 1 | side), w [F] or NULL -> dprior [N][D + P]
void lin_gn_damp(int D, int N, int F, const int *vptr, const int *vadj, const double *prior, const double *flam, const double *w, const double *x, double lambda,
                 double *dprior)
{
    LinParams p{};
    p.N = N; p.F = F; p.vptr = vptr; p.vadj = vadj; p.prior = prior; p.flam = flam; p.w = w;
    for (int v = 0; v < N; ++v) {
        if (D == 3) gn_var_damp<3>(p, v, x, lambda, dprior);
        else gn_var_damp<6>(p, v, x, lambda, dprior);
    }
}

// The prior difference: per variable (x_c - x)^T (Lambda0 (x_c + x) / 2 - eta0) -> diff [N]; returns max |x_c - x|
double lin_gn_diff(int D, int N, const double *prior, const double *x, const double *xc, double *diff)
{
    double mx = 0.0;
    for (int v = 0; v < N; ++v) diff[v] = D == 3 ? gn_var_diff<3>(prior, v, x, xc, mx) : gn_var_diff<6>(prior, v, x, xc, mx);
    return mx;
}

}  // extern "C"
