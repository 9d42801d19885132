// lin_irls_shim.hip -- TEST INFRASTRUCTURE: the host side of the reweight lane of gbp_lin_solve_map_nonlinear_robust (gn_reweight_at,
// gbp_amd/csrc/gbp_lin_gn.hpp) run in a plain loop over the engine's own array layouts, for both models, so that
// tests/test_linear_irls_cpu.py can compare it with the numpy twin of tests/lin_irls_cases.py on a CPU.
// Built host-only by that test with hipcc; nothing in the product links or loads it.
#include "../../gbp_amd/csrc/gbp_lin_gn.hpp"

using namespace gbp;

extern "C" {

// x [N][D]; meas, sinfo [M][F] (SoA, stride F); loss, thr [F] or NULL (no losses set); w [F] holds the old weights on entry (not read
// when `first`) -> feta [2D][F], flam [P2][F], w, flag [F], and per factor the weighted energy (e) and |w_new - w_old| (change).
// Returns the number of flagged factors.
int lin_irls_reweight(int model, int N, int F, const int *va, const int *vb, const double *meas, const double *sinfo, const int *loss, const double *thr,
                      const double *x, int first, double *feta, double *flam, double *w, int *flag, double *e, double *change)
{
    LinParams p{};
    p.N = N; p.F = F; p.va = va; p.vb = vb;
    LinNonlin n{};
    n.meas = meas; n.sinfo = sinfo; n.model = model;
    int count = 0;
    for (int f = 0; f < F; ++f) {
        int fl = 0;
        if (model == GBP_LIN_MODEL_SE3_BETWEEN) e[f] = gn_reweight_at<GBP_LIN_MODEL_SE3_BETWEEN>(p, n, loss, thr, f, x, first != 0, feta, flam, w, flag, change[f], fl);
        else e[f] = gn_reweight_at<GBP_LIN_MODEL_SE2_BETWEEN>(p, n, loss, thr, f, x, first != 0, feta, flam, w, flag, change[f], fl);
        count += fl;
    }
    return count;
}

}  // extern "C"
