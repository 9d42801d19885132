// lin_until_shim.hip -- TEST INFRASTRUCTURE: the per-variable and finishing routines of gbp_lin_iterate_until
// (gbp_amd/csrc/gbp_lin_until.hpp) compiled for the host, so that tests/test_linear_until_cpu.py can compare them with the numpy model of
// tests/lin_until_cases.py on a CPU.  The finishing block is run as the kernel runs it: every thread's strided share first, then the
// levels of the fixed tree one after the other.  Built host-only by that test with hipcc; nothing in the product links or loads it.
// With -DLIN_UNTIL_SHIM_MAIN it is a stand-alone program for a sanitizer pass.
#include "../../gbp_amd/csrc/gbp_lin_until.hpp"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace gbp;

extern "C" {

int lin_until_threads() { return UNTIL_FIN; }

// step[v], sq[v] of n variables from their new and old means [n][d] and (x != NULL) the MAP iterate [n][d]
void lin_until_vars(int D, int n, const double *mu_new, const double *mu_old, const double *x, double *step, double *sq)
{
    lin_dispatch(D, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        for (int v = 0; v < n; ++v) {
            double mu[DD];
            for (int k = 0; k < DD; ++k) mu[k] = mu_new[(size_t)v * DD + k];
            until_var<DD>(mu, mu_old + (size_t)v * DD, x ? x + (size_t)v * DD : nullptr, step[v], sq[v]);
        }
    });
}

// k_until_finish on the host: bel_part [2][nbel] (step partials, then sums of squares), en_part [nen] -> row[3]; returns the reason
int lin_until_finish(int nbel, const double *bel_part, int nen, const double *en_part, int want, double tol_step, double tol_map, double *row)
{
    const UntilRule r{want, tol_step, tol_map};
    std::vector<double> step(UNTIL_FIN), sq(UNTIL_FIN), en(UNTIL_FIN);
    for (int t = 0; t < UNTIL_FIN; ++t) {
        step[t] = until_strided_max(bel_part, nbel, t, UNTIL_FIN);
        sq[t] = (want & GBP_LIN_TRACE_MAP) ? until_strided_sum(bel_part + nbel, nbel, t, UNTIL_FIN) : 0.0;
        en[t] = (want & GBP_LIN_TRACE_ENERGY) ? until_strided_sum(en_part, nen, t, UNTIL_FIN) : 0.0;
    }
    for (int s = UNTIL_FIN / 2; s > 0; s >>= 1)
        for (int t = 0; t < s; ++t) until_fold(step.data(), sq.data(), en.data(), t, s);
    return until_row(r, step[0], sq[0], en[0], row);
}

}  // extern "C"

#ifdef LIN_UNTIL_SHIM_MAIN
// partial counts below, at and above the finishing block's thread count, with the largest step in the first, the last, a middle slot
int main()
{
    unsigned s = 777u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)(s >> 8) / (1 << 24); };
    for (int D = 1; D <= GBP_LIN_MAX_DOFS; ++D) {
        const int n = 11;
        std::vector<double> a((size_t)n * D), b((size_t)n * D), x((size_t)n * D), st(n), sq(n);
        for (auto *v : {&a, &b, &x}) for (double &e : *v) e = rnd();
        lin_until_vars(D, n, a.data(), b.data(), x.data(), st.data(), sq.data());
        for (int v = 0; v < n; ++v) {
            double m = 0.0, q = 0.0;
            for (int k = 0; k < D; ++k) { m = std::fmax(m, std::fabs(a[v * D + k] - b[v * D + k])); q += (a[v * D + k] - x[v * D + k]) * (a[v * D + k] - x[v * D + k]); }
            if (st[v] != m || std::fabs(sq[v] - q) > 1e-12) { std::printf("d=%d v=%d: per-variable values differ\n", D, v); return 1; }
        }
        lin_until_vars(D, n, a.data(), b.data(), nullptr, st.data(), sq.data());
        for (int v = 0; v < n; ++v) if (sq[v] != 0.0) return 1;
    }
    // ... and above 7 x the thread count, where a thread's strided loop takes eight partials at a time (with and without a tail)
    for (int nb : {0, 1, 5, UNTIL_FIN - 1, UNTIL_FIN, UNTIL_FIN + 1, 3 * UNTIL_FIN + 17, 7 * UNTIL_FIN + 1, 8 * UNTIL_FIN + 5, 16 * UNTIL_FIN, 19 * UNTIL_FIN + 9}) {
        for (int where = 0; where < 4; ++where) {
            const int ne = nb > 7 * UNTIL_FIN ? nb - 2 : nb / 2 + 1;
            const int tail = (nb / (8 * UNTIL_FIN)) * 8 * UNTIL_FIN + 2;                          // thread 2's first slot behind its batches
            const int at = where == 0 ? 0 : where == 1 ? nb - 1 : where == 2 ? nb / 2 : (tail < nb ? tail : nb / 3);
            std::vector<double> bel((size_t)2 * nb + 1), en(ne);
            double sum = 0.0, esum = 0.0, mx = 0.0;
            for (int i = 0; i < nb; ++i) { bel[i] = rnd(); bel[nb + i] = rnd(); }
            if (nb) bel[at] = 2.0;
            for (int i = 0; i < nb; ++i) { sum += bel[nb + i]; mx = std::fmax(mx, bel[i]); }
            for (int i = 0; i < ne; ++i) { en[i] = rnd(); esum += en[i]; }
            double row[3];
            const int reason = lin_until_finish(nb, bel.data(), ne, en.data(), GBP_LIN_TRACE_ENERGY | GBP_LIN_TRACE_MAP, 0.0, 1e9, row);
            if (row[0] != mx || std::fabs(row[1] - esum) > 1e-9 * (1.0 + esum) || std::fabs(row[2] - std::sqrt(sum)) > 1e-9 * (1.0 + sum) || reason != GBP_LIN_STOP_MAP) {
                std::printf("nb=%d where=%d: row (%g, %g, %g) reason %d\n", nb, where, row[0], row[1], row[2], reason);
                return 1;
            }
            if (lin_until_finish(nb, bel.data(), ne, en.data(), 0, 4.0, 0.0, row) != GBP_LIN_STOP_STEP || row[1] == row[1] || row[2] == row[2]) return 1;
        }
    }
    std::printf("lin_until_shim OK\n");
    return 0;
}
#endif
