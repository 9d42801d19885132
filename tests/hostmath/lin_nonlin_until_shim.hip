// lin_nonlin_until_shim.hip -- TEST INFRASTRUCTURE: the decision routine of gbp_lin_iterate_until_nonlinear (until_row_settled,
// gbp_amd/csrc/gbp_lin_until.hpp) compiled for the host beside the linear call's until_row, so that
// tests/test_linear_nonlinear_until_cpu.py can compare both with the numpy model of tests/lin_nonlin_until_cases.py on a CPU.  Built
// host-only by that test with hipcc; nothing in the product links or loads it.
#include "../../gbp_amd/csrc/gbp_lin_until.hpp"

using namespace gbp;

extern "C" {

int lin_nl_until_settled_bit() { return GBP_LIN_UNTIL_SETTLED; }

// until_row_settled on reduced values; has_count == 0: the count pointer is NULL
int lin_nl_until_decide(int want, double tol_step, double tol_map, int has_count, int count, double step, double sq, double en, double *row)
{
    const UntilRule r{want, tol_step, tol_map};
    return until_row_settled(r, has_count ? &count : nullptr, step, sq, en, row);
}

// the same through the rule block the finishing kernel takes (UntilSettled) and the overload it calls
int lin_nl_until_decide_block(int want, double tol_step, double tol_map, int count, double step, double sq, double en, double *row)
{
    UntilSettled r;
    r.want = want; r.tol_step = tol_step; r.tol_map = tol_map; r.count = &count;
    return until_decide(r, step, sq, en, row);
}

// the linear call's routine, unchanged
int lin_nl_until_row(int want, double tol_step, double tol_map, double step, double sq, double en, double *row)
{
    const UntilRule r{want, tol_step, tol_map};
    return until_decide(r, step, sq, en, row) == until_row(r, step, sq, en, row) ? until_row(r, step, sq, en, row) : -1;
}

}  // extern "C"
