// lin_extend_shim.hip -- TEST INFRASTRUCTURE: the placement routines of gbp_lin_extend (gbp_amd/csrc/gbp_lin_extend.hpp: where an old
// edge lands, where a new one lands, the new vptr) compiled for the host and run in plain loops in the order of the kernels, so that
// tests/test_linear_extend_cpu.py can compare them with np.lexsort on a CPU.  The stable sort of the new edges by variable, which the
// device takes from gbp_sort.hip, is std::stable_sort here.  Built host-only by that test with hipcc; nothing in the product links or
// loads it.
#define GBP_LIN_EXTEND_ROUTINES_ONLY
#include "../../gbp_amd/csrc/gbp_lin_extend.hpp"

#include <algorithm>
#include <numeric>
#include <vector>

using namespace gbp;

extern "C" {

// old graph: N, F, va / vb [F], vptr [N + 1], vadj [2F]; appended: dN, dF, na / nb [dF].  Out: vptr_new [N + dN + 1], vadj_new,
// [2 (F + dF)], epos_a / epos_b [F + dF], enew [2F] (the new position of every old edge).  Every output is pre-filled by the caller with
// -1, so an entry nobody wrote shows.
void lin_extend_place(int N, int F, int dN, int dF, const int *va, const int *vb, const int *vptr, const int *vadj, const int *na, const int *nb,
                      int *vptr_new, int *vadj_new, int *epos_a, int *epos_b, int *enew)
{
    const int N1 = N + dN, E = 2 * dF;
    std::vector<int> keys(E), vals(E), order(E), skeys(E), svals(E);
    for (int j = 0; j < E; ++j) {                            // k_ext_edges
        keys[j] = (j & 1) ? nb[j >> 1] : na[j >> 1];
        vals[j] = ((F + (j >> 1)) << 1) | (j & 1);
    }
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return keys[x] < keys[y]; });
    for (int j = 0; j < E; ++j) { skeys[j] = keys[order[j]]; svals[j] = vals[order[j]]; }
    for (int v = 0; v <= N1; ++v) vptr_new[v] = lin_ext_new_ptr(vptr, N, skeys.data(), E, v);          // k_ext_vptr
    for (int e = 0; e < 2 * F; ++e) {                        // k_ext_old_edges
        const int fs = vadj[e];
        const int e1 = lin_ext_old_edge_pos(vptr, vptr_new, lin_ext_edge_var(va, vb, fs), e);
        vadj_new[e1] = fs;
        ((fs & 1) ? epos_b : epos_a)[fs >> 1] = e1;
        enew[e] = e1;
    }
    for (int j = 0; j < E; ++j) {                            // k_ext_new_edges
        const int e1 = lin_ext_new_edge_pos(vptr, N, skeys[j], j);
        const int fs = svals[j];
        vadj_new[e1] = fs;
        ((fs & 1) ? epos_b : epos_a)[fs >> 1] = e1;
    }
}

int lin_extend_lower_bound(const int *keys, int n, int v) { return lin_ext_lower_bound(keys, n, v); }

}  // extern "C"
