// lin_shrink_shim.hip -- TEST INFRASTRUCTURE: the index routines of gbp_lin_shrink (gbp_amd/csrc/gbp_lin_shrink.hpp: which factor
// survives, which side a leaving one folds towards, the three maps out of the scan, the new vptr, the renumbered adjacency entry)
// compiled for the host and run in plain loops in the order of the kernels, so that tests/test_linear_shrink_cpu.py can compare them
// with the CSR numpy builds for the survivors' graph on a CPU.  The exclusive scan, which the device takes from rocPRIM, is a running sum
// here.  Built host-only by that test with hipcc; nothing in the product links or loads it.
#define GBP_LIN_SHRINK_ROUTINES_ONLY
#include "../../gbp_amd/csrc/gbp_lin_shrink.hpp"

#include <vector>

using namespace gbp;

extern "C" {

// old graph: N, F, va / vb [F], vptr [N + 1], vadj [2F]; the lists: retire [nr], drop [nd]; fold 0 / 1.  Out: var_map [N], factor_map
// [F], edge_map [2F], fold_side [F], fold_edge [2F] (1: the edge's message is folded into its variable's prior), sizes [3] = N', F',
// 2F', vptr_new [N' + 1], vadj_new [2F'], epos_a / epos_b [F'].  Every output is pre-filled by the caller with -1 and sized for the
// old graph, so an entry nobody wrote shows.
void lin_shrink_place(int N, int F, const int *va, const int *vb, const int *vptr, const int *vadj, int nr, const int *retire, int nd, const int *drop, int fold,
                      int *var_map, int *factor_map, int *edge_map, int *fold_side, int *fold_edge, int *sizes, int *vptr_new, int *vadj_new, int *epos_a, int *epos_b)
{
    const int total = N + 3 * F;
    std::vector<int> vret(N, 0), fdrop(F, 0), keep(total + 1, 0), pos(total + 1, 0);
    for (int i = 0; i < nr; ++i) vret[retire[i]] = 1;        // k_shr_mark
    for (int i = 0; i < nd; ++i) fdrop[drop[i]] = 1;
    for (int i = 0; i <= total; ++i) {                       // k_shr_flags
        if (i == total) { keep[i] = 0; continue; }
        if (i < N) { keep[i] = !vret[i]; continue; }
        const bool edge = i >= N + F;
        const int f = edge ? (vadj[i - N - F] >> 1) : i - N;
        keep[i] = lin_shr_factor_keep(fdrop[f], vret[va[f]], vret[vb[f]]);
        if (!edge) fold_side[f] = lin_shr_fold_side(fdrop[f], vret[va[f]], vret[vb[f]], fold);
    }
    for (int i = 0, run = 0; i <= total; ++i) { pos[i] = run; run += keep[i]; }      // the exclusive scan
    sizes[0] = pos[N]; sizes[1] = pos[N + F] - pos[N]; sizes[2] = pos[total] - pos[N + F];              // k_shr_sizes
    for (int v = 0; v < N; ++v) var_map[v] = lin_shr_var_map(keep.data(), pos.data(), v);                // k_shr_maps
    for (int f = 0; f < F; ++f) factor_map[f] = lin_shr_factor_map(keep.data(), pos.data(), N, f);
    for (int v = 0; v <= N; ++v) {                           // k_shr_vptr
        if (v == N) vptr_new[sizes[0]] = lin_shr_new_ptr(pos.data(), vptr, N, F, N);
        else if (keep[v]) vptr_new[pos[v]] = lin_shr_new_ptr(pos.data(), vptr, N, F, v);
    }
    for (int e = 0; e < 2 * F; ++e) {                        // k_shr_edges
        const int e1 = lin_shr_edge_map(keep.data(), pos.data(), N, F, e);
        edge_map[e] = e1;
        if (e1 < 0) continue;
        const int fs = lin_shr_new_adj(pos.data(), N, vadj[e]);
        vadj_new[e1] = fs;
        ((fs & 1) ? epos_b : epos_a)[fs >> 1] = e1;
    }
    for (int v = 0; v < N; ++v) {                            // k_shr_fold: the edges a surviving variable adds to its prior
        if (!keep[v]) continue;
        for (int e = vptr[v]; e < vptr[v + 1]; ++e) fold_edge[e] = lin_shr_edge_folds(fold_side, vadj[e]) ? 1 : 0;
    }
}

}  // extern "C"
