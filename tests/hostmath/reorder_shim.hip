// reorder_shim.hip -- TEST INFRASTRUCTURE: the landmark-ordering rule of gbp_amd/csrc/gbp_policy.hpp (reorder_class_key,
// reorder_spread_key) behind extern "C" wrappers, driven the way build_graph drives it (statistics, a stable sort by the class key, a
// stable sort by the spread key), so that tests/test_reorder_cpu.py can compare it with its numpy restatement on a CPU.  Built
// host-only by that test with hipcc; nothing in the product links or loads it.
#include "../../gbp_amd/csrc/gbp_fused_plan.hpp"
#include "../../gbp_amd/csrc/gbp_policy.hpp"

#include <algorithm>
#include <climits>
#include <numeric>
#include <vector>

using namespace gbp;

extern "C" {

int reorder_wide_span_of(int C) { return reorder_wide_span(C); }
int reorder_class_key_of(int deg, int lo, int hi, int C) { return reorder_class_key(deg, lo, hi, C); }
int reorder_spread_key_of(int pos, int n_local, int n_wide) { return reorder_spread_key(pos, n_local, n_wide); }
int reorder_fused_max_cams(void) { return fused_max_cams(); }

// internal_of_user[L] of F observations (cam, lmk) over C cameras
void reorder_order(const int *cam, const int *lmk, int F, int C, int L, int *internal_of_user)
{
    std::vector<int> deg((size_t)L, 0), lo((size_t)L, INT_MAX), hi((size_t)L, -1), key((size_t)L), first((size_t)L), key2((size_t)L), pos((size_t)L);
    for (int r = 0; r < F; ++r) { const int l = lmk[r]; ++deg[l]; lo[l] = std::min(lo[l], cam[r]); hi[l] = std::max(hi[l], cam[r]); }
    int n_local = 0, n_wide = 0;
    for (int l = 0; l < L; ++l) { key[l] = reorder_class_key(deg[l], lo[l], hi[l], C); n_local += key[l] < C; n_wide += key[l] == C; }
    std::iota(first.begin(), first.end(), 0);
    std::stable_sort(first.begin(), first.end(), [&](int a, int b) { return key[a] < key[b]; });
    for (int p = 0; p < L; ++p) key2[p] = reorder_spread_key(p, n_local, n_wide);
    std::iota(pos.begin(), pos.end(), 0);
    std::stable_sort(pos.begin(), pos.end(), [&](int a, int b) { return key2[a] < key2[b]; });
    for (int i = 0; i < L; ++i) internal_of_user[first[pos[i]]] = i;
}

}  // extern "C"
