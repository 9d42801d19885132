// build_plan_shim.hip -- TEST INFRASTRUCTURE: the host arithmetic of the graph build (gbp_amd/csrc/gbp_build_plan.hpp) behind extern "C"
// wrappers, so that tests/test_build_plan_host.py can pin the arena's size, the arrays placed in it and the sorts' bit counts on a CPU.
// Built host-only by that test with hipcc; nothing in the product links or loads it.
#include "../../gbp_amd/csrc/gbp_build_plan.hpp"

using namespace gbp;

static BuildSizes sizes(const long long *v)      // F, L, C, T, rows, n_wg, crow, general, remainder, robust, pack_mode
{
    return BuildSizes{(int)v[0], (int)v[1], (int)v[2], (int)v[3], v[4], (int)v[5], (int)v[6], v[7] != 0, v[8] != 0, v[9] != 0, (int)v[10]};
}

extern "C" {

int plan_bits_for(long long n) { return bits_for(n); }
unsigned long long plan_arena_need(const long long *v) { return build_arena_need(sizes(v)); }

// bytes of every array of the table that exists (0: it does not), in the table's order; returns their number
int plan_arena_table(const long long *v, unsigned long long *bytes)
{
    const auto t = build_arena_table(sizes(v));
    for (size_t i = 0; i < t.size(); ++i) bytes[i] = t[i].exists ? t[i].bytes() : 0;
    return (int)t.size();
}
int plan_uploads(int n_wg, int C, long long table_rows, int windowed, unsigned long long *bytes)
{
    const auto t = fused_plan_uploads(n_wg, C, table_rows, windowed != 0);
    for (size_t i = 0; i < t.size(); ++i) bytes[i] = t[i].exists ? t[i].bytes() : 0;
    return (int)t.size();
}
unsigned long long plan_arena_span(const long long *v) { return arena_span(build_arena_table(sizes(v))); }
unsigned long long plan_uploads_span(int n_wg, int C, long long table_rows, int windowed) { return fused_plan_arena_bytes(n_wg, C, table_rows, windowed != 0); }

// the layout constants the test's restatement of the formula is written with
int plan_constants(int *out)
{
    const int v[] = {WTILE, LIN_ROWS, MSG_ROWS, XTRA_ROW, LREC, TROW, CAMREC, CBEL, PART_ROW, RELIN_RING, RELIN_LANES, BLOCK, CSTAGE_ROW, CSTAGE_PLAIN,
                     (int)sizeof(int4), (int)sizeof(int2)};
    const int n = (int)(sizeof v / sizeof v[0]);
    for (int i = 0; i < n; ++i) out[i] = v[i];
    return n;
}

}  // extern "C"
