// gbp_build_plan.hpp -- the arithmetic of gbp::build_graph (gbp_capi_build.hip) that needs no device: which arrays come out of the handle's
// arena and how large they are, how large the arena is, what the fused plan may take from it afterwards, and the bit counts of the sorts.
// Host-only and pure, like gbp_policy.hpp, so tests/test_build_plan_host.py pins on a CPU that the arena covers everything placed in it:
// an array that does not fit is not an error (dev_alloc and arena_take fall back to a separate hipMalloc), it only moves a sweep's
// working set out of the one block -- the slow placement arena_reserve (gbp_handle.hpp) exists to avoid.
#pragma once
#include "gbp_fused_plan.hpp"

#include <array>
#include <cstddef>

namespace gbp {

// smallest b >= 1 with 2^b >= n: the key bits of a radix sort over [0, n), the levels of the packer's pointer doubling
constexpr int bits_for(long long n)
{
    int b = 1;
    while ((1ll << b) < n) ++b;
    return b;
}

// what the build knows when it reserves the arena
struct BuildSizes {
    int F, L, C, T;              // factors, landmarks, cameras, tiles (after the dense decision)
    long long rows;              // rows of the fused sweep's workgroup tables: n_wg * C, or the sum of the camera windows
    int n_wg;                    // workgroups of the fused sweep (fused_workgroups)
    int crow;                    // doubles per row of the general sweep's staging buffer (Params::crow)
    bool general;                // the general sweep may run (general_sweep): its staging buffer comes out of the arena
    bool remainder;              // num_undamped_iters == 0: every factor carries the dense remainder (Params::xtra)
    bool robust;                 // loss != none: adaptive variances (Params::avar)
    int pack_mode;               // != 0: some landmarks span tiles (Params::parts)
    size_t slots() const { return std::max<size_t>((size_t)T * WTILE, 1); }
};

constexpr size_t ARENA_ALIGN = 4096;      // dev_alloc and arena_take start every array on a page
constexpr size_t arena_round(size_t bytes) { return (bytes + ARENA_ALIGN - 1) & ~(ARENA_ALIGN - 1); }

// One array placed in the arena: `count` elements of `elem` bytes, cleared or not, and whether this graph has it at all.
struct ArenaEntry {
    const char *name;
    size_t count, elem;
    bool zero, exists;
    size_t bytes() const { return count * elem; }
};

// The arrays reserve_and_allocate (gbp_capi_build.hip) takes from the arena, IN THE ORDER it takes them -- the order fixes every offset.
// Its list of destinations is indexed by this enum.
enum ArenaArray { A_CSTAGE, A_LIN, A_MSG, A_XTRA, A_AVAR, A_CPOS, A_LREC, A_PARTS, A_CBEL, A_CPRIOR, A_CBELIEF, A_PARTIAL, A_RED, A_RELIN_RING,
                  A_COUNT, A_VARMAX, ARENA_ARRAYS };
inline std::array<ArenaEntry, ARENA_ARRAYS> build_arena_table(const BuildSizes &z)
{
    const size_t S = z.slots(), F1 = (size_t)std::max(z.F, 1), L1 = (size_t)std::max(z.L, 1), C1 = (size_t)std::max(z.C, 1), T1 = (size_t)std::max(z.T, 1);
    const size_t D = sizeof(double), I = sizeof(int);
    return {{
        {"cstage", F1 * z.crow, D, true, z.general && z.F > 0},          // else: on first use (ensure_staging)
        {"lin", S * LIN_ROWS, D, true, true},
        {"msg", S * MSG_ROWS, D, true, true},
        {"xtra", S * XTRA_ROW, D, true, z.remainder},                    // damped in the relinearising sweep: gbp_math.hpp header
        {"avar", S, D, true, z.robust},                                  // adaptive variances: robust losses only
        {"cpos", S, I, true, true},
        {"lrec", L1 * LREC, D, true, true},
        {"parts", 2 * T1 * PART_ROW, D, true, z.pack_mode != 0},
        {"cbel", C1 * CAMREC, D, true, true},
        {"cprior", C1 * 27, D, true, true},
        {"cbelief", C1 * CBEL, D, true, true},
        {"d_partial", C1 * 27, D, true, true},
        {"d_red", 2 * ((S + BLOCK - 1) / BLOCK), D, true, true},
        {"d_relin_ring", (size_t)RELIN_RING * RELIN_LANES, I, true, true},
        {"d_count", 2, I, true, true},
        {"d_varmax", (size_t)std::max(z.C + z.L, 1), D, false, true},
    }};
}

// What fused_plan (gbp_fused.hpp) takes through FusedPlan::alloc, in its order: one entry per fused_upload call there.  table_rows is
// n_wg * C without camera windows, the sum of the workgroups' sets with them; every size is exact (fused_upload rounds an empty array up
// to one element, as here).  The scratch builds of tools/ (GBP_FUSED_DBG_SWITCHES, GBP_PHASE_TIMING) upload a phase buffer on top of
// these; it is not counted, the arena's slack takes it or it falls back.
constexpr int PLAN_UPLOADS = 5;
inline std::array<ArenaEntry, PLAN_UPLOADS> fused_plan_uploads(int n_wg, int C, long long table_rows, bool windowed)
{
    const size_t R = (size_t)std::max<long long>(table_rows, 0), R1 = std::max<size_t>(R, 1);
    return {{
        {"block_partials", std::max<size_t>(R * TROW, 1), sizeof(double), false, true},
        {"win", (size_t)std::max(n_wg, 1), sizeof(int4), false, windowed},
        {"rowidx", R1, sizeof(int), false, windowed},
        {"wgcams", R1, sizeof(int), false, windowed},
        {"cam_rows", (size_t)std::max(C, 1), sizeof(int2), false, windowed},
    }};
}

// the most the arena's fill mark can advance over these entries: each array starts on a page
template <size_t N>
inline size_t arena_span(const std::array<ArenaEntry, N> &t)
{
    size_t n = 0;
    for (const ArenaEntry &e : t) n += e.exists ? arena_round(e.bytes()) : 0;
    return n;
}
inline size_t fused_plan_arena_bytes(int n_wg, int C, long long table_rows, bool windowed) { return arena_span(fused_plan_uploads(n_wg, C, table_rows, windowed)); }

// Bytes of the arena.  The terms follow the arrays and uploads above; the constants are page slack for their starts.  The value fixes
// no offset, but it is kept as it was measured with (a larger block may land elsewhere): change a term only with the array it pays for.
inline size_t build_arena_need(const BuildSizes &z)
{
    const size_t S = z.slots(), F1 = (size_t)std::max(z.F, 1), L1 = (size_t)std::max(z.L, 1), C1 = (size_t)std::max(z.C, 1), T1 = (size_t)std::max(z.T, 1);
    const size_t R1 = (size_t)std::max<long long>(z.rows, 1), D = sizeof(double), I = sizeof(int);
    return (z.general ? F1 * z.crow * D + (64 << 8) : 0)                                  // cstage, and slack for it
           + S * (LIN_ROWS + MSG_ROWS + (z.remainder ? XTRA_ROW : 0) + (z.robust ? 1 : 0)) * D    // lin, msg, xtra, avar
           + S * I                                                                        // cpos
           + L1 * LREC * D                                                                // lrec
           + R1 * (TROW * D + 2 * I)                                                      // plan: block_partials, rowidx, wgcams
           + (size_t)z.n_wg * sizeof(int4)                                                // plan: win
           + C1 * sizeof(int2)                                                            // plan: cam_rows
           + 4 * 4096                                                                     // slack: the starts of the plan's uploads
           + C1 * (CAMREC + CBEL + 27 + 27 + 1) * D                                       // cbel, cbelief, cprior, d_partial, d_varmax (cameras)
           + L1 * D                                                                       // d_varmax (landmarks)
           + 2 * ((S + BLOCK - 1) / BLOCK) * D                                            // d_red
           + (size_t)RELIN_RING * RELIN_LANES * I                                         // d_relin_ring
           + (size_t)(z.n_wg + 1) * I                                                     // d_count, and an int per workgroup nothing uses now
           + (z.pack_mode ? 2 * T1 * PART_ROW * D : 0)                                    // parts
           + (64 << 12);                                                                  // slack: the starts of the arrays
}

}  // namespace gbp
