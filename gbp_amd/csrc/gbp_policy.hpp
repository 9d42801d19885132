// gbp_policy.hpp -- which sweep runs, and in which form: every rule with a measured threshold, and the environment overrides of those
// rules.  Host-only and pure (plain numbers in, the choice out; no HIP runtime), so tests/test_sweep_policy_host.py pins every rule on a
// CPU.  The overrides are read once per handle, by gbp_ba_create (gbp_ba::ovr), for tests, A/B runs and the tools (tools/README.md).
#pragma once
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <optional>

namespace gbp {

struct Overrides {                           // unset: the rule decides
    std::optional<bool> pack_dense;          // GBP_PACK: "dense" -> dense, anything else -> whole landmarks
    std::optional<int> fused_blocks;         // GBP_FUSED_BLOCKS: at most this many workgroups in the fused sweep
    std::optional<bool> windows;             // GBP_WINDOWS: 0 never / else whenever they fit
    std::optional<double> staged_below;      // GBP_STAGED_BELOW: factors per table row below which the staged sweep runs (0: never)
    std::optional<int> rows_wave_max;        // GBP_ROWS_WAVE_MAX: this bound alone decides the reduce behind camera windows (0: tree form)
    std::optional<double> fused_pin_mib;     // GBP_FUSED_PIN_MIB: MiB that stay cacheable (< 0: everything)
    std::optional<int> fused_nt;             // GBP_FUSED_NT: cache-bypass bits of the cacheable tiles of the pinned variant
    std::optional<int> acc_single;           // GBP_ACC_SINGLE: the SINGLE accumulation on (non-zero) / off
    std::optional<int> single_probe_fail;    // GBP_SINGLE_PROBE_FAIL: pretend the lane-order probe saw this failing-pattern mask
    int cam_block = 0;                       // GBP_CAM_BLOCK: threads per camera of the staged reduce (0: by the graph's shape)
    std::optional<int> xchg_blocks;          // GBP_XCHG_BLOCKS: at most this many workgroups in a merged exchange
    bool peer_split = false;                 // GBP_PEER_SPLIT: reduce / push and the waiting finish as two launches
    double peer_timeout_ms = 20000.0;        // GBP_PEER_TIMEOUT_MS: how long a finish wave waits for a peer (at least 1)
    bool rccl_fail = false;                  // GBP_RCCL_FAIL: gbp_ba_comm_unique_id refuses (the callers' fallbacks are tested with it)
    bool plan_debug = false, build_timing = false, debug_layout = false;   // GBP_PLAN_DEBUG, GBP_BUILD_TIMING, GBP_DEBUG_LAYOUT: diagnostics
};

// lookup(name): the value, or NULL when unset -- getenv in the product (env_overrides), a table in the test.  A flag is set by its presence.
template <typename Lookup> inline Overrides parse_overrides(Lookup lookup)
{
    Overrides o;
    if (const char *e = lookup("GBP_PACK")) o.pack_dense = std::strcmp(e, "dense") == 0;
    if (const char *e = lookup("GBP_FUSED_BLOCKS")) o.fused_blocks = std::atoi(e);
    if (const char *e = lookup("GBP_WINDOWS")) o.windows = std::atoi(e) != 0;
    if (const char *e = lookup("GBP_STAGED_BELOW")) o.staged_below = std::atof(e);
    if (const char *e = lookup("GBP_ROWS_WAVE_MAX")) o.rows_wave_max = std::atoi(e);
    if (const char *e = lookup("GBP_FUSED_PIN_MIB")) o.fused_pin_mib = std::atof(e);
    if (const char *e = lookup("GBP_FUSED_NT")) o.fused_nt = std::atoi(e);
    if (const char *e = lookup("GBP_ACC_SINGLE")) o.acc_single = std::atoi(e);
    if (const char *e = lookup("GBP_SINGLE_PROBE_FAIL")) o.single_probe_fail = std::atoi(e);
    if (const char *e = lookup("GBP_CAM_BLOCK")) o.cam_block = std::atoi(e);
    if (const char *e = lookup("GBP_XCHG_BLOCKS")) o.xchg_blocks = std::atoi(e);
    if (const char *e = lookup("GBP_PEER_TIMEOUT_MS")) o.peer_timeout_ms = std::max(1.0, std::atof(e));
    o.peer_split = lookup("GBP_PEER_SPLIT") != nullptr; o.rccl_fail = lookup("GBP_RCCL_FAIL") != nullptr;
    o.plan_debug = lookup("GBP_PLAN_DEBUG") != nullptr; o.build_timing = lookup("GBP_BUILD_TIMING") != nullptr;
    o.debug_layout = lookup("GBP_DEBUG_LAYOUT") != nullptr;
    return o;
}
inline Overrides env_overrides() { return parse_overrides([](const char *name) -> const char * { return std::getenv(name); }); }

// Whole landmarks per tile, or -- when that would leave more than 15 % of the 64 slots of the T tiles empty and every landmark has at
// least three factors -- the dense packing: tile t = factors [64 t, 64 t + 64), landmarks may span tiles (gbp_build.hpp).  One million
// factors at 40 per landmark: 25 000 tiles of 40 -> 15 625 full ones.  "dense" asked for still needs the three factors per landmark.
inline bool dense_packing(long long F, int T, int min_deg, const Overrides &o) { return T > 0 && F > 0 && min_deg >= 3 && (o.pack_dense ? *o.pack_dense : (double)F < 0.85 * 64.0 * (double)T); }

// Workgroups of the fused sweep: one per CU, never more than tiles.  build_graph sizes the camera windows by it and fused_plan launches it.
inline int fused_workgroups(int T, int n_cus, const Overrides &o) { return std::max(1, std::min({T, n_cus, o.fused_blocks.value_or(n_cus)})); }

// Camera WINDOWS (build_graph), where they fit the LDS: when the whole table would not (C > fused_max_cams), or when the workgroups'
// camera sets add up to at most 0.7 of the whole tables (workgroups x cameras rows).  A 125k-factor share of the headline graph, 500
// random cameras: sets 0.63 of the whole tables, 26.6 against 29.2 us per sweep; a 250k share: 0.86, 36.6 against 34.4 (sparse_probe.sh).
inline bool camera_windows(int C, int max_cams, long long set_rows, long long whole_rows, const Overrides &o) { return o.windows ? *o.windows : (C > max_cams || 10 * set_rows <= 7 * whole_rows); }

// Few factors per camera: the fused sweep writes (and its reduce reads back) one 224-byte table row per camera and WORKGROUP whatever
// the graph's size, the staged form one 128-byte row per FACTOR.  Below ~0.75 factors per table row (with windows: the rows the tables
// really have) the staged sweep is the faster one -- 13k / 30k / 60k / 90k factors x 500 cameras: 18.6 / 20.5 / 24.2 / 29.1 against 26.3 /
// 28.6 / 28.9 / 30.2 us per sweep (profiles/r04_shards.json); round 5: 62.5k 22.1 against 28.6; 125k is a tie (30.6 against 31.4, with
// the peer-store exchange in the loop 34.5 against 35.3), 250k 44.6 against 36.9 (profiles/r05_shards.json) -- e.g. a rank's share of
// the headline graph at 16 ranks and beyond.  Not a byte count: fr1desk (13 298 factors, 63 cameras, 221 workgroups: 0.96 per pair)
// runs 13.9 us fused against ~16 staged, so the threshold stays below 1.  The general sweep also runs when it is asked for, when every
// factor carries the dense remainder (num_undamped_iters = 0), or when the whole table does not fit the LDS and there are no windows.
inline bool staged_for_sparseness(long long F, long long table_rows, const Overrides &o) { return (double)F < o.staged_below.value_or(0.75) * (double)table_rows; }
inline bool general_sweep(bool no_fused, bool dense_remainder, int C, int max_cams, bool windowed) { return no_fused || dense_remainder || (C > max_cams && !windowed); }

// Landmark ORDER (GBP_FLAG_REORDER_LMKS, build_graph): camera windows need landmarks numbered along the trajectory, and a file need not
// number them so.  The rule, two integer keys and two stable sorts (ties keep the caller's order, so the order is a pure function of the
// graph and an input already in key order is left alone):
//   1. reorder_class_key: a LOCAL landmark -- its cameras span at most reorder_wide_span(C) ids -- is keyed by its lowest camera; a WIDE
//      one (a place seen again: its cameras have no locality) by C; one without factors by C + 1.  Sorted: the locals along the
//      trajectory, then the wide ones, then the empty ones.
//   2. reorder_spread_key of that position: the wide landmarks are dealt evenly, by rank, through the locals (wide j of n_wide goes in
//      front of local floor((2 j + 1) n_local / (2 n_wide))), the empty ones stay last.
// One per-camera key for all (mean, lowest, median camera) piles the wide landmarks up -- in the middle, at the start or at both ends of
// the order -- and a few workgroups then meet several hundred cameras; dealt evenly every workgroup carries its share (DESIGN 7d has the
// modelled camera sets).  Wide means a span above a quarter of the cameras, and never below 128: a sequence's landmarks span a few dozen
// keyframes (the reference's files: 2 .. 46), ten cameras drawn from anywhere span less than a quarter with probability 4e-5, and a
// graph of up to 128 cameras fits every table whole.
constexpr int REORDER_WIDE_MIN = 128;
constexpr int reorder_wide_span(int C) { return C / 4 > REORDER_WIDE_MIN ? C / 4 : REORDER_WIDE_MIN; }
constexpr int reorder_class_key(int deg, int lo, int hi, int C) { return deg <= 0 ? C + 1 : (hi - lo + 1 > reorder_wide_span(C) ? C : lo); }
constexpr int reorder_spread_key(int pos, int n_local, int n_wide)
{
    return pos < n_local ? 2 * pos + 1
           : pos < n_local + n_wide ? 2 * (int)(((2LL * (pos - n_local) + 1) * n_local) / (2LL * n_wide))
                                    : 2 * n_local + 2;
}

// Few rows per camera ON AVERAGE behind camera windows: one wave adds them (k_cam_reduce_rows).  A wave takes 32 rows per round trip, so
// a camera with many rows costs that launch microseconds where the tree form costs every camera a 1024-thread workgroup (fr1desk_small
// with windows forced: 41 rows per camera, 5.1 us against 3.6) -- which is also why MANY cameras take the wave form whatever their rows
// (tools/manycam_probe.sh, random cameras, us per launch tree / wave: 2 000 cameras x 29 rows 11.4 / 6.8, x 56 rows 12.1 / 8.1; 5 000 x
// 24 24.8 / 9.6; 1 000 x 99 8.3 / 7.7; 500 x 100 5.4 / 6.5, x 160 5.9 / 7.7: tree ~ 2.6 + 0.004 C + 0.017 R, wave ~ 5.2 + 0.0003 C +
// 0.025 R with R in thousands of rows).
constexpr int ROWS_WAVE_MAX = 16;
inline bool rows_wave(size_t table_rows, int C, const Overrides &o)
{
    const int wave_max = o.rows_wave_max.value_or(ROWS_WAVE_MAX);
    return table_rows <= (size_t)wave_max * (size_t)C || (!o.rows_wave_max && (double)C > 662.0 + 2.16e-3 * (double)table_rows);
}

// What a sweep touches against the 256 MiB memory-side cache: everything fits -> nothing bypasses it (< 0).  Beyond it the first tiles of
// every workgroup's range -- the returned MiB, tables and records included -- keep using the cache and stay resident from sweep to sweep;
// the rest stream PAST it, loads and message stores, instead of everything thrashing: 72.8 against 78.0 ps per factor at 1.35M factors,
// 72.8 / 75.8 at 2M, 68.5 / 69.2 at 10M against the earlier policy (lin rows of ALL tiles past the cache), and WORSE below the cache size
// (71.3 against 67.3 at 1.1M): profiles/r04_size_sweep.jsonl.  With the strided walk of the pinned variant (round 6) the cacheable tiles
// are one contiguous piece of the graph: 1.15M factors 73.6 us per launch with 240 MiB against 76.9 with 200; 1.35M 88.1 with 220, 89.0
// with 240, 90.9 with 200, 93.0 with 140; 2M 134.4 with 200, 137.0 with 220, 139.0 with 140, 141.3 with 240; 3M 205.4 with 200, 210.5 with
// 220; 10M flat (profiles/r06_keep_sweep.txt).  pinned_tiles splits it per workgroup (FusedArgs::pin; 0x7fffffff: all): all finish together.
inline double cache_keep_mib(double touched, const Overrides &o) { return o.fused_pin_mib ? *o.fused_pin_mib : touched > 256.0 * (1 << 20) ? (touched < 350.0 * (1 << 20) ? 230.0 : 200.0) : -1.0; }
inline int pinned_tiles(double keep_mib, double fixed, double per_tile, int n_blocks) { return keep_mib < 0.0 ? 0x7fffffff : (int)(std::max(0.0, keep_mib * (1 << 20) - fixed) / per_tile / n_blocks); }

// Few cameras: many factors of a 60-factor tile share one (fr1desk: 63 cameras, up to eight) -- the SINGLE variant of the accumulation.
// 1M factors: 66.1 against 75.1 us per step at 64 cameras, 68.0 / 72.4 at 128, 69.7 / 71.6 at 200, 72.7 / 73.4 at 300, equal at 400,
// 75.2 / 74.3 at 500; beyond the cache size -- the pinned variant -- 2M factors: 135.4 / 148.3 at 100 cameras, 151.0 / 143.7 at 300.
inline int single_accumulation(int table_cams, bool pinned, const Overrides &o) { return o.acc_single ? *o.acc_single : (table_cams <= (pinned ? 200 : 350) ? 1 : 0); }
inline int single_probe_mask(int measured, const Overrides &o) { return o.single_probe_fail.value_or(measured); }

// Threads per camera of the staged reduce.  Short runs (a camera with a few hundred factors) leave most of a 256-thread block idle through
// its reduction and 6x6 solve: 128 threads do 1M factors x 2 000 / 3 000 cameras in 125.6 / 127.4 us per sweep against 134.5 / 143.7, 3M
// factors x 13 682 cameras in 439 against 509; from ~700 factors per camera on the two are equal, at 2 000 per camera 256 threads win
// (122.9 against 128.0); one wave below 200 factors per camera: 1M factors x 20 000 cameras 176 against 243 us, 200k x 5 000 50.5 against
// 65.8.  The block size fixes the order of the sums, so it depends on the graph's shape alone.
inline int cam_block(long long F, int C, const Overrides &o) { return o.cam_block ? o.cam_block : F < 200LL * C ? 64 : F < 640LL * C ? 128 : 256; }

// Under the peer-store exchange everything behind a sweep is ONE launch without a rendezvous hook; logical ranks on one device (the hook
// is set) keep reduce / push and finish apart, with the hook between them, so that they never spin on each other.  That launch's
// workgroups wait for other ranks' workgroups of the same index, so its grid must be resident at once: never more than `resident` (the
// occupancy query), nor than the launch's own `cap`.
inline bool merged_exchange(bool has_hook, bool with_messages, const Overrides &o) { return !has_hook && with_messages && !o.peer_split; }
inline int xchg_blocks(int resident, int cap, const Overrides &o) { return o.xchg_blocks ? std::max(1, std::min({cap, resident, *o.xchg_blocks})) : std::min(cap, resident); }

}  // namespace gbp
