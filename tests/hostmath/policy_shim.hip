// policy_shim.hip -- TEST INFRASTRUCTURE: the sweep policy (gbp_amd/csrc/gbp_policy.hpp) behind extern "C" wrappers, so that
// tests/test_sweep_policy_host.py can pin every rule and override on a CPU.  Built host-only by that test with hipcc; nothing in the
// product links or loads it.  The overrides are parsed from a table the test fills (policy_setenv) instead of the environment.
#include "../../gbp_amd/csrc/gbp_fused_plan.hpp"
#include "../../gbp_amd/csrc/gbp_policy.hpp"

#include <climits>
#include <cmath>
#include <map>
#include <string>

using namespace gbp;

static std::map<std::string, std::string> g_env;
static Overrides g_o;

static void reparse()
{
    g_o = parse_overrides([](const char *name) -> const char * {
        const auto it = g_env.find(name);
        return it == g_env.end() ? nullptr : it->second.c_str();
    });
}

template <typename T>
static double opt(const std::optional<T> &v) { return v ? (double)*v : NAN; }

extern "C" {

void policy_setenv(const char *name, const char *value) { g_env[name] = value; reparse(); }
void policy_clearenv(void) { g_env.clear(); reparse(); }

// the parsed overrides in the order of struct Overrides (NaN: unset)
int policy_overrides(double *out)
{
    const Overrides &o = g_o;
    const double v[] = {opt(o.pack_dense), opt(o.fused_blocks), opt(o.windows), opt(o.staged_below), opt(o.rows_wave_max), opt(o.fused_pin_mib),
                        opt(o.fused_nt), opt(o.acc_single), opt(o.single_probe_fail), (double)o.cam_block, opt(o.xchg_blocks), (double)o.peer_split,
                        o.peer_timeout_ms, (double)o.rccl_fail, (double)o.plan_debug, (double)o.build_timing, (double)o.debug_layout};
    const int n = (int)(sizeof v / sizeof v[0]);
    for (int i = 0; i < n; ++i) out[i] = v[i];
    return n;
}

int policy_dense_packing(long long F, int T, int min_deg) { return dense_packing(F, T, min_deg, g_o); }
int policy_fused_workgroups(int T, int n_cus) { return fused_workgroups(T, n_cus, g_o); }
int policy_camera_windows(int C, int max_cams, long long set_rows, long long whole_rows) { return camera_windows(C, max_cams, set_rows, whole_rows, g_o); }
int policy_staged(long long F, long long table_rows) { return staged_for_sparseness(F, table_rows, g_o); }
int policy_general_sweep(int no_fused, int dense_remainder, int C, int max_cams, int windowed) { return general_sweep(no_fused, dense_remainder, C, max_cams, windowed); }
int policy_rows_wave(long long table_rows, int C) { return rows_wave((size_t)table_rows, C, g_o); }
double policy_keep_mib(double touched_bytes) { return cache_keep_mib(touched_bytes, g_o); }
int policy_pinned_tiles(double keep_mib, double fixed_bytes, double per_tile_bytes, int n_blocks) { return pinned_tiles(keep_mib, fixed_bytes, per_tile_bytes, n_blocks); }
int policy_single(int group_cams, int pinned) { return single_accumulation(group_cams, pinned != 0, g_o); }
int policy_probe_mask(int measured) { return single_probe_mask(measured, g_o); }
int policy_cam_block(long long F, int C) { return cam_block(F, C, g_o); }
int policy_xchg_blocks(int resident, int cap) { return xchg_blocks(resident, cap, g_o); }
int policy_merged_exchange(int has_hook, int with_messages) { return merged_exchange(has_hook, with_messages, g_o); }

// what the launches pass: the caps of the two merged exchanges (fused_cameras, staged_cameras), and the plan's arithmetic
int policy_xchg_cap_fused(void) { return XCHG_BLOCKS; }
int policy_xchg_cap_staged(void) { return INT32_MAX; }
int policy_fused_max_cams(void) { return fused_max_cams(); }
void policy_sweep_bytes(int T, int L, int C, long long table_rows, double *out)
{
    const SweepBytes b = sweep_bytes(T, L, C, (size_t)table_rows);
    out[0] = b.fixed; out[1] = b.touched; out[2] = b.per_tile;
}

}  // extern "C"
