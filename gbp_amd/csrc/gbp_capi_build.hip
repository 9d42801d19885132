// gbp_capi_build.hip -- libgbp_hip.so, the graph build: gbp::build_graph puts the graph of a descriptor onto a handle, on the device
// (kernels: gbp_build.hpp; which arrays the arena holds and how large it is: gbp_build_plan.hpp).  gbp_ba_create runs it on a new handle;
// gbp_ba_extend, gbp_ba_window_step, gbp_ba_cull, gbp_ba_retire and gbp_ba_retire_landmarks run it on the graph they build beside the
// live one (gbp_graft.hpp).  It is a sequence of stages; BuildWork carries what one stage leaves for a later one, everything else is a
// local of its stage.  The host waits for the device where a stage says so and nowhere else.
#include "gbp_handle.hpp"
#include "gbp_build.hpp"

#include <chrono>

namespace {

// GBP_BUILD_TIMING: wall time of the stages of gbp_ba_create on stderr (each mark synchronises the stream: diagnostic only)
struct BuildClock {
    bool on; hipStream_t s; std::chrono::steady_clock::time_point t0;
    BuildClock(bool on_, hipStream_t st) : on(on_), s(st), t0(std::chrono::steady_clock::now()) {}
    void mark(const char *what)
    {
        if (!on) return;
        (void)hipStreamSynchronize(s);
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[gbp build] %-28s %8.1f us\n", what, std::chrono::duration<double, std::micro>(t1 - t0).count());
        t0 = t1;
    }
};

struct BuildWork {
    const gbp_ba_desc_t *d;
    const int C, L, F, n_cus;
    std::vector<void *> &scratch;                // device buffers only the build needs: the caller releases them when build_graph has returned
    BuildClock clk;
    // the inputs on the device (stage_and_check; lmk_means in internal numbering from landmark_order on)
    const int *cam_idx = nullptr, *lmk_idx = nullptr;
    const double *meas = nullptr, *cam_means = nullptr, *lmk_means = nullptr;
    bool sorted = true;                          // the file order is camera-major already
    // orders (reference_order allocates, landmark_major fills the landmark side)
    int *iota = nullptr, *ref_file = nullptr, *lm_key = nullptr, *lm2ref = nullptr, *lptr = nullptr, *cptr = nullptr, *cadj = nullptr, *cpos = nullptr;
    void *sort_tmp = nullptr; size_t sort_bytes = 0;
    int bits_l = 1;
    // tiles (pack_tiles)
    int4 *d_tiles = nullptr;
    int *d_lrow0 = nullptr, *d_lrow1 = nullptr;
    int T = 0;
    // the fused sweep's tables (decide_windows) and which sweep may run (reserve_and_allocate)
    int n_wg = 1, cgmax = 0;
    long long rows = 0;
    bool general = false;                        // the general sweep may run: its staging buffer comes out of the arena
};

// Reads the descriptor's arrays; writes their device copies and `sorted`.  The host waits once, for the two flags: ids out of range end
// the build, and the camera order decides whether reference_order sorts.
int stage_and_check(gbp_ba *h, BuildWork &w)
{
    const bool dev_in = (w.d->flags & GBP_FLAG_DEVICE_INPUT) != 0;
    const size_t Fz = (size_t)w.F;
    CHK(stage_input(h, w.d->cam_idx, Fz, dev_in, w.scratch, &w.cam_idx)); CHK(stage_input(h, w.d->lmk_idx, Fz, dev_in, w.scratch, &w.lmk_idx));
    CHK(stage_input(h, w.d->meas, Fz * 2, dev_in, w.scratch, &w.meas));
    CHK(stage_input(h, w.d->cam_means, (size_t)w.C * 6, dev_in, w.scratch, &w.cam_means));
    CHK(stage_input(h, w.d->lmk_means, (size_t)w.L * 3, dev_in, w.scratch, &w.lmk_means));

    w.clk.mark("stage inputs");
    int *d_flags = nullptr;                      // ids in range?  already camera-major?
    CHK(scratch_alloc(h, w.scratch, &d_flags, 2));
    HIPCHK(hipMemsetAsync(d_flags, 0, 2 * sizeof(int), h->stream));
    if (w.F) hipLaunchKernelGGL(k_check_ids, dim3(grid_for(Fz)), dim3(BLOCK), 0, h->stream, w.cam_idx, w.lmk_idx, w.F, w.C, w.L, d_flags);
    HIPCHK(hipGetLastError());
    int flags[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(flags, d_flags, sizeof flags, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (flags[0]) return fail(GBP_EINVAL, "an observation references a camera outside [0,%d) or a landmark outside [0,%d)", w.C, w.L);
    w.sorted = !flags[1];

    w.clk.mark("check ids");
    return GBP_OK;
}

// Reference order: camera-major, stable in file order (gbp_ba.py:128-130).  Reads the staged ids; writes d_ref_cam, d_ref_lmk, ref_file
// (NULL when the file is in that order already) and cptr, and allocates what landmark_major fills.  No wait.
int reference_order(gbp_ba *h, BuildWork &w)
{
    const size_t Fz = (size_t)w.F;
    CHK(dev_alloc(h, &h->d_ref_cam, std::max<size_t>(Fz, 1), false)); CHK(dev_alloc(h, &h->d_ref_lmk, std::max<size_t>(Fz, 1), false));
    CHK(scratch_alloc(h, w.scratch, &w.iota, Fz)); CHK(scratch_alloc(h, w.scratch, &w.lm_key, Fz)); CHK(scratch_alloc(h, w.scratch, &w.lm2ref, Fz));
    CHK(scratch_alloc(h, w.scratch, &w.lptr, (size_t)w.L + 1));
    CHK(dev_alloc(h, &w.cptr, (size_t)w.C + 1)); CHK(dev_alloc(h, &w.cadj, std::max<size_t>(Fz, 1)));
    const int bits_c = bits_for(w.C);
    w.bits_l = bits_for(w.L);
    w.sort_bytes = w.F ? std::max(sort_pairs_tmp_bytes(Fz, bits_c), sort_pairs_tmp_bytes(Fz, w.bits_l)) : 0;
    if (w.sort_bytes) { HIPCHK(hipMallocAsync(&w.sort_tmp, w.sort_bytes, h->stream)); w.scratch.push_back(w.sort_tmp); }
    if (w.F) hipLaunchKernelGGL(k_iota, dim3(grid_for(Fz)), dim3(BLOCK), 0, h->stream, w.iota, w.F);
    if (w.F && !w.sorted) {
        CHK(scratch_alloc(h, w.scratch, &w.ref_file, Fz));
        HIPCHK((hipError_t)sort_pairs(w.sort_tmp, w.sort_bytes, w.cam_idx, h->d_ref_cam, w.iota, w.ref_file, Fz, bits_c, h->stream));
        hipLaunchKernelGGL(k_gather_int, dim3(grid_for(Fz)), dim3(BLOCK), 0, h->stream, w.lmk_idx, w.ref_file, h->d_ref_lmk, w.F);
    } else if (w.F) {
        HIPCHK(hipMemcpyAsync(h->d_ref_cam, w.cam_idx, Fz * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->d_ref_lmk, w.lmk_idx, Fz * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
    }
    hipLaunchKernelGGL(k_lower_bounds, dim3(grid_for((size_t)w.C + 1)), dim3(BLOCK), 0, h->stream, h->d_ref_cam, w.F, w.cptr, w.C);
    return GBP_OK;
}

// GBP_FLAG_REORDER_LMKS: internal landmark numbers by camera locality (the rule: gbp_policy.hpp; kernels: gbp_build.hpp).  From here on
// d_ref_lmk and lmk_means are in internal numbering and the build is that of the relabelled problem; the two maps stay with the handle
// for its landmark-indexed boundaries.  The host waits once, for its copy of the caller's id -> internal id map (download).
int landmark_order(gbp_ba *h, BuildWork &w)
{
    const int C = w.C, L = w.L, F = w.F;
    h->d_lmk_u2i = h->d_lmk_i2u = nullptr; h->lmk_u2i.clear();
    if (!(h->flags & GBP_FLAG_REORDER_LMKS) || L <= 0) return GBP_OK;
    if (L >= (1 << 30)) return fail(GBP_EINVAL, "GBP_FLAG_REORDER_LMKS supports fewer than 2^30 landmarks");
    const size_t Lz = (size_t)L, Fz = (size_t)F;
    LmkStats st{};
    int *key = nullptr, *key_sorted = nullptr, *l_iota = nullptr, *first = nullptr, *counts = nullptr;
    double *means_int = nullptr;
    CHK(scratch_alloc(h, w.scratch, &st.deg, Lz)); CHK(scratch_alloc(h, w.scratch, &st.lo, Lz)); CHK(scratch_alloc(h, w.scratch, &st.hi, Lz));
    CHK(scratch_alloc(h, w.scratch, &key, Lz)); CHK(scratch_alloc(h, w.scratch, &key_sorted, Lz)); CHK(scratch_alloc(h, w.scratch, &l_iota, Lz));
    CHK(scratch_alloc(h, w.scratch, &first, Lz)); CHK(scratch_alloc(h, w.scratch, &counts, 2)); CHK(scratch_alloc(h, w.scratch, &means_int, Lz * 3));
    CHK(dev_alloc(h, &h->d_lmk_u2i, Lz, false)); CHK(dev_alloc(h, &h->d_lmk_i2u, Lz, false));
    HIPCHK(hipMemsetAsync(st.deg, 0, Lz * sizeof(int), h->stream));
    HIPCHK(hipMemsetAsync(st.lo, 0x7f, Lz * sizeof(int), h->stream));      // 0x7f7f7f7f: above every camera id
    HIPCHK(hipMemsetAsync(st.hi, 0xff, Lz * sizeof(int), h->stream));      // -1
    HIPCHK(hipMemsetAsync(counts, 0, 2 * sizeof(int), h->stream));
    const int bits_k1 = bits_for((long long)C + 2), bits_k2 = bits_for(2ll * L + 3);
    const size_t lsort_bytes = std::max(sort_pairs_tmp_bytes(Lz, bits_k1), sort_pairs_tmp_bytes(Lz, bits_k2));
    void *lsort_tmp = nullptr;
    HIPCHK(hipMallocAsync(&lsort_tmp, std::max<size_t>(lsort_bytes, 1), h->stream)); w.scratch.push_back(lsort_tmp);
    if (F) hipLaunchKernelGGL(k_lmk_stats, dim3(grid_for(Fz)), dim3(BLOCK), 0, h->stream, h->d_ref_cam, h->d_ref_lmk, F, st);
    hipLaunchKernelGGL(k_lmk_class_keys, dim3(grid_for(Lz)), dim3(BLOCK), 0, h->stream, st, L, C, key, counts);
    hipLaunchKernelGGL(k_iota, dim3(grid_for(Lz)), dim3(BLOCK), 0, h->stream, l_iota, L);
    HIPCHK(hipGetLastError());
    HIPCHK((hipError_t)sort_pairs(lsort_tmp, lsort_bytes, key, key_sorted, l_iota, first, Lz, bits_k1, h->stream));
    hipLaunchKernelGGL(k_lmk_spread_keys, dim3(grid_for(Lz)), dim3(BLOCK), 0, h->stream, counts, L, key);
    HIPCHK(hipGetLastError());
    HIPCHK((hipError_t)sort_pairs(lsort_tmp, lsort_bytes, key, key_sorted, first, h->d_lmk_i2u, Lz, bits_k2, h->stream));
    hipLaunchKernelGGL(k_lmk_relabel_vars, dim3(grid_for(Lz)), dim3(BLOCK), 0, h->stream, h->d_lmk_i2u, L, h->d_lmk_u2i, w.lmk_means, means_int);
    if (F) hipLaunchKernelGGL(k_map_int_inplace, dim3(grid_for(Fz)), dim3(BLOCK), 0, h->stream, h->d_ref_lmk, h->d_lmk_u2i, F);
    HIPCHK(hipGetLastError());
    w.lmk_means = means_int;
    CHK(download(h, h->lmk_u2i, h->d_lmk_u2i, Lz));
    w.clk.mark("landmark order");
    return GBP_OK;
}

// Landmark-major, stable in reference id (= VariableNode.adj_factors order, gbp_ba.py:139).  Reads d_ref_lmk; writes lm2ref and lptr.  No wait.
int landmark_major(gbp_ba *h, BuildWork &w)
{
    const size_t Fz = (size_t)w.F;
    if (w.F) HIPCHK((hipError_t)sort_pairs(w.sort_tmp, w.sort_bytes, h->d_ref_lmk, w.lm_key, w.iota, w.lm2ref, Fz, w.bits_l, h->stream));
    hipLaunchKernelGGL(k_lower_bounds, dim3(grid_for((size_t)w.L + 1)), dim3(BLOCK), 0, h->stream, w.lm_key, w.F, w.lptr, w.L);
    HIPCHK(hipGetLastError());

    w.clk.mark("orders (allocs + 2 sorts)");
    return GBP_OK;
}

// Tiles: up to 64 slots / TILE_LMKS whole landmarks each; over-sized landmarks become chunk tiles (a piece of one landmark each).  Next-fit
// packing as list ranking on the device (gbp_build.hpp).  Reads lptr; writes the tile table, the landmarks' slot ranges, T, pack_mode and
// n_big.  The host waits for the tile count and the smallest landmark degree -- the table is sized by the first, and the second decides
// whether the dense packing may replace this one -- and, when it does not, for the number of over-sized landmarks (pack_mode).
int pack_tiles(gbp_ba *h, BuildWork &w)
{
    const int L = w.L, F = w.F, LP = L + 1;
    const int n_pblocks = std::max(1, (L + PACK_BLOCK - 1) / PACK_BLOCK), n_nodes = n_pblocks * TILE_LMKS + 1;   // (block, entry) nodes + the end
    const int levels = bits_for(n_pblocks + 1);
    int *nxt = nullptr, *w0 = nullptr, *jump = nullptr, *wsum = nullptr, *bpos = nullptr, *pos = nullptr, *d_big_list = nullptr, *d_cnt = nullptr;
    CHK(scratch_alloc(h, w.scratch, &nxt, (size_t)LP)); CHK(scratch_alloc(h, w.scratch, &w0, (size_t)LP));
    CHK(scratch_alloc(h, w.scratch, &jump, (size_t)levels * n_nodes)); CHK(scratch_alloc(h, w.scratch, &wsum, (size_t)levels * n_nodes));
    CHK(scratch_alloc(h, w.scratch, &bpos, (size_t)n_nodes)); CHK(scratch_alloc(h, w.scratch, &pos, (size_t)LP));
    CHK(scratch_alloc(h, w.scratch, &w.d_lrow0, (size_t)L)); CHK(scratch_alloc(h, w.scratch, &w.d_lrow1, (size_t)L));
    CHK(scratch_alloc(h, w.scratch, &d_big_list, (size_t)L)); CHK(scratch_alloc(h, w.scratch, &d_cnt, 1));
    HIPCHK(hipMemsetAsync(pos, 0xff, sizeof(int) * (size_t)LP, h->stream));
    HIPCHK(hipMemsetAsync(bpos, 0xff, sizeof(int) * (size_t)n_nodes, h->stream));
    HIPCHK(hipMemsetAsync(bpos, 0, sizeof(int), h->stream));                      // the chain enters block 0 at landmark 0 with tile 0
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_pack_next, dim3(grid_for((size_t)LP)), dim3(BLOCK), 0, h->stream, w.lptr, L, nxt, w0);
    hipLaunchKernelGGL(k_pack_block_walk, dim3(grid_for((size_t)n_nodes)), dim3(BLOCK), 0, h->stream, nxt, w0, L, n_pblocks, jump, wsum);
    for (int k = 0; k + 1 < levels; ++k)
        hipLaunchKernelGGL(k_pack_double, dim3(grid_for((size_t)n_nodes)), dim3(BLOCK), 0, h->stream, jump + (size_t)k * n_nodes, wsum + (size_t)k * n_nodes,
                           jump + (size_t)(k + 1) * n_nodes, wsum + (size_t)(k + 1) * n_nodes, n_nodes);
    for (int k = levels - 1; k >= 0; --k)
        hipLaunchKernelGGL(k_pack_mark, dim3(grid_for((size_t)n_nodes)), dim3(BLOCK), 0, h->stream, jump + (size_t)k * n_nodes, wsum + (size_t)k * n_nodes, bpos,
                           n_nodes);
    hipLaunchKernelGGL(k_pack_block_fill, dim3(grid_for((size_t)n_pblocks)), dim3(BLOCK), 0, h->stream, nxt, w0, L, n_pblocks, bpos, pos);
    HIPCHK(hipGetLastError());
    int T = 0, min_deg = 0x7fffffff, *d_mindeg = nullptr;
    CHK(scratch_alloc(h, w.scratch, &d_mindeg, 1));
    HIPCHK(hipMemcpyAsync(d_mindeg, &min_deg, sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (L) hipLaunchKernelGGL(k_min_degree, dim3(grid_for((size_t)L)), dim3(BLOCK), 0, h->stream, w.lptr, L, d_mindeg);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&T, pos + L, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(&min_deg, d_mindeg, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (L == 0) T = 0;
    const bool dense = dense_packing(F, T, min_deg, h->ovr);
    if (dense) T = (F + WTILE - 1) / WTILE;
    if (T < 0 || (int64_t)T * WTILE > INT32_MAX) return fail(GBP_EINVAL, "the graph needs %d tiles: slot indices would not fit 32 bits", T);
    w.T = h->p.T = T;
    CHK(dev_alloc(h, &w.d_tiles, std::max<size_t>((size_t)T, 1)));
    int n_big = 0;
    if (dense) {
        hipLaunchKernelGGL(k_dense_tiles, dim3(grid_for((size_t)T)), dim3(BLOCK), 0, h->stream, w.lptr, L, F, T, w.d_tiles);
        hipLaunchKernelGGL(k_dense_rows, dim3(grid_for((size_t)L)), dim3(BLOCK), 0, h->stream, w.lptr, L, w.d_lrow0, w.d_lrow1);
        HIPCHK(hipGetLastError());
    } else {
        if (L) hipLaunchKernelGGL(k_pack_emit, dim3(grid_for((size_t)L)), dim3(BLOCK), 0, h->stream, w.lptr, L, nxt, pos, w.d_tiles, w.d_lrow0, w.d_lrow1,
                                  d_big_list, d_cnt);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&n_big, d_cnt, sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    // 0: every landmark inside one tile; 1: whole landmarks, those above 64 factors in chunk tiles; 2: dense.  From 1 on some landmarks span
    // tiles: the tiles write partial sums (Params::parts) and k_lmk_finish_parts forms those beliefs after every sweep.
    h->pack_mode = dense ? 2 : (n_big ? 1 : 0);
    h->n_big = n_big;

    w.clk.mark("tile packing");
    return GBP_OK;
}

// Camera WINDOWS.  Workgroup b of the fused sweep walks the tiles [b T / n, (b + 1) T / n) and needs table rows for the cameras of THOSE
// tiles only.  In a sequence -- landmarks numbered along the trajectory, each seen from neighbouring cameras, now and then from a place
// visited before -- that is a few dozen cameras however many the graph has: the table becomes [set][27] per workgroup (k_wg_cam_sets: the
// distinct cameras of its tiles; a 16-bit map over the interval they lie in turns a camera into its table row), more cameras than fit the
// LDS as a whole still run the fused sweep, and the tables written and reduced every sweep shrink from workgroups x cameras rows to the sum
// of the sets.  When they are taken: camera_windows (gbp_policy.hpp).
// Reads the tiles; writes n_wg, rows and the handle's wg_win / wg_cams (left empty: no windows).  The decision is the host's, so it waits
// up to three times, each for what the next step is sized by: the workgroups' camera intervals (does a map fit the LDS?), the sizes of
// their sets (do windows pay?), and only then the sets themselves.
int decide_windows(gbp_ba *h, BuildWork &w)
{
    const int C = w.C, T = w.T;
    const int n_wg = w.n_wg = fused_workgroups(T, w.n_cus, h->ovr);
    const int cap = w.cgmax = fused_max_cams();      // (host arithmetic on the LDS budget: gbp_fused_plan.hpp)
    h->wg_win.clear(); h->wg_cams.clear();
    w.rows = (long long)n_wg * C;
    if (!(T > 0 && C > 0 && !(h->flags & GBP_FLAG_NO_FUSED) && h->p.num_undamped != 0)) return GBP_OK;
    int2 *d_rng = nullptr;
    int *d_lists = nullptr, *d_counts = nullptr;
    CHK(scratch_alloc(h, w.scratch, &d_rng, (size_t)n_wg));
    CHK(scratch_alloc(h, w.scratch, &d_lists, (size_t)n_wg * cap)); CHK(scratch_alloc(h, w.scratch, &d_counts, (size_t)n_wg));
    hipLaunchKernelGGL(k_wg_cam_range, dim3((n_wg + BLOCK / 64 - 1) / (BLOCK / 64)), dim3(BLOCK), 0, h->stream, w.d_tiles, w.d_lrow0, w.lptr, w.lm2ref,
                       h->d_ref_cam, T, n_wg, d_rng);
    HIPCHK(hipGetLastError());
    std::vector<int2> rng((size_t)n_wg);
    HIPCHK(hipMemcpyAsync(rng.data(), d_rng, sizeof(int2) * (size_t)n_wg, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    int max_width = 0;
    for (const int2 &r : rng) max_width = std::max(max_width, r.y >= r.x ? r.y - r.x + 1 : 0);
    const size_t bm_bytes = ((size_t)(max_width + 31) / 32 + SETS_THREADS + 1) * sizeof(unsigned);
    if (bm_bytes > 64 * 1024 || fused_shmem_windows(1, max_width) > (size_t)LDS_BYTES) return GBP_OK;      // intervals no map of the sweep could cover
    hipLaunchKernelGGL(k_wg_cam_sets, dim3(n_wg), dim3(SETS_THREADS), bm_bytes, h->stream, w.d_tiles, w.d_lrow0, w.lptr, w.lm2ref, h->d_ref_cam, T, n_wg,
                       d_rng, cap, d_lists, d_counts);
    HIPCHK(hipGetLastError());
    std::vector<int> counts((size_t)n_wg);
    HIPCHK(hipMemcpyAsync(counts.data(), d_counts, sizeof(int) * (size_t)n_wg, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    long long sum = 0;
    int max_set = 0;
    for (int n : counts) { sum += n; max_set = std::max(max_set, n); }
    if (!(camera_windows(C, w.cgmax, sum, w.rows, h->ovr) && max_set <= cap && fused_shmem_windows(max_set, max_width) <= (size_t)LDS_BYTES)) return GBP_OK;
    std::vector<int> lists((size_t)n_wg * cap);
    HIPCHK(hipMemcpyAsync(lists.data(), d_lists, sizeof(int) * lists.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    h->wg_win.resize((size_t)n_wg); h->wg_cams.reserve((size_t)sum);
    for (int b = 0; b < n_wg; ++b) {
        const int n = counts[(size_t)b];
        h->wg_win[(size_t)b] = make_int4(n ? rng[(size_t)b].x : 0, n, (int)h->wg_cams.size(), n ? rng[(size_t)b].y - rng[(size_t)b].x + 1 : 0);
        h->wg_cams.insert(h->wg_cams.end(), lists.begin() + (size_t)b * cap, lists.begin() + (size_t)b * cap + n);
    }
    w.rows = sum;
    return GBP_OK;
}

bool in_arena(const gbp_ba *h, const void *q)
{
    const char *a = static_cast<const char *>(h->arena), *c = static_cast<const char *>(q);
    return a && c >= a && c < a + h->arena_bytes;
}

// Which sweep may run (staged_auto, general), then ONE block for everything a sweep streams (arena_reserve, gbp_handle.hpp) and the
// arrays of build_arena_table out of it, in the table's order.  Reads rows, n_wg, T and pack_mode; writes the handle's arrays and cpos.
// No wait.  GBP_DEBUG_LAYOUT: an array the arena had no room for is an error here (without it: its own hipMalloc, silently).
int reserve_and_allocate(gbp_ba *h, BuildWork &w)
{
    Params &p = h->p;
    const bool windowed = !h->wg_win.empty();
    h->staged_auto = staged_for_sparseness(w.F, w.rows, h->ovr) && !(h->flags & (GBP_FLAG_FORCE_FUSED | GBP_FLAG_NO_FUSED));
    if (h->staged_auto) h->flags |= GBP_FLAG_NO_FUSED;
    if (h->flags & GBP_FLAG_NO_FUSED) { h->wg_win.clear(); h->wg_cams.clear(); }
    w.general = general_sweep((h->flags & GBP_FLAG_NO_FUSED) != 0, p.num_undamped == 0, w.C, w.cgmax, windowed);
    const BuildSizes z{w.F, w.L, w.C, w.T, w.rows, w.n_wg, p.crow, w.general, p.num_undamped == 0, p.loss != 0, h->pack_mode};
    CHK(arena_reserve(h, build_arena_need(z)));
    const auto table = build_arena_table(z);
    const auto at = [](auto **q) { return reinterpret_cast<char **>(q); };
    char **const dst[ARENA_ARRAYS] = {at(&p.cstage), at(&p.lin), at(&p.msg), at(&p.xtra), at(&p.avar), at(&w.cpos), at(&p.lrec), at(&p.parts), at(&p.cbel),
                                      at(&p.cprior), at(&p.cbelief), at(&h->d_partial), at(&h->d_red), at(&h->d_relin_ring), at(&h->d_count),
                                      at(&h->d_varmax)};      // in the order of ArenaArray
    for (int i = 0; i < ARENA_ARRAYS; ++i) {
        const ArenaEntry &e = table[(size_t)i];
        if (!e.exists) continue;
        CHK(dev_alloc(h, dst[i], e.bytes(), e.zero));
        if (h->ovr.debug_layout && !in_arena(h, *dst[i])) return fail(GBP_ESTATE, "internal layout error: %s was placed outside the arena", e.name);
    }
    if (table[A_CSTAGE].exists) h->cstage_cap = p.crow;
    return GBP_OK;
}

// Per-slot data (k_build_tiles: one wave per tile) and the variables' records (k_init_vars).  Reads the orders, the tiles and the staged
// means and measurements; writes the arrays of reserve_and_allocate.  No wait.
int fill(gbp_ba *h, BuildWork &w)
{
    Params &p = h->p;
    const int T = w.T;
    p.tiles = w.d_tiles; p.cptr = w.cptr; p.cadj = w.cadj; p.cpos = w.cpos;
    if (T) {
        BuildArgs a{w.d_tiles, w.d_lrow0, w.lptr, w.lm2ref, h->d_ref_cam, w.ref_file, w.cam_means, w.lmk_means, w.meas, w.cadj, w.cpos};
        hipLaunchKernelGGL(k_build_tiles, dim3((T + BLOCK / 64 - 1) / (BLOCK / 64)), dim3(BLOCK), 0, h->stream, p, a);
    }
    w.clk.mark("allocs + k_build_tiles");
    if (w.C + w.L) hipLaunchKernelGGL(k_init_vars, dim3(grid_for((size_t)w.C + w.L)), dim3(BLOCK), 0, h->stream, p, w.cam_means, w.lmk_means, w.d_lrow0, w.d_lrow1);
    HIPCHK(hipGetLastError());

    w.clk.mark("vars + small allocs");
    return GBP_OK;
}

// The fused sweep's plan, which takes its uploads from the arena (fused_plan_uploads, gbp_build_plan.hpp).  The host waits before the plan
// -- tiles[].w (max rank) is written by k_build_tiles -- and at the end: the caller releases the staged inputs when this returns.
// GBP_DEBUG_LAYOUT: the layout is decoded and compared first (one more wait), and an upload outside the arena is an error.
int finish(gbp_ba *h, BuildWork &w)
{
    if (h->ovr.debug_layout) {
        int bad = 0;
        CHK(gbp_ba_check_layout(h, &bad));
        if (bad) return fail(GBP_ESTATE, "internal layout error: %d slots do not decode to their reference factor", bad);
    }
    if (!(h->flags & GBP_FLAG_NO_FUSED) && !h->p.xtra) {
        HIPCHK(hipStreamSynchronize(h->stream));
        h->fused.alloc = arena_take; h->fused.alloc_ctx = h;
        int rc = plan_fused_sweep(h, w.n_cus);
        if (rc < 0) return fail(GBP_EHIP, "building the fused sweep plan failed (%d)", rc);
        if (h->ovr.debug_layout) {
            const FusedArgs &a = h->fused.args;
            const void *const up[PLAN_UPLOADS] = {a.block_partials, a.win, a.rowidx, a.wgcams, h->fused.d_cam_rows};      // in the order of fused_plan_uploads
            const auto names = fused_plan_uploads(0, 0, 0, false);
            for (int i = 0; i < PLAN_UPLOADS; ++i)
                if (up[i] && !in_arena(h, up[i])) return fail(GBP_ESTATE, "internal layout error: the fused plan's %s was placed outside the arena", names[(size_t)i].name);
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    w.clk.mark("fused plan");
    return GBP_OK;
}

}  // namespace

// The graph of a descriptor onto a handle whose Params scalars, flags, overrides and stream are set.  ref_file_out (may be NULL) receives
// the reference id -> file index map the build used, a scratch buffer, or NULL when the file order is camera-major already (identity).
int gbp::build_graph(gbp_ba *h, const gbp_ba_desc_t *d, std::vector<void *> &scratch, int n_cus, const int **ref_file_out)
{
    BuildWork w{d, d->n_cams, d->n_lmks, d->n_factors, n_cus, scratch, BuildClock(h->ovr.build_timing, h->stream)};
    ++h->rebuilds;                                            // (gbp_ba_rebuild_count)
    CHK(stage_and_check(h, w));
    CHK(reference_order(h, w));
    if (ref_file_out) *ref_file_out = w.ref_file;
    CHK(landmark_order(h, w));
    CHK(landmark_major(h, w));
    CHK(pack_tiles(h, w));
    CHK(decide_windows(h, w));
    CHK(reserve_and_allocate(h, w));
    CHK(fill(h, w));
    return finish(h, w);
}
