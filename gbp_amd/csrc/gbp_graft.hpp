// gbp_graft.hpp -- what the calls that rebuild a live handle share (gbp_ba_extend: gbp_capi_extend.hip, gbp_ba_retire:
// gbp_capi_retire.hip, gbp_ba_cull: gbp_capi_cull.hip).  All build the new graph BESIDE the handle by the create path (gbp::build_graph),
// move the state of the factors and variables that live on into the new layout, and swap the new graph in only when everything has
// succeeded.  Here: the per-slot and per-variable moves (device), on the host the settings the new graph inherits, the counters it
// carries and the swap itself, and -- for the two calls that SHRINK a handle -- the whole way from survival flags to the survivors'
// graph (graft_survivors: one scan, the compaction, the create path, the transplant through index maps).
#pragma once
#include "gbp_handle.hpp"

#include <rocprim/device/device_scan.hpp>

#include <new>

namespace gbp {

// A factor's whole state from its old slot `os` (gathered) to its new slot (written as the tile-contiguous row pairs of gbp_kernels.hpp:
// 16 contiguous bytes per lane and pair, 1 KB per wave and pair).  The meta word and the rank field of the state word are the new
// layout's (k_build_tiles wrote them); everything else is the old factor's: linearisation point, measurement, clock stamp, pending /
// robust / damped bits, messages, adaptive variance, dense remainder.
GBP_DEV void transplant_slot(const Params &n, const Params &o, int slot, int os)
{
    double2 *nl = reinterpret_cast<double2 *>(n.lin);
    const double2 *ol = reinterpret_cast<const double2 *>(o.lin);
#pragma unroll
    for (int k = 0; k < LIN_ROWS / 2 - 1; ++k) nl[lin_at(slot, 2 * k) / 2] = ol[lin_at(os, 2 * k) / 2];
    {
        const size_t nix = lin_at(slot, ROW_Z + 1) / 2;     // z[1] | meta, state
        double2 v = ol[lin_at(os, ROW_Z + 1) / 2];
        const double2 mine = nl[nix];
        const unsigned *mw = reinterpret_cast<const unsigned *>(&mine.y);
        unsigned *w = reinterpret_cast<unsigned *>(&v.y);
        w[0] = mw[0];
        w[1] = (w[1] & ~(STATE_RANK_MASK << 2)) | (mw[1] & (STATE_RANK_MASK << 2));
        nl[nix] = v;
    }
    double2 *nm = reinterpret_cast<double2 *>(n.msg);
    const double2 *om = reinterpret_cast<const double2 *>(o.msg);
#pragma unroll
    for (int k = 0; k < MSG_ROWS / 2; ++k) nm[msg_at(slot, 2 * k) / 2] = om[msg_at(os, 2 * k) / 2];
    if (o.avar && n.avar) n.avar[slot] = o.avar[os];
    if (o.xtra && n.xtra) {
#pragma unroll
        for (int k = 0; k < XTRA_ROW; ++k) n.xtra[(size_t)slot * XTRA_ROW + k] = o.xtra[(size_t)os * XTRA_ROW + k];
    }
}

// camera oc of the old graph becomes camera nc of the new one: record, belief view and prior
GBP_DEV void transplant_cam(const Params &n, const Params &o, int nc, int oc)
{
#pragma unroll
    for (int k = 0; k < CAMREC; ++k) n.cbel[(size_t)nc * CAMREC + k] = o.cbel[(size_t)oc * CAMREC + k];
#pragma unroll
    for (int k = 0; k < CBEL; ++k) n.cbelief[(size_t)nc * CBEL + k] = o.cbelief[(size_t)oc * CBEL + k];
#pragma unroll
    for (int k = 0; k < 27; ++k) n.cprior[(size_t)nc * 27 + k] = o.cprior[(size_t)oc * 27 + k];
}

// landmark ol of the old graph becomes landmark nl of the new one: mean | covariance and prior (the slot range of the record is the new layout's)
GBP_DEV void transplant_lmk(const Params &n, const Params &o, int nl, int ol)
{
    double *nr = n.lrec + (size_t)nl * LREC;
    const double *orr = o.lrec + (size_t)ol * LREC;
#pragma unroll
    for (int k = 0; k < LR_ROWS; ++k) nr[k] = orr[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) nr[LR_PRIOR + k] = orr[LR_PRIOR + k];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
template <typename T>
inline int graft_stage(gbp_ba *h, const T *src, size_t n, bool on_device, std::vector<void *> &scratch, const T **out)
{
    if (on_device || !n) { *out = src; return GBP_OK; }
    void *q = nullptr;
    HIPCHK(hipMallocAsync(&q, n * sizeof(T), h->stream));
    scratch.push_back(q);
    HIPCHK(hipMemcpyAsync(q, src, n * sizeof(T), hipMemcpyHostToDevice, h->stream));
    *out = static_cast<const T *>(q);
    return GBP_OK;
}

template <typename T>
inline int graft_scratch(gbp_ba *h, std::vector<void *> &scratch, T **out, size_t n)
{
    void *q = nullptr;
    HIPCHK(hipMallocAsync(&q, std::max<size_t>(n, 1) * sizeof(T), h->stream));
    scratch.push_back(q);
    *out = static_cast<T *>(q);
    return GBP_OK;
}

// what create sets from the descriptor, taken from the old handle `o` as it is (no double -> descriptor -> double round trip), for a
// graph of C cameras, L landmarks and F factors on the fresh handle `n` (which owns nothing of o's)
inline void graft_settings(const gbp_ba *o, gbp_ba *n, int C, int L, int F)
{
    const Params &op = o->p;
    n->device = o->device; n->ovr = o->ovr; n->n_cus = o->n_cus;
    n->stream = o->stream;                                    // (not owned: the handle keeps its streams)
    n->flags = o->staged_auto ? (o->flags & ~GBP_FLAG_NO_FUSED) : o->flags;     // the flags of create, before the sparseness rule added NO_FUSED
    Params &p = n->p;
    p = Params{};
    p.F = F; p.L = L; p.C = C; p.T = 0;
    p.K = op.K; p.sigma2 = op.sigma2; p.nstds = op.nstds; p.beta = op.beta; p.eta_damping = op.eta_damping;
    p.num_undamped = op.num_undamped; p.min_linear = op.min_linear; p.loss = op.loss;
    p.robustify = 0; p.local_relin = 1;
    p.crow = op.num_undamped == 0 ? CSTAGE_ROW : CSTAGE_PLAIN;
    p.clk = op.clk; p.clk_inc = 0;                             // factors the build makes are stamped iters_since_relin = 1 against the handle's clock
    p.reverse_walk = op.reverse_walk;
}

// the counters of the old handle that are part of its state: relinearisation-count ring, sweep count, walk parities, the remainder's watch
inline int graft_counters(const gbp_ba *o, gbp_ba *n)
{
    HIPCHK(hipMemcpyAsync(n->d_relin_ring, o->d_relin_ring, sizeof(int) * (size_t)RELIN_RING * RELIN_LANES, hipMemcpyDeviceToDevice, n->stream));
    n->sweep_count = o->sweep_count; n->walk_parity = o->walk_parity; n->gen_parity = o->gen_parity;
    n->pending_possible = o->pending_possible; n->lazy_since = o->lazy_since;
    return GBP_OK;
}

// a failed build: the half-built graph goes, the message stays (as gbp_ba_create does)
inline int graft_abandon(gbp_ba *n, int rc)
{
    n->stream = nullptr;                                      // (the stream is the old handle's)
    const std::string keep = gbp_last_error();
    gbp_ba_destroy(n);
    return fail(rc, "%s", keep.c_str());
}

// The new graph `n` becomes the handle `h`.  What the handle keeps: its streams, timing settings and instrumentation buffers (the rest
// of it is the new graph's now); the old graph is destroyed.
inline void graft_swap(gbp_ba *h, gbp_ba *n)
{
    std::swap(n->own_stream, h->own_stream);
    std::swap(n->timing, h->timing); std::swap(n->timing_every, h->timing_every); std::swap(n->timing_tick, h->timing_tick);
    std::swap(n->ev, h->ev); std::swap(n->ev_used, h->ev_used);
    std::swap(n->clk_used, h->clk_used); std::swap(n->clk_rate_khz, h->clk_rate_khz);
    std::swap(n->clk_calibrated, h->clk_calibrated); std::swap(n->clk_rate_khz_measured, h->clk_rate_khz_measured);
    std::swap(n->side_stream, h->side_stream); std::swap(n->ev_fork, h->ev_fork); std::swap(n->ev_join, h->ev_join);
    if (h->d_clk) {
        h->allocs.erase(std::remove(h->allocs.begin(), h->allocs.end(), static_cast<void *>(h->d_clk)), h->allocs.end());
        n->allocs.push_back(h->d_clk);
        n->d_clk = h->d_clk; h->d_clk = nullptr;
    }
    n->rebuilds += h->rebuilds;                               // (gbp_ba_rebuild_count: the new graph's own build on top of the handle's)
    std::swap(*h, *n);                                        // h: the new graph; n: what is left of the old handle
    h->fused.alloc_ctx = h;
    n->stream = h->stream;                                    // (synchronised by destroy, not destroyed: own_stream went over)
    gbp_ba_destroy(n);
}

// ---- shrinking: from survival flags to the survivors' graph (gbp_ba_retire, gbp_ba_cull) ----------------------------------------------
// keep[0 .. C): the camera stays; keep[C .. C+L): the landmark (the CALLER's numbering) stays; keep[C+L .. C+L+F): the factor (old
// reference order) stays; keep[C+L+F] = 0, so that the exclusive scan behind it ends with the total.  One scan over all of it gives the
// three renumbering maps: new id = number of survivors below = scan[i] - scan[start of the kind].  A surviving factor's camera and
// landmark survive (the caller's flag kernel sees to that).  o_u2i / o_i2u (NULL: identity) lead to and from a reordered handle's records.
struct Survivors {
    int *o2n;                     // [C + L + F] the three maps one after the other: new id, or -1 for what is gone
    int *f_n2o;                   // [F'] old reference id of every surviving factor
    double *meas; int *cam, *lmk; // [F'] the survivors' observations in old reference order, ids in the NEW numbering
    double *cam_means, *lmk_means;// [C' x 6], [L' x 3] current belief means (node.mu)
};

// The maps and the survivors' inputs for the create path.  A surviving factor's measurement is the z rows of its slot.
// (static: these kernels are instantiated by every unit that shrinks a handle, each for itself)
static __global__ __launch_bounds__(BLOCK) void k_graft_compact(Params o, const int *__restrict__ ref_cam, const int *__restrict__ ref_lmk,
                                                                const int *__restrict__ o_u2i, const int *__restrict__ o_i2u,
                                                                const int *__restrict__ keep, const int *__restrict__ pos, Survivors s)
{
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t C = (size_t)o.C, L = (size_t)o.L, F = (size_t)o.F;
    if (i >= C + L + F) return;
    if (!keep[i]) { s.o2n[i] = -1; return; }
    if (i < C) {
        const int nc = pos[i];
        s.o2n[i] = nc;
#pragma unroll
        for (int k = 0; k < 6; ++k) s.cam_means[(size_t)nc * 6 + k] = o.cbel[i * CAMREC + CAM_MU + k];
    } else if (i < C + L) {
        const int nl = pos[i] - pos[C];
        s.o2n[i] = nl;
#pragma unroll
        for (int k = 0; k < 3; ++k) s.lmk_means[(size_t)nl * 3 + k] = o.lrec[(o_u2i ? (size_t)o_u2i[i - C] : i - C) * LREC + LR_MU + k];
    } else {
        const size_t f = i - C - L;
        const int nf = pos[i] - pos[C + L], os = o.cadj[f];
        s.o2n[i] = nf;
        s.f_n2o[nf] = (int)f;
        s.meas[(size_t)nf * 2] = o.lin[lin_at(os, ROW_Z)];
        s.meas[(size_t)nf * 2 + 1] = o.lin[lin_at(os, ROW_Z + 1)];
        s.cam[nf] = pos[ref_cam[f]];                            // (a surviving factor's camera and landmark survive)
        s.lmk[nf] = pos[C + (size_t)(o_i2u ? o_i2u[ref_lmk[f]] : ref_lmk[f])] - pos[C];
    }
}

// One lane per slot of the survivors' graph: the factor's whole state from its old slot (transplant_slot)
static __global__ __launch_bounds__(BLOCK) void k_graft_slots(Params n, Params o, const int *__restrict__ f_n2o)
{
    const int slot = blockIdx.x * BLOCK + threadIdx.x;
    if (slot >= n.T * WTILE || (slot & 63) >= n.tiles[slot >> 6].z) return;
    const int r = n.cpos[slot];
    if (r < 0 || r >= n.F) return;
    const int f = f_n2o[r];
    if (f < 0 || f >= o.F) return;
    transplant_slot(n, o, slot, o.cadj[f]);
}

// One lane per OLD variable: a surviving camera keeps its record, belief view and prior; a surviving landmark its mean | covariance
// and prior (gbp_ba_retire then writes the landmarks' priors again, with the folds)
static __global__ __launch_bounds__(BLOCK) void k_graft_vars(Params n, Params o, const int *__restrict__ o2n, const int *__restrict__ n_u2i, const int *__restrict__ o_u2i)
{
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= o.C + o.L) return;
    const int nv = o2n[v];
    if (nv < 0) return;
    if (v < o.C) transplant_cam(n, o, nv, v);
    else transplant_lmk(n, o, n_u2i ? n_u2i[nv] : nv, o_u2i ? o_u2i[v - o.C] : v - o.C);
}

// The survivors' graph built beside the old handle `o` into the fresh handle `n` (which owns nothing of o's), from the survival flags
// d_keep[C + L + F + 1] (device, made on n->stream).  `emptied`: the message when nothing survives.  `after_transplant(s)`: what the caller
// launches on n->stream between the transplant and update_all_beliefs (gbp_ba_retire: the fold; gbp_ba_cull: nothing).  maps: the three
// maps one after the other, on the host.
//
// The survivors' "file order" is the old reference order with the departed factors taken out: camera renumbering is monotone, so that
// list is camera-major already, create keeps it as it is (no sort, no ref_file map) and new reference id = position in the list.
template <typename After>
inline int graft_survivors(gbp_ba *o, gbp_ba *n, const int *d_keep, std::vector<void *> &scratch, std::vector<int> &maps, const char *emptied,
                           After &&after_transplant)
{
    const Params &op = o->p;
    const size_t N = (size_t)op.C + op.L + op.F;

    // 1. one prefix sum, the survivors' sizes
    int *d_pos = nullptr;
    CHK(graft_scratch(n, scratch, &d_pos, N + 1));
    size_t scan_bytes = 0;
    HIPCHK(rocprim::exclusive_scan(nullptr, scan_bytes, d_keep, d_pos, 0, N + 1, rocprim::plus<int>(), n->stream));
    void *scan_tmp = nullptr;
    HIPCHK(hipMallocAsync(&scan_tmp, std::max<size_t>(scan_bytes, 1), n->stream));
    scratch.push_back(scan_tmp);
    HIPCHK(rocprim::exclusive_scan(scan_tmp, scan_bytes, d_keep, d_pos, 0, N + 1, rocprim::plus<int>(), n->stream));
    int ends[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(&ends[0], d_pos + op.C, sizeof(int), hipMemcpyDeviceToHost, n->stream));
    HIPCHK(hipMemcpyAsync(&ends[1], d_pos + op.C + op.L, sizeof(int), hipMemcpyDeviceToHost, n->stream));
    HIPCHK(hipMemcpyAsync(&ends[2], d_pos + N, sizeof(int), hipMemcpyDeviceToHost, n->stream));
    HIPCHK(hipStreamSynchronize(n->stream));
    const int C = ends[0], L = ends[1] - ends[0], F = ends[2] - ends[1];
    if (F <= 0 || C <= 0 || L <= 0) return fail(GBP_EINVAL, "%s", emptied);
    graft_settings(o, n, C, L, F);
    Params &p = n->p;

    // 2. the survivors' inputs, on the device
    Survivors s{};
    CHK(graft_scratch(n, scratch, &s.o2n, N)); CHK(graft_scratch(n, scratch, &s.f_n2o, (size_t)F));
    CHK(graft_scratch(n, scratch, &s.meas, (size_t)F * 2)); CHK(graft_scratch(n, scratch, &s.cam, (size_t)F)); CHK(graft_scratch(n, scratch, &s.lmk, (size_t)F));
    CHK(graft_scratch(n, scratch, &s.cam_means, (size_t)C * 6)); CHK(graft_scratch(n, scratch, &s.lmk_means, (size_t)L * 3));
    hipLaunchKernelGGL(k_graft_compact, dim3(grid_for(N)), dim3(BLOCK), 0, n->stream, op, o->d_ref_cam, o->d_ref_lmk, o->d_lmk_u2i, o->d_lmk_i2u, d_keep, d_pos, s);
    HIPCHK(hipGetLastError());

    // 3. the survivors' graph by the create path
    gbp_ba_desc_t d{};
    d.n_cams = C; d.n_lmks = L; d.n_factors = F; d.device = o->device;
    d.cam_means = s.cam_means; d.lmk_means = s.lmk_means; d.meas = s.meas; d.cam_idx = s.cam; d.lmk_idx = s.lmk;
    d.flags = GBP_FLAG_DEVICE_INPUT;                           // (the sweep flags are n->flags)
    const int *ref_file = nullptr;
    CHK(build_graph(n, &d, scratch, n->n_cus, &ref_file));
    if (ref_file) return fail(GBP_ESTATE, "internal error: the survivors' list is not camera-major");

    // 4. a remainder switched on on demand stays on (the fresh handle allocates it exactly as the old one did)
    if (o->lazy_xtra && op.xtra) CHK(enable_remainder(n));

    // 5. the state transplant, and what the caller does to it
    hipLaunchKernelGGL(k_graft_slots, dim3(grid_for(n_slots(n))), dim3(BLOCK), 0, n->stream, p, op, s.f_n2o);
    hipLaunchKernelGGL(k_graft_vars, dim3(grid_for((size_t)op.C + op.L)), dim3(BLOCK), 0, n->stream, p, op, s.o2n, n->d_lmk_u2i, o->d_lmk_u2i);
    after_transplant(s);
    HIPCHK(hipGetLastError());
    CHK(graft_counters(o, n));

    // 6. update_all_beliefs over the survivors
    CHK(gbp_ba_update_beliefs(n));
    maps.resize(N);
    HIPCHK(hipMemcpyAsync(maps.data(), s.o2n, sizeof(int) * N, hipMemcpyDeviceToHost, n->stream));
    HIPCHK(hipStreamSynchronize(n->stream));
    return GBP_OK;
}

// the end of a shrinking call: the scratch goes; on success the maps go out (sizes from BEFORE the call, NULL to skip) and the new
// graph becomes the handle, on failure the half-built graph goes and the handle is what it was
inline int graft_finish_shrink(gbp_ba *h, gbp_ba *n, int rc, std::vector<void *> &scratch, const std::vector<int> &maps,
                               int32_t *cam_old_to_new, int32_t *lmk_old_to_new, int32_t *factor_old_to_new)
{
    for (void *q : scratch) (void)hipFreeAsync(q, h->stream);
    (void)hipStreamSynchronize(h->stream);
    if (rc != GBP_OK) return n ? graft_abandon(n, rc) : rc;
    const size_t C0 = (size_t)h->p.C, L0 = (size_t)h->p.L, F0 = (size_t)h->p.F;     // (h->p is the old graph's until the swap)
    if (cam_old_to_new) std::memcpy(cam_old_to_new, maps.data(), C0 * sizeof(int32_t));
    if (lmk_old_to_new) std::memcpy(lmk_old_to_new, maps.data() + C0, L0 * sizeof(int32_t));
    if (factor_old_to_new) std::memcpy(factor_old_to_new, maps.data() + C0 + L0, F0 * sizeof(int32_t));
    graft_swap(h, n);
    return GBP_OK;
}

// nothing goes: identity maps
inline void graft_identity_maps(const Params &op, int32_t *cam_old_to_new, int32_t *lmk_old_to_new, int32_t *factor_old_to_new)
{
    for (int i = 0; cam_old_to_new && i < op.C; ++i) cam_old_to_new[i] = i;
    for (int i = 0; lmk_old_to_new && i < op.L; ++i) lmk_old_to_new[i] = i;
    for (int i = 0; factor_old_to_new && i < op.F; ++i) factor_old_to_new[i] = i;
}

}  // namespace gbp
