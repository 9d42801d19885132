// gbp_graft.hpp -- what the calls that rebuild a live handle share: gbp_ba_extend (gbp_capi_extend.hip) and the engine behind
// gbp_ba_window_step, gbp_ba_cull, gbp_ba_retire and gbp_ba_retire_landmarks (gbp_capi_window.hip).  Both build the new graph BESIDE the
// handle by the create path (gbp::build_graph), move the state of the factors and variables that live on into the new layout, and swap
// the new graph in only when everything has succeeded.  Here: the per-slot and per-variable moves (device), the arrays a rebuild
// assembles for the create path (Survivors), and on the host what every call asks of the handle and of a batch before it starts
// (live_and_whole, sound_batch), the settings the new graph inherits, the counters it carries, the
// swap itself and the maps of a call that changes nothing.
#pragma once
#include "gbp_handle.hpp"

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
// what every call that rebuilds a handle asks of it before it looks at its arguments
inline int live_and_whole(const gbp_ba *h, const char *to_do)
{
    if (h->xch_fn || h->comm || h->peer.mailbox || h->peer.connected)
        return fail(GBP_ESTATE, "a sharded handle (communicator, exchange callback or peer mailbox) cannot %s", to_do);
    if (!h->has_beliefs) return fail(GBP_ESTATE, "the handle has no beliefs yet (gbp_ba_update_beliefs first)");
    return GBP_OK;
}

// what every call that brings a batch asks of it before its ids are looked at: sizes, flags, arrays, a union that an int can index
// ([C + dC | L + dL | F + dF | 1]: the window engine does) and whose cameras fit the meta word
inline int sound_batch(const Params &op, const gbp_ba_ext_t *e)
{
    const int dC = e->n_new_cams, dL = e->n_new_lmks, dF = e->n_new_factors;
    if (dC < 0 || dL < 0 || dF < 0) return fail(GBP_EINVAL, "negative size");
    if (e->flags & ~GBP_FLAG_DEVICE_INPUT) return fail(GBP_EINVAL, "unknown flags 0x%x (only GBP_FLAG_DEVICE_INPUT)", e->flags);
    if ((dC && !e->cam_means) || (dL && !e->lmk_means)) return fail(GBP_EINVAL, "null initial means");
    if (dF && (!e->meas || !e->cam_idx || !e->lmk_idx)) return fail(GBP_EINVAL, "null observation arrays");
    if ((int64_t)op.C + dC > INT32_MAX || (int64_t)op.L + dL > INT32_MAX || (int64_t)op.F + dF > INT32_MAX ||
        (int64_t)op.C + dC + (int64_t)op.L + dL + (int64_t)op.F + dF >= INT32_MAX)
        return fail(GBP_EINVAL, "sizes exceed int32");
    if (op.C + dC >= (1 << (32 - META_LMK_BITS))) return fail(GBP_EINVAL, "more than %d cameras are not supported", (1 << (32 - META_LMK_BITS)) - 1);
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

// What a rebuild that lets things go assembles on the device for the create path, and its maps (gbp_capi_window.hip fills them, over the
// index space of the old graph followed by the batch; the ids are the CALLER's: new id = number of survivors below)
struct Survivors {
    int *o2n;                     // [C | L | F] the maps one after the other: new id, or -1 for what is gone
    int *f_n2o;                   // [F'] the old id of the factor at every file position of the result
    double *meas; int *cam, *lmk; // [F'] the result's observations in file order, ids in the NEW numbering
    double *cam_means, *lmk_means;// [C' x 6], [L' x 3] current belief means (node.mu) of old variables, the given means of new ones
};

// nothing goes: identity maps
inline void graft_identity_maps(const Params &op, int32_t *cam_old_to_new, int32_t *lmk_old_to_new, int32_t *factor_old_to_new)
{
    for (int i = 0; cam_old_to_new && i < op.C; ++i) cam_old_to_new[i] = i;
    for (int i = 0; lmk_old_to_new && i < op.L; ++i) lmk_old_to_new[i] = i;
    for (int i = 0; factor_old_to_new && i < op.F; ++i) factor_old_to_new[i] = i;
}

}  // namespace gbp
