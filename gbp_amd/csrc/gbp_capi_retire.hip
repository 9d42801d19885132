// gbp_capi_retire.hip -- libgbp_hip.so, shrinking a live handle (gbp_ba_retire, include/gbp_ba.h): the counterpart of gbp_capi_extend.hip.
// Retired cameras leave with all their factors; what those factors told their landmarks -- the factor-to-landmark messages -- is folded
// into the landmarks' priors (GBP's own marginalisation: a factor has one camera, so landmarks are the only surviving neighbours), and
// landmarks left without a factor leave too.  The survivors' graph is BUILT beside the handle by the create path (gbp::build_graph, from
// arrays assembled on the device), the survivors' state is transplanted into its layout through index maps, and it is swapped in only
// when everything has succeeded.
//
// From the survival flags on, the way is the one gbp_ba_cull shares (gbp_graft.hpp: graft_survivors); here: the flags and the fold.
#include "gbp_graft.hpp"

namespace {

// keep[0 .. C): the camera stays; keep[C .. C+L): the landmark has a surviving factor; keep[C+L .. C+L+F): the factor (old reference
// order) stays; keep[C+L+F] = 0, so that the exclusive scan behind it ends with the total.  One scan over all of it gives the three
// renumbering maps: new id = number of survivors below = scan[i] - scan[start of the kind].  Landmarks are walked in the CALLER's numbering
// (the maps are the caller's): o_u2i / o_i2u (NULL: identity) lead to and from a reordered handle's records, here and below.
__global__ __launch_bounds__(BLOCK) void k_retire_flags(Params o, const int *__restrict__ ref_cam, const int *__restrict__ retired, const int *__restrict__ o_u2i,
                                                        int *__restrict__ keep)
{
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t C = (size_t)o.C, L = (size_t)o.L, F = (size_t)o.F;
    if (i < C) {
        keep[i] = retired[i] ? 0 : 1;
    } else if (i < C + L) {
        const int2 rows = *reinterpret_cast<const int2 *>(o.lrec + (o_u2i ? (size_t)o_u2i[i - C] : i - C) * LREC + LR_ROWS);
        int any = 0;
        for (int s = rows.x; s < rows.y && !any; ++s) any = retired[slot_meta(o, s) >> META_LMK_BITS] ? 0 : 1;
        keep[i] = any;
    } else if (i < C + L + F) {
        keep[i] = retired[ref_cam[i - C - L]] ? 0 : 1;
    } else if (i == C + L + F) {
        keep[i] = 0;
    }
}

// One lane per OLD landmark that survives walks its old slot range in adj_factors order; every factor of a retired camera is folded into
// the prior: l.prior += f.messages[1], the full message as the message view reports it (dense_messages: Lambda = J_l^T V J_l and
// eta = J_l^T q_L with J at the factor's stored linearisation point, plus the landmark part of the dense remainder).  Prior first, then
// the folds one by one in fp64: a fixed order, the same result every run.  A landmark none of whose factors goes keeps its prior bit for bit.
__global__ __launch_bounds__(BLOCK) void k_fold_retired(Params n, Params o, const int *__restrict__ lmk_o2n, const int *__restrict__ retired,
                                                        const int *__restrict__ n_u2i, const int *__restrict__ o_u2i)
{
    const int l = blockIdx.x * BLOCK + threadIdx.x;              // the caller's id of an old landmark
    if (l >= o.L) return;
    int nl = lmk_o2n[l];
    if (nl < 0) return;
    if (n_u2i) nl = n_u2i[nl];
    const double *lr = o.lrec + (size_t)(o_u2i ? o_u2i[l] : l) * LREC;
    double acc[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) acc[k] = lr[LR_PRIOR + k];
    const int2 rows = *reinterpret_cast<const int2 *>(lr + LR_ROWS);
    for (int s = rows.x; s < rows.y; ++s) {
        if (!retired[slot_meta(o, s) >> META_LMK_BITS]) continue;
        double eC[6], MC[21], eL[3], ML[6];
        dense_messages(o, s, eC, MC, eL, ML);
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] += eL[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) acc[3 + k] += ML[k];
    }
    double *dst = n.lrec + (size_t)nl * LREC + LR_PRIOR;
#pragma unroll
    for (int k = 0; k < 9; ++k) dst[k] = acc[k];
}

// the survivors' graph built beside the old handle `o` into the fresh handle `n` (which owns nothing of o's); maps: the three maps one
// after the other, on the host
int retire_into(gbp_ba *o, gbp_ba *n, const std::vector<int> &retired, std::vector<void *> &scratch, std::vector<int> &maps)
{
    const Params &op = o->p;
    const size_t N = (size_t)op.C + op.L + op.F;
    n->device = o->device; n->stream = o->stream;              // (graft_settings sets the rest once the sizes are known)
    int *d_ret = nullptr, *d_keep = nullptr;
    CHK(graft_scratch(n, scratch, &d_ret, (size_t)op.C)); CHK(graft_scratch(n, scratch, &d_keep, N + 1));
    HIPCHK(hipMemcpyAsync(d_ret, retired.data(), sizeof(int) * (size_t)op.C, hipMemcpyHostToDevice, n->stream));
    hipLaunchKernelGGL(k_retire_flags, dim3(grid_for(N + 1)), dim3(BLOCK), 0, n->stream, op, o->d_ref_cam, d_ret, o->d_lmk_u2i, d_keep);
    HIPCHK(hipGetLastError());
    // the fold of the retired factors' messages into their landmarks' priors, over the transplanted priors
    return graft_survivors(o, n, d_keep, scratch, maps, "retiring these cameras leaves no factor", [&](const Survivors &s) {
        hipLaunchKernelGGL(k_fold_retired, dim3(grid_for((size_t)op.L)), dim3(BLOCK), 0, n->stream, n->p, op, s.o2n + op.C, d_ret, n->d_lmk_u2i, o->d_lmk_u2i);
    });
}

}  // namespace

extern "C" {

int gbp_ba_retire(gbp_ba_t *h, int32_t n_cams, const int32_t *cam_ids, int32_t *cam_old_to_new, int32_t *lmk_old_to_new, int32_t *factor_old_to_new)
{
    ENTER(h);
    if (h->xch_fn || h->comm || h->peer.mailbox || h->peer.connected)
        return fail(GBP_ESTATE, "a sharded handle (communicator, exchange callback or peer mailbox) cannot retire cameras");
    if (!h->has_beliefs) return fail(GBP_ESTATE, "the handle has no beliefs yet (gbp_ba_update_beliefs first)");
    if (n_cams < 0) return fail(GBP_EINVAL, "negative count");
    if (n_cams && !cam_ids) return fail(GBP_EINVAL, "null camera list");
    const Params &op = h->p;
    if (n_cams == 0) {                                        // nothing goes: nothing changes
        graft_identity_maps(op, cam_old_to_new, lmk_old_to_new, factor_old_to_new);
        return GBP_OK;
    }
    gbp_ba *n = nullptr;
    std::vector<void *> scratch;
    std::vector<int> maps;
    int rc;
    try {
        std::vector<int> retired((size_t)op.C, 0);
        for (int i = 0; i < n_cams; ++i) {
            const int c = cam_ids[i];
            if (c < 0 || c >= op.C) return fail(GBP_EINVAL, "camera %d (entry %d of the list) is outside [0,%d)", c, i, op.C);
            if (retired[(size_t)c]) return fail(GBP_EINVAL, "camera %d is listed twice", c);
            retired[(size_t)c] = 1;
        }
        if (n_cams >= op.C) return fail(GBP_EINVAL, "retiring every camera leaves no factor");
        HIPCHK(hipStreamSynchronize(h->stream));
        n = new (std::nothrow) gbp_ba;
        if (!n) return fail(GBP_ENOMEM, "out of host memory");
        rc = retire_into(h, n, retired, scratch, maps);
    } catch (const std::bad_alloc &) {
        rc = fail(GBP_ENOMEM, "out of host memory");
    }
    return graft_finish_shrink(h, n, rc, scratch, maps, cam_old_to_new, lmk_old_to_new, factor_old_to_new);
}

}  // extern "C"
