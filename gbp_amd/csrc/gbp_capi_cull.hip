// gbp_capi_cull.hip -- libgbp_hip.so, removing single observations from a live handle (gbp_ba_cull, include/gbp_ba.h): the sibling of
// gbp_capi_retire.hip.  A culled factor was WRONG (a bad match the front end found after a few sweeps), so what it told its camera and
// its landmark must vanish: both messages are discarded and nothing is added to any prior -- where retirement folds, culling drops.
// Cameras and landmarks left without a factor leave too.  From the survival flags on, the way is the one gbp_ba_retire goes
// (gbp_graft.hpp: graft_survivors): one scan, the survivors' graph by the create path beside the handle, the state transplant through
// index maps, update_all_beliefs, the swap.  No fold kernel runs.
#include "gbp_graft.hpp"

namespace {

// The survival flags of gbp_graft.hpp from gone[F] (old reference order; 1: the factor is on the list).  A factor stays unless it is
// listed; a variable stays when any of its factors does: a camera looks at its contiguous range of the camera-major reference order
// (cptr), a landmark -- walked in the CALLER's numbering, o_u2i (NULL: identity) leads to a reordered handle's record -- at its slot
// range (cpos: slot -> reference id).  Both stop at the first survivor; a variable that had no factor goes.
__global__ __launch_bounds__(BLOCK) void k_cull_flags(Params o, const int *__restrict__ gone, const int *__restrict__ o_u2i, int *__restrict__ keep)
{
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t C = (size_t)o.C, L = (size_t)o.L, F = (size_t)o.F;
    if (i < C) {
        int any = 0;
        for (int f = o.cptr[i], f1 = o.cptr[i + 1]; f < f1 && !any; ++f) any = gone[f] ? 0 : 1;
        keep[i] = any;
    } else if (i < C + L) {
        const int2 rows = *reinterpret_cast<const int2 *>(o.lrec + (o_u2i ? (size_t)o_u2i[i - C] : i - C) * LREC + LR_ROWS);
        int any = 0;
        for (int s = rows.x; s < rows.y && !any; ++s) {
            const int f = o.cpos[s];
            any = (f >= 0 && f < o.F && !gone[f]) ? 1 : 0;
        }
        keep[i] = any;
    } else if (i < C + L + F) {
        keep[i] = gone[i - C - L] ? 0 : 1;
    } else if (i == C + L + F) {
        keep[i] = 0;
    }
}

// the survivors' graph built beside the old handle `o` into the fresh handle `n` (which owns nothing of o's)
int cull_into(gbp_ba *o, gbp_ba *n, const std::vector<int> &gone, std::vector<void *> &scratch, std::vector<int> &maps)
{
    const Params &op = o->p;
    const size_t N = (size_t)op.C + op.L + op.F;
    n->device = o->device; n->stream = o->stream;              // (graft_settings sets the rest once the sizes are known)
    int *d_gone = nullptr, *d_keep = nullptr;
    CHK(graft_scratch(n, scratch, &d_gone, (size_t)op.F)); CHK(graft_scratch(n, scratch, &d_keep, N + 1));
    HIPCHK(hipMemcpyAsync(d_gone, gone.data(), sizeof(int) * (size_t)op.F, hipMemcpyHostToDevice, n->stream));
    hipLaunchKernelGGL(k_cull_flags, dim3(grid_for(N + 1)), dim3(BLOCK), 0, n->stream, op, d_gone, o->d_lmk_u2i, d_keep);
    HIPCHK(hipGetLastError());
    return graft_survivors(o, n, d_keep, scratch, maps, "culling these factors leaves no factor", [](const Survivors &) {});
}

}  // namespace

extern "C" {

int gbp_ba_cull(gbp_ba_t *h, int32_t n_factors, const int32_t *factor_ids, int32_t *cam_old_to_new, int32_t *lmk_old_to_new, int32_t *factor_old_to_new)
{
    ENTER(h);
    if (h->xch_fn || h->comm || h->peer.mailbox || h->peer.connected)
        return fail(GBP_ESTATE, "a sharded handle (communicator, exchange callback or peer mailbox) cannot cull factors");
    if (!h->has_beliefs) return fail(GBP_ESTATE, "the handle has no beliefs yet (gbp_ba_update_beliefs first)");
    if (n_factors < 0) return fail(GBP_EINVAL, "negative count");
    if (n_factors && !factor_ids) return fail(GBP_EINVAL, "null factor list");
    const Params &op = h->p;
    if (n_factors == 0) {                                     // nothing goes: nothing changes
        graft_identity_maps(op, cam_old_to_new, lmk_old_to_new, factor_old_to_new);
        return GBP_OK;
    }
    gbp_ba *n = nullptr;
    std::vector<void *> scratch;
    std::vector<int> maps;
    int rc;
    try {
        std::vector<int> gone((size_t)op.F, 0);
        for (int i = 0; i < n_factors; ++i) {
            const int f = factor_ids[i];
            if (f < 0 || f >= op.F) return fail(GBP_EINVAL, "factor %d (entry %d of the list) is outside [0,%d)", f, i, op.F);
            if (gone[(size_t)f]) return fail(GBP_EINVAL, "factor %d (entry %d of the list) is listed twice", f, i);
            gone[(size_t)f] = 1;
        }
        if (n_factors >= op.F) return fail(GBP_EINVAL, "culling every factor leaves no factor");
        HIPCHK(hipStreamSynchronize(h->stream));
        n = new (std::nothrow) gbp_ba;
        if (!n) return fail(GBP_ENOMEM, "out of host memory");
        rc = cull_into(h, n, gone, scratch, maps);
    } catch (const std::bad_alloc &) {
        rc = fail(GBP_ENOMEM, "out of host memory");
    }
    return graft_finish_shrink(h, n, rc, scratch, maps, cam_old_to_new, lmk_old_to_new, factor_old_to_new);
}

}  // extern "C"
