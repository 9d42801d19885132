// gbp_capi_retire_lmk.hip -- libgbp_hip.so, letting go of landmarks by name (gbp_ba_retire_landmarks, include/gbp_ba.h): the mirror image
// of gbp_capi_retire.hip.  A listed landmark leaves with all its factors.  A factor has one landmark, so the only surviving neighbours
// of those factors are cameras: in mode FOLD what the factors told their cameras -- the factor-to-camera messages -- is folded into the
// cameras' priors (GBP's own marginalisation, as gbp_ba_retire does it for landmarks); in mode DROP the landmarks were bad and the
// messages vanish, as gbp_ba_cull has it.  Cameras and landmarks left without a factor leave too.  From the survival flags on, the way
// is the one gbp_ba_retire and gbp_ba_cull go (gbp_graft.hpp: graft_survivors); here: the flags and the fold.
#include "gbp_graft.hpp"

namespace {

// whether reference factor f belongs to a listed landmark.  d_ref_lmk holds the handle's INTERNAL landmark ids (gbp_capi.hip relabels it
// in place on a reordered handle), the list is in the CALLER's numbering: o_i2u (NULL: identity) leads back.
GBP_DEV int factor_goes(const int *__restrict__ ref_lmk, const int *__restrict__ o_i2u, const int *__restrict__ retired, int f)
{
    const int li = ref_lmk[f];
    return retired[o_i2u ? o_i2u[li] : li];
}

// The survival flags of gbp_graft.hpp from retired[L] (the caller's numbering; 1: the landmark is on the list).  A factor stays unless
// its landmark is listed; a landmark stays when it is not listed and has a factor (its slot range, cpos: slot -> reference id; o_u2i
// leads to a reordered handle's record); a camera stays when its contiguous range of the camera-major reference order (cptr) holds a
// surviving factor.
__global__ __launch_bounds__(BLOCK) void k_lmk_retire_flags(Params o, const int *__restrict__ ref_lmk, const int *__restrict__ retired,
                                                            const int *__restrict__ o_u2i, const int *__restrict__ o_i2u, int *__restrict__ keep)
{
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t C = (size_t)o.C, L = (size_t)o.L, F = (size_t)o.F;
    if (i < C) {
        int any = 0;
        for (int f = o.cptr[i], f1 = o.cptr[i + 1]; f < f1 && !any; ++f) any = factor_goes(ref_lmk, o_i2u, retired, f) ? 0 : 1;
        keep[i] = any;
    } else if (i < C + L) {
        int any = 0;
        if (!retired[i - C]) {
            const int2 rows = *reinterpret_cast<const int2 *>(o.lrec + (o_u2i ? (size_t)o_u2i[i - C] : i - C) * LREC + LR_ROWS);
            for (int s = rows.x; s < rows.y && !any; ++s) {
                const int f = o.cpos[s];
                any = (f >= 0 && f < o.F) ? 1 : 0;
            }
        }
        keep[i] = any;
    } else if (i < C + L + F) {
        keep[i] = factor_goes(ref_lmk, o_i2u, retired, (int)(i - C - L)) ? 0 : 1;
    } else if (i == C + L + F) {
        keep[i] = 0;
    }
}

// One WAVE per OLD camera that survives: c.prior += f.messages[0] for every factor f of c whose landmark is listed -- the full message
// as the message view reports it (dense_messages: Lambda = J_c^T W J_c and eta = J_c^T q_C with J at the factor's stored linearisation
// point, plus the camera part of the dense remainder).  The camera's factors are its range of the reference order, walked in chunks of
// 64: lane j takes factor cptr[c] + 64 k + j of chunk k and rebuilds its message (a factor that stays, or a lane past the end, holds
// zeros), the 27 sums of the chunk are formed by an xor butterfly over the wave -- a fixed tree, the same in every lane -- and the
// chunk totals are added in ascending k on top of the prior: lane e < 27 keeps entry e.  No atomics: the same bits every run, whatever
// the grid.  A chunk without a departing factor adds nothing, and a camera without one is not written: its prior stays bit for bit.
// (One lane per camera would rebuild a camera's messages one after the other -- 2 000 linearisations in a row at the headline size.)
__global__ __launch_bounds__(BLOCK) void k_fold_retired_lmks(Params n, Params o, const int *__restrict__ cam_o2n, const int *__restrict__ ref_lmk,
                                                             const int *__restrict__ o_i2u, const int *__restrict__ retired)
{
    const int lane = threadIdx.x & (WTILE - 1);
    const int c = blockIdx.x * (BLOCK / WTILE) + (threadIdx.x >> 6);      // wave-uniform from here on
    if (c >= o.C) return;
    const int nc = cam_o2n[c];
    if (nc < 0) return;
    const int f0 = o.cptr[c], f1 = o.cptr[c + 1];
    double mine = lane < 27 ? o.cprior[(size_t)c * 27 + lane] : 0.0;
    bool touched = false;
    for (int base = f0; base < f1; base += WTILE) {
        const int f = base + lane;
        const bool goes = f < f1 && factor_goes(ref_lmk, o_i2u, retired, f);
        if (!__ballot(goes)) continue;
        touched = true;
        double v[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) v[k] = 0.0;
        if (goes) {
            double eC[6], MC[21], eL[3], ML[6];
            dense_messages(o, o.cadj[f], eC, MC, eL, ML);
#pragma unroll
            for (int k = 0; k < 6; ++k) v[k] = eC[k];
#pragma unroll
            for (int k = 0; k < 21; ++k) v[6 + k] = MC[k];
        }
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            double t = v[k];
#pragma unroll
            for (int m = 1; m < WTILE; m <<= 1) t += __shfl_xor(t, m, WTILE);
            if (lane == k) mine += t;
        }
    }
    if (touched && lane < 27) n.cprior[(size_t)nc * 27 + lane] = mine;
}

// the survivors' graph built beside the old handle `o` into the fresh handle `n` (which owns nothing of o's); maps: the three maps one
// after the other, on the host
int retire_lmks_into(gbp_ba *o, gbp_ba *n, const std::vector<int> &retired, bool fold, std::vector<void *> &scratch, std::vector<int> &maps)
{
    const Params &op = o->p;
    const size_t N = (size_t)op.C + op.L + op.F;
    n->device = o->device; n->stream = o->stream;              // (graft_settings sets the rest once the sizes are known)
    int *d_ret = nullptr, *d_keep = nullptr;
    CHK(graft_scratch(n, scratch, &d_ret, (size_t)op.L)); CHK(graft_scratch(n, scratch, &d_keep, N + 1));
    HIPCHK(hipMemcpyAsync(d_ret, retired.data(), sizeof(int) * (size_t)op.L, hipMemcpyHostToDevice, n->stream));
    hipLaunchKernelGGL(k_lmk_retire_flags, dim3(grid_for(N + 1)), dim3(BLOCK), 0, n->stream, op, o->d_ref_lmk, d_ret, o->d_lmk_u2i, o->d_lmk_i2u, d_keep);
    HIPCHK(hipGetLastError());
    // the fold of the departing factors' messages into their cameras' priors, over the transplanted priors (mode DROP: no fold)
    return graft_survivors(o, n, d_keep, scratch, maps, "retiring these landmarks leaves no factor", [&](const Survivors &s) {
        if (!fold) return;
        const int waves = BLOCK / WTILE;
        hipLaunchKernelGGL(k_fold_retired_lmks, dim3((op.C + waves - 1) / waves), dim3(BLOCK), 0, n->stream, n->p, op, s.o2n, o->d_ref_lmk, o->d_lmk_i2u, d_ret);
    });
}

}  // namespace

extern "C" {

int gbp_ba_retire_landmarks(gbp_ba_t *h, int32_t n_lmks, const int32_t *lmk_ids, int32_t mode, int32_t *cam_old_to_new, int32_t *lmk_old_to_new,
                            int32_t *factor_old_to_new)
{
    ENTER(h);
    if (h->xch_fn || h->comm || h->peer.mailbox || h->peer.connected)
        return fail(GBP_ESTATE, "a sharded handle (communicator, exchange callback or peer mailbox) cannot retire landmarks");
    if (!h->has_beliefs) return fail(GBP_ESTATE, "the handle has no beliefs yet (gbp_ba_update_beliefs first)");
    if (n_lmks < 0) return fail(GBP_EINVAL, "negative count");
    if (n_lmks && !lmk_ids) return fail(GBP_EINVAL, "null landmark list");
    if (mode != GBP_RETIRE_FOLD && mode != GBP_RETIRE_DROP) return fail(GBP_EINVAL, "mode %d is neither GBP_RETIRE_FOLD nor GBP_RETIRE_DROP", mode);
    const Params &op = h->p;
    if (n_lmks == 0) {                                        // nothing goes: nothing changes
        graft_identity_maps(op, cam_old_to_new, lmk_old_to_new, factor_old_to_new);
        return GBP_OK;
    }
    gbp_ba *n = nullptr;
    std::vector<void *> scratch;
    std::vector<int> maps;
    int rc;
    try {
        std::vector<int> retired((size_t)op.L, 0);
        for (int i = 0; i < n_lmks; ++i) {
            const int l = lmk_ids[i];
            if (l < 0 || l >= op.L) return fail(GBP_EINVAL, "landmark %d (entry %d of the list) is outside [0,%d)", l, i, op.L);
            if (retired[(size_t)l]) return fail(GBP_EINVAL, "landmark %d (entry %d of the list) is listed twice", l, i);
            retired[(size_t)l] = 1;
        }
        if (n_lmks >= op.L) return fail(GBP_EINVAL, "retiring every landmark leaves no factor");
        HIPCHK(hipStreamSynchronize(h->stream));
        n = new (std::nothrow) gbp_ba;
        if (!n) return fail(GBP_ENOMEM, "out of host memory");
        rc = retire_lmks_into(h, n, retired, mode == GBP_RETIRE_FOLD, scratch, maps);
    } catch (const std::bad_alloc &) {
        rc = fail(GBP_ENOMEM, "out of host memory");
    }
    return graft_finish_shrink(h, n, rc, scratch, maps, cam_old_to_new, lmk_old_to_new, factor_old_to_new);
}

}  // extern "C"
