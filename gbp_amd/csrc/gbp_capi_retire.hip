// gbp_capi_retire.hip -- libgbp_hip.so, shrinking a live handle (gbp_ba_retire, include/gbp_ba.h): the counterpart of gbp_capi_extend.hip.
// Retired cameras leave with all their factors; what those factors told their landmarks -- the factor-to-landmark messages -- is folded
// into the landmarks' priors (GBP's own marginalisation: a factor has one camera, so landmarks are the only surviving neighbours), and
// landmarks left without a factor leave too.  The survivors' graph is BUILT beside the handle by the create path (gbp::build_graph, from
// arrays assembled on the device), the survivors' state is transplanted into its layout through index maps, and it is swapped in only
// when everything has succeeded.
//
// The survivors' "file order" is the old reference order with the retired factors taken out: camera renumbering is monotone, so that
// list is camera-major already, create keeps it as it is (no sort, no ref_file map) and new reference id = position in the list.
#include "gbp_graft.hpp"

#include <rocprim/device/device_scan.hpp>

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

struct Survivors {
    int *o2n;                     // [C + L + F] the three maps one after the other: new id, or -1 for what is gone
    int *f_n2o;                   // [F'] old reference id of every surviving factor
    double *meas; int *cam, *lmk; // [F'] the survivors' observations in old reference order, ids in the NEW numbering
    double *cam_means, *lmk_means;// [C' x 6], [L' x 3] current belief means (node.mu)
};

// The maps and the survivors' inputs for the create path.  A surviving factor's measurement is the z rows of its slot.
__global__ __launch_bounds__(BLOCK) void k_retire_compact(Params o, const int *__restrict__ ref_cam, const int *__restrict__ ref_lmk,
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

// One lane per slot of the survivors' graph: the factor's whole state from its old slot (gbp_graft.hpp: transplant_slot)
__global__ __launch_bounds__(BLOCK) void k_retire_slots(Params n, Params o, const int *__restrict__ f_n2o)
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
// (its prior is k_fold_retired's)
__global__ __launch_bounds__(BLOCK) void k_retire_vars(Params n, Params o, const int *__restrict__ o2n, const int *__restrict__ n_u2i, const int *__restrict__ o_u2i)
{
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= o.C + o.L) return;
    const int nv = o2n[v];
    if (nv < 0) return;
    if (v < o.C) transplant_cam(n, o, nv, v);
    else transplant_lmk(n, o, n_u2i ? n_u2i[nv] : nv, o_u2i ? o_u2i[v - o.C] : v - o.C);
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

    // 1. flags, one prefix sum, the survivors' sizes
    int *d_ret = nullptr, *d_keep = nullptr, *d_pos = nullptr;
    CHK(graft_scratch(n, scratch, &d_ret, (size_t)op.C)); CHK(graft_scratch(n, scratch, &d_keep, N + 1)); CHK(graft_scratch(n, scratch, &d_pos, N + 1));
    HIPCHK(hipMemcpyAsync(d_ret, retired.data(), sizeof(int) * (size_t)op.C, hipMemcpyHostToDevice, n->stream));
    hipLaunchKernelGGL(k_retire_flags, dim3(grid_for(N + 1)), dim3(BLOCK), 0, n->stream, op, o->d_ref_cam, d_ret, o->d_lmk_u2i, d_keep);
    HIPCHK(hipGetLastError());
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
    if (F <= 0 || C <= 0 || L <= 0) return fail(GBP_EINVAL, "retiring these cameras leaves no factor");
    graft_settings(o, n, C, L, F);
    Params &p = n->p;

    // 2. the survivors' inputs, on the device
    Survivors s{};
    CHK(graft_scratch(n, scratch, &s.o2n, N)); CHK(graft_scratch(n, scratch, &s.f_n2o, (size_t)F));
    CHK(graft_scratch(n, scratch, &s.meas, (size_t)F * 2)); CHK(graft_scratch(n, scratch, &s.cam, (size_t)F)); CHK(graft_scratch(n, scratch, &s.lmk, (size_t)F));
    CHK(graft_scratch(n, scratch, &s.cam_means, (size_t)C * 6)); CHK(graft_scratch(n, scratch, &s.lmk_means, (size_t)L * 3));
    hipLaunchKernelGGL(k_retire_compact, dim3(grid_for(N)), dim3(BLOCK), 0, n->stream, op, o->d_ref_cam, o->d_ref_lmk, o->d_lmk_u2i, o->d_lmk_i2u, d_keep, d_pos, s);
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

    // 5. the state transplant, and the fold of the retired factors' messages into their landmarks' priors
    hipLaunchKernelGGL(k_retire_slots, dim3(grid_for(n_slots(n))), dim3(BLOCK), 0, n->stream, p, op, s.f_n2o);
    hipLaunchKernelGGL(k_retire_vars, dim3(grid_for((size_t)op.C + op.L)), dim3(BLOCK), 0, n->stream, p, op, s.o2n, n->d_lmk_u2i, o->d_lmk_u2i);
    hipLaunchKernelGGL(k_fold_retired, dim3(grid_for((size_t)op.L)), dim3(BLOCK), 0, n->stream, p, op, s.o2n + op.C, d_ret, n->d_lmk_u2i, o->d_lmk_u2i);
    HIPCHK(hipGetLastError());
    CHK(graft_counters(o, n));

    // 6. update_all_beliefs over the survivors
    CHK(gbp_ba_update_beliefs(n));
    maps.resize(N);
    HIPCHK(hipMemcpyAsync(maps.data(), s.o2n, sizeof(int) * N, hipMemcpyDeviceToHost, n->stream));
    HIPCHK(hipStreamSynchronize(n->stream));
    return GBP_OK;
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
        for (int i = 0; cam_old_to_new && i < op.C; ++i) cam_old_to_new[i] = i;
        for (int i = 0; lmk_old_to_new && i < op.L; ++i) lmk_old_to_new[i] = i;
        for (int i = 0; factor_old_to_new && i < op.F; ++i) factor_old_to_new[i] = i;
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
    for (void *q : scratch) (void)hipFreeAsync(q, h->stream);
    (void)hipStreamSynchronize(h->stream);
    if (rc != GBP_OK) return n ? graft_abandon(n, rc) : rc;
    const size_t C0 = (size_t)op.C, L0 = (size_t)op.L, F0 = (size_t)op.F;     // (op is the old graph's until the swap)
    if (cam_old_to_new) std::memcpy(cam_old_to_new, maps.data(), C0 * sizeof(int32_t));
    if (lmk_old_to_new) std::memcpy(lmk_old_to_new, maps.data() + C0, L0 * sizeof(int32_t));
    if (factor_old_to_new) std::memcpy(factor_old_to_new, maps.data() + C0 + L0, F0 * sizeof(int32_t));
    graft_swap(h, n);
    return GBP_OK;
}

}  // extern "C"
