// gbp_capi_extend.hip -- libgbp_hip.so, growth of a live handle (gbp_ba_extend, include/gbp_ba.h): the reference appends variable
// and factor objects to Python lists and every piece of solver state survives (gbp_ba.py:114-141); here the union graph is BUILT
// beside the handle by the create path (gbp::build_graph, from arrays assembled on the device), the old factors' and variables' state
// is transplanted into the union's layout, and the union is swapped in only when everything has succeeded.
//
// The union's "file order" is the old factors in the old reference order followed by the batch: create's stable camera-major sort then
// gives exactly the reference's union order (old factors before new ones inside a camera), the new factors are linearised at the right
// points for free (old variables contribute their current means), and the build's ref_file map tells which union factor was which old
// one (file index < F_old: old reference id = file index).
#include "gbp_graft.hpp"

namespace {

// the union's factor arrays in file order: the old factors in reference order (measurement = the z rows of their slot), then the batch.
// Landmark ids go out in the caller's numbering: o_i2u (NULL: identity) turns a reordered handle's internal ids back.
__global__ __launch_bounds__(BLOCK) void k_union_factors(Params o, const int *__restrict__ ref_cam, const int *__restrict__ ref_lmk, const int *__restrict__ o_i2u,
                                                         const double *__restrict__ bmeas, const int *__restrict__ bcam, const int *__restrict__ blmk,
                                                         int n_new, double *__restrict__ meas, int *__restrict__ cam, int *__restrict__ lmk)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i < o.F) {
        const int s = o.cadj[i];
        meas[(size_t)i * 2] = o.lin[lin_at(s, ROW_Z)];
        meas[(size_t)i * 2 + 1] = o.lin[lin_at(s, ROW_Z + 1)];
        cam[i] = ref_cam[i];
        lmk[i] = o_i2u ? o_i2u[ref_lmk[i]] : ref_lmk[i];
    } else if (i < o.F + n_new) {
        const int j = i - o.F;
        meas[(size_t)i * 2] = bmeas[(size_t)j * 2];
        meas[(size_t)i * 2 + 1] = bmeas[(size_t)j * 2 + 1];
        cam[i] = bcam[j];
        lmk[i] = blmk[j];
    }
}

// the union's initial means: the old variables' current belief means (node.mu), then the batch's (o_u2i: caller's landmark id -> the old
// handle's record, NULL: identity)
__global__ __launch_bounds__(BLOCK) void k_union_means(Params o, const int *__restrict__ o_u2i, const double *__restrict__ bcam, const double *__restrict__ blmk, int dC, int dL,
                                                       double *__restrict__ cam_means, double *__restrict__ lmk_means)
{
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t nc = (size_t)(o.C + dC) * 6, nl = (size_t)(o.L + dL) * 3;
    if (i < nc) {
        const size_t c = i / 6, k = i % 6;
        cam_means[i] = c < (size_t)o.C ? o.cbel[c * CAMREC + CAM_MU + k] : bcam[i - (size_t)o.C * 6];
    } else if (i < nc + nl) {
        const size_t j = i - nc, l = j / 3, k = j % 3;
        lmk_means[j] = l < (size_t)o.L ? o.lrec[(o_u2i ? (size_t)o_u2i[l] : l) * LREC + LR_MU + k] : blmk[j - (size_t)o.L * 3];
    }
}

// One lane per slot of the union: an old factor's whole state moves from its old slot (gathered) to its new one (written as the
// tile-contiguous row pairs of gbp_kernels.hpp: 16 contiguous bytes per lane and pair, 1 KB per wave and pair).  The meta word and the
// rank field of the state word are the new layout's (k_build_tiles wrote them); everything else is the old factor's: linearisation point,
// measurement, clock stamp, pending / robust / damped bits, messages, adaptive variance, dense remainder.  New factors keep what the build
// gave them (create's initialisation: iters_since_relin = 1 at the handle's clock, zero messages, sigma^2).
__global__ __launch_bounds__(BLOCK) void k_transplant_slots(Params n, Params o, const int *__restrict__ ref_file, int *__restrict__ old_to_new)
{
    const int slot = blockIdx.x * BLOCK + threadIdx.x;
    if (slot >= n.T * WTILE || (slot & 63) >= n.tiles[slot >> 6].z) return;
    const int r = n.cpos[slot];
    const int f = ref_file ? ref_file[r] : r;
    if (f >= o.F) return;
    const int os = o.cadj[f];
    old_to_new[f] = r;
    transplant_slot(n, o, slot, os);
}

// per-variable state of the old variables: camera records, belief views and priors; landmark mean | covariance and prior (the slot range
// of a landmark record is the new layout's).  A landmark keeps its id in the caller's numbering; on a reordered handle its record moves
// old internal -> caller's -> new internal (o_u2i, n_u2i; NULL: identity).
__global__ __launch_bounds__(BLOCK) void k_transplant_vars(Params n, Params o, const int *__restrict__ n_u2i, const int *__restrict__ o_u2i)
{
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v < o.C) transplant_cam(n, o, v, v);
    else if (v < o.C + o.L) { const int u = v - o.C; transplant_lmk(n, o, n_u2i ? n_u2i[u] : u, o_u2i ? o_u2i[u] : u); }
}

// the union built beside the old handle `o` into the fresh handle `n` (which owns nothing of o's)
int extend_into(gbp_ba *o, gbp_ba *n, const gbp_ba_ext_t *e, std::vector<void *> &scratch, std::vector<int> &old_to_new)
{
    const Params &op = o->p;
    const int dC = e->n_new_cams, dL = e->n_new_lmks, dF = e->n_new_factors;
    const int C = op.C + dC, L = op.L + dL, F = op.F + dF;
    const bool dev_in = (e->flags & GBP_FLAG_DEVICE_INPUT) != 0;
    graft_settings(o, n, C, L, F);
    Params &p = n->p;

    // 1. the union's inputs, on the device
    const double *bcm = nullptr, *blm = nullptr, *bmeas = nullptr;
    const int *bcam = nullptr, *blmk = nullptr;
    CHK(stage_input(n, e->cam_means, (size_t)dC * 6, dev_in, scratch, &bcm)); CHK(stage_input(n, e->lmk_means, (size_t)dL * 3, dev_in, scratch, &blm));
    CHK(stage_input(n, e->meas, (size_t)dF * 2, dev_in, scratch, &bmeas));
    CHK(stage_input(n, e->cam_idx, (size_t)dF, dev_in, scratch, &bcam)); CHK(stage_input(n, e->lmk_idx, (size_t)dF, dev_in, scratch, &blmk));
    double *u_meas = nullptr, *u_cm = nullptr, *u_lm = nullptr;
    int *u_cam = nullptr, *u_lmk = nullptr;
    CHK(scratch_alloc(n, scratch, &u_meas, (size_t)F * 2)); CHK(scratch_alloc(n, scratch, &u_cam, (size_t)F)); CHK(scratch_alloc(n, scratch, &u_lmk, (size_t)F));
    CHK(scratch_alloc(n, scratch, &u_cm, (size_t)C * 6)); CHK(scratch_alloc(n, scratch, &u_lm, (size_t)L * 3));
    if (F) hipLaunchKernelGGL(k_union_factors, dim3(grid_for((size_t)F)), dim3(BLOCK), 0, n->stream, op, o->d_ref_cam, o->d_ref_lmk, o->d_lmk_i2u, bmeas, bcam, blmk, dF,
                              u_meas, u_cam, u_lmk);
    const size_t nv = (size_t)C * 6 + (size_t)L * 3;
    if (nv) hipLaunchKernelGGL(k_union_means, dim3(grid_for(nv)), dim3(BLOCK), 0, n->stream, op, o->d_lmk_u2i, bcm, blm, dC, dL, u_cm, u_lm);
    HIPCHK(hipGetLastError());

    // 2. the union's graph by the create path (ids are checked there: out of range -> GBP_EINVAL)
    gbp_ba_desc_t d{};
    d.n_cams = C; d.n_lmks = L; d.n_factors = F; d.device = o->device;
    d.cam_means = u_cm; d.lmk_means = u_lm; d.meas = u_meas; d.cam_idx = u_cam; d.lmk_idx = u_lmk;
    d.flags = GBP_FLAG_DEVICE_INPUT;                           // (the sweep flags are n->flags)
    const int *ref_file = nullptr;
    CHK(build_graph(n, &d, scratch, n->n_cus, &ref_file));

    // 3. a remainder switched on on demand stays on (the fresh handle allocates it exactly as the old one did)
    if (o->lazy_xtra && op.xtra) CHK(enable_remainder(n));

    // 4. the state transplant
    int *d_o2n = nullptr;
    CHK(scratch_alloc(n, scratch, &d_o2n, (size_t)op.F));
    const size_t S = n_slots(n);
    if (p.T && op.F) hipLaunchKernelGGL(k_transplant_slots, dim3(grid_for(S)), dim3(BLOCK), 0, n->stream, p, op, ref_file, d_o2n);
    if (op.C + op.L) hipLaunchKernelGGL(k_transplant_vars, dim3(grid_for((size_t)op.C + op.L)), dim3(BLOCK), 0, n->stream, p, op, n->d_lmk_u2i, o->d_lmk_u2i);
    HIPCHK(hipGetLastError());
    CHK(graft_counters(o, n));

    // 5. priors of the new variables: the rule over their factors (all of them new), or the given scalars
    const double wf = e->prior_weaker_factor;
    const bool rule = wf > 0.0;
    if (rule && ((dC && !e->cam_prior_lambda) || (dL && !e->lmk_prior_lambda))) CHK(variable_lambda_max(n));
    if (!rule) {
        if (dC && !e->cam_prior_lambda) HIPCHK(hipMemsetAsync(n->d_varmax + op.C, 0, sizeof(double) * (size_t)dC, n->stream));
        if (dL && !e->lmk_prior_lambda) HIPCHK(hipMemsetAsync(n->d_varmax + C + op.L, 0, sizeof(double) * (size_t)dL, n->stream));
    }
    if (dC && e->cam_prior_lambda)
        HIPCHK(hipMemcpyAsync(n->d_varmax + op.C, e->cam_prior_lambda, sizeof(double) * (size_t)dC, hipMemcpyHostToDevice, n->stream));
    if (dL && e->lmk_prior_lambda)
        HIPCHK(hipMemcpyAsync(n->d_varmax + C + op.L, e->lmk_prior_lambda, sizeof(double) * (size_t)dL, hipMemcpyHostToDevice, n->stream));
    CHK(prior_scalars_range(n, op.C, op.L, e->cam_prior_lambda || !rule ? 1.0 : wf * wf, e->lmk_prior_lambda || !rule ? 1.0 : wf * wf,
                            e->lmk_prior_lambda || !rule));

    // 6. update_all_beliefs over the union
    CHK(gbp_ba_update_beliefs(n));
    old_to_new.resize((size_t)op.F);
    if (op.F) HIPCHK(hipMemcpyAsync(old_to_new.data(), d_o2n, sizeof(int) * (size_t)op.F, hipMemcpyDeviceToHost, n->stream));
    HIPCHK(hipStreamSynchronize(n->stream));
    return GBP_OK;
}

}  // namespace

extern "C" {

int gbp_ba_extend(gbp_ba_t *h, const gbp_ba_ext_t *e, int32_t *old_to_new)
{
    ENTER(h);
    if (!e) return fail(GBP_EINVAL, "null argument");
    CHK(live_and_whole(h, "grow"));
    CHK(sound_batch(h->p, e));
    const Params &op = h->p;
    const int dC = e->n_new_cams, dL = e->n_new_lmks, dF = e->n_new_factors;
    if (!(e->flags & GBP_FLAG_DEVICE_INPUT)) {            // host ids: checked here, before anything is allocated
        for (int i = 0; i < dF; ++i)
            if (e->cam_idx[i] < 0 || e->cam_idx[i] >= op.C + dC || e->lmk_idx[i] < 0 || e->lmk_idx[i] >= op.L + dL)
                return fail(GBP_EINVAL, "new observation %d references a camera outside [0,%d) or a landmark outside [0,%d)", i, op.C + dC, op.L + dL);
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    gbp_ba *n = new (std::nothrow) gbp_ba;
    if (!n) return fail(GBP_ENOMEM, "out of host memory");
    std::vector<void *> scratch;
    std::vector<int> o2n;
    int rc;
    try {
        rc = extend_into(h, n, e, scratch, o2n);
    } catch (const std::bad_alloc &) {
        rc = fail(GBP_ENOMEM, "out of host memory");
    }
    for (void *q : scratch) (void)hipFreeAsync(q, h->stream);
    (void)hipStreamSynchronize(h->stream);
    if (rc != GBP_OK) return graft_abandon(n, rc);
    graft_swap(h, n);
    if (old_to_new && !o2n.empty()) std::memcpy(old_to_new, o2n.data(), o2n.size() * sizeof(int32_t));
    return GBP_OK;
}

}  // extern "C"
