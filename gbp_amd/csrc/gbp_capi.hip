// gbp_capi.hip -- libgbp_hip.so, life cycle: error strings, create / destroy (the graph build itself: gbp_capi_build.hip),
// streams, priors, the BAL reader, what the plan decided, layout checks.  The other translation units: gbp_handle.hpp.
//
// No CPU compute path lives in this library: every sweep, belief update and diagnostic is a HIP kernel, and so is the graph build
// (ordering, tile packing, slot assignment, initial linearisation points, prior maxima).  Host code only (a) sizes the allocations
// from the tile count the device reports, (b) packs / unpacks symmetric matrices for the views, (c) owns handles, streams and the
// optional RCCL communicator.
#include "gbp_handle.hpp"
#include "gbp_prior_kernels.hpp"
#include "gbp_balio.hpp"

#include <cmath>
#include <cstdarg>
#include <mutex>
#include <new>

static thread_local std::string g_err;

namespace gbp {
int set_error(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
}  // namespace gbp

extern "C" {


int gbp_abi_version(void) { return GBP_ABI_VERSION; }
const char *gbp_last_error(void) { return g_err.c_str(); }

void gbp_ba_destroy(gbp_ba_t *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void *ptr : h->allocs) (void)hipFree(ptr);
    if (h->d_tmp) (void)hipFree(h->d_tmp);
    for (void *q : h->snap) if (q) (void)hipFree(q);
    if (h->d_send) (void)hipFree(h->d_send);
    if (h->d_recv) (void)hipFree(h->d_recv);
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    if (h->copy_stream) { (void)hipStreamSynchronize(h->copy_stream); (void)hipStreamDestroy(h->copy_stream); }
    for (int i = 0; i < 2; ++i) { if (h->h_mu[i]) (void)hipHostFree(h->h_mu[i]); if (h->ev_landed[i]) (void)hipEventDestroy(h->ev_landed[i]); }
    if (h->ev_packed) (void)hipEventDestroy(h->ev_packed);
    shard_comm_release(h);
    peer_release(h);
    if (h->peer.mailbox) (void)hipFree(h->peer.mailbox);
    if (h->peer.d_ctl) (void)hipFree(h->peer.d_ctl);
    if (h->side_stream) (void)hipStreamDestroy(h->side_stream);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    fused_destroy(h->fused);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
}

static int create_impl(gbp_ba *h, const gbp_ba_desc_t *d)
{
    const int C = d->n_cams;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(GBP_ENODEV, "no HIP device visible: libgbp_hip.so has no CPU path");
    if (d->device < 0 || d->device >= ndev) return fail(GBP_EINVAL, "device %d out of range (%d visible)", d->device, ndev);
    h->device = d->device;
    HIPCHK(hipSetDevice(h->device));
    // hipGetDeviceProperties costs ~1 ms: asked once per device and process
    static std::mutex prop_mutex;
    static std::vector<std::pair<int, std::string>> prop_cache;       // [device] = {CU count, arch}
    int n_cus = 0;
    std::string arch;
    {
        std::lock_guard<std::mutex> lock(prop_mutex);
        if ((int)prop_cache.size() < ndev) prop_cache.resize(ndev, {0, std::string()});
        if (prop_cache[h->device].first == 0) {
            hipDeviceProp_t prop;
            HIPCHK(hipGetDeviceProperties(&prop, h->device));
            prop_cache[h->device] = {prop.multiProcessorCount, std::string(prop.gcnArchName)};
        }
        n_cus = prop_cache[h->device].first; arch = prop_cache[h->device].second;
    }
    if (strncmp(arch.c_str(), "gfx950", 6) != 0)
        return fail(GBP_ENODEV, "device %d is %s; this library is built for gfx950 (MI355X) only", h->device, arch.c_str());
    HIPCHK(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
    h->stream = h->own_stream;
    h->flags = d->flags;


    Params &p = h->p;
    p.F = d->n_factors; p.L = d->n_lmks; p.C = C; p.T = 0;
    p.K = Intrinsics{d->K[0], d->K[1], d->K[2], d->K[3]};
    p.sigma2 = d->gauss_noise_std * d->gauss_noise_std;
    p.nstds = d->nstds; p.beta = d->beta; p.eta_damping = d->eta_damping;
    p.num_undamped = d->num_undamped_iters; p.min_linear = d->min_linear_iters; p.loss = d->loss;
    p.robustify = 0; p.local_relin = 1;
    p.crow = d->num_undamped_iters == 0 ? CSTAGE_ROW : CSTAGE_PLAIN;      // (xtra rows carry the dense remainder too)
    if (d->num_undamped_iters > ITERS_MAX || d->min_linear_iters > ITERS_MAX)
        return fail(GBP_EINVAL, "num_undamped_iters / min_linear_iters above %d are not supported (iters_since_relin saturates there)", ITERS_MAX);
    if (C >= (1 << (32 - META_LMK_BITS))) return fail(GBP_EINVAL, "more than %d cameras are not supported", (1 << (32 - META_LMK_BITS)) - 1);

    h->n_cus = n_cus;
    std::vector<void *> scratch;                             // device buffers only the build needs
    const int rc = build_graph(h, d, scratch, n_cus);
    for (void *q : scratch) (void)hipFreeAsync(q, h->stream);
    (void)hipStreamSynchronize(h->stream);
    return rc;
}

int gbp_ba_create(gbp_ba_t **out, const gbp_ba_desc_t *d)
{
    if (!out || !d) return fail(GBP_EINVAL, "null argument");
    *out = nullptr;
    if (d->n_cams < 0 || d->n_lmks < 0 || d->n_factors < 0) return fail(GBP_EINVAL, "negative size");
    if (d->n_factors > 0 && (!d->meas || !d->cam_idx || !d->lmk_idx)) return fail(GBP_EINVAL, "null observation arrays");
    if ((d->n_cams > 0 && !d->cam_means) || (d->n_lmks > 0 && !d->lmk_means)) return fail(GBP_EINVAL, "null initial means");
    if (d->loss < GBP_LOSS_NONE || d->loss > GBP_LOSS_CONSTANT) return fail(GBP_EINVAL, "unknown loss %d", d->loss);
    if (!(d->gauss_noise_std > 0)) return fail(GBP_EINVAL, "gauss_noise_std must be positive");
    gbp_ba *h = new (std::nothrow) gbp_ba;
    if (!h) return fail(GBP_ENOMEM, "out of host memory");
    int rc;
    try {
        h->ovr = env_overrides();
        rc = create_impl(h, d);
    } catch (const std::bad_alloc &) {
        rc = fail(GBP_ENOMEM, "out of host memory");
    }
    if (rc != GBP_OK) { std::string keep = g_err; gbp_ba_destroy(h); g_err = keep; return rc; }
    *out = h;
    return GBP_OK;
}

int gbp_ba_set_stream(gbp_ba_t *h, void *hip_stream)
{
    ENTER(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    h->stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : h->own_stream;
    return GBP_OK;
}

// A finish wave of the peer-store exchange that gave up waiting for a peer's partial sums leaves a mark; everything that hands results
// to the caller (sync, beliefs, means, are / energy, checkpoints) looks at it first, so a timed-out sweep cannot pass for a result.
// The mark stays until gbp_ba_sync has reported it.
}  // extern "C"
int gbp::peer_check(gbp_ba *h, bool clear)
{
    if (!h->peer.connected || !h->peer.d_ctl) return GBP_OK;
    HIPCHK(hipStreamSynchronize(h->stream));
    int err = 0;
    HIPCHK(hipMemcpy(&err, h->peer.d_ctl + 1, sizeof(int), hipMemcpyDeviceToHost));
    if (!err) return GBP_OK;
    if (clear) HIPCHK(hipMemset(h->peer.d_ctl + 1, 0, sizeof(int)));
    return fail(GBP_ESTATE, "peer-store exchange timed out: a rank's camera partial sums did not arrive (the camera beliefs since then are invalid)");
}

extern "C" {
int gbp_ba_sync(gbp_ba_t *h)
{
    ENTER(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    return peer_check(h, true);
}

// ------------------------------------------------------------------------------- priors ---

int gbp_ba_factor_lambda_max(gbp_ba_t *h, double *cam_max, double *lmk_max)
{
    ENTER(h);
    const Params &p = h->p;
    CHK(variable_lambda_max(h));
    if (cam_max && p.C) HIPCHK(hipMemcpyAsync(cam_max, h->d_varmax, sizeof(double) * (size_t)p.C, hipMemcpyDeviceToHost, h->stream));
    if (lmk_max && p.L && h->lmk_u2i.empty()) HIPCHK(hipMemcpyAsync(lmk_max, h->d_varmax + p.C, sizeof(double) * (size_t)p.L, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (lmk_max && p.L && !h->lmk_u2i.empty()) {           // d_varmax is in internal numbering
        std::vector<double> m;
        CHK(download(h, m, h->d_varmax + p.C, (size_t)p.L));
        for (int l = 0; l < p.L; ++l) lmk_max[l] = m[(size_t)h->lmk_u2i[(size_t)l]];
    }
    return GBP_OK;
}

int gbp_ba_set_prior_scalars(gbp_ba_t *h, const double *cam_lambda, const double *lmk_lambda)
{
    ENTER(h);
    h->resid_ok = false;
    const Params &p = h->p;
    if (!cam_lambda || !lmk_lambda) return fail(GBP_EINVAL, "null argument");
    if (p.C) HIPCHK(hipMemcpyAsync(h->d_varmax, cam_lambda, sizeof(double) * (size_t)p.C, hipMemcpyHostToDevice, h->stream));
    if (p.L) HIPCHK(hipMemcpyAsync(h->d_varmax + p.C, lmk_lambda, sizeof(double) * (size_t)p.L, hipMemcpyHostToDevice, h->stream));
    if (p.C + p.L) hipLaunchKernelGGL(k_prior_scalars, dim3(grid_for((size_t)p.C + p.L)), dim3(BLOCK), 0, h->stream, p, h->d_varmax, h->d_varmax + p.C, 1.0,
                                      0, p.C, 0, p.L, h->d_lmk_u2i, 1);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));               // the arrays are the caller's
    return GBP_OK;
}

int gbp_ba_generate_priors(gbp_ba_t *h, double weaker_factor)
{
    ENTER(h);
    h->resid_ok = false;
    if (!(weaker_factor != 0.0)) return fail(GBP_EINVAL, "weaker_factor must be non-zero");
    const Params &p = h->p;
    CHK(variable_lambda_max(h));                           // nothing F-sized leaves the device
    if (p.C + p.L) hipLaunchKernelGGL(k_prior_scalars, dim3(grid_for((size_t)p.C + p.L)), dim3(BLOCK), 0, h->stream, p, h->d_varmax,
                                      h->d_varmax + p.C, weaker_factor * weaker_factor, 0, p.C, 0, p.L, h->d_lmk_u2i, 0);
    HIPCHK(hipGetLastError());
    return GBP_OK;
}

int gbp_ba_set_priors(gbp_ba_t *h, const double *cam_eta, const double *cam_lam, const double *lmk_eta, const double *lmk_lam)
{
    ENTER(h);
    h->resid_ok = false;
    const Params &p = h->p;
    if (!cam_eta || !cam_lam || !lmk_eta || !lmk_lam) return fail(GBP_EINVAL, "null argument");
    std::vector<double> cp((size_t)std::max(p.C, 1) * 27, 0.0), lp((size_t)std::max(p.L, 1) * 9, 0.0);
    for (int c = 0; c < p.C; ++c) {
        for (int k = 0; k < 6; ++k) cp[(size_t)c * 27 + k] = cam_eta[(size_t)c * 6 + k];
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j)
                cp[(size_t)c * 27 + 6 + Sym<6>::at(i, j)] = 0.5 * (cam_lam[(size_t)c * 36 + i * 6 + j] + cam_lam[(size_t)c * 36 + j * 6 + i]);
    }
    for (int l = 0; l < p.L; ++l) {
        for (int k = 0; k < 3; ++k) lp[(size_t)l * 9 + k] = lmk_eta[(size_t)l * 3 + k];
        for (int i = 0; i < 3; ++i)
            for (int j = i; j < 3; ++j)
                lp[(size_t)l * 9 + 3 + Sym<3>::at(i, j)] = 0.5 * (lmk_lam[(size_t)l * 9 + i * 3 + j] + lmk_lam[(size_t)l * 9 + j * 3 + i]);
    }
    CHK(upload(h, p.cprior, cp));
    CHK(ensure_tmp(h, sizeof(double) * lp.size()));
    CHK(upload(h, h->d_tmp, lp));
    if (p.L) hipLaunchKernelGGL(k_scatter_lmk_priors, dim3(grid_for((size_t)p.L * 9)), dim3(BLOCK), 0, h->stream, p, h->d_tmp, h->d_lmk_u2i);
    HIPCHK(hipGetLastError());
    return GBP_OK;
}

int gbp_ba_weaken_priors(gbp_ba_t *h, double factor)
{
    ENTER(h);
    h->resid_ok = false;
    const Params &p = h->p;
    const size_t n = (size_t)p.C * 27 + (size_t)p.L * 9;
    if (n) hipLaunchKernelGGL(k_weaken_priors, dim3(grid_for(n)), dim3(BLOCK), 0, h->stream, p, factor);
    HIPCHK(hipGetLastError());
    return GBP_OK;
}

// ------------------------------------------------------------------------------ BAL files ---
// utils/read_balfile.py:4-37 (called from create_ba_graph gbp_ba.py:108-109); host only.

int gbp_bal_header(const char *path, int32_t *n_cams, int32_t *n_lmks, int32_t *n_obs)
{
    if (!path || !n_cams || !n_lmks || !n_obs) return fail(GBP_EINVAL, "NULL argument");
    BalText t;
    std::string err;
    long C, L, F;
    if (t.open(path, err) || bal_header(t, C, L, F, err)) return fail(GBP_EINVAL, "%s: %s", path, err.c_str());
    if (C > INT32_MAX || L > INT32_MAX || F > INT32_MAX) return fail(GBP_EINVAL, "%s: sizes exceed int32", path);
    *n_cams = (int32_t)C; *n_lmks = (int32_t)L; *n_obs = (int32_t)F;
    return GBP_OK;
}

int gbp_bal_read(const char *path, int32_t n_cams, int32_t n_lmks, int32_t n_obs, double *K4, double *cam_means,
                 double *lmk_means, double *meas, int32_t *cam_idx, int32_t *lmk_idx)
{
    if (!path || !K4 || !cam_means || !lmk_means || !meas || !cam_idx || !lmk_idx) return fail(GBP_EINVAL, "NULL argument");
    BalText t;
    std::string err;
    long C, L, F;
    if (t.open(path, err) || bal_header(t, C, L, F, err)) return fail(GBP_EINVAL, "%s: %s", path, err.c_str());
    if (C != n_cams || L != n_lmks || F != n_obs) return fail(GBP_EINVAL, "%s: sizes differ from gbp_bal_header's", path);
    if (bal_body(t, C, L, F, K4, cam_means, lmk_means, meas, cam_idx, lmk_idx, err)) return fail(GBP_EINVAL, "%s: %s", path, err.c_str());
    return GBP_OK;
}

int gbp_ba_check_layout(gbp_ba_t *h, int32_t *bad_slots)
{
    ENTER(h);
    if (!bad_slots) return fail(GBP_EINVAL, "null argument");
    *bad_slots = 0;
    if (!h->p.T) return GBP_OK;
    HIPCHK(hipMemsetAsync(h->d_count, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_check_layout, dim3(grid_for(n_slots(h))), dim3(BLOCK), 0, h->stream, h->p, h->d_ref_cam, h->d_ref_lmk, h->d_count);
    HIPCHK(hipGetLastError());
    int v = 0;
    HIPCHK(hipMemcpyAsync(&v, h->d_count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    *bad_slots = v;
    return GBP_OK;
}

int gbp_ba_get_lmk_order(gbp_ba_t *h, int32_t *internal_of_user)
{
    if (!h || (h->p.L > 0 && !internal_of_user)) return fail(GBP_EINVAL, "null argument");
    for (int l = 0; l < h->p.L; ++l) internal_of_user[l] = h->lmk_u2i.empty() ? l : h->lmk_u2i[(size_t)l];
    return (h->flags & GBP_FLAG_REORDER_LMKS) ? 1 : 0;
}

int gbp_ba_rebuild_count(gbp_ba_t *h, int64_t *count)
{
    if (!h || !count) return fail(GBP_EINVAL, "null argument");
    *count = (int64_t)h->rebuilds;
    return GBP_OK;
}

int gbp_ba_fused_max_cams(void)
{
    return fused_max_cams();
}

int gbp_ba_plan_info(gbp_ba_t *h, int32_t *out, int32_t n)
{
    if (!h || (n > 0 && !out)) return fail(GBP_EINVAL, "null argument");
    const bool pinned = h->fused.enabled && h->fused.args.pin != 0x7fffffff;
    const int32_t v[GBP_PLAN_INFO_FIELDS] = {
        h->fused.enabled ? 1 : 0, h->staged_auto ? 1 : 0, h->fused.enabled ? h->fused.single : 0, h->fused.single_probe,
        pinned ? h->fused.args.pin : -1, h->fused.enabled ? h->fused.n_blocks : std::max(1, std::min(h->p.T, h->n_cus)), h->p.T,
        h->pack_mode, h->fused.enabled && h->fused.windowed ? h->fused.max_window : 0,
        h->fused.enabled ? (int32_t)std::min<long long>(h->fused.windowed ? h->fused.table_rows : (long long)h->fused.n_blocks * h->p.C, INT32_MAX) : 0,
        h->fused.enabled && h->fused.windowed ? h->fused.rows_wave : 0};
    for (int i = 0; i < n && i < GBP_PLAN_INFO_FIELDS; ++i) out[i] = v[i];
    return GBP_OK;
}

int gbp_ba_info(gbp_ba_t *h, int32_t *fused_path, int32_t *n_tiles, int32_t *n_blocks)
{
    if (!h) return fail(GBP_EINVAL, "null handle");
    if (fused_path) *fused_path = h->fused.enabled ? 1 : 0;
    if (n_tiles) *n_tiles = h->p.T;
    if (n_blocks) *n_blocks = h->fused.n_blocks;
    return GBP_OK;
}


}  // extern "C"

// max over the adjacent factors of every variable of max(Lambda_f) (gbp_ba.py:27-31) into d_varmax = cameras | landmarks
int gbp::variable_lambda_max(gbp_ba *h)
{
    const Params &p = h->p;
    const size_t S = n_slots(h);
    CHK(ensure_tmp(h, sizeof(double) * S));
    if (p.T) hipLaunchKernelGGL(k_factor_lambda_max, dim3(grid_for(S)), dim3(BLOCK), 0, h->stream, p, h->d_tmp);
    if (p.C) hipLaunchKernelGGL(k_cam_max, dim3(p.C), dim3(BLOCK), 0, h->stream, p, h->d_tmp, h->d_varmax);
    if (p.L) hipLaunchKernelGGL(k_lmk_max, dim3(grid_for((size_t)p.L)), dim3(BLOCK), 0, h->stream, p, h->d_tmp, h->d_varmax + p.C);
    HIPCHK(hipGetLastError());
    return GBP_OK;
}

// prior Lambda = (lambda / w2) I, eta = Lambda mu on cameras [c0, C) and landmarks [l0, L) (the caller's ids) only, lambda from d_varmax
// (gbp_ba_extend: the NEW variables; w2 = weaker_factor^2 for the rule, 1 for given scalars).  The landmark half of d_varmax is indexed
// by the caller's id when it came from outside (lmk_lambda_by_user), by the internal one when variable_lambda_max wrote it.
int gbp::prior_scalars_range(gbp_ba *h, int c0, int l0, double w2_cam, double w2_lmk, bool lmk_lambda_by_user)
{
    const Params &p = h->p;
    if (p.C > c0) hipLaunchKernelGGL(k_prior_scalars, dim3(grid_for((size_t)p.C)), dim3(BLOCK), 0, h->stream, p, h->d_varmax, h->d_varmax + p.C, w2_cam,
                                     c0, p.C, p.L, p.L, nullptr, 0);
    if (p.L > l0) hipLaunchKernelGGL(k_prior_scalars, dim3(grid_for((size_t)p.C + p.L)), dim3(BLOCK), 0, h->stream, p, h->d_varmax, h->d_varmax + p.C,
                                     w2_lmk, p.C, p.C, l0, p.L, h->d_lmk_u2i, lmk_lambda_by_user ? 1 : 0);
    HIPCHK(hipGetLastError());
    return GBP_OK;
}

// digest of the layout: a state blob restores only into a handle of the same graph
int gbp::graph_hash(gbp_ba *h, uint64_t *out)
{
    if (!h->hash_ok) {
        unsigned long long *d = reinterpret_cast<unsigned long long *>(h->d_count);      // 8 bytes
        HIPCHK(hipMemsetAsync(d, 0, sizeof(unsigned long long), h->stream));
        if (h->p.F) hipLaunchKernelGGL(k_graph_hash, dim3(grid_for((size_t)h->p.F)), dim3(BLOCK), 0, h->stream, h->p.cadj, h->d_ref_cam,
                                       h->d_ref_lmk, h->p.F, d);
        HIPCHK(hipGetLastError());
        unsigned long long v = 0;
        HIPCHK(hipMemcpyAsync(&v, d, sizeof v, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->flags & GBP_FLAG_REORDER_LMKS) v ^= 0x4c4d4b4f52444552ull;      // a reordered handle's blob holds its records in its own order
        h->hash = v; h->hash_ok = true;
    }
    *out = h->hash;
    return GBP_OK;
}
