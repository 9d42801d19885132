// gbp_capi_sweep.hip -- libgbp_hip.so, every launch of a sweep: the fused sweep and its plan (gbp_fused.hpp), the general sweep and the
// stage-wise calls (gbp_sweep_kernels.hpp), the dense message remainder on demand, the camera finish, diagnostics (ARE / energy) and the
// kernel-time instrumentation.  The kernels are instantiated HERE and nowhere else (gbp_handle.hpp).
#include "gbp_handle.hpp"
#include "gbp_sweep_kernels.hpp"
#include "gbp_fused.hpp"

#include <chrono>
#include <cmath>
#include <thread>

int gbp::plan_fused_sweep(gbp_ba *h, int n_cus) { return fused_plan(h->fused, h->p, h->stream, n_cus, h->ovr, h->wg_win.data(), h->wg_cams.data(), (int)h->wg_win.size()); }
int gbp::fused_max_cams_of_this_build() { return fused_max_cams(); }

// ------------------------------------------------------------------------------ launches --

// HIP events around the dominant kernel of every timing_every-th sweep while gbp_ba_set_kernel_timing is on (pairs in h->ev)
template <typename Launch>
static int timed(gbp_ba *h, Launch &&launch)
{
    const bool now = h->timing && (h->timing_tick++ % h->timing_every) == 0;
    if (now) {
        if (h->ev_used + 2 > h->ev.size())
            for (int i = 0; i < 2; ++i) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); h->ev.push_back(e); }
        HIPCHK(hipEventRecord(h->ev[h->ev_used], h->stream));
    }
    const int rc = launch();
    if (now) {
        HIPCHK(hipEventRecord(h->ev[h->ev_used + 1], h->stream));
        h->ev_used += 2;
    }
    return rc;
}

// this sweep's slot of the relinearisation-count ring; half of the ring is cleared whenever the sweep index enters it
static int relin_slot_advance(gbp_ba *h)
{
    const int slot = (int)(h->sweep_count % RELIN_RING);
    if (slot % (RELIN_RING / 2) == 0)
        HIPCHK(hipMemsetAsync(h->d_relin_ring + (size_t)slot * RELIN_LANES, 0, sizeof(int) * (RELIN_RING / 2) * RELIN_LANES, h->stream));
    h->p.relin_slot = h->d_relin_ring + (size_t)slot * RELIN_LANES;
    h->sweep_count++;
    return GBP_OK;
}

// the kernel templates' instantiations by loss (GBP_LOSS_*: None, Huber, else Constant) and by the staged reduce's block (cam_block)
static int loss_class(int loss) { return loss == GBP_LOSS_NONE ? 0 : loss == GBP_LOSS_HUBER ? 1 : 2; }
using FactorTileKernel = void (*)(Params);
static constexpr FactorTileKernel FACTOR_TILE[2][3] = {{k_factor_tile<0, true>, k_factor_tile<1, true>, k_factor_tile<2, true>},       // [0: with the dense remainder]
                                                       {k_factor_tile<0, false>, k_factor_tile<1, false>, k_factor_tile<2, false>}};
static_assert(BLOCK == 256, "cam_block's widest choice is the BLOCK variant");
static int cam_class(int cam_block) { return cam_block == 64 ? 0 : cam_block == 128 ? 1 : 2; }
static constexpr int CAM_THREADS[3] = {64, 128, BLOCK};
using CamXchgKernel = void (*)(Params, double *, PeerOut, PeerWait);
using CamPartialKernel = void (*)(Params, double *, int);
static constexpr CamXchgKernel CAM_STAGED_XCHG[3] = {k_cam_staged_xchg<64>, k_cam_staged_xchg<128>, k_cam_staged_xchg<BLOCK>};
static constexpr CamPartialKernel CAM_PARTIAL_STAGED[3] = {k_cam_partial_staged<64>, k_cam_partial_staged<128>, k_cam_partial_staged<BLOCK>};

static Params params_for(const gbp_ba *h, const SweepStep &s)
{
    Params p = h->p;
    p.robustify = s.robustify; p.local_relin = s.local_relin;
    return p;
}

static int launch_factor_stage(gbp_ba *h, const SweepStep &s)
{
    const Params p = params_for(h, s);
    if (!p.T) return GBP_OK;
    const int nb = (p.T + BLOCK / 64 - 1) / (BLOCK / 64);
    h->cstage_x0_ok = false;                                // (this kernel's rows may be the wide ones: the next staged sweep writes whole rows)
    CHK(timed(h, [&] { hipLaunchKernelGGL(FACTOR_TILE[p.xtra ? 0 : 1][loss_class(p.loss)], dim3(nb), dim3(BLOCK), 0, h->stream, p); return GBP_OK; }));
    HIPCHK(hipGetLastError());
    return GBP_OK;
}

static int launch_lmk_beliefs(gbp_ba *h)
{
    if (!h->p.L) return GBP_OK;
    hipLaunchKernelGGL(k_lmk_belief, dim3(grid_for(h->p.L)), dim3(BLOCK), 0, h->stream, h->p);
    HIPCHK(hipGetLastError());
    return GBP_OK;
}

static int launch_cam_partial(gbp_ba *h, double *partial)
{
    if (!h->p.C) return GBP_OK;
    hipLaunchKernelGGL(k_cam_partial, dim3(h->p.C), dim3(BLOCK), 0, h->stream, h->p, partial);
    HIPCHK(hipGetLastError());
    return GBP_OK;
}

int gbp::launch_cam_finish(gbp_ba *h, const double *gathered, int n_parts, size_t stride, const PeerWait *wait)
{
    if (!h->p.C) return GBP_OK;
    PeerWait w{};
    if (wait) w = *wait;
    w.clk = h->clk_cur ? h->clk_cur + 4 : nullptr;
    hipLaunchKernelGGL(k_cam_finish, dim3((h->p.C + FINISH_BLOCK / 64 - 1) / (FINISH_BLOCK / 64)), dim3(FINISH_BLOCK), 0, h->stream, h->p, gathered,
                       n_parts, stride, w);
    HIPCHK(hipGetLastError());
    return GBP_OK;
}

// camera-major staging of the general sweep, allocated on first use (F x 27 doubles; the slot -> row map cpos is made by the build)
static int ensure_staging(gbp_ba *h)
{
    if (!h->p.cstage || h->cstage_cap < h->p.crow) {
        CHK(dev_alloc(h, &h->p.cstage, std::max<size_t>((size_t)h->p.F, 1) * h->p.crow));
        h->cstage_cap = h->p.crow;
        h->cstage_x0_ok = false;
    }
    return GBP_OK;
}

int gbp::launch_finish_parts(gbp_ba *h, hipStream_t stream)
{
    if (!h->p.parts || !h->p.T) return GBP_OK;
    hipLaunchKernelGGL(k_lmk_finish_parts, dim3(grid_for((size_t)h->p.T)), dim3(BLOCK), 0, stream, h->p);
    HIPCHK(hipGetLastError());
    return GBP_OK;
}

// general sweep / update_all_beliefs under the peer-store exchange: the finished partial sums go into every rank's mailbox
static int launch_peer_push(gbp_ba *h, const double *partial, const PeerOut &peer)
{
    if (!h->p.C) return GBP_OK;
    hipLaunchKernelGGL(k_peer_push, dim3((h->p.C + BLOCK / 64 - 1) / (BLOCK / 64)), dim3(BLOCK), 0, h->stream, partial, h->p.C, peer);
    HIPCHK(hipGetLastError());
    return GBP_OK;
}

// the general sweep's factor kernel: messages + the tiles' landmark beliefs + camera messages staged camera-major
static int launch_general_sweep(gbp_ba *h, const SweepStep &s, const SweepLaunch &at)
{
    h->p.reverse_walk = at.reverse;
    CHK(ensure_staging(h));
    if (h->p.xtra) return launch_factor_stage(h, s);        // the dense remainder rides in k_factor_tile (one wave per tile)
    const Params p = params_for(h, s);                       // the persistent loop, staging instead of a camera table
    const int rc = timed(h, [&] { return staged_launch(p, at, h->cstage_x0_ok ? 0 : 1, &h->staged_attr_set); });
    h->cstage_x0_ok = true;
    if (rc > 0) return fail(GBP_EHIP, "general sweep launch failed: %s", hipGetErrorString((hipError_t)rc));
    return rc;
}

// the camera messages a general sweep staged camera-major -> the camera sums, left where c.sink says
static int staged_cameras(gbp_ba *h, const SweepCall &c, const SweepLaunch &at)
{
    if (!h->p.C) return GBP_OK;
    const int cls = cam_class(gbp::cam_block(h->p.F, h->p.C, h->ovr));
    const dim3 block(CAM_THREADS[cls]);
    if (c.sink == CamSink::PeerMerged) {                    // sum -> push -> wait -> finish in this one launch (peer-store exchange)
        const int xb = resident_blocks(&h->staged_xchg_blocks[cls], reinterpret_cast<const void *>(CAM_STAGED_XCHG[cls]), CAM_THREADS[cls], INT32_MAX, at);
        if (!xb) return fail(GBP_EHIP, "occupancy query of the staged exchange kernel failed");
        PeerWait w = *c.wait;
        w.clk = h->clk_cur ? h->clk_cur + 2 : nullptr;
        hipLaunchKernelGGL(CAM_STAGED_XCHG[cls], dim3(std::min(h->p.C, xb)), block, 0, h->stream, h->p, c.partial, *c.peer, w);
        HIPCHK(hipGetLastError());
        return GBP_OK;
    }
    hipLaunchKernelGGL(CAM_PARTIAL_STAGED[cls], dim3(h->p.C), block, 0, h->stream, h->p, c.partial, c.sink == CamSink::Finish ? 1 : 0);
    HIPCHK(hipGetLastError());
    return c.sink == CamSink::PeerPush ? launch_peer_push(h, c.partial, *c.peer) : GBP_OK;
}

int gbp::run_sweep(gbp_ba *h, const SweepCall &c)
{
    h->clk_cur = (h->timing && h->d_clk && h->clk_used < CLK_RING) ? h->d_clk + 6 * (size_t)h->clk_used++ : nullptr;
    if (!c.step.messages) {                                  // update_all_beliefs: from the stored messages
        CHK(launch_lmk_beliefs(h));
        CHK(launch_cam_partial(h, c.partial));
        if (c.sink == CamSink::PeerPush || c.sink == CamSink::PeerMerged) CHK(launch_peer_push(h, c.partial, *c.peer));
        if (c.sink == CamSink::Finish) return launch_cam_finish(h, c.partial, 1, 0, nullptr);
        return c.sink == CamSink::PeerMerged ? launch_cam_finish(h, nullptr, c.peer->n, 0, c.wait) : GBP_OK;
    }
    clock_tick(h, c.step.local_relin != 0);
    CHK(relin_slot_advance(h));
    // Every other sweep walks each workgroup's tile range backwards: what the last sweep touched last is touched first, so
    // whatever part of the state the Infinity Cache still holds is used before it is evicted.  With arena_reserve this removed
    // the slow mode of the 1M-factor graph (12 of 12 fresh processes at 11.6-12.1k sweeps/s; 7 of 12 at 10.0-10.7k without both).
    // (The fused sweep's parity is part of the state, gbp_handle.hpp; the general sweep's sums do not depend on the order.)
    const bool fused = h->fused.enabled;
    uint32_t &parity = fused ? h->walk_parity : h->gen_parity;
    const SweepLaunch at{h->stream, (int)(parity & 1u), fused ? h->clk_cur : nullptr, h->n_cus, &h->ovr};
    parity ^= 1u;
    if (!fused) {
        CHK(launch_general_sweep(h, c.step, at));
        if (!c.defer_parts) CHK(launch_finish_parts(h, h->stream));
        return staged_cameras(h, c, at);
    }
    h->cstage_x0_ok = false;                                // (a fused sweep moves linearisation points without staging them)
    const Params p = params_for(h, c.step);
    CHK(timed(h, [&] { fused_launch(h->fused, p, at); return GBP_OK; }));
    if (!c.defer_parts) CHK(launch_finish_parts(h, h->stream));
    const int rc = fused_cameras(h->fused, p, c, at);
    if (rc != 0) return fail(GBP_EHIP, "fused sweep launch failed: %s", hipGetErrorString((hipError_t)rc));
    return GBP_OK;
}


int gbp::launch_peer_selftest(gbp_ba *h, const PeerOut &po, double *mine, int rank, long long ticks, int *d_out)
{
    hipLaunchKernelGGL(k_peer_selftest, dim3(1), dim3(64), 0, h->stream, po, mine, rank, ticks, d_out);
    HIPCHK(hipGetLastError());
    return GBP_OK;
}

// -------------------------------------------------------------------------------- sweep ---

// ---- the dense message remainder on demand -------------------------------------------------------------------------------
// A message is stored as coefficients in the rows of its factor's Jacobian (gbp_math.hpp).  The one thing that does not fit is a
// factor that is DAMPED in the message computation that moves its linearisation point: d * (old eta) lies in the span of the OLD
// Jacobian.  The reference allows it at any time (compute_all_factors with damping on, gbp.py:60-62; relinearise_factors followed by
// compute_all_messages(local_relin=False), gbp.py:46-54); graphs created with num_undamped_iters = 0 carry the out-of-span part
// from the start (Params::xtra, 9 doubles per factor), every other graph gets it HERE, the first time such a call sequence
// shows up, and runs the general sweep (the kernels with the XTRA template flag) until every remainder has decayed to exactly
// zero again -- which the next undamped message of a factor does (x' = d x), i.e. after the next relinearisation wave.
int gbp::enable_remainder(gbp_ba *h)
{
    Params &p = h->p;
    if (p.xtra) return GBP_OK;
    const size_t n = n_slots(h) * XTRA_ROW;
    if (!h->xtra_buf) {
        HIPCHK(hipMalloc(reinterpret_cast<void **>(&h->xtra_buf), n * sizeof(double)));
        h->allocs.push_back(h->xtra_buf);
    }
    HIPCHK(hipMemsetAsync(h->xtra_buf, 0, n * sizeof(double), h->stream));
    p.xtra = h->xtra_buf;
    p.crow = CSTAGE_ROW;                                     // staged rows carry the remainder too: ensure_staging widens the buffer if need be
    h->lazy_xtra = true; h->lazy_since = 0;
    h->fused_suspended = h->fused.enabled;
    h->fused.enabled = false;
    return GBP_OK;
}

// before a message computation: does a pending relinearisation meet a non-zero damping?  (only after stage-wise calls, state loads)
int gbp::remainder_guard(gbp_ba *h, int local_relin, int no_test)
{
    if (!h->pending_possible || h->p.xtra || h->p.eta_damping == 0.0 || !h->p.T) return GBP_OK;
    HIPCHK(hipMemsetAsync(h->d_count, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_count_pending_damped, dim3(grid_for(n_slots(h))), dim3(BLOCK), 0, h->stream, h->p, local_relin, no_test, h->d_count);
    HIPCHK(hipGetLastError());
    int c = 0;
    HIPCHK(hipMemcpyAsync(&c, h->d_count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (c) CHK(enable_remainder(h));
    return GBP_OK;
}

// after a sweep on a remainder that was switched on on demand: back to the fused sweep once nothing is left of it
int gbp::remainder_release(gbp_ba *h)
{
    if (!h->lazy_xtra || !h->p.xtra || (++h->lazy_since & 15) != 0) return GBP_OK;
    const size_t n = n_slots(h) * XTRA_ROW;
    HIPCHK(hipMemsetAsync(h->d_count, 0, sizeof(int), h->stream));
    hipLaunchKernelGGL(k_count_nonzero, dim3(grid_for(n)), dim3(BLOCK), 0, h->stream, h->p.xtra, n, h->d_count);
    HIPCHK(hipGetLastError());
    int c = 0;
    HIPCHK(hipMemcpyAsync(&c, h->d_count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return c ? GBP_OK : remainder_drop(h);
}

// a handle whose remainder was switched on on demand goes back to the state "no remainder" (nothing is left of it, or a checkpoint
// without one is restored) and to the fused sweep if it ran one
int gbp::remainder_drop(gbp_ba *h)
{
    if (!h->lazy_xtra || !h->p.xtra) return GBP_OK;
    h->p.xtra = nullptr;                                     // (the buffer stays for the next time)
    h->p.crow = CSTAGE_PLAIN;                                // the staged rows are 16 doubles wide again (the buffer keeps its size)
    h->lazy_xtra = false;
    if (h->fused_suspended) h->fused.enabled = true;
    return GBP_OK;
}

extern "C" {

int gbp_ba_update_beliefs(gbp_ba_t *h)
{
    ENTER(h);
    h->resid_ok = false;
    CHK(run_sweep(h, SweepCall::finish({false, 0, 0}, h->d_partial)));
    h->has_beliefs = true;
    return GBP_OK;
}

int gbp_ba_iterate(gbp_ba_t *h, int32_t n_iters, int32_t robustify, int32_t local_relin)
{
    ENTER(h);
    h->resid_ok = false;
    if (n_iters < 0) return fail(GBP_EINVAL, "n_iters < 0");
    const SweepCall call = SweepCall::finish({true, robustify, local_relin}, h->d_partial);
    for (int it = 0; it < n_iters; ++it) CHK(guarded_sweep(h, local_relin, [&] { return run_sweep(h, call); }));
    h->has_beliefs = true;
    return GBP_OK;
}

// ---- the reference's stage-wise entry points (gbp.py:46-84) ------------------------------------------------------------
// synchronous_iteration is these four in a row (gbp.py:86-92) and runs as one fused kernel; called one by one they run as stage
// kernels on the same state.  A relinearisation decided by gbp_ba_relinearise / gbp_ba_compute_factors is applied when the
// messages are next computed (gbp_kernels.hpp, state word header).

int gbp_ba_robustify(gbp_ba_t *h)
{
    ENTER(h);
    h->resid_ok = false;
    const Params &p = h->p;
    if (!p.T || p.loss == GBP_LOSS_NONE) return GBP_OK;            // loss None: adaptive variance = gauss_noise_var, nothing stored (gbp.py:302-303)
    const int nb = grid_for(n_slots(h));
    if (p.loss == GBP_LOSS_HUBER) hipLaunchKernelGGL(k_stage_robustify<1>, dim3(nb), dim3(BLOCK), 0, h->stream, p);
    else hipLaunchKernelGGL(k_stage_robustify<2>, dim3(nb), dim3(BLOCK), 0, h->stream, p);
    HIPCHK(hipGetLastError());
    return GBP_OK;
}

int gbp_ba_relinearise(gbp_ba_t *h)
{
    ENTER(h);
    h->resid_ok = false;
    if (!h->has_beliefs) return fail(GBP_ESTATE, "relinearise_factors needs beliefs (call update_all_beliefs first; the reference inverts zero matrices here, gbp.py:73)");
    clock_tick(h, true);
    if (h->p.T) hipLaunchKernelGGL(k_stage_relinearise, dim3(grid_for(n_slots(h))), dim3(BLOCK), 0, h->stream, h->p, 0);
    HIPCHK(hipGetLastError());
    h->pending_possible = true;
    return GBP_OK;
}

int gbp_ba_compute_factors(gbp_ba_t *h)
{
    ENTER(h);
    h->resid_ok = false;
    if (!h->has_beliefs) return fail(GBP_ESTATE, "compute_all_factors linearises at the belief means: call update_all_beliefs first");
    // (a factor that is damped when it moves leaves the span its message coefficients live in: the message computation that applies
    //  the move checks for that and switches the dense remainder on, remainder_guard)
    if (h->p.T) hipLaunchKernelGGL(k_stage_relinearise, dim3(grid_for(n_slots(h))), dim3(BLOCK), 0, h->stream, h->p, 1);
    HIPCHK(hipGetLastError());
    h->pending_possible = true;
    return GBP_OK;
}

int gbp_ba_compute_messages(gbp_ba_t *h, int32_t local_relin)
{
    ENTER(h);
    h->resid_ok = false;
    if (!h->has_beliefs) return fail(GBP_ESTATE, "compute_all_messages needs beliefs (call update_all_beliefs first)");
    CHK(remainder_guard(h, local_relin, 1));
    CHK(relin_slot_advance(h));
    h->p.stage = STAGE_NO_TEST | STAGE_NO_BELIEFS;
    clock_tick(h, false);                                    // (no relinearisation test in this call: nobody ages)
    h->p.reverse_walk = 0;
    const int rc = launch_factor_stage(h, {true, 0, local_relin});
    h->p.stage = 0;
    h->pending_possible = false;
    return rc;
}

int gbp_ba_shard_begin(gbp_ba_t *h, int32_t with_messages, int32_t robustify, int32_t local_relin, double *partial_dev)
{
    ENTER(h);
    h->resid_ok = false;
    if (!partial_dev) return fail(GBP_EINVAL, "null partial buffer");
    const SweepCall call = SweepCall::partials({with_messages != 0, robustify, local_relin}, partial_dev, false);
    return with_messages ? guarded_sweep(h, local_relin, [&] { return run_sweep(h, call); }) : run_sweep(h, call);
}

int gbp_ba_shard_end(gbp_ba_t *h, const double *gathered_dev, int32_t n_ranks)
{
    ENTER(h);
    h->resid_ok = false;
    if (!gathered_dev || n_ranks < 1) return fail(GBP_EINVAL, "bad gathered buffer / rank count");
    CHK(launch_cam_finish(h, gathered_dev, n_ranks, (size_t)h->p.C * 27, nullptr));
    h->has_beliefs = true;
    return GBP_OK;
}

// --------------------------------------------------------------------------- diagnostics ---

int gbp_ba_residual_sums(gbp_ba_t *h, double out[2])
{
    ENTER(h);
    CHK(peer_check(h, false));
    if (!out) return fail(GBP_EINVAL, "null argument");
    const Params &p = h->p;
    out[0] = out[1] = 0.0;
    if (!p.F) return GBP_OK;
    if (!h->resid_ok) {                                 // are() then energy() on the same state: one kernel, one round trip
        const int nb = grid_for(n_slots(h));
        hipLaunchKernelGGL(k_residual, dim3(nb), dim3(BLOCK), 0, h->stream, p, h->d_red);
        HIPCHK(hipGetLastError());
        std::vector<double> part;
        CHK(download(h, part, h->d_red, 2 * (size_t)nb));
        h->resid[0] = h->resid[1] = 0.0;
        for (int b = 0; b < nb; ++b) { h->resid[0] += part[2 * b]; h->resid[1] += part[2 * b + 1]; }
        h->resid_ok = true;
    }
    out[0] = h->resid[0]; out[1] = h->resid[1];
    return GBP_OK;
}

int gbp_ba_are(gbp_ba_t *h, double *out)
{
    if (!out) return fail(GBP_EINVAL, "null argument");
    double s[2];
    CHK(gbp_ba_residual_sums(h, s));
    *out = s[0] / (double)h->p.F;               // divides by len(self.factors)  gbp_ba.py:69
    return GBP_OK;
}

int gbp_ba_energy(gbp_ba_t *h, double *out)
{
    if (!out) return fail(GBP_EINVAL, "null argument");
    double s[2];
    CHK(gbp_ba_residual_sums(h, s));
    *out = s[1];
    return GBP_OK;
}

// ------------------------------------------------------------------------ instrumentation ---

int gbp_ba_set_kernel_timing(gbp_ba_t *h, int32_t enable)
{
    ENTER(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    h->timing = enable != 0;
    h->timing_every = enable > 1 ? enable : 1;
    h->timing_tick = 0;
    h->ev_used = 0;
    h->clk_used = 0; h->clk_cur = nullptr;
    if (enable) {
        if (!h->d_clk) {
            HIPCHK(hipMalloc(reinterpret_cast<void **>(&h->d_clk), sizeof(unsigned long long) * 6 * CLK_RING));
            h->allocs.push_back(h->d_clk);
            HIPCHK(hipDeviceGetAttribute(&h->clk_rate_khz, hipDeviceAttributeWallClockRate, h->device));
        }
        if (!h->clk_calibrated) {
            // The rate of wall_clock64: hipDeviceAttributeWallClockRate says 100 MHz, and on some boxes of the pool the counter runs
            // ~7 % faster than that (stamped kernel times came out longer than the step that contains them, while HIP events and the
            // wall clock agreed with each other).  Measured once per handle: two stamps 20 ms apart against the HIP events around them.
            unsigned long long *d_cal = nullptr, cal[2] = {0, 0};
            hipEvent_t e0, e1;
            HIPCHK(hipMalloc(reinterpret_cast<void **>(&d_cal), 2 * sizeof(unsigned long long)));
            HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
            hipLaunchKernelGGL(k_clk_stamp, dim3(1), dim3(64), 0, h->stream, d_cal);
            HIPCHK(hipEventRecord(e0, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            std::this_thread::sleep_for(std::chrono::milliseconds(20));
            hipLaunchKernelGGL(k_clk_stamp, dim3(1), dim3(64), 0, h->stream, d_cal + 1);
            HIPCHK(hipEventRecord(e1, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, e0, e1));
            HIPCHK(hipMemcpy(cal, d_cal, sizeof cal, hipMemcpyDeviceToHost));
            (void)hipFree(d_cal); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
            if (ms > 1.f && cal[1] > cal[0]) {
                const double khz = (double)(cal[1] - cal[0]) / (double)ms;
                if (khz > 0.5 * h->clk_rate_khz && khz < 2.0 * h->clk_rate_khz) h->clk_rate_khz_measured = khz;
            }
            h->clk_calibrated = true;
        }
        hipLaunchKernelGGL(k_clk_init, dim3((6 * CLK_RING + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, h->stream, h->d_clk, 6 * CLK_RING);
        HIPCHK(hipGetLastError());
    }
    return GBP_OK;
}

int gbp_ba_get_sweep_clocks(gbp_ba_t *h, double *us6, int32_t cap, int32_t *n_sweeps)
{
    ENTER(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    const int n = std::min(h->clk_used, CLK_RING);
    if (n_sweeps) *n_sweeps = n;
    if (!us6 || !n || cap <= 0) return GBP_OK;
    std::vector<unsigned long long> raw;
    CHK(download(h, raw, h->d_clk, 6 * (size_t)n));
    unsigned long long t0 = ~0ull;
    for (unsigned long long v : raw) if (v != 0ull && v != ~0ull) t0 = std::min(t0, v);
    const double khz = h->clk_rate_khz_measured > 0.0 ? h->clk_rate_khz_measured : (double)h->clk_rate_khz;
    const double us_per_tick = khz > 0.0 ? 1e3 / khz : 0.01;
    for (int i = 0; i < n && i < cap; ++i)
        for (int k = 0; k < 6; ++k) {
            const unsigned long long v = raw[6 * (size_t)i + k];
            us6[6 * (size_t)i + k] = (v == 0ull || v == ~0ull) ? NAN : (double)(v - t0) * us_per_tick;
        }
    return GBP_OK;
}

int gbp_ba_get_kernel_timing(gbp_ba_t *h, double *total_ms, int32_t *n_launches, const char **kernel_name)
{
    ENTER(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    double tot = 0.0;
    for (size_t i = 0; i + 1 < h->ev_used; i += 2) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, h->ev[i], h->ev[i + 1]));
        tot += ms;
    }
    if (total_ms) *total_ms = tot;
    if (n_launches) *n_launches = (int32_t)(h->ev_used / 2);
    if (kernel_name) *kernel_name = dominant_kernel(h);
    h->ev_used = 0;
    return GBP_OK;
}

int gbp_ba_get_kernel_times(gbp_ba_t *h, double *ms, int32_t cap, int32_t *n_launches)
{
    ENTER(h);
    HIPCHK(hipStreamSynchronize(h->stream));
    const int32_t n = (int32_t)(h->ev_used / 2);
    if (n_launches) *n_launches = n;
    for (int32_t i = 0; i < n && i < cap && ms; ++i) {
        float t = 0.f;
        HIPCHK(hipEventElapsedTime(&t, h->ev[2 * (size_t)i], h->ev[2 * (size_t)i + 1]));
        ms[i] = t;
    }
    return GBP_OK;
}

// phase profile of the last fused sweep (GBP_PHASE_TIMING builds; rows = workgroups x waves, NPHASE columns of s_memtime ticks)
int gbp_ba_phase_profile(gbp_ba_t *h, uint64_t *out, int32_t cap_rows, int32_t *n_rows, int32_t *n_cols)
{
    ENTER(h);
    if (n_rows) *n_rows = 0;
    if (n_cols) *n_cols = NPHASE;
#ifdef GBP_PHASE_TIMING
    if (!h->fused.enabled || !h->fused.args.phase) return fail(GBP_ESTATE, "no phase profile: the fused sweep is not in use");
    const int rows = h->fused.n_blocks * WAT_WAVES;
    if (n_rows) *n_rows = rows;
    if (out && cap_rows >= rows) {
        HIPCHK(hipMemcpyAsync(out, h->fused.args.phase, sizeof(uint64_t) * (size_t)rows * NPHASE, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    return GBP_OK;
#else
    (void)out; (void)cap_rows;
    return fail(GBP_ESTATE, "not a GBP_PHASE_TIMING build (tools/phase_profile.py compiles one)");
#endif
}


}  // extern "C"
