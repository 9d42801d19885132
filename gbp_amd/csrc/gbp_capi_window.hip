// gbp_capi_window.hip -- libgbp_hip.so, the ONE way a live handle shrinks or takes a window step (include/gbp_ba.h): gbp_ba_window_step
// appends a keyframe, drops the observations found wrong, lets the oldest keyframes go and lets go of landmarks by name in one rebuild
// of the handle; gbp_ba_cull, gbp_ba_retire and gbp_ba_retire_landmarks (at the bottom) are that step with one list filled and no
// batch.  The parts differ in why a factor leaves and in what is folded where: a per-factor REASON (window_reason) says the first and drives both
// folds (window_reason).  (gbp_ba_extend goes its own way, gbp_capi_extend.hip: it needs no flags, and a new variable without a factor stays there.)
//
// The way: flags over the union index space [C + dC | L + dL | F + dF | 1], one scan for the six maps, one compaction into the
// result's inputs in file order (the staying old factors in old reference order, then the batch), the create path ONCE
// (gbp::build_graph; its ref_file map is non-NULL when the batch brings factors of old cameras), the state transplant through the
// composed map  new slot -> new reference id -> file position -> old reference id -> old slot,  the two folds, priors of the new
// variables, update_all_beliefs, the swap.  No intermediate union is built: peak device memory is the old handle's plus the result's.
// What a call does not ask for is not run: an empty list is a NULL word array, no batch means no marks and no new priors, a fold
// without a factor to fold is not launched.
#include "gbp_graft.hpp"

#include <rocprim/device/device_scan.hpp>

#include <climits>

namespace {

// why an old factor leaves, by precedence (include/gbp_ba.h, gbp_ba_window_step c.)
enum : int { W_STAYS = 0, W_CULLED = 1, W_CAM_RETIRED = 2, W_LMK_LISTED = 3 };

// the caller's lists as 0 / 1 words: gone[F] (old reference order), cam[C + dC], lmk[L + dL] (the caller's numbering; new ids: 0);
// NULL: the list is empty
struct WindowLists {
    const int *gone, *cam, *lmk;
    GBP_DEV bool culled(int f) const { return gone && gone[f]; }
    GBP_DEV bool retired(size_t c) const { return cam && cam[c]; }
    GBP_DEV bool listed(size_t l) const { return lmk && lmk[l]; }
};

// d_ref_lmk holds the handle's INTERNAL landmark ids, the list is in the CALLER's numbering: o_i2u (NULL: identity) leads back
GBP_DEV int window_reason(const WindowLists &w, const int *__restrict__ ref_cam, const int *__restrict__ ref_lmk, const int *__restrict__ o_i2u, int f)
{
    if (w.culled(f)) return W_CULLED;
    if (w.retired(ref_cam[f])) return W_CAM_RETIRED;
    if (!w.lmk) return W_STAYS;
    const int li = ref_lmk[f];
    return w.lmk[o_i2u ? o_i2u[li] : li] ? W_LMK_LISTED : W_STAYS;
}

// One lane per batch factor: its camera and its landmark have a surviving factor (seen[C + dC | L + dL], cleared before; every lane
// that writes a word writes the same 1: plain stores, no atomics).  An entry that names an id beyond the union, a retired camera or a
// listed landmark marks nothing and reports itself: *bad = the lowest such entry.
__global__ __launch_bounds__(BLOCK) void k_window_mark(const int *__restrict__ bcam, const int *__restrict__ blmk, int dF, int Cu, int Lu, WindowLists w,
                                                       int *__restrict__ seen, int *__restrict__ bad)
{
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= dF) return;
    const int c = bcam[j], l = blmk[j];
    if (c < 0 || c >= Cu || l < 0 || l >= Lu || w.retired(c) || w.listed(l)) { atomicMin(bad, j); return; }
    seen[c] = 1;
    seen[Cu + l] = 1;
}

// The survival flags over the union index space.  A factor stays when it has no reason to go
// (a batch factor always); a variable stays when it is not listed and any staying factor names it: the batch's marks (seen; NULL: the
// batch has no factor), or -- an old variable -- a staying factor of its own: a camera looks at its contiguous range of the
// camera-major reference order (cptr), a landmark -- walked in the CALLER's numbering, o_u2i (NULL: identity) leads to a reordered
// handle's record -- at its slot range (cpos: slot -> reference id).  Both stop at the first survivor.  bare_cams (gbp_ba_retire): a
// camera that is not listed stays, with or without a factor.  keep[last] = 0, so that the exclusive scan ends with the total.
__global__ __launch_bounds__(BLOCK) void k_window_flags(Params o, int dC, int dL, int dF, WindowLists w, int bare_cams, const int *__restrict__ seen,
                                                        const int *__restrict__ ref_cam, const int *__restrict__ ref_lmk,
                                                        const int *__restrict__ o_u2i, const int *__restrict__ o_i2u,
                                                        int *__restrict__ keep)
{
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t C = (size_t)o.C, L = (size_t)o.L, F = (size_t)o.F;
    const size_t Cu = C + (size_t)dC, Lu = L + (size_t)dL, Fu = F + (size_t)dF;
    if (i < Cu) {
        int any = 0;
        if (!w.retired(i)) {
            any = bare_cams | (seen ? seen[i] : 0);
            if (i < C)
                for (int f = o.cptr[i], f1 = o.cptr[i + 1]; f < f1 && !any; ++f) any = window_reason(w, ref_cam, ref_lmk, o_i2u, f) == W_STAYS ? 1 : 0;
        }
        keep[i] = any;
    } else if (i < Cu + Lu) {
        const size_t l = i - Cu;
        int any = 0;
        if (!w.listed(l)) {
            any = seen ? seen[i] : 0;
            if (l < L && !any) {
                const int2 rows = *reinterpret_cast<const int2 *>(o.lrec + (o_u2i ? (size_t)o_u2i[l] : l) * LREC + LR_ROWS);
                for (int s = rows.x; s < rows.y && !any; ++s) {
                    const int f = o.cpos[s];
                    any = (f >= 0 && f < o.F && window_reason(w, ref_cam, ref_lmk, o_i2u, f) == W_STAYS) ? 1 : 0;
                }
            }
        }
        keep[i] = any;
    } else if (i < Cu + Lu + Fu) {
        const size_t f = i - Cu - Lu;
        keep[i] = (f >= F || window_reason(w, ref_cam, ref_lmk, o_i2u, (int)f) == W_STAYS) ? 1 : 0;
    } else if (i == Cu + Lu + Fu) {
        keep[i] = 0;
    }
}

// the batch as the device sees it
struct Batch {
    int dC, dL, dF;
    const double *cam_means, *lmk_means, *meas;
    const int *cam, *lmk;
};

// The result's inputs for the create path and the maps (gbp_graft.hpp: Survivors, over the union): o2n[C + dC | L + dL | F + dF] = new id
// or -1 -- for a factor its FILE position, which k_window_slots turns into the new reference id; f_n2o[F'] = the union id of the factor
// at each file position (below F: an old reference id; from F on: F + the batch entry).  File order: the staying old factors in old
// reference order (measurement = the z rows of the slot), then the batch in batch order.  Means: the current belief means of old
// variables, the given means of new ones.
__global__ __launch_bounds__(BLOCK) void k_window_compact(Params o, Batch b, const int *__restrict__ ref_cam, const int *__restrict__ ref_lmk,
                                                          const int *__restrict__ o_u2i, const int *__restrict__ o_i2u,
                                                          const int *__restrict__ keep, const int *__restrict__ pos, Survivors s)
{
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t C = (size_t)o.C, L = (size_t)o.L, F = (size_t)o.F;
    const size_t Cu = C + (size_t)b.dC, Lu = L + (size_t)b.dL, Fu = F + (size_t)b.dF;
    if (i >= Cu + Lu + Fu) return;
    if (!keep[i]) { s.o2n[i] = -1; return; }
    if (i < Cu) {
        const int nc = pos[i];
        s.o2n[i] = nc;
#pragma unroll
        for (int k = 0; k < 6; ++k) s.cam_means[(size_t)nc * 6 + k] = i < C ? o.cbel[i * CAMREC + CAM_MU + k] : b.cam_means[(i - C) * 6 + k];
    } else if (i < Cu + Lu) {
        const size_t l = i - Cu;
        const int nl = pos[i] - pos[Cu];
        s.o2n[i] = nl;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            s.lmk_means[(size_t)nl * 3 + k] = l < L ? o.lrec[(o_u2i ? (size_t)o_u2i[l] : l) * LREC + LR_MU + k] : b.lmk_means[(l - L) * 3 + k];
    } else {
        const size_t f = i - Cu - Lu;
        const int nf = pos[i] - pos[Cu + Lu];
        s.o2n[i] = nf;
        s.f_n2o[nf] = (int)f;
        int c, l;                                               // (a staying factor's camera and landmark stay)
        if (f < F) {
            const int os = o.cadj[f];
            s.meas[(size_t)nf * 2] = o.lin[lin_at(os, ROW_Z)];
            s.meas[(size_t)nf * 2 + 1] = o.lin[lin_at(os, ROW_Z + 1)];
            c = ref_cam[f];
            l = o_i2u ? o_i2u[ref_lmk[f]] : ref_lmk[f];
        } else {
            const size_t j = f - F;
            s.meas[(size_t)nf * 2] = b.meas[j * 2];
            s.meas[(size_t)nf * 2 + 1] = b.meas[j * 2 + 1];
            c = b.cam[j];
            l = b.lmk[j];
        }
        s.cam[nf] = pos[c];
        s.lmk[nf] = pos[Cu + (size_t)l] - pos[Cu];
    }
}

// One lane per slot of the result, through the composed map: new slot -> new reference id (cpos) -> file position (ref_file, NULL:
// identity) -> union factor id (f_n2o).  The factor's map entry becomes its new reference id; an old factor's whole state moves from
// its old slot (transplant_slot), a new one keeps what the build gave it (create's initialisation).
__global__ __launch_bounds__(BLOCK) void k_window_slots(Params n, Params o, const int *__restrict__ ref_file, const int *__restrict__ f_n2o, int Fu,
                                                        int *__restrict__ factor_map)
{
    const int slot = blockIdx.x * BLOCK + threadIdx.x;
    if (slot >= n.T * WTILE || (slot & 63) >= n.tiles[slot >> 6].z) return;
    const int r = n.cpos[slot];
    if (r < 0 || r >= n.F) return;
    const int fp = ref_file ? ref_file[r] : r;
    if (fp < 0 || fp >= n.F) return;
    const int f = f_n2o[fp];
    if (f < 0 || f >= Fu) return;
    factor_map[f] = r;
    if (f < o.F) transplant_slot(n, o, slot, o.cadj[f]);
}

// One lane per OLD variable: a surviving camera keeps its record, belief view and prior; a surviving landmark its mean | covariance
// and prior (the folds then write the priors again).  cam_o2n[C + dC], lmk_o2n[L + dL]: the union's maps.
__global__ __launch_bounds__(BLOCK) void k_window_vars(Params n, Params o, const int *__restrict__ cam_o2n, const int *__restrict__ lmk_o2n,
                                                       const int *__restrict__ n_u2i, const int *__restrict__ o_u2i)
{
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v >= o.C + o.L) return;
    const int nv = v < o.C ? cam_o2n[v] : lmk_o2n[v - o.C];
    if (nv < 0) return;
    if (v < o.C) transplant_cam(n, o, nv, v);
    else transplant_lmk(n, o, n_u2i ? n_u2i[nv] : nv, o_u2i ? o_u2i[v - o.C] : v - o.C);
}

// The fold of gbp_ba_retire, driven by the factor's reason: one lane per OLD landmark that survives walks its old slot range in
// adj_factors order; every factor that leaves because its camera is retired is folded into the prior: l.prior += f.messages[1], the
// full message as the message view reports it (dense_messages: Lambda = J_l^T V J_l and eta = J_l^T q_L with J at the factor's stored
// linearisation point, plus the landmark part of the dense remainder).  Prior first, then the folds one by one in fp64: a fixed order, the
// same result every run.  A culled factor is not folded; a landmark none of whose factors is folded keeps its prior bit for bit.
__global__ __launch_bounds__(BLOCK) void k_window_fold_lmks(Params n, Params o, const int *__restrict__ lmk_o2n, WindowLists w,
                                                            const int *__restrict__ ref_cam, const int *__restrict__ ref_lmk,
                                                            const int *__restrict__ n_u2i, const int *__restrict__ o_u2i, const int *__restrict__ o_i2u)
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
        const int f = o.cpos[s];
        if (f < 0 || f >= o.F || window_reason(w, ref_cam, ref_lmk, o_i2u, f) != W_CAM_RETIRED) continue;
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

// The fold of gbp_ba_retire_landmarks (mode FOLD), driven by the factor's reason: one WAVE per OLD camera that survives: c.prior +=
// f.messages[0] for every factor f of c that leaves because its landmark is listed.  The camera's factors are its range of the OLD
// reference order, walked in chunks of 64: lane j takes factor cptr[c] + 64 k + j of chunk k and rebuilds its message (every other
// lane holds zeros), the 27 sums of the chunk are formed by an xor butterfly over the wave -- a fixed tree, the same in every lane --
// and the chunk totals are added in ascending k on top of the prior: lane e < 27 keeps entry e.  No atomics: the same bits every run.
// A camera without such a factor is not written: its prior stays bit for bit.  (One lane per camera would rebuild a camera's messages
// one after the other -- 2 000 linearisations in a row at the headline size.)
__global__ __launch_bounds__(BLOCK) void k_window_fold_cams(Params n, Params o, const int *__restrict__ cam_o2n, WindowLists w,
                                                            const int *__restrict__ ref_cam, const int *__restrict__ ref_lmk, const int *__restrict__ o_i2u)
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
        const bool goes = f < f1 && window_reason(w, ref_cam, ref_lmk, o_i2u, f) == W_LMK_LISTED;
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

// One request to the engine: the caller's three lists as they came (old factors in reference order, old cameras, old landmarks in the
// caller's numbering; a count of 0: nothing listed), the batch, and what the four calls do differently.
struct Step {
    int32_t n_gone, n_cam, n_lmk;
    const int32_t *gone, *cam, *lmk;
    bool fold;                                                  // the listed landmarks' messages go into the cameras' priors (else: dropped)
    const gbp_ba_ext_t *e;                                      // never NULL (no_batch stands in)
    bool bare_cams;                                             // gbp_ba_retire: a camera that is not listed stays, with or without a factor
    const char *all_listed;                                     // the refusal when a list names every factor / camera / landmark (NULL: the batch may bring others)
    const char *emptied;                                        // the refusal when nothing survives
};
const gbp_ba_ext_t no_batch{};

// the lists after their checks, as 0 / 1 words: gone[F], cam[C + dC], lmk[L + dL]; an empty vector: nothing listed
struct Words {
    std::vector<int> gone, cam, lmk;
};


// the result built beside the old handle `o` into the fresh handle `n` (which owns nothing of o's); maps: the six maps in union order
// [C + dC | L + dL | F + dF], on the host
int window_into(gbp_ba *o, gbp_ba *n, const Step &st, const Words &wd, std::vector<void *> &scratch, std::vector<int> &maps)
{
    const Params &op = o->p;
    const gbp_ba_ext_t *e = st.e;
    const int dC = e->n_new_cams, dL = e->n_new_lmks, dF = e->n_new_factors;
    const size_t Cu = (size_t)op.C + dC, Lu = (size_t)op.L + dL, Fu = (size_t)op.F + dF, N = Cu + Lu + Fu;
    const bool dev_in = (e->flags & GBP_FLAG_DEVICE_INPUT) != 0;
    n->device = o->device; n->stream = o->stream;              // (graft_settings sets the rest once the sizes are known)

    // 1. the lists and the batch on the device; which variables the batch's factors keep alive (and whether their ids are sound)
    WindowLists w{nullptr, nullptr, nullptr};                  // (an empty list stays NULL: nothing is allocated or uploaded for it)
    if (!wd.gone.empty()) CHK(stage_input(n, wd.gone.data(), wd.gone.size(), false, scratch, &w.gone));
    if (!wd.cam.empty()) CHK(stage_input(n, wd.cam.data(), wd.cam.size(), false, scratch, &w.cam));
    if (!wd.lmk.empty()) CHK(stage_input(n, wd.lmk.data(), wd.lmk.size(), false, scratch, &w.lmk));
    int *d_seen = nullptr, *d_bad = nullptr, *d_keep = nullptr, *d_pos = nullptr;
    CHK(scratch_alloc(n, scratch, &d_keep, N + 1)); CHK(scratch_alloc(n, scratch, &d_pos, N + 1));
    Batch b{dC, dL, dF, nullptr, nullptr, nullptr, nullptr, nullptr};
    CHK(stage_input(n, e->cam_means, (size_t)dC * 6, dev_in, scratch, &b.cam_means)); CHK(stage_input(n, e->lmk_means, (size_t)dL * 3, dev_in, scratch, &b.lmk_means));
    CHK(stage_input(n, e->meas, (size_t)dF * 2, dev_in, scratch, &b.meas));
    CHK(stage_input(n, e->cam_idx, (size_t)dF, dev_in, scratch, &b.cam)); CHK(stage_input(n, e->lmk_idx, (size_t)dF, dev_in, scratch, &b.lmk));
    if (dF) {
        CHK(scratch_alloc(n, scratch, &d_seen, Cu + Lu)); CHK(scratch_alloc(n, scratch, &d_bad, 1));
        HIPCHK(hipMemsetAsync(d_seen, 0, sizeof(int) * (Cu + Lu), n->stream));
        HIPCHK(hipMemsetAsync(d_bad, 0x7f, sizeof(int), n->stream));      // 0x7f7f7f7f: above every entry
        hipLaunchKernelGGL(k_window_mark, dim3(grid_for((size_t)dF)), dim3(BLOCK), 0, n->stream, b.cam, b.lmk, dF, (int)Cu, (int)Lu, w, d_seen, d_bad);
    }

    // 2. flags, one prefix sum, the result's sizes (without new cameras ends[0] = ends[1], without new landmarks ends[2] = ends[3])
    hipLaunchKernelGGL(k_window_flags, dim3(grid_for(N + 1)), dim3(BLOCK), 0, n->stream, op, dC, dL, dF, w, st.bare_cams ? 1 : 0, d_seen, o->d_ref_cam,
                       o->d_ref_lmk, o->d_lmk_u2i, o->d_lmk_i2u, d_keep);
    HIPCHK(hipGetLastError());
    size_t scan_bytes = 0;
    HIPCHK(rocprim::exclusive_scan(nullptr, scan_bytes, d_keep, d_pos, 0, N + 1, rocprim::plus<int>(), n->stream));
    void *scan_tmp = nullptr;
    HIPCHK(hipMallocAsync(&scan_tmp, std::max<size_t>(scan_bytes, 1), n->stream));
    scratch.push_back(scan_tmp);
    HIPCHK(rocprim::exclusive_scan(scan_tmp, scan_bytes, d_keep, d_pos, 0, N + 1, rocprim::plus<int>(), n->stream));
    int ends[5] = {0, 0, 0, 0, 0}, bad = 0;                     // surviving old cameras | cameras | + old landmarks | + landmarks | + factors
    if (dC) HIPCHK(hipMemcpyAsync(&ends[0], d_pos + op.C, sizeof(int), hipMemcpyDeviceToHost, n->stream));
    HIPCHK(hipMemcpyAsync(&ends[1], d_pos + Cu, sizeof(int), hipMemcpyDeviceToHost, n->stream));
    if (dL) HIPCHK(hipMemcpyAsync(&ends[2], d_pos + Cu + op.L, sizeof(int), hipMemcpyDeviceToHost, n->stream));
    HIPCHK(hipMemcpyAsync(&ends[3], d_pos + Cu + Lu, sizeof(int), hipMemcpyDeviceToHost, n->stream));
    HIPCHK(hipMemcpyAsync(&ends[4], d_pos + N, sizeof(int), hipMemcpyDeviceToHost, n->stream));
    if (dF) HIPCHK(hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, n->stream));
    HIPCHK(hipStreamSynchronize(n->stream));
    if (!dC) ends[0] = ends[1];
    if (!dL) ends[2] = ends[3];
    if (dF && bad < dF)
        return fail(GBP_EINVAL, "new observation %d references a camera outside [0,%d), a landmark outside [0,%d), a retired camera or a listed landmark",
                    bad, (int)Cu, (int)Lu);
    const int C = ends[1], L = ends[3] - ends[1], F = ends[4] - ends[3];
    const int c0 = ends[0], l0 = ends[2] - ends[1];             // the surviving new variables are cameras [c0, C) and landmarks [l0, L)
    if (F <= 0 || C <= 0 || L <= 0) return fail(GBP_EINVAL, "%s", st.emptied);
    if (C >= (1 << (32 - META_LMK_BITS))) return fail(GBP_EINVAL, "more than %d cameras are not supported", (1 << (32 - META_LMK_BITS)) - 1);
    graft_settings(o, n, C, L, F);
    Params &p = n->p;

    // 3. the result's inputs, on the device
    Survivors s{};
    CHK(scratch_alloc(n, scratch, &s.o2n, N)); CHK(scratch_alloc(n, scratch, &s.f_n2o, (size_t)F));
    CHK(scratch_alloc(n, scratch, &s.meas, (size_t)F * 2)); CHK(scratch_alloc(n, scratch, &s.cam, (size_t)F)); CHK(scratch_alloc(n, scratch, &s.lmk, (size_t)F));
    CHK(scratch_alloc(n, scratch, &s.cam_means, (size_t)C * 6)); CHK(scratch_alloc(n, scratch, &s.lmk_means, (size_t)L * 3));
    hipLaunchKernelGGL(k_window_compact, dim3(grid_for(N)), dim3(BLOCK), 0, n->stream, op, b, o->d_ref_cam, o->d_ref_lmk, o->d_lmk_u2i, o->d_lmk_i2u, d_keep, d_pos, s);
    HIPCHK(hipGetLastError());

    // 4. the result's graph by the create path, once
    gbp_ba_desc_t d{};
    d.n_cams = C; d.n_lmks = L; d.n_factors = F; d.device = o->device;
    d.cam_means = s.cam_means; d.lmk_means = s.lmk_means; d.meas = s.meas; d.cam_idx = s.cam; d.lmk_idx = s.lmk;
    d.flags = GBP_FLAG_DEVICE_INPUT;                           // (the sweep flags are n->flags)
    const int *ref_file = nullptr;
    CHK(build_graph(n, &d, scratch, n->n_cus, &ref_file));

    // 5. a remainder switched on on demand stays on (the fresh handle allocates it exactly as the old one did)
    if (o->lazy_xtra && op.xtra) CHK(enable_remainder(n));

    // 6. the state transplant and the folds, over the transplanted priors (a fold none of whose factors leaves would write the same bits)
    const int *cam_o2n = s.o2n, *lmk_o2n = s.o2n + Cu;
    hipLaunchKernelGGL(k_window_slots, dim3(grid_for(n_slots(n))), dim3(BLOCK), 0, n->stream, p, op, ref_file, s.f_n2o, (int)Fu, s.o2n + Cu + Lu);
    if (op.C + op.L) hipLaunchKernelGGL(k_window_vars, dim3(grid_for((size_t)op.C + op.L)), dim3(BLOCK), 0, n->stream, p, op, cam_o2n, lmk_o2n, n->d_lmk_u2i, o->d_lmk_u2i);
    if (!wd.cam.empty() && op.L) hipLaunchKernelGGL(k_window_fold_lmks, dim3(grid_for((size_t)op.L)), dim3(BLOCK), 0, n->stream, p, op, lmk_o2n, w, o->d_ref_cam, o->d_ref_lmk,
                                                     n->d_lmk_u2i, o->d_lmk_u2i, o->d_lmk_i2u);
    if (st.fold && !wd.lmk.empty() && op.C) {
        const int waves = BLOCK / WTILE;
        hipLaunchKernelGGL(k_window_fold_cams, dim3((op.C + waves - 1) / waves), dim3(BLOCK), 0, n->stream, p, op, cam_o2n, w, o->d_ref_cam, o->d_ref_lmk, o->d_lmk_i2u);
    }
    HIPCHK(hipGetLastError());
    CHK(graft_counters(o, n));
    maps.resize(N);
    HIPCHK(hipMemcpyAsync(maps.data(), s.o2n, sizeof(int) * N, hipMemcpyDeviceToHost, n->stream));
    HIPCHK(hipStreamSynchronize(n->stream));

    // 7. priors of the new variables that stay (cameras [c0, C), landmarks [l0, L)): the rule over their factors -- all of them new --
    //    or the given scalars, as gbp_ba_extend step 5
    const int nC = C - c0, nL = L - l0;
    const double wf = e->prior_weaker_factor;
    const bool rule = wf > 0.0;
    if (nC || nL) {
        if (rule && ((nC && !e->cam_prior_lambda) || (nL && !e->lmk_prior_lambda))) CHK(variable_lambda_max(n));
        std::vector<double> given;
        if (nC && (e->cam_prior_lambda || !rule)) {
            given.assign((size_t)nC, 0.0);
            for (int j = 0; e->cam_prior_lambda && j < dC; ++j)
                if (maps[(size_t)op.C + j] >= 0) given[(size_t)(maps[(size_t)op.C + j] - c0)] = e->cam_prior_lambda[j];
            HIPCHK(hipMemcpyAsync(n->d_varmax + c0, given.data(), sizeof(double) * (size_t)nC, hipMemcpyHostToDevice, n->stream));
            HIPCHK(hipStreamSynchronize(n->stream));             // `given` is reused
        }
        if (nL && (e->lmk_prior_lambda || !rule)) {
            given.assign((size_t)nL, 0.0);
            for (int j = 0; e->lmk_prior_lambda && j < dL; ++j)
                if (maps[Cu + (size_t)op.L + j] >= 0) given[(size_t)(maps[Cu + (size_t)op.L + j] - l0)] = e->lmk_prior_lambda[j];
            HIPCHK(hipMemcpyAsync(n->d_varmax + C + l0, given.data(), sizeof(double) * (size_t)nL, hipMemcpyHostToDevice, n->stream));
            HIPCHK(hipStreamSynchronize(n->stream));
        }
        CHK(prior_scalars_range(n, c0, l0, e->cam_prior_lambda || !rule ? 1.0 : wf * wf, e->lmk_prior_lambda || !rule ? 1.0 : wf * wf,
                                e->lmk_prior_lambda || !rule));
    }

    // 8. update_all_beliefs over the result
    CHK(gbp_ba_update_beliefs(n));
    HIPCHK(hipStreamSynchronize(n->stream));
    return GBP_OK;
}

// a list of the step onto its 0 / 1 words[size]: ids in [0, limit), none twice (an empty list leaves the words empty)
int list_words(const char *what, int32_t count, const int32_t *ids, int limit, size_t size, std::vector<int> &words)
{
    if (count) words.assign(size, 0);
    for (int i = 0; i < count; ++i) {
        const int v = ids[i];
        if (v < 0 || v >= limit) return fail(GBP_EINVAL, "%s %d (entry %d of its list) is outside [0,%d)", what, v, i, limit);
        if (words[(size_t)v]) return fail(GBP_EINVAL, "%s %d (entry %d of its list) is listed twice", what, v, i);
        words[(size_t)v] = 1;
    }
    return GBP_OK;
}

// The engine: the lists are checked, the result is built beside the handle (window_into), the scratch goes; on success the maps go out
// (sizes from BEFORE the call, NULL to skip) and the result becomes the handle, on failure the half-built graph goes and the handle is
// what it was.  The caller has checked its own arguments and answered a step that changes nothing.
int run_step(gbp_ba *h, const Step &st, const gbp_ba_window_maps_t &out)
{
    const Params &op = h->p;
    const gbp_ba_ext_t *e = st.e;
    const int dC = e->n_new_cams, dL = e->n_new_lmks, dF = e->n_new_factors;
    const int Cu = op.C + dC, Lu = op.L + dL;
    gbp_ba *n = nullptr;
    std::vector<void *> scratch;
    std::vector<int> maps;
    int rc;
    try {
        Words wd;
        CHK(list_words("factor", st.n_gone, st.gone, op.F, (size_t)op.F, wd.gone));
        CHK(list_words("camera", st.n_cam, st.cam, op.C, (size_t)Cu, wd.cam));
        CHK(list_words("landmark", st.n_lmk, st.lmk, op.L, (size_t)Lu, wd.lmk));
        if (st.all_listed && (st.n_gone >= op.F || st.n_cam >= op.C || st.n_lmk >= op.L)) return fail(GBP_EINVAL, "%s", st.all_listed);
        if (!(e->flags & GBP_FLAG_DEVICE_INPUT)) {            // host ids: checked here, before anything is allocated
            for (int i = 0; i < dF; ++i) {
                const int c = e->cam_idx[i], l = e->lmk_idx[i];
                if (c < 0 || c >= Cu || l < 0 || l >= Lu)
                    return fail(GBP_EINVAL, "new observation %d references a camera outside [0,%d) or a landmark outside [0,%d)", i, Cu, Lu);
                if (st.n_cam && wd.cam[(size_t)c]) return fail(GBP_EINVAL, "new observation %d references camera %d, which this step retires", i, c);
                if (st.n_lmk && wd.lmk[(size_t)l]) return fail(GBP_EINVAL, "new observation %d references landmark %d, which this step lets go of", i, l);
            }
        }
        HIPCHK(hipStreamSynchronize(h->stream));
        n = new (std::nothrow) gbp_ba;
        if (!n) return fail(GBP_ENOMEM, "out of host memory");
        rc = window_into(h, n, st, wd, scratch, maps);
    } catch (const std::bad_alloc &) {
        rc = fail(GBP_ENOMEM, "out of host memory");
    }
    for (void *q : scratch) (void)hipFreeAsync(q, h->stream);
    (void)hipStreamSynchronize(h->stream);
    if (rc != GBP_OK) return n ? graft_abandon(n, rc) : rc;
    const size_t C0 = (size_t)op.C, L0 = (size_t)op.L, F0 = (size_t)op.F;     // (h->p is the old graph's until the swap)
    const int *m = maps.data();
    if (out.cam_old_to_new) std::memcpy(out.cam_old_to_new, m, C0 * sizeof(int32_t));
    if (out.new_cam_ids) std::memcpy(out.new_cam_ids, m + C0, (size_t)dC * sizeof(int32_t));
    if (out.lmk_old_to_new) std::memcpy(out.lmk_old_to_new, m + Cu, L0 * sizeof(int32_t));
    if (out.new_lmk_ids) std::memcpy(out.new_lmk_ids, m + Cu + L0, (size_t)dL * sizeof(int32_t));
    if (out.factor_old_to_new) std::memcpy(out.factor_old_to_new, m + Cu + Lu, F0 * sizeof(int32_t));
    if (out.new_factor_ids) std::memcpy(out.new_factor_ids, m + Cu + Lu + F0, (size_t)dF * sizeof(int32_t));
    graft_swap(h, n);
    return GBP_OK;
}

}  // namespace

extern "C" {

int gbp_ba_window_step(gbp_ba_t *h, const gbp_ba_window_t *step, const gbp_ba_window_maps_t *out)
{
    ENTER(h);
    if (!step) return fail(GBP_EINVAL, "null argument");
    CHK(live_and_whole(h, "take a window step"));
    if (step->n_cull < 0 || step->n_retire_cams < 0 || step->n_retire_lmks < 0) return fail(GBP_EINVAL, "negative count");
    if (step->n_cull && !step->cull_ids) return fail(GBP_EINVAL, "null factor list");
    if (step->n_retire_cams && !step->retire_cam_ids) return fail(GBP_EINVAL, "null camera list");
    if (step->n_retire_lmks && !step->retire_lmk_ids) return fail(GBP_EINVAL, "null landmark list");
    if (step->lmk_mode != GBP_RETIRE_FOLD && step->lmk_mode != GBP_RETIRE_DROP)
        return fail(GBP_EINVAL, "mode %d is neither GBP_RETIRE_FOLD nor GBP_RETIRE_DROP", step->lmk_mode);
    const gbp_ba_ext_t *e = step->batch ? step->batch : &no_batch;
    CHK(sound_batch(h->p, e));
    const Params &op = h->p;
    const int dC = e->n_new_cams, dL = e->n_new_lmks, dF = e->n_new_factors;
    const gbp_ba_window_maps_t maps = out ? *out : gbp_ba_window_maps_t{};
    if (!step->n_cull && !step->n_retire_cams && !step->n_retire_lmks && !dC && !dL && !dF) {      // an empty step: nothing changes
        graft_identity_maps(op, maps.cam_old_to_new, maps.lmk_old_to_new, maps.factor_old_to_new);
        return GBP_OK;
    }
    return run_step(h, Step{step->n_cull, step->n_retire_cams, step->n_retire_lmks, step->cull_ids, step->retire_cam_ids, step->retire_lmk_ids,
                            step->lmk_mode == GBP_RETIRE_FOLD, e, false, nullptr, "this window step leaves no factor"}, maps);
}

// ---- the three calls that only shrink: a step with one list and no batch ---------------------------------------------------------------
// A culled factor was WRONG: what it told its camera and its landmark vanishes, nothing is folded.  Variables left without a factor go.
int gbp_ba_cull(gbp_ba_t *h, int32_t n_factors, const int32_t *factor_ids, int32_t *cam_old_to_new, int32_t *lmk_old_to_new, int32_t *factor_old_to_new)
{
    ENTER(h);
    CHK(live_and_whole(h, "cull factors"));
    if (n_factors < 0) return fail(GBP_EINVAL, "negative count");
    if (n_factors && !factor_ids) return fail(GBP_EINVAL, "null factor list");
    if (n_factors == 0) {                                     // nothing goes: nothing changes
        graft_identity_maps(h->p, cam_old_to_new, lmk_old_to_new, factor_old_to_new);
        return GBP_OK;
    }
    return run_step(h, Step{n_factors, 0, 0, factor_ids, nullptr, nullptr, false, &no_batch, false, "culling every factor leaves no factor",
                            "culling these factors leaves no factor"}, {cam_old_to_new, lmk_old_to_new, factor_old_to_new, nullptr, nullptr, nullptr});
}

// Retired cameras leave with all their factors; what those told their landmarks is folded into the landmarks' priors (GBP's own
// marginalisation), landmarks left without a factor go.  Every other camera stays, with or without a factor.
int gbp_ba_retire(gbp_ba_t *h, int32_t n_cams, const int32_t *cam_ids, int32_t *cam_old_to_new, int32_t *lmk_old_to_new, int32_t *factor_old_to_new)
{
    ENTER(h);
    CHK(live_and_whole(h, "retire cameras"));
    if (n_cams < 0) return fail(GBP_EINVAL, "negative count");
    if (n_cams && !cam_ids) return fail(GBP_EINVAL, "null camera list");
    if (n_cams == 0) {                                        // nothing goes: nothing changes
        graft_identity_maps(h->p, cam_old_to_new, lmk_old_to_new, factor_old_to_new);
        return GBP_OK;
    }
    return run_step(h, Step{0, n_cams, 0, nullptr, cam_ids, nullptr, false, &no_batch, true, "retiring every camera leaves no factor",
                            "retiring these cameras leaves no factor"}, {cam_old_to_new, lmk_old_to_new, factor_old_to_new, nullptr, nullptr, nullptr});
}

// A listed landmark leaves with all its factors; mode FOLD: what they told their cameras is folded into the cameras' priors, mode DROP:
// it vanishes (the landmarks were bad).  Variables left without a factor go.
int gbp_ba_retire_landmarks(gbp_ba_t *h, int32_t n_lmks, const int32_t *lmk_ids, int32_t mode, int32_t *cam_old_to_new, int32_t *lmk_old_to_new,
                            int32_t *factor_old_to_new)
{
    ENTER(h);
    CHK(live_and_whole(h, "retire landmarks"));
    if (n_lmks < 0) return fail(GBP_EINVAL, "negative count");
    if (n_lmks && !lmk_ids) return fail(GBP_EINVAL, "null landmark list");
    if (mode != GBP_RETIRE_FOLD && mode != GBP_RETIRE_DROP) return fail(GBP_EINVAL, "mode %d is neither GBP_RETIRE_FOLD nor GBP_RETIRE_DROP", mode);
    if (n_lmks == 0) {                                        // nothing goes: nothing changes
        graft_identity_maps(h->p, cam_old_to_new, lmk_old_to_new, factor_old_to_new);
        return GBP_OK;
    }
    return run_step(h, Step{0, 0, n_lmks, nullptr, nullptr, lmk_ids, mode == GBP_RETIRE_FOLD, &no_batch, false, "retiring every landmark leaves no factor",
                            "retiring these landmarks leaves no factor"}, {cam_old_to_new, lmk_old_to_new, factor_old_to_new, nullptr, nullptr, nullptr});
}

}  // extern "C"
