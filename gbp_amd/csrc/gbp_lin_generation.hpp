// gbp_lin_generation.hpp -- host code only: what gbp_lin_create, gbp_lin_extend and gbp_lin_shrink (and the two calls that grow and
// shrink a nonlinear handle, gbp_lin_extend_nonlinear / gbp_lin_shrink_nonlinear) share.  Each of them builds a complete
// new GENERATION of the handle's graph arrays while the old one is only read, synchronises, and commits:
//   LinScratch       the device memory of one call: `keep` becomes the handle's at the commit, `temp` goes with the call
//   LinGen           the arrays of one generation; lin_gen_alloc is the one place that says which they are and how large each is
//   lin_gen_commit   the one swap: frees the generation that is replaced, drops what a change of N or F invalidates, installs the new one
// and the host routines that pack the caller's factors and priors and that check a list of losses.  The builds themselves stay with
// their entry points: they are different algorithms (upload, sort-and-merge, scan-and-gather).
#pragma once
#include "gbp_lin_handle.hpp"

#include <cmath>

// `keep` becomes the handle's at lin_gen_commit; what is still held when the call ends is freed, so a failed build needs no clean-up
// beyond a synchronisation of the stream BEFORE this goes out of scope (its kernels and copies may still be running)
struct LinScratch {
    std::vector<void *> keep, temp;
    LinScratch() = default;
    LinScratch(const LinScratch &) = delete;
    LinScratch &operator=(const LinScratch &) = delete;
    ~LinScratch() { release(keep); release(temp); }
    template <typename T> int get(T **out, size_t n, bool kept)
    {
        void *q = nullptr;
        LHIPCHK(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)));
        (kept ? keep : temp).push_back(q);
        *out = static_cast<T *>(q);
        return GBP_OK;
    }
    static void release(std::vector<void *> &v) { for (void *q : v) (void)hipFree(q); v.clear(); }
};

// the arrays that replace the handle's (LinParams, LinRobust and LinNonlin say what each holds)
struct LinGen {
    int N = 0, F = 0;
    int *va = nullptr, *vb = nullptr, *vptr = nullptr, *vadj = nullptr, *epos_a = nullptr, *epos_b = nullptr;
    double *feta = nullptr, *flam = nullptr, *fconst = nullptr, *msg_a = nullptr, *msg_b = nullptr, *bel = nullptr, *prior = nullptr, *vmsg = nullptr;
    double *d_red = nullptr;                        // nullptr: the handle's stays
    int red_blocks = 0;
    bool robust = false;                            // losses are set after the commit: the five arrays below exist
    int *loss = nullptr, *flag = nullptr;
    double *thr = nullptr, *nvar = nullptr, *w = nullptr;
    bool nonlinear = false;                         // the handle is nonlinear: the five per-factor arrays below exist
    double *meas = nullptr, *sinfo = nullptr, *linpoint = nullptr, *fdamp = nullptr;
    int *iters = nullptr;
};

// Every array of a generation of N1 variables and F1 factors, nothing written yet.  grow_red: a larger d_red where ceil(F1 / 256)
// exceeds what the handle has (a new handle has none).  nonlinear: the per-factor arrays of LinNonlin too (a nonlinear handle has d = 3).
inline int lin_gen_alloc(gbp_lin *h, LinScratch &mem, LinGen &g, int N1, int F1, bool robust, bool grow_red, bool nonlinear = false)
{
    const size_t D = (size_t)h->D, P = D * (D + 1) / 2, P2 = D * (2 * D + 1), R = D + P, REC = D + P + D, N = (size_t)N1, F = (size_t)F1;
    g.N = N1; g.F = F1; g.robust = robust;
    LCHK(mem.get(&g.va, F, true)); LCHK(mem.get(&g.vb, F, true));
    LCHK(mem.get(&g.feta, 2 * D * F, true)); LCHK(mem.get(&g.flam, P2 * F, true)); LCHK(mem.get(&g.fconst, F, true));
    LCHK(mem.get(&g.msg_a, R * F, true)); LCHK(mem.get(&g.msg_b, R * F, true));
    LCHK(mem.get(&g.bel, N * REC, true)); LCHK(mem.get(&g.prior, N * R, true));
    LCHK(mem.get(&g.vptr, N + 1, true)); LCHK(mem.get(&g.vadj, 2 * F, true));
    LCHK(mem.get(&g.epos_a, F, true)); LCHK(mem.get(&g.epos_b, F, true));
    LCHK(mem.get(&g.vmsg, 2 * F * R, true));
    const int red_blocks = std::max(1, (F1 + 255) / 256);
    if (grow_red && red_blocks > h->red_blocks) {
        LCHK(mem.get(&g.d_red, (size_t)red_blocks, true));
        g.red_blocks = red_blocks;
    }
    if (robust) {
        LCHK(mem.get(&g.loss, F, true)); LCHK(mem.get(&g.thr, F, true)); LCHK(mem.get(&g.nvar, F, true));
        LCHK(mem.get(&g.w, F, true)); LCHK(mem.get(&g.flag, F, true));
    }
    g.nonlinear = nonlinear;
    if (nonlinear) {
        LCHK(mem.get(&g.meas, NL_M * F, true)); LCHK(mem.get(&g.sinfo, NL_M * F, true)); LCHK(mem.get(&g.linpoint, 2 * NL_D * F, true));
        LCHK(mem.get(&g.iters, F, true)); LCHK(mem.get(&g.fdamp, F, true));
    }
    return GBP_OK;
}

// The MAP and marginal workspaces are sized by N and F: the next solve re-makes them.
inline void lin_drop_solvers(gbp_lin *h)
{
    if (h->map_alloc) {
        const LinMap &m = h->map;
        for (const void *q : {(const void *)m.ldl, (const void *)m.jeta, (const void *)m.x, (const void *)m.r, (const void *)m.z, (const void *)m.p, (const void *)m.q,
                              (const void *)m.ebuf, (const void *)m.pq_part, (const void *)m.rz_part, (const void *)m.rr_part})
            lin_free(h, q);
        h->map = LinMap{};
    }
    h->map_alloc = h->map_ready = h->map_solved = false;
    h->map_eta_norm = 0.0;
    if (h->marg_ready) {                                    // the staging of the outputs does not depend on N or F and stays
        LinMarg &m = h->marg;
        for (const void *q : {(const void *)m.x, (const void *)m.r, (const void *)m.z, (const void *)m.p, (const void *)m.q, (const void *)m.ebuf, (const void *)m.pq_part,
                              (const void *)m.rz_part, (const void *)m.rr_part})
            lin_free(h, q);
        m.x = m.r = m.z = m.p = m.q = m.ebuf = m.pq_part = m.rz_part = m.rr_part = nullptr;
        h->marg_ready = false;
    }
    // gbp_lin_iterate_until's partials are one per block of the belief and energy stages; its stop word and trace buffer stay
    lin_free(h, h->until.bel_part); lin_free(h, h->until.en_part);
    h->until.bel_part = h->until.en_part = nullptr;
    h->until.nbel = h->until.nen = 0;
}

// The swap, after the synchronisation that ends the build of `g`: nothing here can fail.  The arrays that are replaced are freed and
// taken out of `allocs` (a handle rebuilt a thousand times holds one generation) -- the robust ones of a handle whose losses were
// cleared too: they are stale and not carried -- and the call's `temp` with them; `keep` becomes the handle's.  A nonlinear handle's
// five per-factor arrays go the same way, and LinNonlin::feta / flam -- what the relinearise stage writes -- are re-pointed at the new
// generation's factor arrays: the old ones are freed here.  The per-sweep counts buffer does not depend on F and stays.
inline void lin_gen_commit(gbp_lin *h, LinScratch &mem, const LinGen &g)
{
    LinScratch::release(mem.temp);
    LinParams &p = h->p;
    for (const void *q : {(const void *)p.va, (const void *)p.vb, (const void *)p.feta, (const void *)p.flam, (const void *)p.fconst, (const void *)p.msg_a,
                          (const void *)p.msg_b, (const void *)p.bel, (const void *)p.prior, (const void *)p.vptr, (const void *)p.vadj, (const void *)p.vmsg,
                          (const void *)p.epos_a, (const void *)p.epos_b})
        lin_free(h, q);
    if (h->rob_alloc)
        for (const void *q : {(const void *)h->rob.loss, (const void *)h->rob.thr, (const void *)h->rob.nvar, (const void *)h->rob.w, (const void *)h->rob.flag}) lin_free(h, q);
    if (g.nonlinear)
        for (const void *q : {(const void *)h->nl.meas, (const void *)h->nl.sinfo, (const void *)h->nl.linpoint, (const void *)h->nl.iters, (const void *)h->nl.fdamp}) lin_free(h, q);
    lin_drop_solvers(h);
    if (g.d_red) { lin_free(h, h->d_red); h->d_red = g.d_red; h->red_blocks = g.red_blocks; }
    h->allocs.insert(h->allocs.end(), mem.keep.begin(), mem.keep.end());
    mem.keep.clear();
    p.N = g.N; p.F = g.F;
    p.va = g.va; p.vb = g.vb; p.feta = g.feta; p.flam = g.flam; p.fconst = g.fconst; p.msg_a = g.msg_a; p.msg_b = g.msg_b;
    p.bel = g.bel; p.prior = g.prior; p.vptr = g.vptr; p.vadj = g.vadj; p.vmsg = g.vmsg; p.epos_a = g.epos_a; p.epos_b = g.epos_b;
    p.w = g.robust ? g.w : nullptr;
    h->rob = g.robust ? LinRobust{g.loss, g.thr, g.nvar, g.w, g.flag} : LinRobust{};
    h->rob_alloc = g.robust;
    if (g.nonlinear) {
        LinNonlin &nl = h->nl;
        nl.meas = g.meas; nl.sinfo = g.sinfo; nl.linpoint = g.linpoint; nl.iters = g.iters; nl.fdamp = g.fdamp;
        nl.feta = g.feta; nl.flam = g.flam;
    }
}

// ---- host routines without a HIP call (tests/hostmath/lin_pack_shim.hip runs them on a CPU) ----

// index of (i, j), i <= j, in the packed upper triangle of a symmetric n x n matrix
inline int lin_packed_at(int n, int i, int j) { return i * n - (i * (i - 1)) / 2 + (j - i); }

// `count` factors, eta [count][2D] and lam [count][2D][2D] row-major -> SoA rows with stride `count`: out_eta [2D][count],
// out_lam [D(2D+1)][count], the upper triangle packed
inline void lin_pack_factors(int D, int count, const double *eta, const double *lam, double *out_eta, double *out_lam)
{
    const int D2 = 2 * D;
    for (int f = 0; f < count; ++f)
        for (int i = 0; i < D2; ++i) {
            out_eta[(size_t)i * count + f] = eta[(size_t)f * D2 + i];
            for (int j = i; j < D2; ++j) out_lam[(size_t)lin_packed_at(D2, i, j) * count + f] = lam[((size_t)f * D2 + i) * D2 + j];
        }
}

// `count` priors, eta [count][D] and lam [count][D][D] row-major -> records out [count][D + D(D+1)/2]: eta, then the upper triangle packed
inline void lin_pack_priors(int D, int count, const double *eta, const double *lam, double *out)
{
    const int R = D + D * (D + 1) / 2;
    for (int v = 0; v < count; ++v)
        for (int i = 0; i < D; ++i) {
            out[(size_t)v * R + i] = eta[(size_t)v * D + i];
            for (int j = i; j < D; ++j) out[(size_t)v * R + D + lin_packed_at(D, i, j)] = lam[((size_t)v * D + i) * D + j];
        }
}

// The rules for a list of `count` losses (include/gbp_lin.h, gbp_lin_set_robust); `prefix` names a factor in the message.  Refused, in
// this order: thr == NULL; then per factor an unknown loss, a threshold that is not positive and finite (0, negative, NaN, inf), the
// constant loss with nvar == NULL, a noise variance that is not positive and finite.  Thresholds and variances of factors at NONE are
// not looked at.  *any: some factor has a loss other than NONE.
inline int lin_check_losses(const int32_t *loss, const double *thr, const double *nvar, int count, const char *prefix, bool *any)
{
    *any = false;
    if (!thr) return set_error(GBP_EINVAL, "threshold is NULL");
    for (int f = 0; f < count; ++f) {
        const int l = loss[f];
        if (l != GBP_LIN_LOSS_NONE && l != GBP_LIN_LOSS_HUBER && l != GBP_LIN_LOSS_CONSTANT) return set_error(GBP_EINVAL, "%s %d: unknown loss %d", prefix, f, l);
        if (l == GBP_LIN_LOSS_NONE) continue;
        *any = true;
        if (!(thr[f] > 0.0) || !std::isfinite(thr[f])) return set_error(GBP_EINVAL, "%s %d: the threshold must be positive", prefix, f);
        if (l == GBP_LIN_LOSS_CONSTANT) {
            if (!nvar) return set_error(GBP_EINVAL, "%s %d has the constant loss: noise_var must be given", prefix, f);
            if (!(nvar[f] > 0.0) || !std::isfinite(nvar[f])) return set_error(GBP_EINVAL, "%s %d: noise_var must be positive", prefix, f);
        }
    }
    return GBP_OK;
}
