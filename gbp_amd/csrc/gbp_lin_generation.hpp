// gbp_lin_generation.hpp -- host code only: what gbp_lin_create, gbp_lin_extend and gbp_lin_shrink (and the two calls that grow and
// shrink a nonlinear handle, gbp_lin_extend_nonlinear / gbp_lin_shrink_nonlinear) share.  Each of them builds a complete
// new GENERATION of the handle's graph arrays while the old one is only read, synchronises, and commits:
//   LinScratch        the device memory of one call: `keep` becomes the handle's at the commit, `temp` goes with the call
//   LinGen            the arrays of one generation, in the handle's own structs (LinParams, LinRobust, LinNonlin)
//   lin_gen_columns   the one list of the arrays with stride F: rows, the value an appended factor starts with, the handle's old array.
//                     lin_gen_alloc, lin_gen_commit, the restrides of extend, the gathers of shrink and the first allocations of
//                     gbp_lin_set_robust / gbp_lin_set_nonlinear all walk it; lin_gen_others lists the five arrays of another stride
//   lin_gen_commit    the one swap: frees the generation that is replaced, drops what a change of N or F invalidates, installs the new one
// and the host routines that pack the caller's factors, priors and measurements and that check a list of losses or of measurements.
// The builds themselves stay with their entry points: they are different algorithms (upload, sort-and-merge, scan-and-gather).
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

// rows of the SoA arrays and lengths of the records of a handle of d dofs (LinParams says which is which):
// 2d; d(2d+1), packed upper 2d x 2d; d + d(d+1)/2, a message or a prior; that + d, a belief
struct LinRows { int eta2, lam2, msg, rec; };
inline LinRows lin_rows(int D) { return {2 * D, D * (2 * D + 1), D + D * (D + 1) / 2, D + D * (D + 1) / 2 + D}; }

enum LinGroup { LIN_GRAPH, LIN_ROBUST, LIN_NONLIN };    // whose arrays: LinParams, LinRobust, LinNonlin
enum LinCol { LC_VA, LC_VB, LC_FETA, LC_FLAM, LC_FCONST, LC_MSG_A, LC_MSG_B, LC_EPOS_A, LC_EPOS_B, LC_LOSS, LC_THR, LC_NVAR, LC_W, LC_FLAG,
              LC_MEAS, LC_SINFO, LC_LINPOINT, LC_ITERS, LC_FDAMP, LC_COUNT };

// What a factor holds before anything was said or computed about it: no loss (its threshold and variance are then not read), weight 1,
// not flagged; and until the linearise pass (NL_INIT, gbp_lin_nonlin.hpp) writes the last three: a linearisation point of 0,
// iters_since_relin 1, damping 0.  gbp_lin_set_robust and lin_gen_columns (the factors appended by an extend) both start from these.
constexpr int LIN_NEW_LOSS = GBP_LIN_LOSS_NONE, LIN_NEW_FLAG = 0, LIN_NEW_ITERS = 1;
constexpr double LIN_NEW_THR = 1.0, LIN_NEW_NVAR = 1.0, LIN_NEW_W = 1.0, LIN_NEW_SINFO = 1.0, LIN_NEW_FDAMP = 0.0;

// the arrays that replace the handle's.  Of `p`, damping and w are the commit's to set; of `nl`, only the five per-factor arrays are used
struct LinGen {
    LinParams p{};
    LinRobust rob{};
    LinNonlin nl{};
    double *d_red = nullptr;                        // nullptr: the handle's stays
    int red_blocks = 0;
    bool robust = false;                            // losses are set after the commit: rob's arrays exist
    bool nonlinear = false;                         // the handle is nonlinear: nl's per-factor arrays exist
    bool has(LinGroup grp) const { return grp == LIN_GRAPH || (grp == LIN_ROBUST ? robust : nonlinear); }
};

// a generation's arrays are its build's to write until the commit, whatever the kernels that read them later are promised
template <typename T> T *lin_mut(const T *q) { return const_cast<T *>(q); }

// One array [rows][F] of T.  old: the handle's as a build may read it, nullptr where the handle has none or where its copy is stale;
// owned: the handle's as the commit frees it, nullptr where the handle has none; neu: the generation's; fill: what a factor appended
// by an extend starts with where nothing is uploaded for it
template <typename T> struct LinColumn {
    LinCol id;
    LinGroup group;
    const T *old, *owned;
    T *&neu;
    int rows;
    T fill;
};

// Every array with stride F, whether `g` has its group or not (LinGen::has): visit(LinColumn<int or double>).  A handle whose losses
// were cleared keeps stale losses and weights in its robust arrays: its old factors are at NONE, so `old` is nullptr and the fill applies.
// The three nonlinear arrays wider than a row take their rows from the handle's model (lin_model_rows / lin_model_dofs); a handle that
// is not nonlinear yet has none, and the model its caller is about to install is passed as `model` (gbp_lin_set_nonlinear).
template <typename V>
void lin_gen_columns(const gbp_lin *h, LinGen &g, V &&visit, int model = 0)
{
    const LinRows r = lin_rows(h->D);
    if (h->nonlinear) model = h->nl.model;
    const int nl_m = lin_model_rows(model), nl_d = lin_model_dofs(model);
    const LinParams &o = h->p;
    const LinRobust orob = h->rob_alloc ? h->rob : LinRobust{};
    const LinNonlin onl = h->nonlinear ? h->nl : LinNonlin{};
    auto col = [&](LinCol id, LinGroup grp, const auto *owned, auto *&neu, int rows, auto fill) {
        using T = decltype(fill);
        visit(LinColumn<T>{id, grp, grp == LIN_ROBUST && !o.w ? nullptr : owned, owned, const_cast<T *&>(neu), rows, fill});
    };
    col(LC_VA, LIN_GRAPH, o.va, g.p.va, 1, 0); col(LC_VB, LIN_GRAPH, o.vb, g.p.vb, 1, 0);
    col(LC_FETA, LIN_GRAPH, o.feta, g.p.feta, r.eta2, 0.0); col(LC_FLAM, LIN_GRAPH, o.flam, g.p.flam, r.lam2, 0.0);
    col(LC_FCONST, LIN_GRAPH, o.fconst, g.p.fconst, 1, 0.0);
    col(LC_MSG_A, LIN_GRAPH, o.msg_a, g.p.msg_a, r.msg, 0.0); col(LC_MSG_B, LIN_GRAPH, o.msg_b, g.p.msg_b, r.msg, 0.0);
    col(LC_EPOS_A, LIN_GRAPH, o.epos_a, g.p.epos_a, 1, 0); col(LC_EPOS_B, LIN_GRAPH, o.epos_b, g.p.epos_b, 1, 0);
    col(LC_LOSS, LIN_ROBUST, orob.loss, g.rob.loss, 1, LIN_NEW_LOSS); col(LC_THR, LIN_ROBUST, orob.thr, g.rob.thr, 1, LIN_NEW_THR);
    col(LC_NVAR, LIN_ROBUST, orob.nvar, g.rob.nvar, 1, LIN_NEW_NVAR); col(LC_W, LIN_ROBUST, orob.w, g.rob.w, 1, LIN_NEW_W);
    col(LC_FLAG, LIN_ROBUST, orob.flag, g.rob.flag, 1, LIN_NEW_FLAG);
    col(LC_MEAS, LIN_NONLIN, onl.meas, g.nl.meas, nl_m, 0.0); col(LC_SINFO, LIN_NONLIN, onl.sinfo, g.nl.sinfo, nl_m, LIN_NEW_SINFO);
    col(LC_LINPOINT, LIN_NONLIN, onl.linpoint, g.nl.linpoint, 2 * nl_d, 0.0);
    col(LC_ITERS, LIN_NONLIN, onl.iters, g.nl.iters, 1, LIN_NEW_ITERS); col(LC_FDAMP, LIN_NONLIN, onl.fdamp, g.nl.fdamp, 1, LIN_NEW_FDAMP);
}

// The arrays of a generation with another stride, for N = g.p.N and F = g.p.F: visit(the handle's, the generation's, elements)
template <typename V>
void lin_gen_others(const gbp_lin *h, LinGen &g, V &&visit)
{
    const LinRows r = lin_rows(h->D);
    const size_t N = (size_t)g.p.N, F = (size_t)g.p.F;
    visit(h->p.bel, g.p.bel, N * r.rec); visit(h->p.prior, const_cast<double *&>(g.p.prior), N * r.msg);
    visit(h->p.vptr, const_cast<int *&>(g.p.vptr), N + 1); visit(h->p.vadj, const_cast<int *&>(g.p.vadj), 2 * F);
    visit(h->p.vmsg, g.p.vmsg, 2 * F * r.msg);
}

// Every array of a generation of N1 variables and F1 factors, nothing written yet: the graph's, and those of the groups that g.robust
// and g.nonlinear name (set by the caller).  d_red too where ceil(F1 / 256) exceeds what the handle has: a new handle has none, an
// extend may pass it, and a shrink cannot (F1 <= F, and the handle holds at least ceil(F / 256)).
inline int lin_gen_alloc(gbp_lin *h, LinScratch &mem, LinGen &g, int N1, int F1)
{
    g.p.N = N1; g.p.F = F1;
    int rc = GBP_OK;
    lin_gen_columns(h, g, [&](auto c) { if (rc == GBP_OK && g.has(c.group)) rc = mem.get(&c.neu, (size_t)c.rows * F1, true); });
    lin_gen_others(h, g, [&](const auto *, auto *&neu, size_t n) { if (rc == GBP_OK) rc = mem.get(&neu, n, true); });
    LCHK(rc);
    const int red_blocks = std::max(1, (F1 + 255) / 256);
    if (red_blocks > h->red_blocks) {
        LCHK(mem.get(&g.d_red, (size_t)red_blocks, true));
        g.red_blocks = red_blocks;
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
    if (h->gn.alloc) {                                      // gbp_lin_solve_map_nonlinear's arrays: the next call re-makes them
        const LinGn &g = h->gn;
        for (const void *q : {(const void *)g.feta, (const void *)g.flam, (const void *)g.prior, (const void *)g.x, (const void *)g.e_part, (const void *)g.v_part,
                              (const void *)g.out, (const void *)g.w, (const void *)g.flag, (const void *)g.xs, (const void *)g.w_part, (const void *)g.count,
                              (const void *)g.rout})
            lin_free(h, q);                                 // (the last six are null unless the robust solve ran)
        h->gn = LinGn{};
    }
    // gbp_lin_iterate_until's partials are one per block of the belief and energy stages; its stop word and trace buffer stay
    lin_free(h, h->until.bel_part); lin_free(h, h->until.en_part);
    h->until.bel_part = h->until.en_part = nullptr;
    h->until.nbel = h->until.nen = 0;
}

// LinNonlin::feta / flam -- what the relinearise stage writes -- are the handle's own factor arrays: set here, by whoever changes either
inline void lin_nl_point(gbp_lin *h) { h->nl.feta = const_cast<double *>(h->p.feta); h->nl.flam = const_cast<double *>(h->p.flam); }

// The swap, after the synchronisation that ends the build of `g`: nothing here can fail.  Every array that is replaced is freed and
// taken out of `allocs` (a handle rebuilt a thousand times holds one generation) -- the robust ones of a handle whose losses were
// cleared too: they are stale and not carried -- and the call's `temp` with them; `keep` becomes the handle's.  The parts of `g` are
// installed whole; what does not belong to a generation stays as the handle has it: the damping, the nonlinear settings, and the
// per-sweep counts buffers, which do not depend on F.
inline void lin_gen_commit(gbp_lin *h, LinScratch &mem, LinGen &g)
{
    LinScratch::release(mem.temp);
    lin_gen_columns(h, g, [&](auto c) { lin_free(h, c.owned); });
    lin_gen_others(h, g, [&](const auto *owned, auto *&, size_t) { lin_free(h, owned); });
    lin_drop_solvers(h);
    if (g.d_red) { lin_free(h, h->d_red); h->d_red = g.d_red; h->red_blocks = g.red_blocks; }
    h->allocs.insert(h->allocs.end(), mem.keep.begin(), mem.keep.end());
    mem.keep.clear();
    g.p.damping = h->p.damping;
    g.p.w = g.robust ? g.rob.w : nullptr;
    h->p = g.p;
    h->rob = g.rob;                                 // all nullptr where the generation has no losses
    h->rob_alloc = g.robust;
    if (g.nonlinear) {
        const LinNonlin &o = h->nl;
        g.nl.counts = o.counts; g.nl.cap = o.cap; g.nl.rcounts = o.rcounts; g.nl.rcap = o.rcap;
        g.nl.beta = o.beta; g.nl.num_undamped = o.num_undamped; g.nl.min_linear = o.min_linear; g.nl.model = o.model;
        h->nl = g.nl;
        lin_nl_point(h);
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

// The rules for `count` measurements of `model` with their square-root informations, both [count][M] (include/gbp_lin.h,
// gbp_lin_set_nonlinear); `prefix` names a factor in the message.  Refused, entry by entry: a sqrt_info that is not positive and
// finite, then a measurement that is not finite; then, for GBP_LIN_MODEL_SE3_BETWEEN, factor by factor a measured rotation vector
// (the last three entries) whose norm is not below pi.
inline int lin_check_measurements(int model, const double *meas, const double *sinfo, int count, const char *prefix)
{
    const int M = lin_model_rows(model);
    for (size_t i = 0; i < (size_t)count * M; ++i) {
        if (!(sinfo[i] > 0.0) || !std::isfinite(sinfo[i])) return set_error(GBP_EINVAL, "%s %d: sqrt_info must be positive and finite", prefix, (int)(i / M));
        if (!std::isfinite(meas[i])) return set_error(GBP_EINVAL, "%s %d: the measurement must be finite", prefix, (int)(i / M));
    }
    if (model == GBP_LIN_MODEL_SE3_BETWEEN)
        for (int f = 0; f < count; ++f) {
            const double *w = meas + (size_t)f * M + 3;
            if (!(std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]) < 3.14159265358979323846))
                return set_error(GBP_EINVAL, "%s %d: the measured rotation vector must have a norm below pi", prefix, f);
        }
    return GBP_OK;
}

// the form from before there was a second model: GBP_LIN_MODEL_SE2_BETWEEN
inline int lin_check_measurements(const double *meas, const double *sinfo, int count, const char *prefix)
{
    return lin_check_measurements(GBP_LIN_MODEL_SE2_BETWEEN, meas, sinfo, count, prefix);
}

// the same two lists -> SoA rows with stride `count`: out_meas, out_sinfo [M][count]
inline void lin_pack_measurements(int M, int count, const double *meas, const double *sinfo, double *out_meas, double *out_sinfo)
{
    for (int f = 0; f < count; ++f)
        for (int k = 0; k < M; ++k) { out_meas[(size_t)k * count + f] = meas[(size_t)f * M + k]; out_sinfo[(size_t)k * count + f] = sinfo[(size_t)f * M + k]; }
}
inline void lin_pack_measurements(int count, const double *meas, const double *sinfo, double *out_meas, double *out_sinfo)
{
    lin_pack_measurements(lin_model_rows(GBP_LIN_MODEL_SE2_BETWEEN), count, meas, sinfo, out_meas, out_sinfo);
}
