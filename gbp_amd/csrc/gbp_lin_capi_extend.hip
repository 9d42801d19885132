// gbp_lin_capi_extend.hip -- gbp_lin_extend / gbp_lin_get_sizes of include/gbp_lin.h: appending variables and factors to a live handle
// (graph.var_nodes.append / graph.factors.append / adj_factors.append ndim_posegraph.py:67-88, update_all_beliefs gbp.py:56-58) without
// losing the messages (kernels and the placement argument: gbp_lin_extend.hpp).
//
// One call: validate on the host (only the appended part is looked at), pack and upload the new factors and priors, allocate EVERY new
// array (lin_gen_alloc), build them on the device from the old ones -- which are only read -- and synchronise; only then commit the
// new generation (lin_gen_commit, gbp_lin_generation.hpp) and, where the handle had beliefs, run the belief stage over all variables.
// Which arrays are re-strided, from which old array and with which fill for the appended factors is not said here: ext_build walks
// lin_gen_columns and looks up the uploaded rows of a column by its id.
// A failure before the commit frees what was allocated and leaves the handle as it was.  Host work and host <-> device traffic are
// proportional to dN and dF; no existing array crosses to the host.
//
// gbp_lin_extend_nonlinear is the same call on a handle of gbp_lin_set_nonlinear: the same build with zero eta_f, Lambda_f for the new
// factors (no uploaded rows: the fill) and the per-factor arrays of LinNonlin re-strided with the rest, the same commit, the belief stage, and then
// compute_factor (gbp.py:267-294) over the new factors alone (lin_nonlin_linearise, gbp_lin_capi_nonlin.hip).
#include "gbp_lin_extend.hpp"
#include "gbp_lin_generation.hpp"

#include <climits>

namespace gbp {
size_t sort_pairs_tmp_bytes(size_t n, int bits);                                              // gbp_sort.hip
int sort_pairs(void *tmp, size_t tmp_bytes, const int *keys_in, int *keys_out, const int *vals_in, int *vals_out, size_t n, int bits,
               hipStream_t stream);
}

using namespace gbp;

namespace {

// the appended part packed for upload: owned by gbp_lin_extend, so that these sources of asynchronous copies outlive the stream's work on
// every path, a failure in the middle of ext_build included
struct ExtHost {
    std::vector<int> a, b, loss;
    std::vector<double> feta, flam, fconst, prior, thr, nvar, meas, sinfo;
};

template <typename T>
int ext_upload(gbp_lin *h, LinScratch &mem, const T **out, const std::vector<T> &v)
{
    T *q = nullptr;
    LCHK(mem.get(&q, v.size(), false));
    if (!v.empty()) LHIPCHK(hipMemcpyAsync(q, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
    *out = q;
    return GBP_OK;
}

template <typename T>
void ext_restride(gbp_lin *h, const T *src, const T *tail, T *dst, int rows, int F, int dF, T fill)
{
    if (F + dF > 0)
        hipLaunchKernelGGL((k_ext_restride<T>), dim3((F + dF + EXT_BLOCK - 1) / EXT_BLOCK, rows), dim3(EXT_BLOCK), 0, h->stream, src, tail, dst, F, dF, fill);
}

int ext_blocks(size_t n) { return (int)((n + EXT_BLOCK - 1) / EXT_BLOCK); }

// the uploaded rows [row][dF] of the appended factors, by column; nullptr: the column's fill (lin_gen_columns) applies to them
struct ExtTails {
    const int *i[LC_COUNT] = {};
    const double *d[LC_COUNT] = {};
    const int *of(LinCol c, int) const { return i[c]; }
    const double *of(LinCol c, double) const { return d[c]; }
};

// everything up to and including the synchronisation after which nothing can fail: the new arrays, built on the device.  nl: the
// descriptor of gbp_lin_extend_nonlinear, whose sizes, ends and priors `d` repeats; its factors arrive as measurements, and eta_f,
// Lambda_f (the linearise pass after the commit writes them) and const_f have no uploaded rows: they start at their fill, zero
int ext_build(gbp_lin *h, const gbp_lin_extend_desc_t *d, const gbp_lin_extend_nonlinear_desc_t *nl, LinScratch &mem, ExtHost &host, LinGen &n)
{
    const LinParams &p = h->p;
    const LinRows r = lin_rows(h->D);
    const int R = r.msg, REC = r.rec;
    const int N = p.N, F = p.F, dN = d->n_new_vars, dF = d->n_new_factors, N1 = N + dN, F1 = F + dF;

    // ---- the appended part, packed as gbp_lin_create packs the whole: SoA rows [row][dF], packed upper triangles ----
    host.a.assign(d->var_a, d->var_a + dF); host.b.assign(d->var_b, d->var_b + dF);
    host.prior.resize((size_t)dN * R);
    lin_pack_priors(h->D, dN, d->prior_eta, d->prior_lam, host.prior.data());
    ExtTails t;
    LCHK(ext_upload(h, mem, &t.i[LC_VA], host.a)); LCHK(ext_upload(h, mem, &t.i[LC_VB], host.b));
    if (!nl) {
        host.feta.resize((size_t)r.eta2 * dF); host.flam.resize((size_t)r.lam2 * dF);
        lin_pack_factors(h->D, dF, d->factor_eta, d->factor_lam, host.feta.data(), host.flam.data());
        LCHK(ext_upload(h, mem, &t.d[LC_FETA], host.feta)); LCHK(ext_upload(h, mem, &t.d[LC_FLAM], host.flam));
        if (h->has_const) {
            host.fconst.assign(d->factor_const, d->factor_const + dF);
            LCHK(ext_upload(h, mem, &t.d[LC_FCONST], host.fconst));
        }
    } else {                                                // as gbp_lin_set_nonlinear packs the whole
        const int M = lin_model_rows(h->nl.model);
        host.meas.resize((size_t)M * dF); host.sinfo.resize((size_t)M * dF);
        lin_pack_measurements(M, dF, nl->measurement, nl->sqrt_info, host.meas.data(), host.sinfo.data());
        LCHK(ext_upload(h, mem, &t.d[LC_MEAS], host.meas)); LCHK(ext_upload(h, mem, &t.d[LC_SINFO], host.sinfo));
    }
    if (n.robust && d->loss && dF) {
        host.loss.assign(d->loss, d->loss + dF);
        host.thr.assign((size_t)dF, LIN_NEW_THR); host.nvar.assign((size_t)dF, LIN_NEW_NVAR);
        for (int f = 0; f < dF; ++f) {
            if (host.loss[f] != GBP_LIN_LOSS_NONE) host.thr[f] = d->threshold[f];
            if (host.loss[f] == GBP_LIN_LOSS_CONSTANT) host.nvar[f] = d->noise_var[f];
        }
        LCHK(ext_upload(h, mem, &t.i[LC_LOSS], host.loss)); LCHK(ext_upload(h, mem, &t.d[LC_THR], host.thr)); LCHK(ext_upload(h, mem, &t.d[LC_NVAR], host.nvar));
    }

    // ---- every allocation of the call, before the first kernel ----
    LCHK(lin_gen_alloc(h, mem, n, N1, F1));                 // d_red grows when ceil(F / 256) does
    int *keys = nullptr, *vals = nullptr, *keys_s = nullptr, *vals_s = nullptr, *enew = nullptr;
    void *sort_tmp = nullptr;
    int bits = 1;
    while (bits < 31 && (1 << bits) < N1) ++bits;
    const size_t sort_bytes = dF ? sort_pairs_tmp_bytes((size_t)2 * dF, bits) : 0;
    LCHK(mem.get(&keys, (size_t)2 * dF, false)); LCHK(mem.get(&vals, (size_t)2 * dF, false));
    LCHK(mem.get(&keys_s, (size_t)2 * dF, false)); LCHK(mem.get(&vals_s, (size_t)2 * dF, false));
    LCHK(mem.get(&enew, (size_t)2 * F, false));
    { char *q = nullptr; LCHK(mem.get(&q, sort_bytes, false)); sort_tmp = q; }

    // ---- factor-strided arrays: [row][F] -> [row][F1], the old factors' rows as they are (the fill where the handle has none to
    // give), then the uploaded rows or the fill.  epos_a / epos_b are not among them: the two edge kernels below write them ----
    lin_gen_columns(h, n, [&](auto c) {
        if (n.has(c.group) && c.id != LC_EPOS_A && c.id != LC_EPOS_B) ext_restride(h, c.old, t.of(c.id, c.fill), c.neu, c.rows, F, dF, c.fill);
    });
    LHIPCHK(hipGetLastError());
    // ---- variable-strided records: the old ones as they are, the new priors behind them; new belief records start at zero ----
    double *nbel = n.p.bel, *nprior = lin_mut(n.p.prior);
    int *nvptr = lin_mut(n.p.vptr), *nvadj = lin_mut(n.p.vadj), *nepos_a = lin_mut(n.p.epos_a), *nepos_b = lin_mut(n.p.epos_b);
    if (N) {
        LHIPCHK(hipMemcpyAsync(nbel, p.bel, (size_t)N * REC * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        LHIPCHK(hipMemcpyAsync(nprior, p.prior, (size_t)N * R * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    }
    if (dN) {
        LHIPCHK(hipMemsetAsync(nbel + (size_t)N * REC, 0, (size_t)dN * REC * sizeof(double), h->stream));
        LHIPCHK(hipMemcpyAsync(nprior + (size_t)N * R, host.prior.data(), host.prior.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    if (n.d_red) LHIPCHK(hipMemsetAsync(n.d_red, 0, (size_t)n.red_blocks * sizeof(double), h->stream));
    // ---- the CSR: new edges sorted by variable (stable: ascending factor id within one), merged behind each variable's old list ----
    const int *skeys = keys_s, *svals = vals_s;
    if (dF) {
        hipLaunchKernelGGL(k_ext_edges, dim3(ext_blocks((size_t)2 * dF)), dim3(EXT_BLOCK), 0, h->stream, t.i[LC_VA], t.i[LC_VB], F, dF, keys, vals);
        LHIPCHK(hipGetLastError());
        const int rc = sort_pairs(sort_tmp, sort_bytes, keys, keys_s, vals, vals_s, (size_t)2 * dF, bits, h->stream);
        if (rc != (int)hipSuccess) return set_error(GBP_EHIP, "sorting the new edges failed: %s", hipGetErrorString((hipError_t)rc));
    }
    hipLaunchKernelGGL(k_ext_vptr, dim3(ext_blocks((size_t)N1 + 1)), dim3(EXT_BLOCK), 0, h->stream, p.vptr, N, N1, skeys, 2 * dF, nvptr);
    if (F) {
        hipLaunchKernelGGL(k_ext_old_edges, dim3(ext_blocks((size_t)2 * F)), dim3(EXT_BLOCK), 0, h->stream, p.vptr, (const int *)nvptr, p.vadj, p.va, p.vb,
                           2 * F, nvadj, nepos_a, nepos_b, enew);
        lin_dispatch(h->D, [&](auto dd) {
            constexpr int RR = LinDims<decltype(dd)::value>::P + decltype(dd)::value;
            const size_t cnt = (size_t)2 * F * RR;
            hipLaunchKernelGGL((k_ext_move_vmsg<RR>), dim3(ext_blocks(cnt)), dim3(EXT_BLOCK), 0, h->stream, (const double *)p.vmsg, (const int *)enew, cnt, n.p.vmsg);
        });
    }
    if (dF)
        hipLaunchKernelGGL(k_ext_new_edges, dim3(ext_blocks((size_t)2 * dF * R)), dim3(EXT_BLOCK), 0, h->stream, p.vptr, N, skeys, svals, 2 * dF, R, nvadj,
                           nepos_a, nepos_b, n.p.vmsg);
    LHIPCHK(hipGetLastError());
    LHIPCHK(hipStreamSynchronize(h->stream));              // nothing below can fail
    return GBP_OK;
}

// nl: the call is gbp_lin_extend_nonlinear, whose factors arrive as measurements (checked by its entry point), not as eta_f, Lambda_f
int ext_validate(gbp_lin *h, const gbp_lin_extend_desc_t *d, bool nl)
{
    const int N = h->p.N, F = h->p.F, dN = d->n_new_vars, dF = d->n_new_factors;
    if (dN < 0 || dF < 0) return set_error(GBP_EINVAL, "negative size");
    if ((long long)N + dN > INT_MAX - 1) return set_error(GBP_EINVAL, "%d + %d variables do not fit int32", N, dN);
    if (2LL * ((long long)F + dF) > INT_MAX) return set_error(GBP_EINVAL, "%d + %d factors: 2 F must fit int32 (an adjacency entry is factor << 1 | side)", F, dF);
    if ((dF && (!d->var_a || !d->var_b || (!nl && (!d->factor_eta || !d->factor_lam)))) || (dN && (!d->prior_eta || !d->prior_lam)))
        return set_error(GBP_EINVAL, "NULL array in the descriptor");
    if (!nl && dF && h->has_const != (d->factor_const != nullptr))
        return set_error(GBP_EINVAL, h->has_const ? "the handle was created with factor_const: the new factors need theirs"
                                                  : "the handle was created without factor_const: the new factors cannot have one");
    const int N1 = N + dN;
    for (int f = 0; f < dF; ++f) {
        const int a = d->var_a[f], b = d->var_b[f];
        if (a < 0 || a >= N1 || b < 0 || b >= N1 || a == b)
            return set_error(GBP_EINVAL, "new factor %d joins variables (%d, %d): need two different ids in [0, %d)", f, a, b, N1);
    }
    if (d->loss && dF) {                                    // the rules of gbp_lin_set_robust
        bool any = false;
        LCHK(lin_check_losses(d->loss, d->threshold, d->noise_var, dF, "new factor", &any));
        if ((any || !h->p.w) && !h->has_const)
            return set_error(GBP_EINVAL, "a loss needs the factors' constants: the handle was created with factor_const == NULL");
    }
    return GBP_OK;
}

// what both entry points do once the descriptor is known to be good
int ext_run(gbp_lin *h, const gbp_lin_extend_desc_t *d, const gbp_lin_extend_nonlinear_desc_t *nl, bool robust)
{
    LHIPCHK(hipStreamSynchronize(h->stream));
    LinScratch mem;
    ExtHost host;                                           // read by the stream until the synchronisation in ext_build, or the one below
    LinGen n;
    n.robust = robust;
    n.nonlinear = nl != nullptr;
    const int rc = ext_build(h, d, nl, mem, host, n);
    if (rc != GBP_OK) {                                     // the handle's arrays were only read: it goes on as it was
        (void)hipStreamSynchronize(h->stream);              // before `mem` frees what the stream may still be writing
        return rc;
    }
    lin_gen_commit(h, mem, n);
    // beliefs of the grown graph (update_all_beliefs gbp.py:56-58): old variables add the same messages in the same order plus zeros,
    // new ones hold their prior
    if (h->has_beliefs) return gbp_lin_update_beliefs(h);
    return GBP_OK;
}

}  // namespace

extern "C" {

int gbp_lin_get_sizes(gbp_lin_t *h, int32_t *n_vars, int32_t *n_factors)
{
    LENTER(h);
    if (n_vars) *n_vars = h->p.N;
    if (n_factors) *n_factors = h->p.F;
    return GBP_OK;
}

int gbp_lin_extend(gbp_lin_t *h, const gbp_lin_extend_desc_t *d)
{
    LENTER(h);
    LIN_REFUSE_NONLINEAR(h, "gbp_lin_extend");
    if (!d) return set_error(GBP_EINVAL, "NULL descriptor");
    LCHK(ext_validate(h, d, false));
    if (!d->n_new_vars && !d->n_new_factors) return GBP_OK;
    // losses are on after the call if they are now, or if the new factors bring some
    return ext_run(h, d, nullptr, h->p.w != nullptr || (d->loss && d->n_new_factors));
}

int gbp_lin_extend_nonlinear(gbp_lin_t *h, const gbp_lin_extend_nonlinear_desc_t *nl)
{
    LENTER(h);
    if (!h->nonlinear) return set_error(GBP_ESTATE, "the handle has no nonlinear factors: call gbp_lin_set_nonlinear first, or gbp_lin_extend");
    if (!nl) return set_error(GBP_EINVAL, "NULL descriptor");
    gbp_lin_extend_desc_t d{};                              // sizes, ends and priors: the rules of gbp_lin_extend
    d.n_new_vars = nl->n_new_vars; d.n_new_factors = nl->n_new_factors;
    d.var_a = nl->var_a; d.var_b = nl->var_b; d.prior_eta = nl->prior_eta; d.prior_lam = nl->prior_lam;
    LCHK(ext_validate(h, &d, true));
    const int F = h->p.F, dF = nl->n_new_factors;
    if (dF && (!nl->measurement || !nl->sqrt_info)) return set_error(GBP_EINVAL, "NULL array in the descriptor");
    LCHK(lin_check_measurements(h->nl.model, nl->measurement, nl->sqrt_info, dF, "new factor"));    // the rules of gbp_lin_set_nonlinear
    if (!nl->n_new_vars && !dF) return GBP_OK;
    // Losses (gbp_lin_set_robust_nonlinear) stay set: the old factors carry loss, threshold, weight and flag, the new ones start at the
    // columns' fills -- NONE, weight 1, flag 0 -- until that call gives them a loss by range.  Ends with the belief stage: a nonlinear
    // handle has beliefs
    LCHK(ext_run(h, &d, nl, h->p.w != nullptr));
    // compute_factor on the new factors only (gbp.py:267-294), at the belief means as that stage left them; the joint is stale already
    return lin_nonlin_linearise(h, F, F + dF);
}

}  // extern "C"
