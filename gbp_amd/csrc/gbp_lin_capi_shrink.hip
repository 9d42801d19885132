// gbp_lin_capi_shrink.hip -- gbp_lin_shrink of include/gbp_lin.h: retiring variables and dropping factors from a live handle without
// gbp_lin_destroy + gbp_lin_create, the surviving messages kept and the leaving ones folded into the survivors' priors (kernels and the
// renumbering argument: gbp_lin_shrink.hpp).
//
// One call: validate the two lists on the host (range and repeats: sorted copies, so the work is that of the lists), upload them, make
// the flags, scan them once and bring N', F', 2F' back in one copy; allocate EVERY new array (lin_gen_alloc), build them on the device
// from the old ones -- which are only read -- and synchronise; only then commit the new generation (lin_gen_commit,
// gbp_lin_generation.hpp) and, where the handle had beliefs, run the belief stage over the survivors.  A failure before the commit
// frees what was allocated and leaves the handle as it was.  Host work and host <-> device traffic are proportional to the two lists,
// plus the maps where the caller asks for them; no existing array crosses to the host.
//
// Which arrays are gathered through the list of surviving factors is not said here: shr_build walks lin_gen_columns.
//
// gbp_lin_shrink_nonlinear is the same call on a handle of gbp_lin_set_nonlinear: the per-factor arrays of LinNonlin are columns of the
// same walk.  Nothing relinearises; a folded message is the one its factor computed at its last
// linearisation point and is frozen in the prior from then on.
#include "gbp_lin_shrink.hpp"
#include "gbp_lin_generation.hpp"

#include <rocprim/device/device_scan.hpp>

#include <climits>

using namespace gbp;

namespace {

int shr_blocks(size_t n) { return (int)((n + SHR_BLOCK - 1) / SHR_BLOCK); }

template <typename T>
void shr_gather(gbp_lin *h, const T *src, const int *surv_f, T *dst, int rows, int F, int F1)
{
    if (F1 > 0) hipLaunchKernelGGL((k_shr_gather<T>), dim3(shr_blocks((size_t)F1), rows), dim3(SHR_BLOCK), 0, h->stream, src, surv_f, dst, F, F1);
}

// ids in [0, n), none twice; `what` names the list in the message
int shr_check_list(const int32_t *ids, int count, int n, const char *what)
{
    if (count < 0) return set_error(GBP_EINVAL, "negative count of %s", what);
    if (count && !ids) return set_error(GBP_EINVAL, "the list of %s is NULL", what);
    if (count > n) return set_error(GBP_EINVAL, "%d %s listed, the handle holds %d: an id is out of range or listed twice", count, what, n);
    std::vector<int32_t> s(ids, ids + count);
    std::sort(s.begin(), s.end());
    if (count && (s.front() < 0 || s.back() >= n)) return set_error(GBP_EINVAL, "%s: id %d outside [0, %d)", what, s.front() < 0 ? s.front() : s.back(), n);
    for (int i = 1; i < count; ++i)
        if (s[i] == s[i - 1]) return set_error(GBP_EINVAL, "%s: id %d is listed twice", what, s[i]);
    return GBP_OK;
}

// everything up to and including the synchronisation after which nothing can fail: the new arrays, built on the device
int shr_build(gbp_lin *h, const gbp_lin_shrink_desc_t *d, LinScratch &mem, LinGen &n)
{
    const LinParams &p = h->p;
    const int R = lin_rows(h->D).msg, REC = lin_rows(h->D).rec;
    const int N = p.N, F = p.F, nr = d->n_retire_vars, nd = d->n_drop_factors;
    const size_t total = (size_t)N + 3 * (size_t)F;             // the union index space [ N | F | 2F ], + 1 for the scan's total

    // ---- flags over the union index space, one scan, the sizes in one copy ----
    int *ids_r = nullptr, *ids_d = nullptr, *vret = nullptr, *fdrop = nullptr, *keep = nullptr, *pos = nullptr, *fold_side = nullptr, *sizes = nullptr;
    LCHK(mem.get(&ids_r, (size_t)nr, false)); LCHK(mem.get(&ids_d, (size_t)nd, false));
    LCHK(mem.get(&vret, (size_t)N, false)); LCHK(mem.get(&fdrop, (size_t)F, false));
    LCHK(mem.get(&keep, total + 1, false)); LCHK(mem.get(&pos, total + 1, false));
    LCHK(mem.get(&fold_side, (size_t)F, false)); LCHK(mem.get(&sizes, 3, false));
    size_t scan_bytes = 0;
    LHIPCHK(rocprim::exclusive_scan(nullptr, scan_bytes, keep, pos, 0, total + 1, rocprim::plus<int>(), h->stream));
    { char *q = nullptr; LCHK(mem.get(&q, scan_bytes, false)); }
    void *scan_tmp = mem.temp.back();
    if (nr) LHIPCHK(hipMemcpyAsync(ids_r, d->retire_vars, (size_t)nr * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (nd) LHIPCHK(hipMemcpyAsync(ids_d, d->drop_factors, (size_t)nd * sizeof(int), hipMemcpyHostToDevice, h->stream));
    if (N) LHIPCHK(hipMemsetAsync(vret, 0, (size_t)N * sizeof(int), h->stream));
    if (F) LHIPCHK(hipMemsetAsync(fdrop, 0, (size_t)F * sizeof(int), h->stream));
    if (nr) hipLaunchKernelGGL(k_shr_mark, dim3(shr_blocks((size_t)nr)), dim3(SHR_BLOCK), 0, h->stream, (const int *)ids_r, nr, vret);
    if (nd) hipLaunchKernelGGL(k_shr_mark, dim3(shr_blocks((size_t)nd)), dim3(SHR_BLOCK), 0, h->stream, (const int *)ids_d, nd, fdrop);
    hipLaunchKernelGGL(k_shr_flags, dim3(shr_blocks(total + 1)), dim3(SHR_BLOCK), 0, h->stream, p.va, p.vb, p.vadj, N, F, (const int *)vret, (const int *)fdrop,
                       (int)d->fold, keep, fold_side);
    LHIPCHK(hipGetLastError());
    LHIPCHK(rocprim::exclusive_scan(scan_tmp, scan_bytes, keep, pos, 0, total + 1, rocprim::plus<int>(), h->stream));
    hipLaunchKernelGGL(k_shr_sizes, dim3(1), dim3(64), 0, h->stream, (const int *)pos, N, F, sizes);
    LHIPCHK(hipGetLastError());
    int hs[3] = {0, 0, 0};
    LHIPCHK(hipMemcpyAsync(hs, sizes, sizeof(hs), hipMemcpyDeviceToHost, h->stream));
    LHIPCHK(hipStreamSynchronize(h->stream));
    const int N1 = hs[0], F1 = hs[1];
    if (N1 != N - nr || F1 < 0 || F1 > F - nd || hs[2] != 2 * F1)
        return set_error(GBP_EHIP, "the scan of the keep flags gave %d variables, %d factors, %d edges from %d - %d and %d - %d", N1, F1, hs[2], N, nr, F, nd);

    // ---- every allocation of the new generation, before the first kernel that builds it ----
    // d_red stays: it holds ceil(F / 256) >= max(1, ceil(F' / 256)) partials, and the energy's launch goes by red_blocks (the nonlinear one too: lin_nonlin_energy)
    int *maps = nullptr, *surv_v = nullptr, *surv_f = nullptr;          // maps: [N | F] of before the call
    LCHK(mem.get(&maps, (size_t)N + F, false)); LCHK(mem.get(&surv_v, (size_t)N1, false)); LCHK(mem.get(&surv_f, (size_t)F1, false));
    LCHK(lin_gen_alloc(h, mem, n, N1, F1));
    int *nvptr = lin_mut(n.p.vptr), *nvadj = lin_mut(n.p.vadj), *nepos_a = lin_mut(n.p.epos_a), *nepos_b = lin_mut(n.p.epos_b);

    // ---- the maps and the lists of survivors ----
    const int *ckeep = keep, *cpos = pos, *csurv = surv_f, *cmaps = maps;
    if (N + F) hipLaunchKernelGGL(k_shr_maps, dim3(shr_blocks((size_t)N + F)), dim3(SHR_BLOCK), 0, h->stream, ckeep, cpos, N, F, maps, surv_v, surv_f);
    // ---- factor-strided arrays: [row][F] -> [row][F1], the survivors' rows gathered.  Not va / vb, whose entries are renumbered on
    // the way (k_shr_ends), and not epos_a / epos_b: k_shr_edges below writes them ----
    if (F1) {
        hipLaunchKernelGGL(k_shr_ends, dim3(shr_blocks((size_t)F1)), dim3(SHR_BLOCK), 0, h->stream, p.va, csurv, cmaps, lin_mut(n.p.va), F1);
        hipLaunchKernelGGL(k_shr_ends, dim3(shr_blocks((size_t)F1)), dim3(SHR_BLOCK), 0, h->stream, p.vb, csurv, cmaps, lin_mut(n.p.vb), F1);
    }
    (void)&shr_gather<double>;      // instantiated ahead of <int>, which the walk meets first: the kernels keep their order in the code object
    lin_gen_columns(h, n, [&](auto c) {
        const bool own_kernel = c.id == LC_VA || c.id == LC_VB || c.id == LC_EPOS_A || c.id == LC_EPOS_B;
        if (n.has(c.group) && !own_kernel) shr_gather(h, c.old, csurv, c.neu, c.rows, F, F1);
    });
    LHIPCHK(hipGetLastError());
    // ---- the CSR of the survivors, the rows of vmsg with it ----
    hipLaunchKernelGGL(k_shr_vptr, dim3(shr_blocks((size_t)N + 1)), dim3(SHR_BLOCK), 0, h->stream, ckeep, cpos, p.vptr, N, F, N1, nvptr);
    if (F)
        hipLaunchKernelGGL(k_shr_edges, dim3(shr_blocks((size_t)2 * F * R)), dim3(SHR_BLOCK), 0, h->stream, ckeep, cpos, p.vadj, N, F, R, (const double *)p.vmsg, nvadj,
                           nepos_a, nepos_b, n.p.vmsg);
    // ---- the fold into the priors; the survivors' belief records ----
    if (N)
        hipLaunchKernelGGL(k_shr_fold, dim3(shr_blocks((size_t)N * REC)), dim3(SHR_BLOCK), 0, h->stream, ckeep, cpos, p.vptr, p.vadj, (const int *)fold_side, N, R, REC,
                           p.prior, (const double *)p.vmsg, (const double *)p.bel, lin_mut(n.p.prior), n.p.bel);
    LHIPCHK(hipGetLastError());
    if (d->var_map && N) LHIPCHK(hipMemcpyAsync(d->var_map, maps, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (d->factor_map && F) LHIPCHK(hipMemcpyAsync(d->factor_map, maps + N, (size_t)F * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LHIPCHK(hipStreamSynchronize(h->stream));              // nothing below can fail
    return GBP_OK;
}

int shr_validate(gbp_lin *h, const gbp_lin_shrink_desc_t *d)
{
    const int N = h->p.N, F = h->p.F;
    if (d->fold != 0 && d->fold != 1) return set_error(GBP_EINVAL, "fold is %d: 0 or 1", d->fold);
    LCHK(shr_check_list(d->retire_vars, d->n_retire_vars, N, "retired variables"));
    LCHK(shr_check_list(d->drop_factors, d->n_drop_factors, F, "dropped factors"));
    if ((long long)N + 3LL * F + 1 > INT_MAX) return set_error(GBP_EINVAL, "%d variables and %d factors: N + 3 F + 1 must fit int32 (one scan over variables, factors and edges)", N, F);
    return GBP_OK;
}

// what both entry points do on a handle they accept
int shr_run(gbp_lin *h, const gbp_lin_shrink_desc_t *d)
{
    if (!d) return set_error(GBP_EINVAL, "NULL descriptor");
    LCHK(shr_validate(h, d));
    if (!d->n_retire_vars && !d->n_drop_factors) {          // nothing leaves: the maps are the identity
        if (d->var_map) for (int v = 0; v < h->p.N; ++v) d->var_map[v] = v;
        if (d->factor_map) for (int f = 0; f < h->p.F; ++f) d->factor_map[f] = f;
        return GBP_OK;
    }
    LHIPCHK(hipStreamSynchronize(h->stream));
    LinScratch mem;
    LinGen n;
    n.robust = h->p.w != nullptr;                           // a handle whose losses were cleared keeps stale arrays: they are freed, not carried
    n.nonlinear = h->nonlinear;
    const int rc = shr_build(h, d, mem, n);
    if (rc != GBP_OK) {                                     // the handle's arrays were only read: it goes on as it was
        (void)hipStreamSynchronize(h->stream);              // before `mem` frees what the stream may still be writing
        return rc;
    }
    lin_gen_commit(h, mem, n);
    // beliefs of the shrunk graph (update_all_beliefs gbp.py:56-58): the folded prior, then the surviving messages in adjacency order
    if (h->has_beliefs) return gbp_lin_update_beliefs(h);
    return GBP_OK;
}

}  // namespace

extern "C" {

int gbp_lin_shrink(gbp_lin_t *h, const gbp_lin_shrink_desc_t *d)
{
    LENTER(h);
    LIN_REFUSE_NONLINEAR(h, "gbp_lin_shrink");
    return shr_run(h, d);
}

int gbp_lin_shrink_nonlinear(gbp_lin_t *h, const gbp_lin_shrink_desc_t *d)
{
    LENTER(h);
    if (!h->nonlinear) return set_error(GBP_ESTATE, "the handle has no nonlinear factors: call gbp_lin_set_nonlinear first, or gbp_lin_shrink");
    return shr_run(h, d);
}

}  // extern "C"
