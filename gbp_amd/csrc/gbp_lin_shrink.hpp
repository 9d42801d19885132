// gbp_lin_shrink.hpp -- shrinking a live linear graph on the device (gbp_lin_shrink of include/gbp_lin.h): variables retired and factors
// dropped from a handle, what the leaving factors last told the surviving variables folded into those variables' priors (GBP's own
// marginalisation: the message a factor sends to a variable IS the marginal over the factor's other end, gbp.py:334-373, so adding it
// to the prior keeps the survivor's belief where it was; exact on a tree with converged messages, no fill-in among the neighbours).
//
// Everything the handle holds is strided by F or N, so a shrink is a rebuild of the layout into new arrays, all of it on the device:
//   * the two uploaded id lists are scattered into flags (one thread per list entry; the host has refused a list with a repeated id,
//     so no two threads write one flag); one thread per factor derives `survives` and `folds towards a / b / neither`, one thread per
//     CSR edge `edge survives` (= its factor does);
//   * ONE exclusive scan over the keep flags of [ N variables | F factors | 2F edges | 1 ] gives the three maps and N', F', 2F':
//         new variable id = pos[v],  new factor id = pos[N + f] - pos[N],  new edge = pos[N + F + e] - pos[N + F]
//     -- monotone, so adjacency stays ascending in factor id, a variable's surviving edges stay one run in their old order, and nothing
//     is sorted;
//   * every SoA array [row][F] is gathered to [row][F'] through the list of survivors;
//   * vptr'[v'] is the edge map read at the old vptr[v] (every edge of a retired variable leaves, so the surviving edges below v's list
//     are exactly those of the surviving variables below v); vadj', epos_a', epos_b' and the rows of vmsg follow the maps;
//   * one lane per (surviving variable, record entry) starts from the old prior and adds the vmsg row of every folding edge of the
//     variable's OLD list in list order: prior first, then the folded messages, the order the belief stage adds in.
// No atomics of any kind in these kernels: every destination is written by exactly one thread, at a position that depends on the graph
// and the two lists alone, so two handles given the same calls are bit-identical.  The index routines are GBP_HD and take plain pointers
// so that tests/hostmath/lin_shrink_shim.hip can run them on a CPU against the CSR numpy builds for the survivors' graph.
#pragma once
#include "gbp_lin_handle.hpp"
#include "gbp_math.hpp"

namespace gbp {

// a factor survives unless it is listed or has a retired end
GBP_HD int lin_shr_factor_keep(int dropped, int ret_a, int ret_b) { return !dropped && !ret_a && !ret_b; }

// the side a LEAVING factor folds towards: 1 = a (b retired, a survives), 2 = b, 0 = neither (listed, both ends retired, fold off, or
// the factor survives)
GBP_HD int lin_shr_fold_side(int dropped, int ret_a, int ret_b, int fold)
{
    if (!fold || dropped || ret_a == ret_b) return 0;
    return ret_b ? 1 : 2;
}

// the maps out of the scan `pos` over keep[ N | F | 2F | 1 ]: the new id, or -1 for what leaves
GBP_HD int lin_shr_var_map(const int *keep, const int *pos, int v) { return keep[v] ? pos[v] : -1; }
GBP_HD int lin_shr_factor_map(const int *keep, const int *pos, int N, int f) { return keep[N + f] ? pos[N + f] - pos[N] : -1; }
GBP_HD int lin_shr_edge_map(const int *keep, const int *pos, int N, int F, int e) { return keep[N + F + e] ? pos[N + F + e] - pos[N + F] : -1; }

// vptr' of the surviving old variable v, and of v == N (the end: 2F')
GBP_HD int lin_shr_new_ptr(const int *pos, const int *vptr, int N, int F, int v) { return pos[N + F + vptr[v]] - pos[N + F]; }

// the adjacency entry (factor << 1 | side) of a surviving edge, renumbered
GBP_HD int lin_shr_new_adj(const int *pos, int N, int fs) { return ((pos[N + (fs >> 1)] - pos[N]) << 1) | (fs & 1); }

// whether the edge (factor << 1 | side) of a surviving variable's old list is folded into that variable's prior
GBP_HD bool lin_shr_edge_folds(const int *fold_side, int fs) { return fold_side[fs >> 1] == (fs & 1) + 1; }

#ifndef GBP_LIN_SHRINK_ROUTINES_ONLY    // the host shim takes the routines above and no kernel (a host-only build has no code object to register)

constexpr int SHR_BLOCK = 256;

// flag[ids[i]] = 1: one thread per list entry (the ids are distinct and in range: validated on the host)
__global__ __launch_bounds__(SHR_BLOCK) void k_shr_mark(const int *__restrict__ ids, int n, int *__restrict__ flag)
{
    const int i = blockIdx.x * SHR_BLOCK + threadIdx.x;
    if (i < n) flag[ids[i]] = 1;
}

// keep[ N | F | 2F | 1 ] and the fold side of every factor, one thread per entry of the union index space; keep[last] = 0, so that
// the exclusive scan ends with the total
__global__ __launch_bounds__(SHR_BLOCK) void k_shr_flags(const int *__restrict__ va, const int *__restrict__ vb, const int *__restrict__ vadj, int N, int F,
                                                         const int *__restrict__ vret, const int *__restrict__ fdrop, int fold, int *__restrict__ keep,
                                                         int *__restrict__ fold_side)
{
    const size_t i = (size_t)blockIdx.x * SHR_BLOCK + threadIdx.x, NF = (size_t)N + F, total = NF + 2 * (size_t)F;
    if (i > total) return;
    if (i == total) { keep[i] = 0; return; }
    if (i < (size_t)N) { keep[i] = !vret[i]; return; }
    const bool edge = i >= NF;
    const int f = edge ? (vadj[i - NF] >> 1) : (int)(i - N);
    const int dropped = fdrop[f], ra = vret[va[f]], rb = vret[vb[f]];
    keep[i] = lin_shr_factor_keep(dropped, ra, rb);
    if (!edge) fold_side[f] = lin_shr_fold_side(dropped, ra, rb, fold);
}

// sizes[3] = N', F', 2F' out of the scan, for the one copy to the host
__global__ void k_shr_sizes(const int *__restrict__ pos, int N, int F, int *__restrict__ sizes)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        sizes[0] = pos[N];
        sizes[1] = pos[N + F] - pos[N];
        sizes[2] = pos[(size_t)N + F + 2 * (size_t)F] - pos[N + F];
    }
}

// maps[ N | F ]: new id or -1 (what the caller may ask for); surv_v[v'] = v and surv_f[f'] = f, the lists the gathers go through
__global__ __launch_bounds__(SHR_BLOCK) void k_shr_maps(const int *__restrict__ keep, const int *__restrict__ pos, int N, int F, int *__restrict__ maps,
                                                        int *__restrict__ surv_v, int *__restrict__ surv_f)
{
    const int i = blockIdx.x * SHR_BLOCK + threadIdx.x;
    if (i >= N + F) return;
    if (i < N) {
        const int v1 = lin_shr_var_map(keep, pos, i);
        maps[i] = v1;
        if (v1 >= 0) surv_v[v1] = i;
    } else {
        const int f1 = lin_shr_factor_map(keep, pos, N, i - N);
        maps[i] = f1;
        if (f1 >= 0) surv_f[f1] = i - N;
    }
}

// dst [rows][F1] from src [rows][F] through the survivors; blockIdx.y = row, so that a wave's stores are one contiguous run
template <typename T>
__global__ __launch_bounds__(SHR_BLOCK) void k_shr_gather(const T *__restrict__ src, const int *__restrict__ surv_f, T *__restrict__ dst, int F, int F1)
{
    const int c = blockIdx.x * SHR_BLOCK + threadIdx.x;
    const size_t row = blockIdx.y;
    if (c < F1) dst[row * F1 + c] = src[row * F + surv_f[c]];
}

// va' / vb': the survivors' ends through the variable map (both ends of a survivor survive)
__global__ __launch_bounds__(SHR_BLOCK) void k_shr_ends(const int *__restrict__ src, const int *__restrict__ surv_f, const int *__restrict__ maps, int *__restrict__ dst, int F1)
{
    const int c = blockIdx.x * SHR_BLOCK + threadIdx.x;
    if (c < F1) dst[c] = maps[src[surv_f[c]]];
}

// vptr' [N1 + 1]: one thread per old variable and one for the end
__global__ __launch_bounds__(SHR_BLOCK) void k_shr_vptr(const int *__restrict__ keep, const int *__restrict__ pos, const int *__restrict__ vptr, int N, int F, int N1,
                                                        int *__restrict__ vptr_new)
{
    const int v = blockIdx.x * SHR_BLOCK + threadIdx.x;
    if (v > N) return;
    if (v == N) vptr_new[N1] = lin_shr_new_ptr(pos, vptr, N, F, N);
    else if (keep[v]) vptr_new[pos[v]] = lin_shr_new_ptr(pos, vptr, N, F, v);
}

// R lanes per old edge: a surviving edge's row of vmsg moves to its new position; lane 0 writes its entry of vadj' and of epos_a' / epos_b'
__global__ __launch_bounds__(SHR_BLOCK) void k_shr_edges(const int *__restrict__ keep, const int *__restrict__ pos, const int *__restrict__ vadj, int N, int F, int R,
                                                         const double *__restrict__ vmsg, int *__restrict__ vadj_new, int *__restrict__ epos_a, int *__restrict__ epos_b,
                                                         double *__restrict__ vmsg_new)
{
    const size_t idx = (size_t)blockIdx.x * SHR_BLOCK + threadIdx.x;
    const size_t e = idx / R;
    const int k = (int)(idx - e * R);
    if (e >= 2 * (size_t)F) return;
    const int e1 = lin_shr_edge_map(keep, pos, N, F, (int)e);
    if (e1 < 0) return;
    vmsg_new[(size_t)e1 * R + k] = vmsg[idx];
    if (k == 0) {
        const int fs = lin_shr_new_adj(pos, N, vadj[e]);
        vadj_new[e1] = fs;
        ((fs & 1) ? epos_b : epos_a)[fs >> 1] = e1;
    }
}

// one lane per (old variable, entry of the belief record): a survivor's record is copied; for the first R entries the new prior is the
// old one plus the vmsg rows of the folding edges of the OLD adjacency list, in list order (fp64, prior first)
__global__ __launch_bounds__(SHR_BLOCK) void k_shr_fold(const int *__restrict__ keep, const int *__restrict__ pos, const int *__restrict__ vptr, const int *__restrict__ vadj,
                                                        const int *__restrict__ fold_side, int N, int R, int REC, const double *__restrict__ prior,
                                                        const double *__restrict__ vmsg, const double *__restrict__ bel, double *__restrict__ prior_new,
                                                        double *__restrict__ bel_new)
{
    const size_t idx = (size_t)blockIdx.x * SHR_BLOCK + threadIdx.x;
    const size_t v = idx / REC;
    const int k = (int)(idx - v * REC);
    if (v >= (size_t)N || !keep[v]) return;
    const size_t v1 = (size_t)pos[v];
    bel_new[v1 * REC + k] = bel[idx];
    if (k >= R) return;
    double acc = prior[v * R + k];
    for (int e = vptr[v], e1 = vptr[v + 1]; e < e1; ++e)
        if (lin_shr_edge_folds(fold_side, vadj[e])) acc += vmsg[(size_t)e * R + k];
    prior_new[v1 * R + k] = acc;
}

#endif  // GBP_LIN_SHRINK_ROUTINES_ONLY

}  // namespace gbp
