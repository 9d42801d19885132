// gbp_lin_extend.hpp -- growing a live linear graph on the device (gbp_lin_extend of include/gbp_lin.h): what the reference does with
// graph.var_nodes.append / graph.factors.append / adj_factors.append (ndim_posegraph.py:67-88) and update_all_beliefs() (gbp.py:56-58).
//
// Everything the handle holds is strided by F or N, so an append is a rebuild of the layout into new arrays, all of it on the device:
//   * every SoA array [row][F] is re-strided to [row][F + dF]: the old columns are copied row by row, the tail comes from the uploaded
//     new factors (or is a constant: zero messages gbp.py:222, weight 1, flag 0);
//   * the new edges (variable, factor << 1 | side), written in ascending (factor, side), are sorted by variable with the STABLE radix
//     sort of gbp_sort.hip, so that within a variable they stay in ascending factor id;
//   * the CSR is the merge of the old one with that sorted list.  With lb(v) = the number of new edges on variables below v (a lower
//     bound in the sorted keys) and optr(v) = the old vptr continued flat past the old variables:
//         vptr'[v]             = optr(v) + lb(v)
//         old edge e of v     -> e + lb(v)                 (v's old list keeps its place at the head of v's new list)
//         new edge of rank j  -> optr(v + 1) + j           (= vptr'[v] + old degree + (j - lb(v)): behind v's old list, in sorted order)
//     which is what adj_factors.append produces, and the order the belief stage adds in;
//   * the variable-major copy of the messages (vmsg) moves row by row to the new edge positions; rows of new edges are zero.
// No atomics of any kind: every destination is written by exactly one thread, at a position that depends on the graph alone, so two
// handles given the same calls are bit-identical.  The index routines are GBP_HD and take plain pointers so that
// tests/hostmath/lin_extend_shim.hip can run them on a CPU against np.lexsort.
#pragma once
#include "gbp_lin_handle.hpp"
#include "gbp_math.hpp"

namespace gbp {

// the number of entries of the ascending keys[0..n) that are below v
GBP_HD int lin_ext_lower_bound(const int *keys, int n, int v)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// the old vptr continued past the old variables: a new variable has no old edges (v in [0, N'], N' >= N)
GBP_HD int lin_ext_old_ptr(const int *vptr, int N, int v) { return vptr[v < N ? v : N]; }

// vptr'[v] for v in [0, N']
GBP_HD int lin_ext_new_ptr(const int *vptr, int N, const int *keys, int n_new_edges, int v)
{
    return lin_ext_old_ptr(vptr, N, v) + lin_ext_lower_bound(keys, n_new_edges, v);
}

// the variable of the old edge (factor << 1 | side)
GBP_HD int lin_ext_edge_var(const int *va, const int *vb, int fs) { return (fs & 1) ? vb[fs >> 1] : va[fs >> 1]; }

// where the old edge e of the old variable v lands
GBP_HD int lin_ext_old_edge_pos(const int *vptr, const int *vptr_new, int v, int e) { return e + (vptr_new[v] - vptr[v]); }

// where the new edge of rank j in the sorted list, on variable v, lands
GBP_HD int lin_ext_new_edge_pos(const int *vptr, int N, int v, int j) { return lin_ext_old_ptr(vptr, N, v + 1) + j; }

#ifndef GBP_LIN_EXTEND_ROUTINES_ONLY    // the host shim takes the routines above and no kernel (a host-only build has no code object to register)

constexpr int EXT_BLOCK = 256;

// dst [rows][F + dF] from src [rows][F] (nullptr: `fill`) and tail [rows][dF] (nullptr: `fill`); blockIdx.y = row, so that both the
// loads and the stores of a wave are one contiguous run
template <typename T>
__global__ __launch_bounds__(EXT_BLOCK) void k_ext_restride(const T *__restrict__ src, const T *__restrict__ tail, T *__restrict__ dst, int F, int dF, T fill)
{
    const int c = blockIdx.x * EXT_BLOCK + threadIdx.x;
    const size_t row = blockIdx.y, F1 = (size_t)F + dF;
    if (c >= F + dF) return;
    T v = fill;
    if (c < F) { if (src) v = src[row * F + c]; }
    else if (tail) v = tail[row * dF + (c - F)];
    dst[row * F1 + c] = v;
}

// the new edges in ascending (factor, side): key = variable, value = factor << 1 | side
__global__ __launch_bounds__(EXT_BLOCK) void k_ext_edges(const int *__restrict__ na, const int *__restrict__ nb, int F, int dF, int *__restrict__ keys, int *__restrict__ vals)
{
    const int j = blockIdx.x * EXT_BLOCK + threadIdx.x;
    if (j >= 2 * dF) return;
    const int i = j >> 1, side = j & 1;
    keys[j] = side ? nb[i] : na[i];
    vals[j] = ((F + i) << 1) | side;
}

// vptr' [N1 + 1]
__global__ __launch_bounds__(EXT_BLOCK) void k_ext_vptr(const int *__restrict__ vptr, int N, int N1, const int *__restrict__ keys, int n_new_edges, int *__restrict__ vptr_new)
{
    const int v = blockIdx.x * EXT_BLOCK + threadIdx.x;
    if (v <= N1) vptr_new[v] = lin_ext_new_ptr(vptr, N, keys, n_new_edges, v);
}

// one thread per old edge: its new position (kept in `enew` for the move of vmsg), its entry of vadj' and of epos_a' / epos_b'
__global__ __launch_bounds__(EXT_BLOCK) void k_ext_old_edges(const int *__restrict__ vptr, const int *__restrict__ vptr_new, const int *__restrict__ vadj,
                                                             const int *__restrict__ va, const int *__restrict__ vb, int n_old_edges,
                                                             int *__restrict__ vadj_new, int *__restrict__ epos_a, int *__restrict__ epos_b, int *__restrict__ enew)
{
    const int e = blockIdx.x * EXT_BLOCK + threadIdx.x;
    if (e >= n_old_edges) return;
    const int fs = vadj[e];
    const int e1 = lin_ext_old_edge_pos(vptr, vptr_new, lin_ext_edge_var(va, vb, fs), e);
    vadj_new[e1] = fs;
    ((fs & 1) ? epos_b : epos_a)[fs >> 1] = e1;
    enew[e] = e1;
}

// R lanes per new edge of the sorted list: vadj', epos' and a zero row of vmsg' (Factor.messages start at zero, gbp.py:222)
__global__ __launch_bounds__(EXT_BLOCK) void k_ext_new_edges(const int *__restrict__ vptr, int N, const int *__restrict__ keys, const int *__restrict__ vals, int n_new_edges,
                                                             int R, int *__restrict__ vadj_new, int *__restrict__ epos_a, int *__restrict__ epos_b, double *__restrict__ vmsg_new)
{
    const size_t idx = (size_t)blockIdx.x * EXT_BLOCK + threadIdx.x;
    const int j = (int)(idx / R), k = (int)(idx - (size_t)j * R);
    if (j >= n_new_edges) return;
    const int e1 = lin_ext_new_edge_pos(vptr, N, keys[j], j);
    vmsg_new[(size_t)e1 * R + k] = 0.0;
    if (k == 0) {
        const int fs = vals[j];
        vadj_new[e1] = fs;
        ((fs & 1) ? epos_b : epos_a)[fs >> 1] = e1;
    }
}

// one thread per double of the old vmsg: row e goes to row enew[e].  Rows of one variable stay together and variables stay in order,
// so both sides stream
template <int R>
__global__ __launch_bounds__(EXT_BLOCK) void k_ext_move_vmsg(const double *__restrict__ vmsg, const int *__restrict__ enew, size_t n, double *__restrict__ vmsg_new)
{
    const size_t idx = (size_t)blockIdx.x * EXT_BLOCK + threadIdx.x;
    if (idx >= n) return;
    const size_t e = idx / R;
    vmsg_new[(size_t)enew[e] * R + (idx - e * R)] = vmsg[idx];
}

#endif  // GBP_LIN_EXTEND_ROUTINES_ONLY

}  // namespace gbp
