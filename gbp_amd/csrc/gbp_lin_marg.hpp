// gbp_lin_marg.hpp -- exact marginal covariances of a linear pairwise graph on gfx950: the `sigma` of FactorGraph.joint_distribution_cov
// (gbp.py:128-144) for chosen variables, without the dense N d x N d inverse.
//
// Column (v, k) of Lambda_joint^-1 is the solution of Lambda x = e_(v,k).  MARG_COLS = 8 such systems are iterated TOGETHER by the
// block-Jacobi conjugate gradients of gbp_lin_map.hpp, every column with scalars of its own (no shared Krylov space), so that one pass
// over the factors serves all eight: per factor and iteration d(2d+1) + 8 * 6d doubles against 8 (d(2d+1) + 6d) of eight solves.
// Layout: every multi-column vector is [N][d][8] and the edge buffer [2F][d][8], the column index innermost.  A lane is one
// (item, column) pair:
//   k_marg_factor<D>  8 factors x 8 columns per wave.  The 8 lanes of a factor read the SAME Lambda_f words (one fetch) and gather /
//                     store contiguous 64-byte runs of p and of the edge buffer: no LDS transpose;
//   k_marg_var<D>     one lane per (variable, column): prior block, the contiguous edge run in adj_factors order, partials of p . q;
//   k_marg_step<D>    alpha_k in its head; x += alpha p, r -= alpha q, z = D_v^-1 r (the LDL^T that k_map_setup made); partials;
//   k_marg_dir<D>     beta_k in its head; p = z + beta p;
//   k_marg_restart<D> r = e - q (or e), z, p = z: the start of a recurrence and the TRUE residual;
//   k_marg_gather<D>  rows ids[*] of the batch's columns into the output blocks, so the N d-long columns stay on the device.
// Per-column sums: lanes of equal column are 8 apart, so a wave adds them with __shfl_down by 32, 16, 8 and the block's four waves are
// added in a fixed order, into per-block partials [nb][8].  Every block of the step and direction kernels adds the same partials in the
// same order (map_block_sum's argument): bit-identical scalars everywhere, no host round trip, no floating-point atomics.  The r . z
// partials alternate between two slots by iteration parity as in gbp_lin_map.hpp.  A column whose right-hand side is zero (padding of
// the last batch) stays exactly zero: map_ratio(0, 0) = 0.
// As in gbp_lin_map.hpp the per-(item, column) routines are host/device functions that also run in plain loops on a CPU
// (tests/hostmath/lin_marg_shim.hip); the kernels are thin wrappers.  fp64, no MFMA.
#pragma once
#include "gbp_lin_map.hpp"

namespace gbp {

constexpr int MARG_COLS = GBP_LIN_MARG_COLS;
constexpr int MARG_FACTORS_PER_BLOCK = MAP_BLOCK / MARG_COLS;
static_assert(MARG_COLS == 8 && 64 % MARG_COLS == 0, "the per-column reduction below is written for 8 columns");
static_assert(MAP_BLOCK == 256, "marg_block_sum adds the partials of exactly four waves");

// the right-hand sides of a batch: column c is the unit vector of coordinate k[c] of variable var[c]; var[c] < 0: a zero column
struct MargCols { int var[MARG_COLS], k[MARG_COLS]; };

// ---- per-(item, column) routines (host and device) ---------------------------------------------------------------------------------

// (ya; yb) = Lambda_f (p_a; p_b) for column c of the [N][d][8] vector `src`
template <int D>
GBP_HD void marg_factor_apply(const LinParams &p, int f, int c, const double *src, double (&ya)[D], double (&yb)[D])
{
    constexpr int N2 = 2 * D, K = MARG_COLS;
    const size_t F = (size_t)p.F;
    double x[N2], y[N2];
    const double *pa = src + (size_t)p.va[f] * D * K + c, *pb = src + (size_t)p.vb[f] * D * K + c;
#pragma unroll
    for (int k = 0; k < D; ++k) { x[k] = pa[k * K]; x[D + k] = pb[k * K]; y[k] = 0.0; y[D + k] = 0.0; }
#pragma unroll
    for (int i = 0; i < N2; ++i) {
#pragma unroll
        for (int j = i; j < N2; ++j) {
            const double a = p.flam[(size_t)Sym<N2>::at(i, j) * F + f];
            y[i] += a * x[j];
            if (j != i) y[j] += a * x[i];
        }
    }
    if (p.w) {                                            // the joint at the current robust weights, as map_factor_apply
        const double w = p.w[f];
#pragma unroll
        for (int k = 0; k < N2; ++k) y[k] *= w;
    }
#pragma unroll
    for (int k = 0; k < D; ++k) { ya[k] = y[k]; yb[k] = y[D + k]; }
}

// both products of factor f, column c, into the edge buffer [2F][d][8] at the factor's two CSR positions
template <int D>
GBP_HD void marg_factor_store(const LinParams &p, int f, int c, const double *src, double *ebuf)
{
    constexpr int K = MARG_COLS;
    double ya[D], yb[D];
    marg_factor_apply<D>(p, f, c, src, ya, yb);
    double *ea = ebuf + (size_t)p.epos_a[f] * D * K + c, *eb = ebuf + (size_t)p.epos_b[f] * D * K + c;
#pragma unroll
    for (int k = 0; k < D; ++k) { ea[k * K] = ya[k]; eb[k * K] = yb[k]; }
}

// dst_v = prior Lambda_v src_v + the variable's edge run of ebuf, in adjacency order, for column c.  Returns src_v . dst_v.
template <int D>
GBP_HD double marg_var_gather(const LinParams &p, int v, int c, const double *src, const double *ebuf, double *dst)
{
    constexpr int P = LinDims<D>::P, R = D + P, K = MARG_COLS;
    double x[D], y[D];
#pragma unroll
    for (int k = 0; k < D; ++k) { x[k] = src[((size_t)v * D + k) * K + c]; y[k] = 0.0; }
#pragma unroll
    for (int i = 0; i < D; ++i) {
#pragma unroll
        for (int j = i; j < D; ++j) {
            const double a = p.prior[(size_t)v * R + D + Sym<D>::at(i, j)];
            y[i] += a * x[j];
            if (j != i) y[j] += a * x[i];
        }
    }
    for (int ed = p.vptr[v]; ed < p.vptr[v + 1]; ++ed) {
#pragma unroll
        for (int k = 0; k < D; ++k) y[k] += ebuf[((size_t)ed * D + k) * K + c];
    }
    double xy = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) { dst[((size_t)v * D + k) * K + c] = y[k]; xy += x[k] * y[k]; }
    return xy;
}

// r_v = e_v - q_v (q == nullptr: e_v) for column c, z_v = D_v^-1 r_v, p_v = z_v; adds r.z and r.r of the variable
template <int D>
GBP_HD void marg_var_restart(int v, int c, const MargCols &cols, const double *ldl, const double *q, double *r, double *z, double *pd,
                             double &rz, double &rr)
{
    constexpr int K = MARG_COLS;
    double rv[D], zv[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const double e = (cols.var[c] == v && cols.k[c] == k) ? 1.0 : 0.0;
        rv[k] = q ? e - q[((size_t)v * D + k) * K + c] : e;
    }
    map_block_solve<D>(ldl, v, rv, zv);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const size_t at = ((size_t)v * D + k) * K + c;
        r[at] = rv[k]; z[at] = zv[k]; pd[at] = zv[k];
        rz += rv[k] * zv[k]; rr += rv[k] * rv[k];
    }
}

// x_v += alpha p_v, r_v -= alpha q_v, z_v = D_v^-1 r_v for column c; adds r.z and r.r of the variable
template <int D>
GBP_HD void marg_var_step(int v, int c, double alpha, const double *ldl, const double *pd, const double *q, double *x, double *r, double *z,
                          double &rz, double &rr)
{
    constexpr int K = MARG_COLS;
    double rv[D], zv[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const size_t at = ((size_t)v * D + k) * K + c;
        x[at] += alpha * pd[at];
        rv[k] = r[at] - alpha * q[at];
    }
    map_block_solve<D>(ldl, v, rv, zv);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const size_t at = ((size_t)v * D + k) * K + c;
        r[at] = rv[k]; z[at] = zv[k];
        rz += rv[k] * zv[k]; rr += rv[k] * rv[k];
    }
}

// p_v = z_v + beta p_v for column c
template <int D>
GBP_HD void marg_var_dir(int v, int c, double beta, const double *z, double *pd)
{
    constexpr int K = MARG_COLS;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const size_t at = ((size_t)v * D + k) * K + c;
        pd[at] = z[at] + beta * pd[at];
    }
}

// Output element `e` of a batch whose first column is number c0 of ncols = n_ids d.  With a joint block the elements are
// (j, row, c) over all n_ids rows; without one only the d rows of each column's own variable, (c, row).  Column c0 + c belongs to
// ids[i], coordinate kk; row (ids[j], row) of it goes to sigma_joint[(j d + row)][(i d + kk)] and, when j == i, to sigma[i][row][kk].
template <int D>
GBP_HD void marg_gather_one(long long e, const int *ids, int n_ids, int c0, int ncols, const double *x, double *sigma, double *joint)
{
    constexpr int K = MARG_COLS;
    const int c = (int)(e % K);
    const int row = (int)((e / K) % D);
    const int cg = c0 + c;
    if (cg >= ncols) return;
    const int i = cg / D, kk = cg - i * D;
    const int j = joint ? (int)(e / ((long long)K * D)) : i;
    const double val = x[((size_t)ids[j] * D + row) * K + c];
    if (joint) joint[((size_t)j * D + row) * ((size_t)n_ids * D) + cg] = val;
    if (j == i) sigma[((size_t)i * D + row) * D + kk] = val;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------

// the sum over the block's lanes of equal column (threadIdx.x & 7), the same value in all of them, added in a fixed order; `red`
// ([MAP_BLOCK / 64][8]) is reusable after the call
GBP_DEV double marg_block_sum(double v, double *red)
{
    constexpr int K = MARG_COLS;
    v += __shfl_down(v, 32, 64);
    v += __shfl_down(v, 16, 64);
    v += __shfl_down(v, 8, 64);                              // lanes 0..7 now hold their column's sum over the wave
    const int lane = threadIdx.x & 63, c = threadIdx.x & (K - 1);
    if (lane < K) red[(threadIdx.x >> 6) * K + lane] = v;
    __syncthreads();
    const double s = (red[c] + red[K + c]) + (red[2 * K + c] + red[3 * K + c]);
    __syncthreads();
    return s;
}

// per column: the sum of `nb` per-block partials [nb][8], bit-identical in every thread of that column in every block
GBP_DEV double marg_sum_partials(const double *part, int nb, double *red)
{
    constexpr int K = MARG_COLS;
    const int c = threadIdx.x & (K - 1);
    double a = 0.0;
    for (int i = threadIdx.x / K; i < nb; i += MAP_BLOCK / K) a += part[(size_t)i * K + c];
    return marg_block_sum(a, red);
}

// lane = (factor, column): 32 factors per block, no LDS, no barrier; lanes past the last factor do nothing
template <int D>
__global__ __launch_bounds__(MAP_BLOCK) void k_marg_factor(LinParams p, const double *src, double *ebuf)
{
    const long long f = (long long)blockIdx.x * MARG_FACTORS_PER_BLOCK + threadIdx.x / MARG_COLS;
    if (f < p.F) marg_factor_store<D>(p, (int)f, threadIdx.x & (MARG_COLS - 1), src, ebuf);
}

// The per-variable kernels stride over the N * 8 (variable, column) items by gridDim.x * 256, a multiple of 8: a thread keeps its column.
template <int D>
__global__ __launch_bounds__(MAP_BLOCK) void k_marg_var(LinParams p, const double *src, const double *ebuf, double *dst, double *pq_part)
{
    constexpr int K = MARG_COLS;
    __shared__ double red[MAP_BLOCK / 64 * K];
    const int c = threadIdx.x & (K - 1);
    double acc = 0.0;
    for (long long v = (long long)blockIdx.x * (MAP_BLOCK / K) + threadIdx.x / K; v < p.N; v += (long long)gridDim.x * (MAP_BLOCK / K))
        acc += marg_var_gather<D>(p, (int)v, c, src, ebuf, dst);
    acc = marg_block_sum(acc, red);
    if (threadIdx.x < K) pq_part[(size_t)blockIdx.x * K + c] = acc;
}

// slot: which half of rz_part receives r . z (the parity the NEXT iteration reads as "old")
template <int D>
__global__ __launch_bounds__(MAP_BLOCK) void k_marg_restart(LinMarg m, const double *ldl, MargCols cols, int N, int use_q, int slot)
{
    constexpr int K = MARG_COLS;
    __shared__ double red[MAP_BLOCK / 64 * K];
    const int c = threadIdx.x & (K - 1);
    double rz = 0.0, rr = 0.0;
    for (long long v = (long long)blockIdx.x * (MAP_BLOCK / K) + threadIdx.x / K; v < N; v += (long long)gridDim.x * (MAP_BLOCK / K))
        marg_var_restart<D>((int)v, c, cols, ldl, use_q ? m.q : nullptr, m.r, m.z, m.p, rz, rr);
    rz = marg_block_sum(rz, red);
    rr = marg_block_sum(rr, red);
    if (threadIdx.x < K) {
        m.rz_part[((size_t)slot * m.nb + blockIdx.x) * K + c] = rz;
        m.rr_part[(size_t)blockIdx.x * K + c] = rr;
    }
}

// par = iteration & 1: reads (r.z)_old from the other slot, writes the new one into slot `par`
template <int D>
__global__ __launch_bounds__(MAP_BLOCK) void k_marg_step(LinMarg m, const double *ldl, int N, int par)
{
    constexpr int K = MARG_COLS;
    __shared__ double red[MAP_BLOCK / 64 * K];
    const int c = threadIdx.x & (K - 1);
    const double rz_old = marg_sum_partials(m.rz_part + (size_t)(par ^ 1) * m.nb * K, m.nb, red);
    const double pq = marg_sum_partials(m.pq_part, m.nb, red);
    const double alpha = map_ratio(rz_old, pq);
    double rz = 0.0, rr = 0.0;
    for (long long v = (long long)blockIdx.x * (MAP_BLOCK / K) + threadIdx.x / K; v < N; v += (long long)gridDim.x * (MAP_BLOCK / K))
        marg_var_step<D>((int)v, c, alpha, ldl, m.p, m.q, m.x, m.r, m.z, rz, rr);
    rz = marg_block_sum(rz, red);
    rr = marg_block_sum(rr, red);
    if (threadIdx.x < K) {
        m.rz_part[((size_t)par * m.nb + blockIdx.x) * K + c] = rz;
        m.rr_part[(size_t)blockIdx.x * K + c] = rr;
    }
}

template <int D>
__global__ __launch_bounds__(MAP_BLOCK) void k_marg_dir(LinMarg m, int N, int par)
{
    constexpr int K = MARG_COLS;
    __shared__ double red[MAP_BLOCK / 64 * K];
    const int c = threadIdx.x & (K - 1);
    const double rz_new = marg_sum_partials(m.rz_part + (size_t)par * m.nb * K, m.nb, red);
    const double rz_old = marg_sum_partials(m.rz_part + (size_t)(par ^ 1) * m.nb * K, m.nb, red);
    const double beta = map_ratio(rz_new, rz_old);
    for (long long v = (long long)blockIdx.x * (MAP_BLOCK / K) + threadIdx.x / K; v < N; v += (long long)gridDim.x * (MAP_BLOCK / K))
        marg_var_dir<D>((int)v, c, beta, m.z, m.p);
}

// n_out = n_ids * D * 8 with a joint block, D * 8 without
template <int D>
__global__ __launch_bounds__(MAP_BLOCK) void k_marg_gather(const double *x, const int *ids, int n_ids, int c0, int ncols, long long n_out,
                                                           double *sigma, double *joint)
{
    for (long long e = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; e < n_out; e += (long long)gridDim.x * MAP_BLOCK)
        marg_gather_one<D>(e, ids, n_ids, c0, ncols, x, sigma, joint);
}

}  // namespace gbp
