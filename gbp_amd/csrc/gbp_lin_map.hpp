// gbp_lin_map.hpp -- the batch MAP of a linear pairwise graph on gfx950: FactorGraph.joint_distribution_cov (gbp.py:94-144) without the
// dense N d x N d inverse.
//
// The joint information form (joint_distribution_inf, gbp.py:94-126) is  Lambda = blockdiag(prior Lambda_v) + sum_f scatter(Lambda_f),
// eta = prior eta + sum_f scatter(eta_f): block-sparse and SPD.  Its solution Lambda^-1 eta (the `mu` of gbp.py:139-144) is found by
// conjugate gradients preconditioned with the d x d diagonal blocks (block Jacobi).  Lambda is never assembled: a product
// q = Lambda p is the sweep's two-stage, atomics-free pattern,
//   k_map_factor<D>   one lane per factor: Lambda_f [p_a; p_b] -> two d-vectors, written in CSR edge order through an LDS transpose
//                     (contiguous runs per store, as k_lin_factor's stage_out does for the messages);
//   k_map_var<D>      one lane per variable: q_v = prior Lambda_v p_v + its contiguous edge run, added in adj_factors order; and the
//                     block's partial of p . q.
// The vector work of an iteration is two more kernels, because alpha needs all of p . q and beta all of r . z:
//   k_map_step<D>     alpha = (r.z)_old / (p.q) in its head; x += alpha p, r -= alpha q, z = D_v^-1 r, partials of r . z and r . r;
//   k_map_dir<D>      beta = (r.z)_new / (r.z)_old in its head; p = z + beta p.
// alpha and beta never visit the host: every block of a kernel adds the SAME array of per-block partials in the SAME order (strided
// per thread, then a fixed tree), so all blocks hold bit-identical scalars, and two solves of one handle are bit-identical.  The r . z
// partials alternate between two slots by iteration parity: k_map_dir reads both the new and the old ones, and no kernel writes a
// slot that a kernel of the same iteration reads.  No floating-point atomics.
//   k_map_setup<D>    once per handle: D_v = prior Lambda_v + the factors' own diagonal blocks (side from vadj's low bit), stored as
//                     its LDL^T (ldl_factor); eta_joint,v; partial of |eta|^2.  Sums in adjacency order.
//   k_map_restart<D>  r = eta - q (or eta), z = D_v^-1 r, p = z, partials: the start of a recurrence, and -- after q = Lambda x --
//                     the TRUE residual when the recurrence claims convergence.
// The per-factor and per-variable routines are host/device functions over the engine's own arrays, so that the same code runs in plain
// loops on a CPU (tests/hostmath/lin_map_shim.hip); the kernels are thin wrappers.  fp64, no MFMA: like the sweep this is bound by HBM
// (per factor and iteration d(2d+1) + 6d doubles against d(2d+1) + 2d + 8(d+P) of a sweep).
// Per-variable kernels: 256 threads, at most MAP_MAX_BLOCKS blocks striding over the variables, so the partials stay a few KiB.
#pragma once
#include "gbp_lin_handle.hpp"
#include "gbp_math.hpp"

namespace gbp {

constexpr int MAP_BLOCK = 256, MAP_MAX_BLOCKS = 1024;

// ---- per-factor / per-variable routines (host and device) --------------------------------------------------------------------------

// (ya; yb) = Lambda_f (p_a; p_b), Lambda_f packed upper 2d x 2d in SoA rows [at][F], p gathered from the [N][d] vector `src`
template <int D>
GBP_HD void map_factor_apply(const LinParams &p, int f, const double *src, double (&ya)[D], double (&yb)[D])
{
    constexpr int N2 = 2 * D;
    const size_t F = (size_t)p.F;
    double x[N2], y[N2];
    const double *pa = src + (size_t)p.va[f] * D, *pb = src + (size_t)p.vb[f] * D;
#pragma unroll
    for (int k = 0; k < D; ++k) { x[k] = pa[k]; x[D + k] = pb[k]; y[k] = 0.0; y[D + k] = 0.0; }
#pragma unroll
    for (int i = 0; i < N2; ++i) {
#pragma unroll
        for (int j = i; j < N2; ++j) {
            const double a = p.flam[(size_t)Sym<N2>::at(i, j) * F + f];
            y[i] += a * x[j];
            if (j != i) y[j] += a * x[i];
        }
    }
    if (p.w) {                                            // the joint at the current robust weights (gbp_lin_robust.hpp; gbp.py:94-98)
        const double w = p.w[f];
#pragma unroll
        for (int k = 0; k < N2; ++k) y[k] *= w;
    }
#pragma unroll
    for (int k = 0; k < D; ++k) { ya[k] = y[k]; yb[k] = y[D + k]; }
}

// D_v = prior Lambda_v + sum over the adjacency run of the factor's own diagonal block (times its robust weight, if losses are set)
// -> LDL^T in ldl[v] = (packed factor | 1/d); eta_joint,v -> jeta[v].  Returns |eta_joint,v|^2.
template <int D>
GBP_HD double map_var_setup(const LinParams &p, int v, double *ldl, double *jeta)
{
    constexpr int P = LinDims<D>::P, R = D + P;
    const size_t F = (size_t)p.F;
    double a[P], e[D], invd[D];
#pragma unroll
    for (int k = 0; k < D; ++k) e[k] = p.prior[(size_t)v * R + k];
#pragma unroll
    for (int k = 0; k < P; ++k) a[k] = p.prior[(size_t)v * R + D + k];
    for (int ed = p.vptr[v]; ed < p.vptr[v + 1]; ++ed) {
        const int f = p.vadj[ed] >> 1, o = (p.vadj[ed] & 1) * D;
        const double w = p.w ? p.w[f] : 1.0;              // times 1 is exact: the plain joint keeps its bits
#pragma unroll
        for (int k = 0; k < D; ++k) e[k] += w * p.feta[(size_t)(o + k) * F + f];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = i; j < D; ++j) a[Sym<D>::at(i, j)] += w * p.flam[(size_t)(o ? Sym<2 * D>::at(D + i, D + j) : Sym<2 * D>::at(i, j)) * F + f];
    }
    ldl_factor<D>(a, invd);
    double ee = 0.0;
#pragma unroll
    for (int k = 0; k < P; ++k) ldl[(size_t)v * R + k] = a[k];
#pragma unroll
    for (int k = 0; k < D; ++k) { ldl[(size_t)v * R + P + k] = invd[k]; jeta[(size_t)v * D + k] = e[k]; ee += e[k] * e[k]; }
    return ee;
}

// z = D_v^-1 r from the stored LDL^T
template <int D>
GBP_HD void map_block_solve(const double *ldl, int v, const double (&r)[D], double (&z)[D])
{
    constexpr int P = LinDims<D>::P, R = D + P;
    double a[P];
#pragma unroll
    for (int k = 0; k < P; ++k) a[k] = ldl[(size_t)v * R + k];
#pragma unroll
    for (int k = 0; k < D; ++k) z[k] = r[k];
    ldl_forward<D>(a, z);
#pragma unroll
    for (int k = 0; k < D; ++k) z[k] *= ldl[(size_t)v * R + P + k];
    ldl_backward<D>(a, z);
}

// dst_v = prior Lambda_v src_v + the variable's edge run of ebuf, in adjacency order.  Returns src_v . dst_v.
template <int D>
GBP_HD double map_var_gather(const LinParams &p, int v, const double *src, const double *ebuf, double *dst)
{
    constexpr int P = LinDims<D>::P, R = D + P;
    double x[D], y[D];
#pragma unroll
    for (int k = 0; k < D; ++k) { x[k] = src[(size_t)v * D + k]; y[k] = 0.0; }
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
        for (int k = 0; k < D; ++k) y[k] += ebuf[(size_t)ed * D + k];
    }
    double xy = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) { dst[(size_t)v * D + k] = y[k]; xy += x[k] * y[k]; }
    return xy;
}

// r_v = eta_v - q_v (q == nullptr: eta_v), z_v = D_v^-1 r_v, p_v = z_v; adds r.z and r.r of the variable
template <int D>
GBP_HD void map_var_restart(int v, const double *ldl, const double *jeta, const double *q, double *r, double *z, double *pd, double &rz, double &rr)
{
    double rv[D], zv[D];
#pragma unroll
    for (int k = 0; k < D; ++k) rv[k] = q ? jeta[(size_t)v * D + k] - q[(size_t)v * D + k] : jeta[(size_t)v * D + k];
    map_block_solve<D>(ldl, v, rv, zv);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        r[(size_t)v * D + k] = rv[k]; z[(size_t)v * D + k] = zv[k]; pd[(size_t)v * D + k] = zv[k];
        rz += rv[k] * zv[k]; rr += rv[k] * rv[k];
    }
}

// x_v += alpha p_v, r_v -= alpha q_v, z_v = D_v^-1 r_v; adds r.z and r.r of the variable
template <int D>
GBP_HD void map_var_step(int v, double alpha, const double *ldl, const double *pd, const double *q, double *x, double *r, double *z, double &rz, double &rr)
{
    double rv[D], zv[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        x[(size_t)v * D + k] += alpha * pd[(size_t)v * D + k];
        rv[k] = r[(size_t)v * D + k] - alpha * q[(size_t)v * D + k];
    }
    map_block_solve<D>(ldl, v, rv, zv);
#pragma unroll
    for (int k = 0; k < D; ++k) {
        r[(size_t)v * D + k] = rv[k]; z[(size_t)v * D + k] = zv[k];
        rz += rv[k] * zv[k]; rr += rv[k] * rv[k];
    }
}

// p_v = z_v + beta p_v
template <int D>
GBP_HD void map_var_dir(int v, double beta, const double *z, double *pd)
{
#pragma unroll
    for (int k = 0; k < D; ++k) pd[(size_t)v * D + k] = z[(size_t)v * D + k] + beta * pd[(size_t)v * D + k];
}

// a / b of two sums of the recurrence; 0 once the residual is exactly zero (further iterations then change nothing)
GBP_HD double map_ratio(double a, double b) { return b > 0.0 ? a / b : 0.0; }

// ---- kernels -----------------------------------------------------------------------------------------------------------------------

// the same value in every thread of a 256-thread block, added in a fixed order; `red` is reusable after the call
GBP_DEV double map_block_sum(double v, double *red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const double s = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return s;
}

// sum of `nb` per-block partials, bit-identical in every thread of every block
GBP_DEV double map_sum_partials(const double *part, int nb, double *red)
{
    double a = 0.0;
    for (int i = threadIdx.x; i < nb; i += MAP_BLOCK) a += part[i];
    return map_block_sum(a, red);
}

// One wave per block (the LDS transpose below is ordered by s_waitcnt alone, as in k_lin_factor).  Lanes past the last factor redo it and
// store nothing.
template <int D>
__global__ __launch_bounds__(64) void k_map_factor(LinParams p, const double *src, double *ebuf)
{
    __shared__ double tr[64 * D];
    __shared__ int tp[64];
    const int lane = threadIdx.x;
    const int nlive = min(64, p.F - (int)blockIdx.x * 64);  // factors of this wave (> 0 by the launch grid)
    const int f = blockIdx.x * 64 + min(lane, nlive - 1);
    double ya[D], yb[D];
    map_factor_apply<D>(p, f, src, ya, yb);
    // 64 d-vectors staged in LDS and written as contiguous d-double runs, 64/d records per store instruction
    auto stage_out = [&](const double (&y)[D], const int *epos) {
#pragma unroll
        for (int k = 0; k < D; ++k) tr[lane * D + k] = y[k];
        tp[lane] = epos[f];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // one wave per block
        constexpr int G = 64 / D;
        const int g = lane / D, k = lane - g * D;
        if (g < G) {
            if (nlive == 64) {
#pragma unroll
                for (int j0 = 0; j0 < 64; j0 += G) {
                    const int j = j0 + g;
                    if (j < 64) ebuf[(size_t)tp[j] * D + k] = tr[j * D + k];
                }
            } else {
                for (int j = g; j < nlive; j += G) ebuf[(size_t)tp[j] * D + k] = tr[j * D + k];
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    };
    stage_out(ya, p.epos_a);
    stage_out(yb, p.epos_b);
}

template <int D>
__global__ __launch_bounds__(MAP_BLOCK) void k_map_var(LinParams p, const double *src, const double *ebuf, double *dst, double *pq_part)
{
    __shared__ double red[MAP_BLOCK / 64];
    double acc = 0.0;
    for (long long v = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; v < p.N; v += (long long)gridDim.x * MAP_BLOCK)
        acc += map_var_gather<D>(p, (int)v, src, ebuf, dst);
    acc = map_block_sum(acc, red);
    if (threadIdx.x == 0) pq_part[blockIdx.x] = acc;
}

template <int D>
__global__ __launch_bounds__(MAP_BLOCK) void k_map_setup(LinParams p, LinMap m)
{
    __shared__ double red[MAP_BLOCK / 64];
    double acc = 0.0;
    for (long long v = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; v < p.N; v += (long long)gridDim.x * MAP_BLOCK)
        acc += map_var_setup<D>(p, (int)v, m.ldl, m.jeta);
    acc = map_block_sum(acc, red);
    if (threadIdx.x == 0) m.rr_part[blockIdx.x] = acc;      // |eta|^2, read by the host right after
}

// slot: which half of rz_part receives r . z (the parity the NEXT iteration reads as "old")
template <int D>
__global__ __launch_bounds__(MAP_BLOCK) void k_map_restart(LinMap m, int N, int use_q, int slot)
{
    __shared__ double red[MAP_BLOCK / 64];
    double rz = 0.0, rr = 0.0;
    for (long long v = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; v < N; v += (long long)gridDim.x * MAP_BLOCK)
        map_var_restart<D>((int)v, m.ldl, m.jeta, use_q ? m.q : nullptr, m.r, m.z, m.p, rz, rr);
    rz = map_block_sum(rz, red);
    rr = map_block_sum(rr, red);
    if (threadIdx.x == 0) { m.rz_part[(size_t)slot * m.nb + blockIdx.x] = rz; m.rr_part[blockIdx.x] = rr; }
}

// par = iteration & 1: reads (r.z)_old from the other slot, writes the new one into slot `par`
template <int D>
__global__ __launch_bounds__(MAP_BLOCK) void k_map_step(LinMap m, int N, int par)
{
    __shared__ double red[MAP_BLOCK / 64];
    const double rz_old = map_sum_partials(m.rz_part + (size_t)(par ^ 1) * m.nb, m.nb, red);
    const double pq = map_sum_partials(m.pq_part, m.nb, red);
    const double alpha = map_ratio(rz_old, pq);
    double rz = 0.0, rr = 0.0;
    for (long long v = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; v < N; v += (long long)gridDim.x * MAP_BLOCK)
        map_var_step<D>((int)v, alpha, m.ldl, m.p, m.q, m.x, m.r, m.z, rz, rr);
    rz = map_block_sum(rz, red);
    rr = map_block_sum(rr, red);
    if (threadIdx.x == 0) { m.rz_part[(size_t)par * m.nb + blockIdx.x] = rz; m.rr_part[blockIdx.x] = rr; }
}

template <int D>
__global__ __launch_bounds__(MAP_BLOCK) void k_map_dir(LinMap m, int N, int par)
{
    __shared__ double red[MAP_BLOCK / 64];
    const double rz_new = map_sum_partials(m.rz_part + (size_t)par * m.nb, m.nb, red);
    const double rz_old = map_sum_partials(m.rz_part + (size_t)(par ^ 1) * m.nb, m.nb, red);
    const double beta = map_ratio(rz_new, rz_old);
    for (long long v = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; v < N; v += (long long)gridDim.x * MAP_BLOCK)
        map_var_dir<D>((int)v, beta, m.z, m.p);
}

// x0 = the belief means (warm start)
template <int D>
__global__ __launch_bounds__(MAP_BLOCK) void k_map_load_means(LinParams p, LinMap m)
{
    constexpr int REC = LinDims<D>::REC, R = D + LinDims<D>::P;
    for (long long v = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; v < p.N; v += (long long)gridDim.x * MAP_BLOCK)
#pragma unroll
        for (int k = 0; k < D; ++k) m.x[(size_t)v * D + k] = p.bel[(size_t)v * REC + R + k];
}

// per-block partials of |means - x|^2 (ndim_posegraph.py:108) into pq_part
template <int D>
__global__ __launch_bounds__(MAP_BLOCK) void k_map_distance(LinParams p, LinMap m)
{
    constexpr int REC = LinDims<D>::REC, R = D + LinDims<D>::P;
    __shared__ double red[MAP_BLOCK / 64];
    double acc = 0.0;
    for (long long v = (long long)blockIdx.x * MAP_BLOCK + threadIdx.x; v < p.N; v += (long long)gridDim.x * MAP_BLOCK)
#pragma unroll
        for (int k = 0; k < D; ++k) { const double d = p.bel[(size_t)v * REC + R + k] - m.x[(size_t)v * D + k]; acc += d * d; }
    acc = map_block_sum(acc, red);
    if (threadIdx.x == 0) m.pq_part[blockIdx.x] = acc;
}

}  // namespace gbp
