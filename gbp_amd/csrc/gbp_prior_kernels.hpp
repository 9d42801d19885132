// gbp_prior_kernels.hpp -- the kernels of gbp_capi.hip: the layout check, the priors (generate_priors_var gbp_ba.py:20-34, weaken_priors
// gbp_ba.py:36-42) and the digest of the layout.  The priors are a per-slot max of Lambda_f (k_factor_lambda_max), a segmented max per
// landmark over its contiguous slots, a per-camera max through the camera's adj_factors list, and k_prior_scalars -- no F-sized array
// crosses PCIe after the observations themselves went up.  (The kernels of the graph build: gbp_build.hpp -> gbp_capi_build.hip.)
#pragma once
#include "gbp_kernels.hpp"

namespace gbp {

// Debug check of the layout the build produced (GBP_DEBUG_LAYOUT=1 and the tests): every used slot decodes to the camera and
// landmark of the reference factor it holds, and the two maps invert each other.  err[0] = number of bad slots.
__global__ __launch_bounds__(BLOCK) void k_check_layout(Params p, const int *__restrict__ ref_cam, const int *__restrict__ ref_lmk,
                                                        int *__restrict__ err)
{
    const int slot = blockIdx.x * BLOCK + threadIdx.x;
    int cam, lmk;
    if (slot >= p.T * WTILE || !slot_info(p, slot, cam, lmk)) return;
    const int r = p.cpos[slot];
    if (r < 0 || r >= p.F || p.cadj[r] != slot || ref_cam[r] != cam || ref_lmk[r] != lmk || lmk < 0 || lmk >= p.L) atomicAdd(err, 1);
}

// ---- priors: generate_priors_var gbp_ba.py:20-34 ------------------------------------------------------------------------
// max over a landmark's adjacent factors of max(Lambda_f): its slots are contiguous
__global__ __launch_bounds__(BLOCK) void k_lmk_max(Params p, const double *__restrict__ fm, double *__restrict__ lmk_max)
{
    const int l = blockIdx.x * BLOCK + threadIdx.x;
    if (l >= p.L) return;
    const int2 rows = *reinterpret_cast<const int2 *>(p.lrec + (size_t)l * LREC + LR_ROWS);
    double m = 0.0;                                     // max_factor_lam = 0.  gbp_ba.py:27
    for (int s = rows.x; s < rows.y; ++s) m = fmax(m, fm[s]);
    lmk_max[l] = m;
}

// one workgroup per camera: max over its adj_factors list (cadj = reference id -> slot)
__global__ __launch_bounds__(BLOCK) void k_cam_max(Params p, const double *__restrict__ fm, double *__restrict__ cam_max)
{
    __shared__ double red[BLOCK / 64];
    const int c = blockIdx.x;
    double m = 0.0;
    for (int e = p.cptr[c] + threadIdx.x; e < p.cptr[c + 1]; e += BLOCK) m = fmax(m, fm[p.cadj[e]]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < BLOCK / 64; ++w) m = fmax(m, red[w]);
        cam_max[c] = m;
    }
}

// prior Lambda = (lambda / w2) I, eta = Lambda mu   (gbp_ba.py:32-34; w2 = weaker_factor^2, 1 when the caller gives Lambda), on cameras
// [c0, c1) and landmarks [l0, l1) (all of them but after gbp_ba_extend, which sets the new variables' priors alone).  Landmarks are
// walked, and the range is meant, in the CALLER's numbering: lmk_map (NULL: identity) turns it into the internal one, and lmk_lambda is
// indexed by the caller's id (lambda_by_user: scalars that came in from outside) or by the internal one (the maxima of k_lmk_max).
__global__ __launch_bounds__(BLOCK) void k_prior_scalars(Params p, const double *__restrict__ cam_lambda, const double *__restrict__ lmk_lambda,
                                                         double w2, int c0, int c1, int l0, int l1, const int *__restrict__ lmk_map, int lambda_by_user)
{
    const int v = blockIdx.x * BLOCK + threadIdx.x;
    if (v < p.C ? (v < c0 || v >= c1) : (v - p.C < l0 || v - p.C >= l1)) return;
    if (v < p.C) {
        const double lam = cam_lambda[v] / w2;
        double *pr = p.cprior + (size_t)v * 27;
#pragma unroll
        for (int k = 0; k < 27; ++k) pr[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) { pr[k] = lam * p.cbel[(size_t)v * CAMREC + CAM_MU + k]; pr[6 + Sym<6>::at(k, k)] = lam; }
    } else if (v < p.C + p.L) {
        const int u = v - p.C, l = lmk_map ? lmk_map[u] : u;
        const double lam = lmk_lambda[lambda_by_user ? u : l] / w2;
        double *lr = p.lrec + (size_t)l * LREC;
#pragma unroll
        for (int k = 0; k < 9; ++k) lr[LR_PRIOR + k] = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) { lr[LR_PRIOR + k] = lam * lr[LR_MU + k]; lr[LR_PRIOR + 3 + Sym<3>::at(k, k)] = lam; }
    }
}

// packed landmark priors (eta 3 | Lambda 6), in the caller's numbering, into the landmark records (lmk_map: caller's id -> internal, NULL: identity)
__global__ __launch_bounds__(BLOCK) void k_scatter_lmk_priors(Params p, const double *__restrict__ pri, const int *__restrict__ lmk_map)
{
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= (size_t)p.L * 9) return;
    const size_t u = i / 9, l = lmk_map ? (size_t)lmk_map[u] : u;
    p.lrec[l * LREC + LR_PRIOR + (i % 9)] = pri[i];
}

// order-independent 64-bit digest of the factor layout (reference id -> slot, camera, landmark): pins a state blob to its graph
__global__ __launch_bounds__(BLOCK) void k_graph_hash(const int *__restrict__ ref2slot, const int *__restrict__ ref_cam,
                                                      const int *__restrict__ ref_lmk, int F, unsigned long long *__restrict__ out)
{
    const int r = blockIdx.x * BLOCK + threadIdx.x;
    unsigned long long v = 0ull;
    if (r < F) {
        v = ((unsigned long long)(unsigned)r << 32) ^ (unsigned)ref2slot[r];
        v = (v ^ (v >> 33)) * 0xff51afd7ed558ccdull;
        v ^= ((unsigned long long)(unsigned)ref_cam[r] << 32) | (unsigned)ref_lmk[r];
        v = (v ^ (v >> 33)) * 0xc4ceb9fe1a85ec53ull;
        v ^= v >> 33;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(out, v);
}

// ---- priors: per-factor maximum of Lambda_f (gbp_ba.py:27-31), weaken_priors (gbp_ba.py:36-42) ----
// np.max(factor.factor.lam) per factor at its current linearisation point (gbp_ba.py:31); 0 for empty slots
__global__ __launch_bounds__(BLOCK) void k_factor_lambda_max(Params p, double *__restrict__ fmax_out)
{
    const int slot = blockIdx.x * BLOCK + threadIdx.x;
    if (slot >= p.T * WTILE) return;
    int cam, lmk;
    if (!slot_info(p, slot, cam, lmk)) { fmax_out[slot] = 0.0; return; }
    double x0[9], Jc[2][6], Jl[2][3], h[2];
#pragma unroll
    for (int k = 0; k < 9; ++k) x0[k] = p.lin[lin_at(slot, ROW_X0 + k)];
    linearise(x0, p.K, Jc, Jl, h);
    const double av = slot_avar(p, slot);
    fmax_out[slot] = factor_lambda_max(Jc, Jl, 1.0 / av);
}


// BAFactorGraph.weaken_priors (gbp_ba.py:36-42): prior eta and Lambda of every variable times `factor`
__global__ __launch_bounds__(BLOCK) void k_weaken_priors(Params p, double factor)
{
    const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    const size_t nc = (size_t)p.C * 27, nl = (size_t)p.L * 9;
    if (i < nc) p.cprior[i] *= factor;
    else if (i < nc + nl) {
        const size_t j = i - nc;
        p.lrec[(j / 9) * LREC + LR_PRIOR + (j % 9)] *= factor;
    }
}


}  // namespace gbp
