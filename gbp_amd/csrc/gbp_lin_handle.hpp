// gbp_lin_handle.hpp -- what the translation units of the linear engine (include/gbp_lin.h) share: the kernel parameter block, the
// handle behind gbp_lin_t, the error / entry macros and the host helpers every entry point uses (the handle's one allocator among them).
// What create, extend and shrink share on the host -- a generation of the graph's arrays and its commit -- is gbp_lin_generation.hpp.
//   gbp_lin_capi.hip       create / destroy, the plain sweep and energy (launches; the stage kernels are gbp_lin_sweep.hpp), getters
//   gbp_lin_capi_map.hip   the batch MAP by block-Jacobi conjugate gradients (kernels in gbp_lin_map.hpp)
//   gbp_lin_capi_marg.hip  exact marginal covariances by the same iteration on 8 columns at a time (kernels in gbp_lin_marg.hpp)
//   gbp_lin_capi_robust.hip  robust losses: one weight per factor from the current belief means (kernels in gbp_lin_robust.hpp)
//   gbp_lin_capi_extend.hip  growing a live graph: the layout rebuilt on the device (kernels in gbp_lin_extend.hpp)
//   gbp_lin_capi_shrink.hip  shrinking a live graph: retired variables folded into priors (kernels in gbp_lin_shrink.hpp)
//   gbp_lin_capi_until.hip   sweeps until a tolerance is met, decided on the device, with a per-sweep trace: the gated and traced forms of
//                            the same stage kernels (parameter blocks LinGated / LinTraced below), and what is the call's alone
//                            (gbp_lin_until.hpp)
//   gbp_lin_capi_until_nonlin.hip  the same on a handle with nonlinear factors: the relinearise, factor and energy stages of such a sweep in
//                            their gated forms (LinGated, LinRelinGated below), the traced belief stage, and the finishing kernel reading
//                            the sweep's relinearisation count (UntilSettled, gbp_lin_until.hpp)
//   gbp_lin_capi_nonlin.hip  nonlinear pairwise factors relinearised on the device (kernels in gbp_lin_nonlin.hpp): the relinearise stage,
//                            the factor stage with per-factor damping (parameter block LinRelin below), the model-aware energy; growing and
//                            shrinking such a handle are gbp_lin_extend_nonlinear / gbp_lin_shrink_nonlinear in the extend / shrink units
//   gbp_lin_capi_map_nonlin.hip  the nonlinear batch MAP of such a handle by Levenberg-Marquardt: linearisation at a point of the solver's
//                            own, damped priors and the step test (kernels in gbp_lin_gn.hpp) around the conjugate gradients of
//                            gbp_lin_capi_map.hip, which run on a LinParams copy pointing at the solver's arrays
//   gbp_lin_capi_map_irls.hip  the robust nonlinear batch MAP: that Levenberg-Marquardt loop (gn_lm, one function for both entry points)
//                            inside rounds of re-made weights -- a reweight lane at the solver's own x (k_gn_reweight, gbp_lin_gn.hpp)
//                            into weights of the solver's own, which the round's LinParams::w points at
//   gbp_lin_capi_nonlin_robust.hip  robust losses on such a handle: the weight made at the linearisation point by the relinearise lane
//                            (k_lin_relin<MODEL, true>), and the factor stage with weight and per-factor damping together
#pragma once
#include "../../include/gbp_ba.h"
#include "../../include/gbp_lin.h"
#include "gbp_math.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <vector>

namespace gbp {
int set_error(int code, const char *fmt, ...);      // gbp_capi.hip: thread-local message behind gbp_last_error()

struct LinParams {
    int N, F;
    double damping;
    const int *va, *vb;          // [F]
    const double *feta, *flam;   // [2D][F], [D(2D+1)][F] packed upper
    const double *fconst;        // [F]
    double *msg_a, *msg_b;       // [D + D(D+1)/2][F] each: eta rows then packed Lambda rows
    double *bel;                 // [N][D + P + D]
    const double *prior;         // [N][D + P]
    const int *vptr, *vadj;      // CSR: variable -> (factor << 1 | side), ascending factor id
    double *vmsg;                // [2F][D + P]: the same messages in VARIABLE-major (CSR edge) order, for the belief stage
    const int *epos_a, *epos_b;  // [F]: CSR edge index of (factor, side)
    const double *w;             // [F] robust weights of the nominal factors (gbp_lin_robust.hpp), or nullptr: no losses set, all 1
};

// Robust losses (gbp_lin_robust.hpp): device memory owned by gbp_lin::allocs, allocated by the first gbp_lin_set_robust of a handle.
struct LinRobust {
    const int *loss;             // [F] GBP_LIN_LOSS_*
    const double *thr, *nvar;    // [F] Mahalanobis threshold, noise variance (read for the constant loss only)
    double *w;                   // [F] what LinParams::w points at while losses are set
    int *flag;                   // [F] Factor.robust_flag
};

template <int D> struct LinDims {
    static constexpr int P = D * (D + 1) / 2;       // packed d x d
    static constexpr int P2 = D * (2 * D + 1);      // packed 2d x 2d
    static constexpr int REC = D + P + D;           // belief record
};

// Batch-MAP solver state (gbp_lin_map.hpp): every pointer is device memory owned by gbp_lin::allocs, allocated on the first call that needs it.
struct LinMap {
    double *ldl, *jeta;              // [N][P + D] LDL^T of the joint's diagonal blocks (packed factor | 1/d), [N][D] joint eta
    double *x, *r, *z, *p, *q;       // [N][D] each: iterate, residual, preconditioned residual, direction, Lambda_joint p
    double *ebuf;                    // [2F][D]: per-(factor, side) products in CSR edge order
    double *pq_part, *rz_part, *rr_part;   // [nb], [2][nb], [nb]: per-block partial sums (rz: one slot per iteration parity)
    int nb;                          // blocks of every per-variable kernel = number of partials
};

// Multi-column workspace of the marginal covariances (gbp_lin_marg.hpp), K = GBP_LIN_MARG_COLS columns innermost: device memory owned by
// gbp_lin::allocs, allocated by the first gbp_lin_solve_marginals of a handle.  The LDL^T of the diagonal blocks is LinMap's.
struct LinMarg {
    double *x, *r, *z, *p, *q;       // [N][D][K] each
    double *ebuf;                    // [2F][D][K]
    double *pq_part, *rz_part, *rr_part;   // [nb][K], [2][nb][K], [nb][K]: per-block, per-column partial sums
    int nb;                          // blocks of every per-variable kernel
    void *stage;                     // the outputs (sigma | sigma_joint) then the ids of the call in progress; grows as calls need
    size_t stage_bytes;
};

// Workspace of gbp_lin_iterate_until (gbp_lin_until.hpp): device memory owned by gbp_lin::allocs, allocated by the first call.  The
// partials are sized by N and F and go with a generation (lin_drop_solvers); the stop word and the trace buffer stay.
struct LinUntil {
    double *bel_part;                // [2][nbel] per block of the traced belief stage: max |mu_new - mu_old|, then sum (mu - x)^2
    double *en_part;                 // [nen] per block of the energy pass
    int nbel, nen;
    double *trace;                   // [cap][3]: row i = (step, energy, MAP distance) after sweep i + 1 of the call in progress
    int cap;                         // rows of `trace`: the largest max_iters seen
    int *stop;                       // [2]: GBP_LIN_STOP_* (0: go on), and the sweep that decided
};

// Workspace of gbp_lin_solve_map_nonlinear (gbp_lin_gn.hpp): device memory owned by gbp_lin::allocs, allocated by the first call, sized
// by N and F and dropped with a generation (lin_drop_solvers).  The inner solves run in LinMap's workspace; LinMap::x is the candidate.
struct LinGn {
    double *feta, *flam;             // [2D][F], [P2][F]: the linearisation at x -- the solver's, never the handle's
    double *prior;                   // [N][D + P]: the damped copy of the priors
    double *x;                       // [N][D]: the current point
    double *e_part;                  // [2][nen]: per-block partials of the factor energy at x, and at the candidate
    double *v_part;                  // [2][nb]: per-block partials of the prior difference, and of max |x_c - x|
    double *out;                     // [GN_OUT]: what the host downloads per step
    int nen, nb;
    bool alloc;
    // gbp_lin_solve_map_nonlinear_robust (gbp_lin_capi_map_irls.hip) adds its own, all or nothing on ITS first call (`irls`):
    double *w;                       // [F]: the solver's weights, made at x -- never LinRobust::w
    int *flag;                       // [F]: M_f(x) > t_f
    double *xs;                      // [N][D]: x at the start of the round
    double *w_part;                  // [nen]: per-block partials of max |w_new - w_old|
    int *count;                      // [1]: the flagged factors of the last reweight
    double *rout;                    // [GN_RW_OUT]: what the host downloads per reweight
    bool irls;
};

// Nonlinear factors (gbp_lin_nonlin.hpp): device memory owned by gbp_lin::allocs, allocated by gbp_lin_set_nonlinear.  Everything
// per-factor is SoA with stride F like the rest of the handle, and travels with a generation: gbp_lin_extend_nonlinear /
// gbp_lin_shrink_nonlinear rebuild the five per-factor arrays with the graph's, and lin_gen_commit (gbp_lin_generation.hpp) installs
// them.  feta / flam are the handle's own factor arrays (LinParams::feta / flam), writable; the same commit re-points them.
// Per model: D, the dofs of a variable, and M, the rows of a measurement -- 3 and 3 for GBP_LIN_MODEL_SE2_BETWEEN, 6 and 6 for
// GBP_LIN_MODEL_SE3_BETWEEN.  NonlinModel<MODEL>::D / ::M (gbp_lin_nonlin.hpp) are the same numbers where the model is a template
// argument; these two are for the host code that has the handle's model as a value (0: not a model).
constexpr int lin_model_dofs(int model) { return model == GBP_LIN_MODEL_SE2_BETWEEN ? 3 : model == GBP_LIN_MODEL_SE3_BETWEEN ? 6 : 0; }
constexpr int lin_model_rows(int model) { return lin_model_dofs(model); }
struct LinNonlin {
    const double *meas, *sinfo;      // [M][F] measurement z, square-root information s
    double *linpoint;                // [2D][F] Factor.linpoint gbp.py:231 = [xa; xb]
    int *iters;                      // [F] Factor.iters_since_relin gbp.py:249
    double *fdamp;                   // [F] Factor.eta_damping gbp.py:248
    double *feta, *flam;             // what the relinearise stage rewrites
    int *counts;                     // [cap] factors relinearised per sweep of the call in progress
    int cap;                         // the largest n_iters seen (at least 1)
    int *rcounts;                    // [rcap] factors flagged per sweep of gbp_lin_iterate_nonlinear_robust; allocated with the robust arrays
    int rcap;                        // the largest n_iters that call has seen (at least 1 once losses were set; 0 before)
    double beta;                     // FactorGraph.beta gbp.py:32
    int num_undamped, min_linear;    // gbp.py:33-34
    int model;                       // GBP_LIN_MODEL_*
};

// The parameter block selects the form of a stage kernel (gbp_lin_sweep.hpp, gbp_lin_robust.hpp).  LinParams: the plain form;
// lin_stopped() is the constant false and the gate compiles away.  LinGated: a sweep queued by gbp_lin_iterate_until, which returns at
// its head once stop[0] != 0 (an earlier sweep of the call met a tolerance).  LinTraced: the belief stage of such a sweep, gated and with
// the trace of its block; x: the MAP iterate [N][D], or nullptr when the distance is not asked for.
struct LinGated : LinParams {
    const int *stop;
};
struct LinTraced : LinParams {
    LinUntil u;
    const double *x;
};
// LinRelin: the factor stage of a sweep of gbp_lin_iterate_nonlinear, where every factor has a damping of its own (gbp.py:50-52).
struct LinRelin : LinParams {
    const double *fdamp;         // [F] Factor.eta_damping gbp.py:248
};
// LinRelinGated: that factor stage in a sweep queued by gbp_lin_iterate_until_nonlinear: the factor's own damping, and the stop word.
struct LinRelinGated : LinRelin {
    const int *stop;
};
GBP_DEV double lin_damping(const LinParams &p, int) { return p.damping; }
GBP_DEV double lin_damping(const LinRelin &p, int f) { return p.fdamp[f]; }
GBP_DEV double lin_damping(const LinRelinGated &p, int f) { return p.fdamp[f]; }
GBP_DEV bool lin_stopped(const LinParams &) { return false; }
GBP_DEV bool lin_stopped(const LinGated &p) { return p.stop[0] != 0; }
GBP_DEV bool lin_stopped(const LinTraced &p) { return p.u.stop[0] != 0; }
GBP_DEV bool lin_stopped(const LinRelinGated &p) { return p.stop[0] != 0; }

}  // namespace gbp

using namespace gbp;

struct gbp_lin {
    LinParams p{};
    int D = 0, device = 0;
    hipStream_t stream = nullptr;
    std::vector<void *> allocs;
    double *d_red = nullptr;
    int red_blocks = 0;
    bool has_beliefs = false, has_const = false;
    LinMap map{};                    // gbp_lin_capi_map.hip
    bool map_alloc = false;          // the workspace exists
    bool map_ready = false;          // the LDL^T of the diagonal blocks and the joint eta are those of the current weights
    bool map_solved = false;
    double map_eta_norm = 0.0;
    LinMarg marg{};                  // gbp_lin_capi_marg.hip
    bool marg_ready = false;
    LinRobust rob{};                 // gbp_lin_capi_robust.hip
    bool rob_alloc = false;          // rob's arrays exist; losses are set while p.w != nullptr
    LinUntil until{};                // gbp_lin_capi_until.hip
    LinNonlin nl{};                  // gbp_lin_capi_nonlin.hip
    bool nonlinear = false;          // gbp_lin_set_nonlinear was called: (eta_f, Lambda_f) are those of nl.linpoint
    LinGn gn{};                      // gbp_lin_capi_map_nonlin.hip
};

#define LHIPCHK(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t e__ = (expr);                                                                            \
        if (e__ != hipSuccess)                                                                              \
            return set_error(e__ == hipErrorOutOfMemory ? GBP_ENOMEM : GBP_EHIP, "%s failed: %s (%s:%d)",   \
                             #expr, hipGetErrorString(e__), __FILE__, __LINE__);                            \
    } while (0)
#define LCHK(expr) do { int rc__ = (expr); if (rc__ != GBP_OK) return rc__; } while (0)
#define LENTER(h)                                                                        \
    do {                                                                                 \
        if (!(h)) return set_error(GBP_EINVAL, "NULL handle");                           \
        LHIPCHK(hipSetDevice((h)->device));                                              \
    } while (0)

namespace gbp {
int lin_map_prepare(gbp_lin *h);                    // gbp_lin_capi_map.hip: LinMap's workspace (once per handle), LDL^T and joint eta (per set of weights)
// gbp_lin_capi_map.hip, the host side of the conjugate gradients over ANY joint: `p` names the factors, priors and weights (the handle's
// own LinParams, or a copy pointing elsewhere), `m` the workspace.  None of them reads or writes map_ready / map_solved / map_eta_norm.
int lin_map_workspace(gbp_lin *h);                  // LinMap's workspace, once per generation
int lin_map_setup(gbp_lin *h, const LinParams &p, const LinMap &m, double *eta_norm);   // LDL^T of the diagonal blocks, joint eta, |eta|
int lin_map_matvec(gbp_lin *h, const LinParams &p, const LinMap &m, const double *src, double *dst);   // dst = Lambda_joint src; partials of src . dst in pq_part
int lin_map_restart(gbp_lin *h, const LinParams &p, const LinMap &m, int use_q, int next_it, double *rnorm);   // r = eta - q (or eta), z, p = z; *rnorm = |r|
enum { LIN_MAP_FROM_ZERO = 0, LIN_MAP_FROM_MEANS = 1, LIN_MAP_FROM_X = 2 };   // x0 of lin_map_solve: 0, the belief means, what m.x holds
int lin_map_solve(gbp_lin *h, const LinParams &p, const LinMap &m, double eta_norm, const gbp_lin_map_opts_t &o, int start, gbp_lin_map_info_t *info,
                  double *rnorm0 /* |eta - Lambda x0|, or NULL */);
int lin_sweep(gbp_lin *h);                          // gbp_lin_capi.hip: one synchronous iteration at the weights as they stand, queued on the stream
int lin_nonlin_energy(gbp_lin *h, double *out);     // gbp_lin_capi_nonlin.hip: red_blocks partials (one per block of 256 factors, 0 past F) into `out` = d_red, queued on the stream
int lin_nonlin_linearise(gbp_lin *h, int f0, int f1);   // gbp_lin_capi_nonlin.hip: compute_factor on the factors [f0, f1) at their belief means, queued
void lin_nonlin_factor_stage(gbp_lin *h);           // gbp_lin_capi_nonlin.hip: the factor stage with per-factor damping, at the weights as they stand (if any), queued
int lin_nonlin_grow_counts(gbp_lin *h, int *&buf, int &cap, int n);   // gbp_lin_capi_nonlin.hip: a per-sweep counts buffer of at least n slots
int lin_until_workspace(gbp_lin *h, int max_iters); // gbp_lin_capi_until.hip: LinUntil's trace buffer of at least max_iters rows, the stop word, this generation's partials
}

// the entry points that a nonlinear handle refuses (include/gbp_lin.h): decided before anything changes
#define LIN_REFUSE_NONLINEAR(h, what)                                                                                       \
    do {                                                                                                                    \
        if ((h)->nonlinear) return set_error(GBP_ESTATE, what " is not available on a handle with nonlinear factors");      \
    } while (0)

// n elements of device memory (at least one), owned by the handle: gbp_lin_destroy frees whatever `allocs` still lists
template <typename T>
static int lin_alloc(gbp_lin *h, T **out, size_t n)
{
    void *q = nullptr;
    LHIPCHK(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)));
    h->allocs.push_back(q);
    *out = static_cast<T *>(q);
    return GBP_OK;
}

// gives one of the handle's arrays back before the handle goes; nullptr is nothing to free
inline void lin_free(gbp_lin *h, const void *q)
{
    if (!q) return;
    auto at = std::find(h->allocs.begin(), h->allocs.end(), q);
    if (at != h->allocs.end()) h->allocs.erase(at);
    (void)hipFree(const_cast<void *>(q));
}

template <typename K>
static void lin_dispatch(int D, K &&k)
{
    switch (D) {
    case 1: k(std::integral_constant<int, 1>{}); break;
    case 2: k(std::integral_constant<int, 2>{}); break;
    case 3: k(std::integral_constant<int, 3>{}); break;
    case 4: k(std::integral_constant<int, 4>{}); break;
    case 5: k(std::integral_constant<int, 5>{}); break;
    default: k(std::integral_constant<int, 6>{}); break;
    }
}

// the handle's model as a template argument: k(std::integral_constant<int, GBP_LIN_MODEL_*>).  gbp_lin_set_nonlinear admits no other value
template <typename K>
static void lin_model_dispatch(int model, K &&k)
{
    if (model == GBP_LIN_MODEL_SE3_BETWEEN) k(std::integral_constant<int, GBP_LIN_MODEL_SE3_BETWEEN>{});
    else k(std::integral_constant<int, GBP_LIN_MODEL_SE2_BETWEEN>{});
}
