/* gbp_lin.h -- C ABI of the MI355X engine for LINEAR pairwise Gaussian belief propagation (libgbp_hip.so).
 *
 * the generic path of joeaortiz/gbp (gbp/gbp.py FactorGraph with
 * nonlinear_factors=False, as built by ndim_posegraph.py with gbp/factors/linear_displacement.py:8-14)
 * for graphs whose factors all join TWO variables of the same size d <= 6.  A linear factor never
 * relinearises, so it is handed over once as its information form (eta_f, Lambda_f) over the
 * stacked variables [a; b] (Factor.compute_factor gbp.py:267-294 evaluated by the caller), and the
 * device runs FactorGraph.synchronous_iteration (gbp.py:86-92) = compute_all_messages with the
 * graph-level damping (gbp.py:52-54) + update_all_beliefs (gbp.py:56-58).
 *
 * Conventions as in gbp_ba.h: 0 or a negative GBP_E* code, message from gbp_last_error(); host
 * pointers caller-owned, contiguous C-order float64 / int32; dense matrices row-major; information form.
 * Variables and factors keep the caller's numbering; a variable's adjacency order (the order its
 * belief adds messages in, VariableNode.adj_factors gbp.py:160) is ascending factor id, which is what
 * ndim_posegraph.py:86-88 produces.
 *
 * Beside the sweep: the batch MAP (the `mu` of FactorGraph.joint_distribution_cov) and exact marginal covariances (its `sigma`, for
 * chosen variables), both by block-Jacobi conjugate gradients on the block-sparse joint; robust losses; growing and shrinking a live
 * graph; sweeps to convergence with the stop decided on the device (gbp_lin_iterate_until); and one NONLINEAR factor family, the SE(2)
 * relative-pose factor, relinearised on the device by the reference's local schedule (gbp_lin_set_nonlinear), on a handle that grows
 * and shrinks too (gbp_lin_extend_nonlinear / gbp_lin_shrink_nonlinear) and takes robust losses of its own, made at the linearisation
 * point as the reference makes them (gbp_lin_set_robust_nonlinear / gbp_lin_iterate_nonlinear_robust), and iterates to convergence on
 * the device as well (gbp_lin_iterate_until_nonlinear) -- below.
 */
#ifndef GBP_LIN_H
#define GBP_LIN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GBP_LIN_MAX_DOFS 6

typedef struct gbp_lin gbp_lin_t;

typedef struct {
    int32_t n_vars, dofs, n_factors, device;
    const int32_t *var_a, *var_b;  /* F each: Factor.adj_vIDs (gbp.py:225), a != b                          */
    const double *factor_eta;      /* F x 2d            Factor.factor.eta  gbp.py:291                         */
    const double *factor_lam;      /* F x 2d x 2d       Factor.factor.lam  gbp.py:292                         */
    const double *factor_const;    /* F or NULL: 0.5 |z - h(0)|^2 / sigma^2, the constant of Factor.energy gbp.py:261-265 */
    const double *prior_eta;       /* N x d             VariableNode.prior.eta  gbp.py:170                    */
    const double *prior_lam;       /* N x d x d         VariableNode.prior.lam                                 */
    double eta_damping;            /* FactorGraph.eta_damping  gbp.py:18                                       */
} gbp_lin_desc_t;

int  gbp_lin_create(gbp_lin_t **out, const gbp_lin_desc_t *d);                  /* graph construction ndim_posegraph.py:67-91 */
void gbp_lin_destroy(gbp_lin_t *h);
int  gbp_lin_sync(gbp_lin_t *h);
int  gbp_lin_update_beliefs(gbp_lin_t *h);                                      /* FactorGraph.update_all_beliefs gbp.py:56-58 */
int  gbp_lin_iterate(gbp_lin_t *h, int32_t n_iters);                            /* n x synchronous_iteration gbp.py:86-92      */
/* FactorGraph.energy gbp.py:36-44: sum_f 0.5 |h(mu) - z|^2 / sigma^2, evaluated per factor in residual form from a pivoted LDL^T of
 * Lambda_f (0.5 sum_k d_k (l_k^T x - y_k)^2 + const - 0.5 sum_k d_k y_k^2), not as 0.5 x^T Lambda_f x - eta_f^T x + const, which
 * cancels far from the origin; exact differences x_a - x_b for linear_displacement factors */
int  gbp_lin_energy(gbp_lin_t *h, double *out);
int  gbp_lin_get_beliefs(gbp_lin_t *h, double *eta, double *lam);               /* N x d, N x d x d   VariableNode.belief      */
int  gbp_lin_get_means(gbp_lin_t *h, double *mu);                               /* N x d   FactorGraph.get_means gbp.py:146-153 */
int  gbp_lin_get_messages(gbp_lin_t *h, double *eta_a, double *lam_a, double *eta_b, double *lam_b);   /* Factor.messages gbp.py:222 */

/* ---- batch MAP: FactorGraph.joint_distribution_inf / joint_distribution_cov (gbp.py:94-144) without the dense N d x N d inverse ----
 * The joint information form  Lambda = blockdiag(prior Lambda) + sum_f scatter(Lambda_f),  eta = prior eta + sum_f scatter(eta_f)
 * (gbp.py:94-126) is block-sparse and SPD; its solution Lambda^-1 eta (the means of gbp.py:139-144, the "MAP" that
 * ndim_posegraph.py:94,108 measures the GBP means against) is found on the device by conjugate gradients preconditioned with the d x d
 * diagonal blocks.  No floating-point atomics: two solves of one handle with the same options are bit-identical.  The sweep's state
 * (messages, beliefs) is neither read -- except by warm_start and gbp_lin_map_distance -- nor written.
 *
 * gbp_lin_map_opts_t: stop at |eta - Lambda x| <= rel_tol |eta|; the recurrence's residual is read every check_every iterations (every
 * iteration on a graph without factors, where one iteration is exact), so `iters` is a multiple of it unless max_iters cuts it short;
 * warm_start 1: x0 = the current belief means (GBP_ESTATE without beliefs), 0: x0 = 0.  NULL opts = {1e-12, 10000, 8, 0};
 * rel_tol <= 0, max_iters < 0 or check_every < 1: GBP_EINVAL.
 * gbp_lin_map_info_t: rel_residual is that of the TRUE residual, recomputed with one product when the recurrence claims convergence or
 * max_iters runs out (the recurrence restarts from it when the claim was wrong); converged = 0 with GBP_OK when max_iters ran out --
 * the iterate reached is still retrievable; eta_norm = |eta|_2.  eta = 0 gives x = 0, converged, 0 iterations.  info may be NULL. */
typedef struct { double rel_tol; int32_t max_iters, check_every, warm_start; } gbp_lin_map_opts_t;
typedef struct { int32_t iters, converged; double rel_residual, eta_norm; } gbp_lin_map_info_t;

int  gbp_lin_joint_matvec(gbp_lin_t *h, const double *x, double *y);            /* host N x d in / out: y = Lambda_joint x (joint_distribution_inf gbp.py:94-126) */
int  gbp_lin_joint_eta(gbp_lin_t *h, double *eta);                              /* host N x d: prior eta + scattered factor eta (gbp.py:94-126)                  */
int  gbp_lin_solve_map(gbp_lin_t *h, const gbp_lin_map_opts_t *opts, gbp_lin_map_info_t *info);   /* joint_distribution_cov's mu gbp.py:128-144; stays on the device */
int  gbp_lin_get_map(gbp_lin_t *h, double *mu);                                 /* N x d, the solution of the last solve (gbp.py:139-144); GBP_ESTATE before one   */
int  gbp_lin_map_distance(gbp_lin_t *h, double *out);                           /* |means - map|_2 on the device (gbp.py:94-144, ndim_posegraph.py:108); GBP_ESTATE without beliefs or a solve */

/* ---- exact marginal covariances: the `sigma` of FactorGraph.joint_distribution_cov (gbp.py:128-144) for chosen variables ----
 * Block (ids[i], ids[i]) of Lambda_joint^-1 -- and, on request, Lambda_joint^-1 restricted to ids x ids -- without the dense inverse:
 * column c = (ids[c / d], c % d) of the inverse solves Lambda x = e_c (a unit right-hand side), by the conjugate gradients above run on
 * GBP_LIN_MARG_COLS columns at a time, in order, each column with scalars of its own; one pass over the factors per iteration serves
 * the whole batch.  The last batch is padded with zero right-hand sides, which stay exactly zero.
 *
 * opts as for gbp_lin_solve_map (NULL = the same defaults, the same GBP_EINVAL rules); warm_start must be 0 (GBP_EINVAL).  max_iters is
 * per batch.  A batch iterates until EVERY column has |e - Lambda x| <= rel_tol; the recurrence's residuals are read every check_every
 * iterations (every iteration without factors); when all columns claim convergence or max_iters runs out the true residuals are formed
 * with one more multi-column product, and the recurrence restarts from them if a claim was wrong.
 * gbp_lin_marg_info_t: iters summed over the batches; converged = 1 only if every column of every batch passed (0 with GBP_OK when
 * max_iters ran out); rel_residual = the worst column's true residual; batches = ceil(n_ids d / GBP_LIN_MARG_COLS).  info may be NULL.
 * sigma[i] holds rows ids[i] of that variable's d columns, sigma_joint rows ids[*] of all columns, both as computed (not symmetrised)
 * and gathered on the device: the N d-long columns never cross to the host.
 * n_ids == 0: GBP_OK, nothing written, info {0, 1, 0, 0, 0.0}.  ids NULL with n_ids > 0, sigma NULL, an id out of range or listed twice:
 * GBP_EINVAL.  The call neither reads nor writes the sweep's state, and leaves the MAP solver's alone (gbp_lin_get_map returns the
 * same bits before and after); it shares the LDL^T of the diagonal blocks and has a workspace of its own (8 x that of the MAP solver),
 * allocated on first use and freed with the handle; the device staging of the outputs is kept with it and grows to the largest call
 * seen, so a repeated call allocates nothing.  No floating-point atomics: two identical calls on one handle are bit-identical. */
#define GBP_LIN_MARG_COLS 8
typedef struct { int32_t iters, converged, batches, reserved; double rel_residual; } gbp_lin_marg_info_t;

int  gbp_lin_solve_marginals(gbp_lin_t *h, const int32_t *ids, int32_t n_ids, const gbp_lin_map_opts_t *opts,
                             double *sigma,        /* n_ids x d x d: block (ids[i], ids[i]) of Lambda_joint^-1                   */
                             double *sigma_joint,  /* NULL, or (n_ids d) x (n_ids d): Lambda_joint^-1 restricted to ids x ids   */
                             gbp_lin_marg_info_t *info);

/* ---- robust losses: Factor(loss=, mahalanobis_threshold=) and Factor.robustify_loss (gbp.py:209-210, 296-332) for linear factors ----
 * A robust factor is the handle's stored NOMINAL factor (eta_f, Lambda_f, const_f; noise variance sigma_f^2) times one weight
 * w_f = sigma_f^2 / adaptive_gauss_noise_var, re-made from the current belief means x = [mu_a; mu_b]:
 *   M_f^2 = 2 (0.5 x^T Lambda_f x - eta_f^T x + const_f) = |h(x) - z|^2 / sigma_f^2                        (gbp.py:312, 322)
 *   loss none     : w_f = 1
 *   loss huber    : w_f = (2 t M - t^2) / M^2  if M > t, else 1                                             (gbp.py:313-319)
 *   loss constant : w_f = sigma_f^2 / M^2      if M > t, else 1    (the reference sets the adaptive variance to M^2, not sigma^2 M^2:
 *                                                                   kept, and the only use of noise_var)   (gbp.py:323-328)
 *   robust_flag_f = (M > t)
 * M_f^2 is evaluated in the residual form of gbp_lin_energy (no cancellation far from the origin), so it needs factor_const.  The
 * weight multiplies the nominal factor wherever it is used: messages (gbp.py:334-373), the energy term w_f e_f (gbp.py:43) and the
 * joint (gbp.py:94-126) -- the reference rescales its factor in place by old / new (gbp.py:331-332), which differs by rounding only.
 * DEPARTURE from the reference: robustify_loss evaluates h at Factor.linpoint (gbp.py:309), which a linear factor never moves after
 * compute_all_factors(), so read literally its weights stay those of the prior means.  Here M is taken at the CURRENT belief means:
 * exactly the reference's own arithmetic with every factor.linpoint set to its adjacent belief means before each
 * synchronous_iteration(robustify=True).
 *
 * With losses set, gbp_lin_iterate runs at the weights as they stand (the reference's robustify=False), gbp_lin_energy returns
 * sum_f w_f e_f, and gbp_lin_joint_matvec / joint_eta / solve_map / solve_marginals describe the joint at the current weights (the
 * reference takes it from factor.factor as it stands, gbp.py:94-98): a solve after a robustify is one step of iteratively reweighted
 * least squares.  Every call that changes the weights marks the solver's diagonal-block LDL^T and joint eta stale; the next solve
 * re-makes them in the same workspace (nothing allocated).  The last MAP iterate stays retrievable by gbp_lin_get_map until the next
 * solve.  No floating-point atomics: two identical call sequences on two handles are bit-identical. */
#define GBP_LIN_LOSS_NONE 0
#define GBP_LIN_LOSS_HUBER 1
#define GBP_LIN_LOSS_CONSTANT 2
int  gbp_lin_set_robust(gbp_lin_t *h, const int32_t *loss, const double *threshold, const double *noise_var);
        /* Factor(loss=, mahalanobis_threshold=) gbp.py:209-210, 243-244.  F each; loss NULL = clear (all weights 1, handle back to the
           plain path); threshold > 0 where loss != none; noise_var may be NULL unless some loss is CONSTANT, then > 0 there; resets every
           weight to 1.  An unknown loss, a bad threshold or noise_var, or any loss on a handle created with factor_const == NULL: GBP_EINVAL */
int  gbp_lin_robustify(gbp_lin_t *h);                       /* robustify_all_factors gbp.py:82-84: weights from the current belief means;
                                                               GBP_ESTATE before beliefs exist or without losses set */
int  gbp_lin_iterate_robust(gbp_lin_t *h, int32_t n_iters); /* n x synchronous_iteration(robustify=True) gbp.py:86-92, no host round trip;
                                                               GBP_ESTATE as gbp_lin_robustify */
int  gbp_lin_get_weights(gbp_lin_t *h, double *w, int32_t *robust_flag /* NULL ok */);   /* F each: sigma^2 / Factor.adaptive_gauss_noise_var,
                                                               Factor.robust_flag (gbp.py:314-328); all 1 / 0 without losses set */

/* ---- growing a live graph: graph.var_nodes.append / graph.factors.append / adj_factors.append (ndim_posegraph.py:67-88) followed by
 * FactorGraph.update_all_beliefs (gbp.py:56-58), without gbp_lin_destroy + gbp_lin_create and without losing the messages ----
 * New variables get ids N .. N + dN - 1, new factors F .. F + dF - 1; everything older keeps the caller's numbering.  The state of the
 * old factors is kept bit for bit (both messages; weight and flag where losses are set); new factors start with zero messages
 * (gbp.py:222), weight 1 and flag 0.  Adjacency stays ascending in factor id: an old variable's list is its old list followed by its
 * new factors, which is what adj_factors.append produces.  If the handle had beliefs the call ends with the belief stage over all
 * variables: old variables' records come out bit-identical (the same sum in the same order, plus zero messages), new variables hold
 * their prior and its mean; a handle without beliefs stays without.
 * Losses: `loss` != NULL on a handle without losses turns them on with the old factors at NONE (needs factor_const, as
 * gbp_lin_set_robust does); `loss` == NULL on a handle with losses gives the new factors NONE.
 * Solvers: the MAP and marginal workspaces are sized by N and F and are dropped; gbp_lin_get_map and gbp_lin_map_distance return
 * GBP_ESTATE until the next solve, which describes the joint of the grown graph at the current weights.
 * GBP_EINVAL -- after validation, before anything is changed, so the handle goes on bit-identically -- for a needed array that is NULL,
 * an id outside [0, N + dN) or a == b, factor_const given to a handle created without it or missing on one created with it, a bad
 * loss / threshold / noise_var, or 2 (F + dF) not fitting int32.  An allocation failure (GBP_ENOMEM) also leaves the handle as it was.
 * dN == dF == 0: GBP_OK, nothing changes.  All of the rebuild runs on the device; host work and traffic are proportional to dN and dF.
 * Replaced arrays are freed in the call.  No atomics: two identical call sequences on two handles are bit-identical. */
typedef struct {
    int32_t n_new_vars, n_new_factors;      /* dN, dF >= 0                                                          */
    const int32_t *var_a, *var_b;           /* dF: ids in [0, N + dN), a != b; old-old, old-new and new-new allowed */
    const double *factor_eta, *factor_lam;  /* dF x 2d, dF x 2d x 2d                                                */
    const double *factor_const;             /* dF; required iff the handle was created with factor_const            */
    const double *prior_eta, *prior_lam;    /* dN x d, dN x d x d                                                   */
    const int32_t *loss;                    /* dF GBP_LIN_LOSS_* or NULL (= none for the new factors)               */
    const double *threshold, *noise_var;    /* dF, rules of gbp_lin_set_robust                                      */
} gbp_lin_extend_desc_t;
int  gbp_lin_extend(gbp_lin_t *h, const gbp_lin_extend_desc_t *d);              /* ndim_posegraph.py:67-88 appends + gbp.py:56-58 */
int  gbp_lin_get_sizes(gbp_lin_t *h, int32_t *n_vars, int32_t *n_factors);      /* len(graph.var_nodes), len(graph.factors) gbp.py:13-14; either may be NULL */

/* ---- shrinking a live graph: variables and factors taken out of graph.var_nodes / graph.factors / adj_factors (gbp.py:13-14, 160), what
 * the leaving factors last told the surviving variables folded into those variables' priors, followed by FactorGraph.update_all_beliefs
 * (gbp.py:56-58) -- without gbp_lin_destroy + gbp_lin_create and without losing the surviving messages.  With gbp_lin_extend: a
 * fixed-lag smoother ----
 * Which factors leave: every factor on drop_factors, and every factor with at least one retired end; every other factor survives.  A
 * variable left without factors survives unless it is listed.
 * The fold (fold == 1): a leaving factor that is NOT on drop_factors and has exactly one surviving end s hands s its stored message to s
 * (Factor.messages gbp.py:222) as it stands -- the robust weight and the damping are already inside it -- and that message is added to
 * s's prior, eta and Lambda (VariableNode.prior gbp.py:170).  GBP's own marginalisation: exact on a tree with converged messages, no
 * fill-in among the neighbours.  Per variable the order is the prior first, then the folded messages one after the other in adjacency
 * order (ascending old factor id), in fp64.  A factor on drop_factors, or with both ends retired, folds nothing: its messages are
 * dropped (the `cull` meaning).  fold == 0: every leaving message is dropped.
 * Renumbering is monotone: new id = old id - the number of removed ids below it, for variables and for factors; adjacency stays
 * ascending in factor id.  var_map / factor_map (host, N / F of BEFORE the call, either may be NULL) receive the new id or -1.
 * What stays bit for bit: a surviving factor keeps eta_f, Lambda_f, const_f, both messages, weight, flag, loss, threshold and noise
 * variance.  A surviving variable none of whose factors leaves keeps its prior and its belief record.  A surviving variable whose
 * leaving factors are all folded and form a PREFIX of its adjacency list keeps its belief record (the same sum in the same order: the
 * fixed-lag case, where the oldest factors go).  Any other surviving variable's belief is equal up to the order of the sum (folded) or
 * changed (dropped).
 * Beliefs: if the handle had beliefs the call ends with the belief stage over all survivors; a handle without beliefs stays without.
 * Solvers: as gbp_lin_extend -- the MAP and marginal workspaces are dropped (the marginals' output staging stays); gbp_lin_get_map and
 * gbp_lin_map_distance return GBP_ESTATE until the next solve, which describes the joint of the shrunk graph, with the folded priors, at
 * the current weights.  Losses stay set if they were; a handle whose losses were cleared stays on the plain path.
 * GBP_EINVAL -- after validation, before anything is changed, so the handle goes on bit-identically -- for a NULL list with a positive
 * count, a negative count, an id out of range, an id listed twice, fold not 0 or 1, or N + 3 F + 1 not fitting int32.  An allocation
 * failure (GBP_ENOMEM) also leaves the handle as it was.  Both counts 0: GBP_OK, nothing changes, the maps are the identity.  Retiring
 * every variable is legal (N' = F' = 0; gbp_lin_extend grows such a handle again).
 * All of the rebuild runs on the device; host work and traffic are proportional to the two lists, plus the maps where they are asked
 * for.  Replaced arrays are freed in the call.  No floating-point atomics and no write that two threads race for: two identical call
 * sequences on two handles are bit-identical. */
typedef struct {
    int32_t n_retire_vars;  const int32_t *retire_vars;   /* ids in [0, N), none listed twice                                     */
    int32_t n_drop_factors; const int32_t *drop_factors;  /* ids in [0, F), none listed twice                                     */
    int32_t fold;                                         /* 1: fold (above); 0: every leaving message is dropped                 */
    int32_t *var_map, *factor_map;                        /* out, host, N / F of BEFORE the call: new id or -1; either may be NULL */
} gbp_lin_shrink_desc_t;
int  gbp_lin_shrink(gbp_lin_t *h, const gbp_lin_shrink_desc_t *d);

/* ---- iterating to convergence on the device: the loop of ndim_posegraph.py:104-108,
 *        for i in range(n): graph.synchronous_iteration(); print(graph.energy(), norm(graph.get_means() - mu))
 * (synchronous_iteration gbp.py:86-92, energy gbp.py:36-44, get_means gbp.py:146-153) in ONE call, without a host round trip per sweep ----
 * Up to max_iters sweeps of gbp_lin_iterate (robustify 0) or gbp_lin_iterate_robust (robustify 1) are queued; after each one the device
 * forms a trace row and decides whether to stop.  Row i (0-based, written for i < iters only) describes the state after sweep i + 1:
 *   column 0  step      max over variables v and coordinates k of |mu_new[v][k] - mu_old[v][k]|, mu_old the belief mean the sweep
 *                       overwrote.  Always computed, inside the belief stage (no second pass over the beliefs).  A maximum does not depend
 *                       on the order it is taken in: bit-equal to the same expression over two gbp_lin_get_means downloads.
 *   column 1  energy    what gbp_lin_energy would return after this sweep: the same per-factor terms (times w_f where losses are set),
 *                       added in a fixed order on the device.  NaN unless GBP_LIN_TRACE_ENERGY is in `want`.
 *   column 2  distance  what gbp_lin_map_distance would return after this sweep: |means - x|_2 against the iterate of the last
 *                       gbp_lin_solve_map -- after robust sweeps still the distance from that solve, whatever the weights have become.
 *                       NaN unless GBP_LIN_TRACE_MAP is in `want`.
 * The stop rule: after the first sweep whose step <= tol_step (tol_step > 0), reason STEP; else after the first sweep whose distance <=
 * tol_map (tol_map > 0), reason MAP; STEP is tested first when one sweep meets both.  The device sets a stop word in its memory, and every
 * kernel of a later sweep already queued reads it at its head and returns.  The host reads the word only every check_every sweeps and
 * after the last one, so
 *   - info->iters is the deciding sweep, not a multiple of check_every;
 *   - the handle's state after the call is bit for bit the state after gbp_lin_iterate(h, iters) (or gbp_lin_iterate_robust): both
 *     messages, beliefs, means, weights and flags, for every check_every;
 *   - max_iters running out is converged = 0, reason NONE, GBP_OK.
 * No floating-point atomics: two identical calls on two identical handles give bit-identical traces.
 * GBP_ESTATE: no beliefs yet; robustify without losses set; GBP_LIN_TRACE_MAP without a solve (also after gbp_lin_extend / gbp_lin_shrink,
 * until the next solve).  GBP_EINVAL: opts NULL; max_iters < 0; check_every < 1; robustify not 0 or 1; unknown bits in want; a tolerance
 * that is negative or not finite; tol_map > 0 without GBP_LIN_TRACE_MAP.  A refused call changes nothing.  max_iters == 0: GBP_OK, iters 0,
 * converged 0, nothing written.  Without factors the energy is 0 and the step exactly 0 from the first sweep (tol_step > 0 converges at
 * sweep 1); without variables the step is 0.  With robustify the call marks the solver's LDL^T and joint eta stale, as gbp_lin_robustify does.
 * Workspace: per-block partials (sized by N and F: dropped by gbp_lin_extend / gbp_lin_shrink like the solver workspaces), the stop word,
 * and a device trace buffer of max_iters rows (24 bytes each) that grows to the largest call seen; allocated on first use, freed with the
 * handle.  max_iters has no other bound: a value whose trace buffer does not fit is GBP_ENOMEM, the graph's state and the buffers the
 * handle already held unchanged.  gbp_lin_get_alloc_count: the number of device allocations the handle owns (every array of the graph
 * and every workspace), for callers and tests that want to see that a repeated call allocates nothing. */
#define GBP_LIN_TRACE_ENERGY 1   /* column 1: what gbp_lin_energy would return after this sweep              */
#define GBP_LIN_TRACE_MAP    2   /* column 2: what gbp_lin_map_distance would return after this sweep        */
#define GBP_LIN_STOP_NONE 0      /* max_iters ran out */
#define GBP_LIN_STOP_STEP 1
#define GBP_LIN_STOP_MAP  2
typedef struct {
    int32_t max_iters, check_every;  /* >= 0, >= 1                                                          */
    int32_t robustify;               /* 0: sweeps of gbp_lin_iterate, 1: of gbp_lin_iterate_robust          */
    int32_t want;                    /* mask of GBP_LIN_TRACE_*                                             */
    double tol_step;                 /* > 0: stop after the first sweep whose step <= tol_step; 0: off      */
    double tol_map;                  /* > 0: stop after the first sweep whose MAP distance <= tol_map; 0: off; needs TRACE_MAP */
} gbp_lin_until_opts_t;
typedef struct { int32_t iters, converged, reason, reserved; } gbp_lin_until_info_t;
int  gbp_lin_iterate_until(gbp_lin_t *h, const gbp_lin_until_opts_t *opts,
                           double *trace /* host, max_iters x 3, or NULL */, gbp_lin_until_info_t *info /* or NULL */);
int  gbp_lin_get_alloc_count(gbp_lin_t *h, int32_t *count);

/* ---- nonlinear pairwise factors, relinearised on the device: FactorGraph(nonlinear_factors=True) (gbp.py:30-34) with relinearise_factors
 * (gbp.py:64-80), the per-factor damping that a relinearisation switches off and num_undamped_iters sweeps later restores (gbp.py:46-54),
 * and Factor.compute_factor at a moving linearisation point (gbp.py:267-294) -- without a host round trip per sweep ----
 * Two factor families, both relative-pose ("between") factors; a model has D dofs per variable and M rows per measurement, and every
 * array below is as wide as the handle's model says: measurement and sqrt_info F x M, linpoint F x 2D.
 *   GBP_LIN_MODEL_SE2_BETWEEN   D = M = 3   planar poses (tx, ty, theta)
 *   GBP_LIN_MODEL_SE3_BETWEEN   D = M = 6   spatial poses (t, w), w a rotation vector               (further below)
 * GBP_LIN_MODEL_SE2_BETWEEN: the planar relative-pose factor on variables x = (tx, ty, theta),
 * d = 3.  A factor joins a and b and has a measurement z in R^3 and positive square-root information s in R^3, one per component (the
 * reference knows a scalar noise std only: this is its arithmetic with std 1 and a whitened meas_fn / jac_fn).  With c = cos theta_a,
 * s_ = sin theta_a, dx = xb - xa, dy = yb - ya:
 *   h(xa, xb) = diag(s) [ c dx + s_ dy ;  -s_ dx + c dy ;  theta_b - theta_a ]                       (Factor.meas_fn gbp.py:237)
 *   J = diag(s) [ -c  -s_  (-s_ dx + c dy) |  c   s_  0 ]                                            (Factor.jac_fn gbp.py:238)
 *               [  s_ -c   (-c dx - s_ dy) | -s_  c   0 ]
 *               [  0   0        -1         |  0   0   1 ]
 *   Lambda_f = J^T J,  eta_f = J^T (J x0 + diag(s) z - h(x0))  at the linearisation point x0         (gbp.py:280-289, noise variance 1)
 * (J x0 - h(x0) is formed after its cancellation, as diag(s) [ (-s_ dx + c dy) theta_a ; (-c dx - s_ dy) theta_a ; 0 ]: eta_f is accurate
 * to rounding whatever the size of the angles and translations).
 * ANGLES ARE NOT WRAPPED anywhere -- not in h, not in the distance of the relinearisation test, not in the beliefs -- because the
 * reference does not wrap: the caller keeps theta continuous along the trajectory (a pose 1.5 turns on has theta = 3 pi + ...).
 *
 * GBP_LIN_MODEL_SE3_BETWEEN: a variable is x = (t, w) in R^6, translation then rotation vector, R = Exp(w) by Rodrigues; GBP adds and
 * subtracts variables as plain vectors, as the reference does everywhere.  A factor joins a and b and has a measurement z = (z_t, z_w)
 * in R^6 -- the pose of b in the frame of a, the relative rotation as a rotation vector -- and positive square-root information s in
 * R^6.  With u = R_a^T (t_b - t_a), E = R_a^T R_b and phi = Log(E), the principal value:
 *   h(xa, xb) = diag(s) [ u ; phi ]
 *   J = diag(s) [ -R_a^T   [u]x Jr(w_a)               R_a^T   0                   ]
 *               [  0       -Jr^-1(phi) E^T Jr(w_a)    0       Jr^-1(phi) Jr(w_b)  ]
 *   Jr(w)      = I - (1 - cos th)/th^2 [w]x + (th - sin th)/th^3 [w]x^2                              (th = |w|; series near 0)
 *   Jr^-1(phi) = I + 1/2 [phi]x + (1/th^2 - (1 + cos th)/(2 th sin th)) [phi]x^2                     (th = |phi|; series near 0;
 *                the coefficient as 1/th^2 - cot(th/2)/(2 th) past th = 2.6: the first form is 0/0 at pi)
 *   Log(E):      th = atan2(|skew part|, trace part); the axis from the skew part sin th a, and past cos th = -0.875, where that
 *                vanishes, from the symmetric part (E + E^T)/2 = cos th I + (1 - cos th) a a^T
 *   Lambda_f = J^T J,  eta_f = J^T (J x0 + diag(s) z - h(x0))                                        (gbp.py:280-289, noise variance 1)
 * THE DOMAIN, as SE(2)'s "angles are never wrapped": w IS NEVER WRAPPED, and the caller keeps it continuous along the trajectory;
 * |w| > pi is legal.  Relative rotations -- Log(R_a^T R_b) at every point a factor is evaluated at -- and z_w stay below pi in norm.
 * On all of |phi| < pi, up to pi itself, h, eta_f and Lambda_f are accurate to rounding: no digits are lost as |phi| nears pi.
 * Jr(w) loses rank at |w| = 2 pi k, k >= 1: a pose there has a direction of w that turns nothing.
 *
 * gbp_lin_set_nonlinear (Factor(meas_fn=, jac_fn=) gbp.py:207-208, 237-239; compute_all_factors gbp.py:60-62, 273-276; the per-factor
 * state gbp.py:248-249): legal on a handle whose dofs are the model's D (3 for GBP_LIN_MODEL_SE2_BETWEEN, 6 for
 * GBP_LIN_MODEL_SE3_BETWEEN), without losses set, and not already nonlinear; GBP_EINVAL for a NULL
 * descriptor or array (with F > 0), an unknown model, dofs other than the model's, a negative num_undamped_iters / min_linear_iters, beta negative or NaN
 * (+inf is legal: never relinearise), a sqrt_info that is not positive and finite, a measurement that is not finite or (SE(3)) a
 * measured rotation vector z_w whose norm is not below pi; GBP_ESTATE with
 * losses set or on a handle that is already nonlinear; all decided before anything changes.  The eta_f, Lambda_f given at create are
 * ignored and overwritten, factor_const is not used.  If the handle has no beliefs the belief stage runs first (belief = prior); then
 * every factor is computed at linpoint = its adjacent belief means, iters_since_relin = 1 and the per-factor damping = 0.  Messages are
 * left as they are.
 *
 * gbp_lin_iterate_nonlinear: n x synchronous_iteration(local_relin=True, robustify=False) (gbp.py:86-92), three kernels per sweep queued
 * on the handle's stream:
 *   relinearise (gbp.py:64-80)  per factor dist = |linpoint - [mu_a; mu_b]|_2; if dist > beta && iters_since_relin >= min_linear_iters:
 *                               eta_f, Lambda_f and the linpoint re-made at the means, iters = 0, the factor's damping = 0; else iters += 1.
 *                               Then the switch of gbp.py:50-51: a factor whose iters == num_undamped_iters takes the graph's eta_damping.
 *                               Kept as the reference has it: iters starts at 1 and is incremented BEFORE the test, so a factor that has
 *                               never relinearised never meets num_undamped_iters <= 1, and with num_undamped_iters == 0 the switch fires
 *                               only in the very sweep a factor relinearises (iters == 0 there).
 *   factor (gbp.py:52)          the messages, each factor with ITS damping;
 *   belief (gbp.py:56-58)       the existing stage.
 * relin_counts[i] (host, n_iters, or NULL): the number of factors relinearised in sweep i, counted on the device -- integer adds, which
 * do not depend on their order -- and downloaded once after the call.  The device buffer of the counts grows to the largest n_iters
 * seen, like the trace buffer of gbp_lin_iterate_until.  n_iters < 0: GBP_EINVAL.
 * gbp_lin_relinearise: relinearise_factors (gbp.py:64-80) alone -- the test, the re-made factors, iters; not the damping switch, which
 * belongs to compute_all_messages.  n_relinearised may be NULL.
 * gbp_lin_get_linearisation: Factor.linpoint (gbp.py:231, F x 2D = [xa; xb]: F x 6, SE(3) F x 12), Factor.iters_since_relin and Factor.eta_damping
 * (gbp.py:248-249); any of the three may be NULL.
 * On a handle that is not nonlinear the three return GBP_ESTATE.
 *
 * The older entry points on a nonlinear handle:
 *   gbp_lin_iterate          synchronous_iteration(local_relin=False): no relinearisation, the graph-level damping (gbp.py:54), iters untouched;
 *   gbp_lin_energy           sum_f 0.5 |h(mu) - diag(s) z|^2 at the CURRENT belief means through the nonlinear h (gbp.py:36-44, 251-265),
 *                            per-block partials added in a fixed order as before;
 *   gbp_lin_joint_matvec / joint_eta / solve_map / solve_marginals   the joint "at the current linearisation point" (gbp.py:96-97):
 *                            eta_f, Lambda_f live where the solvers read them.  Every call that may relinearise marks the solver's
 *                            LDL^T and joint eta stale, as a change of robust weights does; a solve after it is one Gauss-Newton step;
 *   gbp_lin_set_robust, gbp_lin_robustify, gbp_lin_iterate_robust, gbp_lin_iterate_until, gbp_lin_extend, gbp_lin_shrink
 *                            GBP_ESTATE with a message; nothing changes.  (gbp_lin_extend takes eta_f, Lambda_f, which a nonlinear
 *                            handle owns: such a handle grows and shrinks through the two calls below; the first three take M at the
 *                            belief means: such a handle has its losses from gbp_lin_set_robust_nonlinear, further below.)
 * No floating-point atomics: two identical call sequences on two handles are bit-identical, counts included. */
#define GBP_LIN_MODEL_SE2_BETWEEN 1
#define GBP_LIN_MODEL_SE3_BETWEEN 2
typedef struct {
    int32_t model;                      /* GBP_LIN_MODEL_*                                                     */
    int32_t num_undamped_iters;         /* FactorGraph.num_undamped_iters gbp.py:33, >= 0                      */
    int32_t min_linear_iters;           /* FactorGraph.min_linear_iters gbp.py:34, >= 0                        */
    int32_t reserved;
    double beta;                        /* FactorGraph.beta gbp.py:32, >= 0; +inf = never relinearise          */
    const double *measurement;          /* F x M   Factor.measurement gbp.py:233 (not whitened); M = 3 or 6    */
    const double *sqrt_info;            /* F x M, positive and finite                                          */
} gbp_lin_nonlinear_desc_t;
int  gbp_lin_set_nonlinear(gbp_lin_t *h, const gbp_lin_nonlinear_desc_t *d);    /* compute_all_factors gbp.py:60-62 */
int  gbp_lin_relinearise(gbp_lin_t *h, int32_t *n_relinearised /* or NULL */);  /* relinearise_factors gbp.py:64-80 */
int  gbp_lin_iterate_nonlinear(gbp_lin_t *h, int32_t n_iters, int32_t *relin_counts /* host, n_iters, or NULL */);   /* n x synchronous_iteration(local_relin=True) gbp.py:86-92 */
int  gbp_lin_get_linearisation(gbp_lin_t *h, double *linpoint /* F x 2D */, int32_t *iters_since_relin /* F */, double *eta_damping /* F */);   /* Factor.linpoint gbp.py:231, iters_since_relin / eta_damping gbp.py:248-249; any may be NULL */

/* ---- growing and shrinking a live NONLINEAR handle: a fixed-lag smoother for SE(2) and SE(3) pose graphs ----
 * Both calls return GBP_ESTATE on a handle without nonlinear factors, validate completely before anything changes, leave the handle
 * bit-identical on any failure before the commit (GBP_EINVAL, GBP_ENOMEM), drop the solver workspaces and mark the joint stale as
 * gbp_lin_extend / gbp_lin_shrink do, and leave the handle holding ONE generation of arrays: gbp_lin_get_alloc_count does not grow
 * with repeated calls.  beta, num_undamped_iters, min_linear_iters and the graph's eta_damping stay the handle's.  No atomics.
 * After the commit only a failed kernel launch (GBP_EHIP) can still be returned, by the belief stage or by the linearise pass of
 * gbp_lin_extend_nonlinear: the handle then holds the new graph, but its beliefs -- and the new factors' eta_f, Lambda_f (zero) and
 * linpoint -- are not those of a completed call, and it should be destroyed.
 *
 * gbp_lin_extend_nonlinear: var_nodes.append / factors.append / adj_factors.append, update_all_beliefs() (gbp.py:56-58), then
 * compute_factor() on the NEW factors only (gbp.py:267-294).  Ids, adjacency order and the index and size rules are those of
 * gbp_lin_extend; measurements must be finite and sqrt_info positive and finite (SE(3): |z_w| < pi), as for gbp_lin_set_nonlinear.  A new factor is
 * linearised at its two adjacent belief means as they are AFTER the belief update -- a new variable's belief is its prior, so the
 * caller puts the odometry prediction there -- and starts with zero messages, iters_since_relin = 1 and damping 0 (gbp.py:222,
 * 248-249).  Every old factor keeps eta_f, Lambda_f, linpoint, iters_since_relin, damping and both messages bit for bit, and every old
 * variable its belief record: nothing relinearises in the call.  The linearisation runs over the new factors alone (work and traffic
 * go by dF), with the lane code of gbp_lin_set_nonlinear: a handle created with the first K factors and extended by the rest before any
 * sweep is bit-identical to the handle created whole.  dN == dF == 0: GBP_OK, nothing changes.
 *
 * gbp_lin_shrink_nonlinear: the descriptor and the semantics of gbp_lin_shrink -- retired variables leave with their factors, listed
 * factors are dropped, with `fold` a leaving unlisted factor with one surviving end adds its stored message to that end's prior,
 * survivors are renumbered monotonically, var_map / factor_map are returned.  A surviving factor keeps eta_f, Lambda_f, measurement,
 * sqrt_info, linpoint, iters_since_relin, damping and both messages bit for bit; nothing relinearises in the call.  THE FOLD IS FROZEN:
 * the folded message is the one the leaving factor computed at its LAST linearisation point, and once it is part of a prior it never
 * relinearises again (the reference's priors are linear too). */
typedef struct {
    int32_t n_new_vars, n_new_factors;      /* dN, dF >= 0                                                          */
    const int32_t *var_a, *var_b;           /* dF: ids in [0, N + dN), a != b; old-old, old-new and new-new allowed */
    const double *measurement;              /* dF x M, finite (not whitened); the handle's model: M = 3 or 6        */
    const double *sqrt_info;                /* dF x M, positive and finite                                          */
    const double *prior_eta, *prior_lam;    /* dN x D, dN x D x D                                                   */
} gbp_lin_extend_nonlinear_desc_t;
int  gbp_lin_extend_nonlinear(gbp_lin_t *h, const gbp_lin_extend_nonlinear_desc_t *d);   /* appends + gbp.py:56-58 + compute_factor gbp.py:267-294 on the new factors */
int  gbp_lin_shrink_nonlinear(gbp_lin_t *h, const gbp_lin_shrink_desc_t *d);

/* ---- robust losses on a NONLINEAR handle: Factor(loss=, mahalanobis_threshold=) on FactorGraph(nonlinear_factors=True) and
 * synchronous_iteration(local_relin=True, robustify=True) (gbp.py:86-92) -- odometry clean, loop closures with a loss ----
 * For a nonlinear factor robustify_loss evaluates meas_fn at Factor.linpoint, NOT at the belief means (gbp.py:309), and the linpoint
 * moves with every relinearisation: the reference is read literally here (the linear path above departs from it because a linear
 * factor's linpoint never moves).  With the whitened model of gbp_lin_set_nonlinear the noise variance is 1:
 *   M_f = | diag(s_f) z_f - h(linpoint_f) |_2                                                            (gbp.py:312, 322)
 *   loss huber    : w_f = (2 t M - t^2) / M^2  if M > t, else 1                                          (gbp.py:313-319)
 *   loss constant : w_f = 1 / M^2              if M > t, else 1                                          (gbp.py:324, variance 1)
 *   robust_flag_f = (M > t)
 * The weight multiplies the factor AS LINEARISED (eta_f, Lambda_f at linpoint_f) wherever it is used -- messages, the energy
 * sum_f w_f 0.5 |h(mu) - diag(s) z|^2 at the current means (gbp.py:43, 265), and the joint -- where the reference rescales in place by
 * old / new (gbp.py:331-332) and compute_factor divides by the adaptive variance (gbp.py:287): rounding apart, the same.  A
 * relinearisation re-makes the nominal factor; the weight stays.
 *
 * gbp_lin_set_robust_nonlinear: loss and threshold of the factors [first, first + count) (count each); their weights become 1 and their
 * flags 0, and every other factor keeps loss, threshold, weight and flag bit for bit -- a live smoother gives a loss to the closures it
 * has just appended without disturbing the rest.  On a handle without losses set every factor outside the range is at NONE, 1, 0.  The
 * first call on a handle allocates the robust arrays and the buffer of the flag counts; later calls allocate nothing.  loss == NULL with
 * first == 0 && count == F clears: all weights 1, the handle back on the plain nonlinear path; loss == NULL otherwise is GBP_EINVAL.
 * The rules of gbp_lin_set_robust for a loss and a threshold apply (there is no noise_var: it is 1); a range outside [0, F] or a
 * negative count: GBP_EINVAL.  A handle that is not nonlinear: GBP_ESTATE.  All decided before anything changes; count == 0: GBP_OK,
 * nothing changes.
 * gbp_lin_robustify_nonlinear: robustify_all_factors (gbp.py:82-84) alone, at the linpoints.  GBP_ESTATE without nonlinear factors or
 * without losses set.
 * gbp_lin_iterate_nonlinear_robust: n sweeps in the order of gbp.py:86-92 -- (1) robustify every factor at its linpoint as it stands
 * BEFORE this sweep's relinearisation, (2) relinearise (gbp.py:64-80), (3) messages, each factor with its own damping and its weight,
 * (4) beliefs -- as three kernels per sweep: (1) and (2) are one lane per factor on the same linpoint, z and s, and run fused.
 * relin_counts as in gbp_lin_iterate_nonlinear; robust_counts[i] (host, n_iters, or NULL): the number of factors flagged in sweep i,
 * counted the same way, its device buffer growing to the largest n_iters seen.  GBP_ESTATE as gbp_lin_robustify_nonlinear; n_iters < 0:
 * GBP_EINVAL.  Marks the solver's LDL^T and joint eta stale.
 *
 * The older calls on a nonlinear handle with losses set:
 *   gbp_lin_iterate_nonlinear, gbp_lin_iterate, gbp_lin_relinearise   at the weights as they stand (the reference's robustify=False);
 *   gbp_lin_energy           the weighted sum above;   gbp_lin_get_weights   w and the flags;
 *   gbp_lin_joint_matvec / joint_eta / solve_map / solve_marginals   the weighted joint: a solve after a robust sweep is one
 *                            reweighted Gauss-Newton step;
 *   gbp_lin_extend_nonlinear / gbp_lin_shrink_nonlinear   every old or surviving factor keeps loss, threshold, weight and flag bit for
 *                            bit; appended factors start at NONE, weight 1, flag 0; gbp_lin_get_alloc_count still does not grow with
 *                            repeated calls;
 *   gbp_lin_set_robust, gbp_lin_robustify, gbp_lin_iterate_robust, gbp_lin_iterate_until, gbp_lin_extend, gbp_lin_shrink   stay
 *                            refused with GBP_ESTATE; gbp_lin_set_nonlinear on a handle with linear losses set stays GBP_ESTATE.
 *                            (Sweeps to convergence on such a handle: gbp_lin_iterate_until_nonlinear, at the end of this header.)
 * No floating-point atomics: two identical call sequences on two handles are bit-identical, both counts included. */
int  gbp_lin_set_robust_nonlinear(gbp_lin_t *h, int32_t first, int32_t count, const int32_t *loss, const double *threshold);   /* Factor(loss=, mahalanobis_threshold=) gbp.py:209-210 */
int  gbp_lin_robustify_nonlinear(gbp_lin_t *h);                                 /* robustify_all_factors gbp.py:82-84, at the linpoints */
int  gbp_lin_iterate_nonlinear_robust(gbp_lin_t *h, int32_t n_iters, int32_t *relin_counts /* n_iters or NULL */,
                                      int32_t *robust_counts /* n_iters or NULL */);   /* n x synchronous_iteration(local_relin=True, robustify=True) gbp.py:86-92 */

/* ---- iterating a NONLINEAR handle to convergence on the device: the loop
 *        for i in range(n): graph.synchronous_iteration(local_relin=True[, robustify=True]); print(graph.energy(), norm(graph.get_means() - mu))
 * in ONE call, without a synchronisation and two downloads per sweep ----
 * gbp_lin_iterate_until_nonlinear takes the options and the info of gbp_lin_iterate_until (which stays refused on a nonlinear handle).
 * Up to max_iters sweeps are queued; robustify 0: each is exactly one sweep of gbp_lin_iterate_nonlinear (relinearise; factor with
 * per-factor damping, at the standing weights if losses are set; belief), robustify 1: exactly one of gbp_lin_iterate_nonlinear_robust
 * (the fused robustify + relinearise lane; factor; belief) -- the same three kernels, plus the energy pass when asked for, plus the
 * one-block finishing kernel.  Row i of the trace (written for i < iters only) describes the state after sweep i + 1:
 *   column 0  step      max |mu_new - mu_old|, taken inside the belief stage as in gbp_lin_iterate_until: bit-equal to the same expression
 *                       over two gbp_lin_get_means downloads.
 *   column 1  energy    what gbp_lin_energy returns on this handle after the sweep: sum_f w_f 0.5 |h(mu) - diag(s) z|^2 through the
 *                       nonlinear h (w_f = 1 without losses), added in a fixed order on the device.  NaN unless GBP_LIN_TRACE_ENERGY.
 *   column 2  distance  |means - x|_2 against the iterate of the last gbp_lin_solve_map.  That solve is ONE Gauss-Newton step at the
 *                       linearisation point and the weights it found; the distance is from that solve, wherever the linearisation has
 *                       moved since.  NaN unless GBP_LIN_TRACE_MAP.
 * relin_counts[i] / robust_counts[i] (host, max_iters each, or NULL): what gbp_lin_iterate_nonlinear / gbp_lin_iterate_nonlinear_robust
 * return for sweep i, counted the same way (one ballot, one popcount and one integer atomic add per wave) in the handle's own count
 * buffers, which grow to max_iters; downloaded once after the call, and only the first `iters` entries are written.
 * The stop rule is gbp_lin_iterate_until's: STEP is tested before MAP, the device decides and sets the stop word.  With
 * GBP_LIN_UNTIL_SETTLED in `want` a sweep in which ANY factor relinearised decides neither: a step can be small in the very sweep that
 * moves linearisation points, and only the device knows.  (The finishing kernel reads that sweep's count slot; the stream orders it behind
 * the relinearise kernel's adds.)  A graph that relinearises in every sweep therefore never stops under this bit: converged = 0, reason
 * NONE, GBP_OK.  The bit belongs to this call alone: gbp_lin_iterate_until answers it with GBP_EINVAL like any unknown bit.
 * Every kernel of a sweep queued behind the deciding one returns at its head, the relinearise lane included: it writes no iters,
 * linpoint, factor, damping, weight or flag and adds to no count.  So after the call both messages, beliefs and means, eta_f, Lambda_f,
 * linpoint, iters_since_relin and the per-factor damping, weights and flags are bit for bit those of gbp_lin_iterate_nonlinear(h, iters)
 * (or gbp_lin_iterate_nonlinear_robust) on an identical handle, for every check_every.
 * The call marks the solver's LDL^T and joint eta stale (the linearisation point and the weights may have moved).  It reuses the
 * workspace of gbp_lin_iterate_until: the partials are dropped by gbp_lin_extend_nonlinear / gbp_lin_shrink_nonlinear and re-made by the
 * next call; a repeated call of the same size allocates nothing (gbp_lin_get_alloc_count).  No floating-point atomics: two identical call
 * sequences on two handles give bit-identical traces and counts.
 * GBP_ESTATE: a handle without nonlinear factors; robustify without losses set; GBP_LIN_TRACE_MAP without a solve (also after
 * gbp_lin_extend_nonlinear / gbp_lin_shrink_nonlinear, until the next solve).  GBP_EINVAL: opts NULL; max_iters < 0; check_every < 1;
 * robustify not 0 or 1; bits in want outside ENERGY | MAP | SETTLED; a tolerance that is negative or not finite; tol_map > 0 without
 * GBP_LIN_TRACE_MAP; robust_counts != NULL with robustify == 0.  All decided before anything changes.  max_iters == 0: GBP_OK, nothing
 * written.  Without factors the step is exactly 0 from the first sweep and both counts are 0. */
#define GBP_LIN_UNTIL_SETTLED 4   /* in `want`, this call only: a sweep in which any factor relinearised decides nothing */
int  gbp_lin_iterate_until_nonlinear(gbp_lin_t *h, const gbp_lin_until_opts_t *opts,
                                     double *trace          /* host, max_iters x 3, or NULL */,
                                     int32_t *relin_counts  /* host, max_iters, or NULL */,
                                     int32_t *robust_counts /* host, max_iters, or NULL; must be NULL when opts->robustify == 0 */,
                                     gbp_lin_until_info_t *info /* or NULL */);

/* ---- the NONLINEAR batch MAP on the device, by Levenberg-Marquardt: what ndim_posegraph.py:94,108 measures linear GBP against
 * (joint_distribution_cov's mu, gbp.py:128-144), for FactorGraph(nonlinear_factors=True) -- the minimiser of the nonlinear least-squares
 * problem itself, not one Gauss-Newton step at wherever the sweeps' linearisation stands ----
 * On a nonlinear handle (SE(2) or SE(3)) the call minimises
 *   Phi(x) = sum_f w_f 0.5 |h_f(x) - diag(s_f) z_f|^2 + sum_v (0.5 x_v^T Lambda0_v x_v - eta0_v^T x_v)
 * over x in R^(N D): the first sum is what gbp_lin_energy reports (factors only, w_f = 1 without losses), the second the priors, the
 * folded priors of gbp_lin_shrink_nonlinear included.  THE WEIGHTS ARE FIXED during the call, at what they are when it is made:
 * iteratively reweighted solves are gbp_lin_solve_map_nonlinear_robust below, which makes weights of its own at its own x.
 * It neither reads nor writes the sweep's state, except for the belief means when they are the starting point: messages, beliefs,
 * means, the handle's eta_f / Lambda_f, linpoint, iters_since_relin, per-factor damping, weights, flags and both count buffers are bit
 * for bit what they were, whatever the call returns.
 *
 * One outer iteration at (x, lambda):
 *   1. every factor is linearised at x, into arrays of the solver's own, by the lane code of the relinearise stage; the same pass
 *      leaves the factor energy E(x);
 *   2. a damped copy of the priors: Lambda0_v + lambda diag(D_v), eta0_v + lambda diag(D_v) x_v, D_v the joint's diagonal block at x
 *      (at the weights as they stand), each diagonal entry floored at 1e-12 (GN_DIAG_FLOOR);
 *   3. the conjugate gradients of gbp_lin_solve_map (options `cg`) on that joint, started at x: the first true residual is
 *      eta - Lambda x = -grad Phi(x); grad_norm is its 2-norm, and tol_grad is tested there, before any CG iteration, at every x that
 *      is new (x0 and after every accepted step).  It is formed from the DAMPED system, (eta + lambda D x) - (Lambda + lambda D) x:
 *      the lambda D x terms cancel exactly only in exact arithmetic and leave a rounding of about 1e-16 lambda max(D |x|) in
 *      grad_norm -- with an anchor prior of 1e6 and, after a run of rejections, lambda >= 1, that is 1e-10 |x| or more, comparable with
 *      a tol_grad of 1e-8; at the lambda of accepted steps (<= 1e-3 by default) it is below the rounding of eta - Lambda x itself;
 *   4. the candidate x_c is judged by dPhi = [E(x_c) - E(x)] + sum_v (x_c - x)_v^T (Lambda0_v (x_c + x)_v / 2 - eta0_v), the prior
 *      part in difference form (no cancellation far from the origin), every sum in a fixed order;
 *   5. the host decides: max |x_c - x| <= tol_step (tol_step > 0): stop, reason STEP, converged, x_c taken only if dPhi <= 0;
 *      else dPhi < 0: accepted, x = x_c, lambda = max(lambda lambda_down, lambda_min); anything else -- a NaN included, which is what
 *      an SE(3) candidate whose relative rotation leaves the domain gives -- rejected: x stays, and if the lambda just used is above
 *      lambda_max the call ends with reason STALL, converged 0, GBP_OK, else lambda = lambda lambda_up.  A rejected step relinearises
 *      nothing.  max_outer running out: reason NONE, converged 0, GBP_OK.
 * trace row i (written for i < info->outer): E(x) before the step, the lambda used, max |x_c - x|, dPhi, taken (1 / 0).
 * info: outer = accepted + rejected = rows written; cg_iters summed over the inner solves; energy0 / energy = E at x0 and at the final
 * x (comparable with gbp_lin_energy when the means equal x); grad_norm at the last new x it was formed at; lambda: what the next
 * iteration would use.
 * NULL opts = { max_outer 50, init FROM_MEANS, lambda0 1e-4, lambda_up 10, lambda_down 0.1, lambda_min 1e-12, lambda_max 1e8,
 *               tol_step 1e-10, tol_grad 1e-8, cg {1e-12, 10000, 8, 0} }.
 * WHAT tol_grad CAN REACH: the decrease test compares values of Phi, and E(x) is known to about 1e-16 E.  A step from a point with
 * gradient g lowers Phi by about g^2 / (2 curvature); once that is below the rounding of E -- g below about sqrt(2e-16 E curvature),
 * e.g. 5e-6 at E = 130 and curvatures of 400 -- steps are rejected on noise and the call ends in STEP (tol_step on) or STALL.  The
 * default tol_grad of 1e-8 is therefore reached only by problems whose energy at the optimum is of order 1e-3 or less; on the others
 * the defaults end in STEP, which is the expected way for them to end.  Ask for a tol_grad above that floor to end in GRAD.
 * The final x lands where gbp_lin_solve_map leaves its iterate: gbp_lin_get_map, gbp_lin_map_distance and GBP_LIN_TRACE_MAP of
 * gbp_lin_iterate_until_nonlinear then measure against the nonlinear MAP.  The inner solves use that solver's workspace and leave its
 * LDL^T and joint eta stale: the next gbp_lin_solve_map re-makes them in place, as after a change of weights.  The solver's own arrays
 * (linearisation, damped priors, x, partials) are allocated on first use, dropped by gbp_lin_extend_nonlinear /
 * gbp_lin_shrink_nonlinear with the other solver workspaces and re-made by the next call; a repeated call of the same size allocates
 * nothing (gbp_lin_get_alloc_count).  No floating-point atomics: two identical call sequences on two handles give bit-identical x, info
 * and trace.
 * Refusals, all before anything changes: a handle that is not nonlinear, init FROM_MEANS without beliefs, init FROM_MAP without a
 * solve: GBP_ESTATE.  max_outer < 0, an unknown init, a lambda that is not positive and finite, lambda_up <= 1, lambda_down >= 1,
 * lambda_min <= lambda0 <= lambda_max violated, a tolerance negative or not finite, the cg rules of gbp_lin_solve_map, cg.warm_start
 * != 0: GBP_EINVAL.
 * max_outer == 0: x = x0, energy0 = energy = E(x0).  Without factors Phi is the priors' quadratic: ONE step with lambda = 0 (so the
 * trace row says) reaches its minimiser and the call ends converged, reason GRAD.  Without variables: GBP_OK, converged, reason GRAD. */
#define GBP_LIN_NLMAP_FROM_MEANS 0   /* x0 = the belief means                               */
#define GBP_LIN_NLMAP_FROM_MAP   1   /* x0 = the iterate gbp_lin_get_map would return       */
#define GBP_LIN_NLMAP_NONE  0        /* max_outer ran out                                    */
#define GBP_LIN_NLMAP_STEP  1
#define GBP_LIN_NLMAP_GRAD  2
#define GBP_LIN_NLMAP_STALL 3
typedef struct {
    int32_t max_outer;        /* >= 0 LM iterations (accepted + rejected)                         */
    int32_t init;             /* GBP_LIN_NLMAP_FROM_MEANS 0: x0 = belief means (GBP_ESTATE without beliefs);
                                 GBP_LIN_NLMAP_FROM_MAP   1: x0 = the iterate gbp_lin_get_map would return (GBP_ESTATE without one) */
    double lambda0, lambda_up, lambda_down, lambda_min, lambda_max;   /* > 0, up > 1, 0 < down < 1, min <= lambda0 <= max */
    double tol_step;          /* > 0: stop after a step with max |dx| <= tol_step; 0: off        */
    double tol_grad;          /* > 0: stop when |eta - Lambda x|_2 at x <= tol_grad; 0: off      */
    gbp_lin_map_opts_t cg;    /* the inner solves; warm_start must be 0 (CG always starts at x)   */
} gbp_lin_nlmap_opts_t;
typedef struct { int32_t outer, accepted, rejected, cg_iters, converged, reason;   /* NONE / STEP / GRAD / STALL */
                 double energy0, energy, grad_norm, lambda; } gbp_lin_nlmap_info_t;
int gbp_lin_solve_map_nonlinear(gbp_lin_t *h, const gbp_lin_nlmap_opts_t *opts,
                                double *trace /* host, max_outer x 5, or NULL */, gbp_lin_nlmap_info_t *info /* or NULL */);

/* ---- The ROBUST nonlinear batch MAP by reweighted Levenberg-Marquardt ----
 * With losses set, gbp_lin_solve_map_nonlinear minimises at the weights as they stand -- weights the sweeps made at whatever
 * linearisation points they had reached, so its answer depends on the state of the thing it is a yardstick for.  What robust nonlinear
 * GBP converges to is independent of any sweep: at a fixed point of synchronous_iteration(local_relin=True, robustify=True)
 * (gbp.py:86-92) the linpoints equal the means, the weights are Factor.robustify_loss at those linpoints (gbp.py:296-332), and the
 * means solve the joint at that linearisation and those weights (gbp.py:94-144):
 *     x* = argmin_x  sum_f w_f(x*) 0.5 |h_f(x) - diag(s_f) z_f|^2 + priors(x),     w_f(x*) = the reference's weight from M_f(x*).
 * This call finds x* as the fixed point of "make the weights at x, minimise at those weights, repeat" -- iteratively reweighted least
 * squares with the reference's own, ENERGY-MATCHED weights (Huber: w 0.5 M^2 = t M - 0.5 t^2; not the textbook rho'/M) -- and reports
 * the weights and the flags (M_f > t_f: the closures the optimum calls outliers) at x*.
 *
 * x is the solver's own point, as in gbp_lin_solve_map_nonlinear; the weights and flags are arrays of the solver's own too, NEVER the
 * handle's (gbp_lin_get_weights).
 *   Reweight r = 0, 1, ...: every factor with a loss gets the weight and flag of gbp.py:311-328 from M_f = |diag(s_f) z_f - h_f(x)| at
 *     the solver's x, noise variance 1 as on every nonlinear handle, with the handle's own loss / threshold
 *     (gbp_lin_set_robust_nonlinear); a factor at GBP_LIN_LOSS_NONE, and every factor of a handle without losses, gets 1 / 0.  The same
 *     lane leaves the linearisation at x, the weighted energy sum_f w_f 0.5 M_f^2, weight_change = max_f |w_new - w_old| (defined as 0
 *     at r = 0) and the number of flagged factors.
 *   Stop test at r >= 1, in this order: tol_weight > 0 and weight_change <= tol_weight: reason WEIGHTS; tol_move > 0 and
 *     move_{r-1} <= tol_move: reason MOVE.  With max_rounds spent: reason NONE, converged 0, GBP_OK.  The final weights are therefore
 *     always the ones made at the final x: a run of R rounds makes R + 1 reweights and writes R + 1 rows.
 *   Round r: exactly the Levenberg-Marquardt loop of gbp_lin_solve_map_nonlinear (options `lm`) at those weights, from x, started at
 *     lm.lambda0; its first linearisation is the one the reweight made.  move_r = max |x_end - x_start| over the round.  A round that
 *     ends in STALL or NONE is not an error: the loop goes on to the next reweight.
 * round_trace row r: the weighted energy at the reweight, the flagged count, weight_change, move_{r-1} (0 at r = 0), the LM outer
 * iterations of round r and its GBP_LIN_NLMAP_* reason (both 0 on the last row).  lm_trace: the rows gbp_lin_solve_map_nonlinear would
 * have written, round after round WITHOUT gaps (round r's rows follow round r - 1's; column 4 of round_trace says how many each has;
 * info->outer rows in all).  weights / robust_flag: w_f and M_f > t_f at the final x.
 * info: rounds run, outer / accepted / rejected / cg_iters summed over the rounds, flagged / energy / weight_change / move of the last
 * reweight, energy0 of the first, grad_norm of the last round.
 * NULL opts = { max_rounds 20, 0, tol_weight 1e-9, tol_move 1e-10, lm = the defaults of gbp_lin_solve_map_nonlinear }.
 * The final x lands where gbp_lin_solve_map leaves its iterate, map_solved set and the LDL^T stale, exactly as after
 * gbp_lin_solve_map_nonlinear.  Like that call it WRITES NOTHING OF THE SWEEP, whatever it returns: messages, beliefs, means, the
 * handle's eta_f / Lambda_f, linpoint, iters, damping, THE HANDLE'S WEIGHTS AND FLAGS and the count buffers stay bit for bit; only the
 * means are read, when lm.init is FROM_MEANS.  Its arrays (weights, flags, a copy of x, partials) join that call's workspace: allocated
 * all or nothing on first use, dropped with a generation, and a repeated call of the same size allocates nothing.  No floating-point
 * atomics: two identical call sequences on two handles give bit-identical x, traces, weights and flags (the flagged count is integer
 * adds).
 * Refusals, all before anything changes: a handle that is not nonlinear, and the GBP_ESTATE rules of lm.init: GBP_ESTATE.
 * max_rounds < 0, a tolerance negative or not finite, every GBP_EINVAL rule of gbp_lin_nlmap_opts_t: GBP_EINVAL.
 * A handle WITHOUT LOSSES is legal: every weight is 1, round 1's reweight finds weight_change == 0, and with tol_weight > 0 the call
 * ends after one round, reason WEIGHTS, its x bit-identical to gbp_lin_solve_map_nonlinear with opts->lm.
 * Without variables: GBP_OK, converged, WEIGHTS, 0 rounds (one row of zeros).  Without factors: one round of one exact step, then
 * WEIGHTS.  max_rounds == 0: one reweight at x0, x = x0, and weights / robust_flag describe x0.
 * Out of scope: writing the solver's weights back into the handle; rho'/M weights or a Triggs correction; covariances at the robust
 * MAP (gbp_lin_solve_marginals still describes the joint at the sweeps' linearisation and weights). */
#define GBP_LIN_IRLS_NONE    0   /* max_rounds ran out                                              */
#define GBP_LIN_IRLS_WEIGHTS 1   /* the weights made at x differ from the round's by <= tol_weight  */
#define GBP_LIN_IRLS_MOVE    2   /* the last round moved x by <= tol_move                           */
typedef struct {
    int32_t max_rounds;          /* >= 0                                                            */
    int32_t reserved;
    double tol_weight;           /* > 0: on; 0: off                                                 */
    double tol_move;             /* > 0: on; 0: off                                                 */
    gbp_lin_nlmap_opts_t lm;     /* every round: the options of gbp_lin_solve_map_nonlinear; lm.init
                                    names x0 of round 0 only, later rounds start where the last ended;
                                    every round starts at lm.lambda0                                */
} gbp_lin_irls_opts_t;
typedef struct { int32_t rounds, outer, accepted, rejected, cg_iters, converged, reason, flagged;
                 double energy0, energy, weight_change, move, grad_norm; } gbp_lin_irls_info_t;
int gbp_lin_solve_map_nonlinear_robust(gbp_lin_t *h, const gbp_lin_irls_opts_t *opts,
        double *round_trace /* host, (max_rounds + 1) x 6, or NULL */,
        double *lm_trace    /* host, max_rounds * lm.max_outer x 5, or NULL: the rounds' LM rows, one after the other */,
        double *weights     /* host, F, or NULL: w_f at the final x */,
        int32_t *robust_flag/* host, F, or NULL: M_f(x) > t_f at the final x */,
        gbp_lin_irls_info_t *info /* or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* GBP_LIN_H */
