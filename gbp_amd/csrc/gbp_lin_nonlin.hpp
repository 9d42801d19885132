// gbp_lin_nonlin.hpp -- nonlinear pairwise factors of the linear engine on gfx950, relinearised on the device: FactorGraph(
// nonlinear_factors=True) with relinearise_factors (gbp.py:64-80), the per-factor damping of compute_all_messages (gbp.py:46-54) and
// Factor.compute_factor at a moving linearisation point (gbp.py:267-294).  include/gbp_lin.h states the semantics.
//
// The model is a template parameter of what evaluates it: NonlinModel<MODEL> names its D (dofs of a variable) and M (rows of a
// measurement), and everything below sizes its arrays from them.  There are two.
// GBP_LIN_MODEL_SE2_BETWEEN (D = M = 3): x = (tx, ty, theta), and with c = cos theta_a, s_ = sin theta_a, dx = xb - xa, dy = yb - ya
//   h = diag(s) [ c dx + s_ dy ;  -s_ dx + c dy ;  theta_b - theta_a ]
//   J = diag(s) [ -c  -s_  (-s_ dx + c dy) |  c   s_  0 ;   s_ -c  (-c dx - s_ dy) | -s_  c  0 ;   0  0  -1 | 0  0  1 ]
//   Lambda_f = J^T J,  eta_f = J^T (J x0 + diag(s) z - h(x0))                                      (gbp.py:280-289, noise variance 1)
// where J x0 - h(x0) is formed as what is left after its cancellation, diag(s) [ (-s_ dx + c dy) theta_a ; (-c dx - s_ dy) theta_a ; 0 ].
// Angles are never wrapped: the reference does not wrap, and the caller keeps theta continuous.
// GBP_LIN_MODEL_SE3_BETWEEN (D = M = 6): x = (t, w), R = Exp(w) by Rodrigues; with Q = R_a^T, u = Q (t_b - t_a), E = Q R_b, phi = Log(E)
//   h = diag(s) [ u ; phi ]
//   J = diag(s) [ -Q   [u]x Jr(w_a)               Q   0
//                  0   -Jr^-1(phi) E^T Jr(w_a)    0   Jr^-1(phi) Jr(w_b) ]
//   Jr(w) = I - (1 - cos th)/th^2 [w]x + (th - sin th)/th^3 [w]x^2,   Jr^-1(phi) = I + 1/2 [phi]x + (1/th^2 - (1 + cos th)/(2 th sin th)) [phi]x^2
// with the coefficients from their series below th = 0.2 (se3_coeffs, se3_jrinv_coeff) and Log from atan2(|skew part|, trace part).
// Beside pi both change form, since (1 + cos th)/sin th is 0/0 there and the skew part sin th * axis vanishes: past th = 2.6 the
// coefficient is 1/th^2 - cot(th/2)/(2 th), and past cos th = -0.875 Log takes the axis from the symmetric part cos th I +
// (1 - cos th) a a^T (se3_log).  The model is then good to rounding on all of |phi| < pi (fixture G31, tests/golden/make_g31.py).
// w is never wrapped either (|w| > pi is legal; Jr(w) loses rank at |w| = 2 pi k); relative rotations stay below pi.  J is block
// sparse: Lambda_f is made block by block from the five 3 x 3 blocks and every entry is stored as it is made (factor_store) -- no
// 6 x 12 J, no 78 products held at once.
//   NonlinModel<MODEL>::eval   h at a point
//   nonlin_factor<SE2> / NonlinModel<SE3>::factor_store   eta_f and packed-upper Lambda_f at a linearisation point, into arrays / at a stride
//   lin_relin_one<MODEL>   one lane, one factor: the test of gbp.py:75, the factor re-made where it passes, iters, and the damping
//                          switch of gbp.py:50-51
//   k_lin_relin<MODEL>     that over every factor; the relinearised factors of a wave are counted by a popcount and ONE integer atomic add
//   k_lin_relin_range<MODEL>  that over a range of factors (the ones gbp_lin_extend_nonlinear appended), uncounted
//   k_lin_energy_nl<MODEL> sum_f w_f 0.5 |h(mu) - diag(s) z|^2 at the belief means (w_f = 1 without losses), in the block / partials
//                          shape of k_lin_energy
// k_lin_relin and k_lin_energy_nl take the parameter block as a template argument like the stages of gbp_lin_sweep.hpp: LinParams is
// the plain form, LinGated the one gbp_lin_iterate_until_nonlinear queues (gbp_lin_capi_until_nonlin.hip).
// Robust losses on such factors (include/gbp_lin.h, gbp_lin_set_robust_nonlinear):
//   nonlin_mahalanobis2<MODEL>   |diag(s) z - h(x)|^2 at a point;
//   nonlin_robustify_one<MODEL>  w_f and the flag of one factor from M at its LINPOINT (gbp.py:309), through lin_robust_weight;
//   lin_relin_one / k_lin_relin <MODEL, true>   the same lane with that in front: robustify and relinearise are both one lane per
//                          factor on the same linpoint, z and s, so the robust sweep stays at three launches.
// The factor stage of such a sweep is k_lin_factor<D, false, LinRelin>, with losses set k_lin_factor<D, true, LinRelin> (gbp_lin_sweep.hpp),
// D = 3 and D = 6 both instantiated in gbp_lin_capi_nonlin.hip.
// The model routines are host/device, so a host program can run them (tests/hostmath/lin_se3_shim.hip).
#pragma once
#include "gbp_lin_handle.hpp"
#include "gbp_lin_robust.hpp"
#include "gbp_math.hpp"

namespace gbp {

// how k_lin_relin is run
constexpr int NL_SWEEP = 0;                               // the stage of a sweep: test, iters, damping switch
constexpr int NL_ALONE = 1;                               // relinearise_factors alone (gbp.py:64-80): no damping switch
constexpr int NL_INIT = 2;                                // compute_all_factors (gbp.py:60-62): every factor, iters = 1, damping = 0
constexpr int NL_ROBUSTIFY = 3;                           // robustify_all_factors alone (gbp.py:82-84): k_lin_relin<MODEL, true> only

template <int MODEL> struct NonlinModel;

template <> struct NonlinModel<GBP_LIN_MODEL_SE2_BETWEEN> {
    static constexpr int D = 3, M = 3;
    static constexpr bool dense = true;                   // J is a small dense array: nonlin_factor below
    // h(x) whitened, and the two entries of J that depend on the translation; c, sn = cos, sin of theta_a
    static GBP_HD void h(const double (&x)[6], const double (&s)[3], double c, double sn, double (&out)[3])
    {
        const double dx = x[3] - x[0], dy = x[4] - x[1];
        out[0] = s[0] * (c * dx + sn * dy);
        out[1] = s[1] * (-sn * dx + c * dy);
        out[2] = s[2] * (x[5] - x[2]);
    }
    static GBP_HD void jac(const double (&x)[6], const double (&s)[3], double c, double sn, double (&J)[3][6])
    {
        const double dx = x[3] - x[0], dy = x[4] - x[1];
        J[0][0] = -s[0] * c;  J[0][1] = -s[0] * sn; J[0][2] = s[0] * (-sn * dx + c * dy); J[0][3] = s[0] * c;   J[0][4] = s[0] * sn; J[0][5] = 0.0;
        J[1][0] = s[1] * sn;  J[1][1] = -s[1] * c;  J[1][2] = s[1] * (-c * dx - sn * dy); J[1][3] = -s[1] * sn; J[1][4] = s[1] * c;  J[1][5] = 0.0;
        J[2][0] = 0.0;        J[2][1] = 0.0;        J[2][2] = -s[2];                      J[2][3] = 0.0;        J[2][4] = 0.0;       J[2][5] = s[2];
    }
    // h at a point
    static GBP_HD void eval(const double (&x)[6], const double (&s)[3], double (&out)[3])
    {
        double sn, c;
        sincos(x[2], &sn, &c);
        h(x, s, c, sn, out);
    }
};

// ---- SO(3) pieces of the SE(3) model: 3 x 3 matrices row-major in double[9], every loop unrolled so that they stay in registers ----

// sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3 from t = th^2.  Below th = 0.2 the closed forms of the last two cancel (an
// absolute error of eps / t); six terms of the series are then exact to 1e-17.
GBP_HD void se3_coeffs(double t, double &A, double &B, double &C)
{
    if (t < 0.04) {
        A = 1.0 + t * (-1.0 / 6 + t * (1.0 / 120 + t * (-1.0 / 5040 + t * (1.0 / 362880 + t * (-1.0 / 39916800)))));
        B = 0.5 + t * (-1.0 / 24 + t * (1.0 / 720 + t * (-1.0 / 40320 + t * (1.0 / 3628800 + t * (-1.0 / 479001600)))));
        C = 1.0 / 6 + t * (-1.0 / 120 + t * (1.0 / 5040 + t * (-1.0 / 362880 + t * (1.0 / 39916800 + t * (-1.0 / 6227020800.0)))));
    } else {
        double sn, cs;
        const double th = sqrt(t);
        sincos(th, &sn, &cs);
        A = sn / th;
        B = (1.0 - cs) / t;
        C = (th - sn) / (t * th);
    }
}

// The rotations past which Log and Jr^-1 take their forms for the neighbourhood of pi: th > 2.6 for the coefficient (t = th^2) and
// cos th < -0.875 (th > 2.636) for Log.  Below them nothing computes differently from the forms that lose digits only near pi.
constexpr double SE3_NEAR_PI_T = 6.76, SE3_NEAR_PI_COS = -0.875;

// 1/th^2 - (1 + cos th) / (2 th sin th) from t = th^2, 0 <= th < pi: the coefficient of [phi]x^2 in Jr^-1(phi).  (1 + cos th) / sin th
// is 0 / 0 at pi and loses eps / (pi - th) before it; it equals cot(th / 2), which has no cancellation there: past th = 2.6 that form.
GBP_HD double se3_jrinv_coeff(double t)
{
    if (t < 0.04) return 1.0 / 12 + t * (1.0 / 720 + t * (1.0 / 30240 + t * (1.0 / 1209600 + t * (1.0 / 47900160 + t * (691.0 / 1307674368000.0)))));
    double sn, cs;
    const double th = sqrt(t);
    if (t > SE3_NEAR_PI_T) {
        sincos(0.5 * th, &sn, &cs);
        return 1.0 / t - cs / (2.0 * th * sn);
    }
    sincos(th, &sn, &cs);
    return 1.0 / t - (1.0 + cs) / (2.0 * th * sn);
}

// I + a [w]x + b [w]x^2   ([w]x^2 = w w^T - |w|^2 I)
GBP_HD void se3_ik(const double (&w)[3], double a, double b, double (&out)[9])
{
    const double d = 1.0 - b * (w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    out[0] = d + b * w[0] * w[0];        out[1] = b * w[0] * w[1] - a * w[2]; out[2] = b * w[0] * w[2] + a * w[1];
    out[3] = b * w[1] * w[0] + a * w[2]; out[4] = d + b * w[1] * w[1];        out[5] = b * w[1] * w[2] - a * w[0];
    out[6] = b * w[2] * w[0] - a * w[1]; out[7] = b * w[2] * w[1] + a * w[0]; out[8] = d + b * w[2] * w[2];
}

// X Y and X^T Y
GBP_HD void se3_mul(const double (&X)[9], const double (&Y)[9], double (&out)[9])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) out[3 * i + j] = X[3 * i] * Y[j] + X[3 * i + 1] * Y[3 + j] + X[3 * i + 2] * Y[6 + j];
}
GBP_HD void se3_tmul(const double (&X)[9], const double (&Y)[9], double (&out)[9])
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) out[3 * i + j] = X[i] * Y[j] + X[3 + i] * Y[3 + j] + X[6 + i] * Y[6 + j];
}

// entry (i, j) of X^T diag(w) Y
GBP_HD double se3_wtmul(const double (&X)[9], const double (&w)[3], const double (&Y)[9], int i, int j)
{
    return X[i] * w[0] * Y[j] + X[3 + i] * w[1] * Y[3 + j] + X[6 + i] * w[2] * Y[6 + j];
}

// Log of a rotation matrix, the principal value: the skew part is sin th * axis and the trace part cos th, so th = atan2 of the two is
// accurate at small and at moderate angles alike (acos of the trace alone loses half the digits near 0); |phi| < pi is the domain.
// The skew part vanishes at pi, and an axis taken from it loses eps / (pi - th).  Past cos th = SE3_NEAR_PI_COS the axis a comes from
// the symmetric part (E + E^T) / 2 = cos th I + (1 - cos th) a a^T instead: the component with the largest diagonal entry from a square
// root (a_k^2 >= 1/3: no cancellation), the other two from the off-diagonal entries (1 - cos th) a_k a_j divided by it (the square root
// of a small diagonal difference would lose half the digits), the sign from the skew part (sin th > 0), the angle from the same atan2.
// Selects, no indexing: everything stays in registers.
GBP_HD void se3_log(const double (&E)[9], double (&phi)[3])
{
    const double v0 = 0.5 * (E[7] - E[5]), v1 = 0.5 * (E[2] - E[6]), v2 = 0.5 * (E[3] - E[1]);
    const double nv = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
    const double cs = 0.5 * (E[0] + E[4] + E[8] - 1.0);
    const double th = atan2(nv, cs);
    if (cs < SE3_NEAR_PI_COS) {
        const bool k0 = E[0] >= E[4] && E[0] >= E[8], k1 = !k0 && E[4] >= E[8];
        const double s01 = 0.5 * (E[1] + E[3]), s02 = 0.5 * (E[2] + E[6]), s12 = 0.5 * (E[5] + E[7]), oc = 1.0 - cs;
        const double ak = copysign(sqrt(((k0 ? E[0] : k1 ? E[4] : E[8]) - cs) / oc), k0 ? v0 : k1 ? v1 : v2), den = oc * ak;
        phi[0] = th * (k0 ? ak : (k1 ? s01 : s02) / den);
        phi[1] = th * (k1 ? ak : (k0 ? s01 : s12) / den);
        phi[2] = th * (k0 ? s02 / den : k1 ? s12 / den : ak);
        return;
    }
    const double k = nv > 0.0 ? th / nv : 1.0;
    phi[0] = k * v0; phi[1] = k * v1; phi[2] = k * v2;
}

template <> struct NonlinModel<GBP_LIN_MODEL_SE3_BETWEEN> {
    static constexpr int D = 6, M = 6;
    static constexpr bool dense = false;                  // J is block sparse: factor_store below
    // Q = R_a^T, E = Q R_b, u = Q (t_b - t_a), phi = Log(E), and the right Jacobians of both rotation vectors (a caller that uses
    // none of them -- eval -- pays for none: everything here is inlined)
    static GBP_HD void pose(const double (&x)[12], double (&Q)[9], double (&E)[9], double (&u)[3], double (&phi)[3], double (&Jra)[9], double (&Jrb)[9])
    {
        const double wa[3] = {x[3], x[4], x[5]}, wb[3] = {x[9], x[10], x[11]};
        double A, B, C, Rb[9];
        se3_coeffs(wa[0] * wa[0] + wa[1] * wa[1] + wa[2] * wa[2], A, B, C);
        se3_ik(wa, -A, B, Q);
        se3_ik(wa, -B, C, Jra);
        se3_coeffs(wb[0] * wb[0] + wb[1] * wb[1] + wb[2] * wb[2], A, B, C);
        se3_ik(wb, A, B, Rb);
        se3_ik(wb, -B, C, Jrb);
        se3_mul(Q, Rb, E);
        const double d0 = x[6] - x[0], d1 = x[7] - x[1], d2 = x[8] - x[2];
#pragma unroll
        for (int i = 0; i < 3; ++i) u[i] = Q[3 * i] * d0 + Q[3 * i + 1] * d1 + Q[3 * i + 2] * d2;
        se3_log(E, phi);
    }
    // h at a point
    static GBP_HD void eval(const double (&x)[12], const double (&s)[6], double (&out)[6])
    {
        double Q[9], E[9], u[3], phi[3], Jra[9], Jrb[9];
        pose(x, Q, E, u, phi, Jra, Jrb);
#pragma unroll
        for (int k = 0; k < 3; ++k) { out[k] = s[k] * u[k]; out[3 + k] = s[3 + k] * phi[k]; }
    }
    // Factor.compute_factor at linpoint x (gbp.py:280-289): eta_f (12 entries) at eta[i * stride], Lambda_f packed upper (78) at
    // lam[Sym<12>::at(i, j) * stride], each stored as it is made.  With U = [u]x Jr(w_a), C = Jr^-1(phi) E^T Jr(w_a), G = Jr^-1(phi) Jr(w_b),
    // S1, S2 = diag of the two halves of s, and the variables in the order (t_a, w_a, t_b, w_b):
    //   J = [ -S1 Q  S1 U  S1 Q  0 ;  0  -S2 C  0  S2 G ],   b = J x0 + diag(s) z - h(x0) = [ S1 (U w_a + z_t) ;  S2 (G w_b - C w_a + z_w - phi) ]
    // (the translations of x0 cancel against u), and with W = Q^T S1^2 Q, X = Q^T S1^2 U
    //   Lambda_f = [ W  -X  -W  0 ;  .  U^T S1^2 U + C^T S2^2 C   X^T   -C^T S2^2 G ;  .  .  W  0 ;  .  .  .  G^T S2^2 G ]
    static GBP_HD void factor_store(const double (&x)[12], const double (&z)[6], const double (&s)[6], double *eta, double *lam, size_t stride)
    {
        double Q[9], U[9], Cm[9], G[9], phi[3];
        {
            double E[9], u[3], Jra[9], Jrb[9], Ji[9], T[9];
            pose(x, Q, E, u, phi, Jra, Jrb);
#pragma unroll
            for (int j = 0; j < 3; ++j) {                   // [u]x Jr(w_a)
                U[j] = u[1] * Jra[6 + j] - u[2] * Jra[3 + j];
                U[3 + j] = u[2] * Jra[j] - u[0] * Jra[6 + j];
                U[6 + j] = u[0] * Jra[3 + j] - u[1] * Jra[j];
            }
            se3_ik(phi, 0.5, se3_jrinv_coeff(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]), Ji);
            se3_tmul(E, Jra, T);
            se3_mul(Ji, T, Cm);
            se3_mul(Ji, Jrb, G);
        }
        double g1[3], g2[3];                                // S1 b_t, S2 b_w
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            g1[k] = s[k] * s[k] * (U[3 * k] * x[3] + U[3 * k + 1] * x[4] + U[3 * k + 2] * x[5] + z[k]);
            g2[k] = s[3 + k] * s[3 + k] * (G[3 * k] * x[9] + G[3 * k + 1] * x[10] + G[3 * k + 2] * x[11] - (Cm[3 * k] * x[3] + Cm[3 * k + 1] * x[4] + Cm[3 * k + 2] * x[5])
                                           + z[3 + k] - phi[k]);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const double q = Q[i] * g1[0] + Q[3 + i] * g1[1] + Q[6 + i] * g1[2];
            eta[i * stride] = -q;
            eta[(6 + i) * stride] = q;
            eta[(3 + i) * stride] = U[i] * g1[0] + U[3 + i] * g1[1] + U[6 + i] * g1[2] - (Cm[i] * g2[0] + Cm[3 + i] * g2[1] + Cm[6 + i] * g2[2]);
            eta[(9 + i) * stride] = G[i] * g2[0] + G[3 + i] * g2[1] + G[6 + i] * g2[2];
        }
        const double w1[3] = {s[0] * s[0], s[1] * s[1], s[2] * s[2]}, w2[3] = {s[3] * s[3], s[4] * s[4], s[5] * s[5]};
        auto put = [&](int i, int j, double v) { lam[(size_t)Sym<12>::at(i, j) * stride] = v; };
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double W = se3_wtmul(Q, w1, Q, i, j), X = se3_wtmul(Q, w1, U, i, j);
                if (j >= i) {
                    put(i, j, W);
                    put(6 + i, 6 + j, W);
                    put(3 + i, 3 + j, se3_wtmul(U, w1, U, i, j) + se3_wtmul(Cm, w2, Cm, i, j));
                    put(9 + i, 9 + j, se3_wtmul(G, w2, G, i, j));
                }
                put(i, 6 + j, -W);
                put(i, 3 + j, -X);
                put(3 + j, 6 + i, X);
                put(3 + i, 9 + j, -se3_wtmul(Cm, w2, G, i, j));
                put(i, 9 + j, 0.0);
                put(6 + i, 9 + j, 0.0);
            }
        }
    }
};

// 0.5 |h(x) - diag(s) z|^2 (Factor.energy gbp.py:261-265 with noise variance 1)
template <int MODEL>
GBP_HD double nonlin_energy(const double (&x)[2 * NonlinModel<MODEL>::D], const double (&z)[NonlinModel<MODEL>::M], const double (&s)[NonlinModel<MODEL>::M])
{
    constexpr int M = NonlinModel<MODEL>::M;
    double h[M], e = 0.0;
    NonlinModel<MODEL>::eval(x, s, h);
#pragma unroll
    for (int k = 0; k < M; ++k) { const double r = h[k] - s[k] * z[k]; e += r * r; }
    return 0.5 * e;
}

// Factor.compute_factor at linpoint x (gbp.py:280-289) of a model with a dense J (SE(2)): eta_f [6], Lambda_f packed upper [21] (the
// layout k_lin_factor reads).
template <int MODEL>
GBP_HD void nonlin_factor(const double (&x)[6], const double (&z)[3], const double (&s)[3], double (&eta)[6], double (&lam)[Sym<6>::size])
{
    static_assert(NonlinModel<MODEL>::dense && NonlinModel<MODEL>::D == 3 && NonlinModel<MODEL>::M == 3, "a block-sparse model has factor_store");
    constexpr int M = 3;
    double sn, c, J[3][6], b[3];
    sincos(x[2], &sn, &c);
    NonlinModel<MODEL>::jac(x, s, c, sn, J);
    // b = J x0 + diag(s) z - h(x0) with what cancels cancelled, as factor_store does for SE(3): the translation columns of J times x0
    // are h's first two rows and (theta_b - theta_a) its third, so only the theta_a column is left.  Added up term by term the sum loses
    // eps |x0| s -- with angles that are never wrapped, of any size.
    b[0] = s[0] * z[0] + J[0][2] * x[2];
    b[1] = s[1] * z[1] + J[1][2] * x[2];
    b[2] = s[2] * z[2];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double e = 0.0;
#pragma unroll
        for (int k = 0; k < M; ++k) e += J[k][i] * b[k];
        eta[i] = e;
#pragma unroll
        for (int j = i; j < 6; ++j) {
            double v = 0.0;
#pragma unroll
            for (int k = 0; k < M; ++k) v += J[k][i] * J[k][j];
            lam[Sym<6>::at(i, j)] = v;
        }
    }
}

// |diag(s) z - h(x)|^2 at a point: the squared Mahalanobis distance of Factor.robustify_loss (gbp.py:312, 322) with noise variance 1
template <int MODEL>
GBP_HD double nonlin_mahalanobis2(const double (&x)[2 * NonlinModel<MODEL>::D], const double (&z)[NonlinModel<MODEL>::M], const double (&s)[NonlinModel<MODEL>::M])
{
    constexpr int M = NonlinModel<MODEL>::M;
    double h[M], m2 = 0.0;
    NonlinModel<MODEL>::eval(x, s, h);
#pragma unroll
    for (int k = 0; k < M; ++k) { const double r = s[k] * z[k] - h[k]; m2 += r * r; }
    return m2;
}

// Factor.robustify_loss (gbp.py:296-332) of nonlinear factor f, one lane: h is evaluated at Factor.linpoint (gbp.py:309) AS IT STANDS,
// which is the reference's reading -- here the linpoint moves with every relinearisation.  Writes w_f and the flag with plain vector
// stores; a factor without a loss loads nothing but its loss.  Returns the flag.
template <int MODEL>
GBP_DEV bool nonlin_robustify_one(const LinParams &p, const LinNonlin &n, const LinRobust &r, int f)
{
    const size_t F = (size_t)p.F;
    const int loss = r.loss[f];
    int flag = 0;
    double w = 1.0;
    if (loss != GBP_LIN_LOSS_NONE) {
        constexpr int D = NonlinModel<MODEL>::D, M = NonlinModel<MODEL>::M;
        double x[2 * D], z[M], s[M];
#pragma unroll
        for (int k = 0; k < 2 * D; ++k) x[k] = n.linpoint[k * F + f];
#pragma unroll
        for (int k = 0; k < M; ++k) { z[k] = n.meas[k * F + f]; s[k] = n.sinfo[k * F + f]; }
        w = lin_robust_weight(loss, r.thr[f], 1.0, 0.5 * nonlin_mahalanobis2<MODEL>(x, z, s), flag);
    }
    r.w[f] = w;
    r.flag[f] = flag;
    return flag != 0;
}

// The relinearise stage for factor f, one lane: shared by the two kernels below so that a factor linearised over a range comes out bit
// for bit as one linearised with the whole graph.  A lane that does not relinearise writes iters only (and its damping in the sweep in
// which that switches); a relinearising lane writes the 2D + D(2D+1) doubles of the factor (6 + 21; SE(3): 12 + 78), the 2D of the linpoint, iters and its
// damping.  A
// lane that is not `live` neither loads nor stores.  Returns whether the factor was relinearised.
// ROBUST (losses are set): the lane FIRST makes w_f and the flag from the linpoint as it stands (robustify_all_factors comes before
// relinearise_factors in synchronous_iteration, gbp.py:87-90), then runs the test and the re-make below unchanged -- the re-made factor
// is the nominal one, and the weight stays.  In mode NL_ROBUSTIFY that is all it does.  `flagged`: whether the factor was flagged.
// The `false` instantiation reads nothing of `r` and is the code of a handle without losses.
template <int MODEL, bool ROBUST = false>
GBP_DEV bool lin_relin_one(const LinParams &p, const LinNonlin &n, const LinRobust &r, int mode, int f, bool live, bool &flagged)
{
    constexpr int D = NonlinModel<MODEL>::D, M = NonlinModel<MODEL>::M, P = LinDims<D>::P, REC = LinDims<D>::REC;
    const size_t F = (size_t)p.F;
    bool relin = false;
    flagged = false;
    if constexpr (ROBUST) {
        if (live) flagged = nonlin_robustify_one<MODEL>(p, n, r, f);
        if (mode == NL_ROBUSTIFY) return false;
    }
    if (live) {
        const double *ma = p.bel + (size_t)p.va[f] * REC + D + P, *mb = p.bel + (size_t)p.vb[f] * REC + D + P;
        double x[2 * D];
#pragma unroll
        for (int k = 0; k < D; ++k) { x[k] = ma[k]; x[D + k] = mb[k]; }
        int it = 1;
        if (mode == NL_INIT) relin = true;
        else {
            it = n.iters[f];
            double d2 = 0.0;
#pragma unroll
            for (int k = 0; k < 2 * D; ++k) { const double d = n.linpoint[k * F + f] - x[k]; d2 += d * d; }
            relin = sqrt(d2) > n.beta && it >= n.min_linear;                      // gbp.py:75
            it = relin ? 0 : it + 1;                                               // gbp.py:77, 80
        }
        n.iters[f] = it;
        if (relin) {
            double z[M], s[M];
#pragma unroll
            for (int k = 0; k < M; ++k) { z[k] = n.meas[k * F + f]; s[k] = n.sinfo[k * F + f]; }
            if constexpr (NonlinModel<MODEL>::dense) {
                double eta[6], lam[Sym<6>::size];
                nonlin_factor<MODEL>(x, z, s, eta, lam);
#pragma unroll
                for (int k = 0; k < 6; ++k) { n.feta[k * F + f] = eta[k]; n.linpoint[k * F + f] = x[k]; }
#pragma unroll
                for (int k = 0; k < Sym<6>::size; ++k) n.flam[(size_t)k * F + f] = lam[k];
            } else {                                        // entries stored as they are made, at stride F
                NonlinModel<MODEL>::factor_store(x, z, s, n.feta + f, n.flam + f, F);
#pragma unroll
                for (int k = 0; k < 2 * D; ++k) n.linpoint[k * F + f] = x[k];
            }
        }
        // gbp.py:78, then the switch of gbp.py:50-51 on the iters just written (0 after a relinearisation: fires when num_undamped == 0)
        if (mode == NL_SWEEP && it == n.num_undamped) n.fdamp[f] = p.damping;
        else if (relin) n.fdamp[f] = 0.0;
    }
    return relin;
}

// One lane per factor of the graph.  Lanes past F neither load nor store.  `count`: the slot of this sweep (nullptr for NL_INIT): one
// integer atomic add per wave that relinearised anything.
// ROBUST: the fused robustify + relinearise lane; `r` is read and `rcount` counted (the same way: one ballot, one popcount, one integer
// atomic add per wave that flagged anything) under it only.
// PT = LinGated (a sweep queued by gbp_lin_iterate_until_nonlinear): the whole kernel -- the lane and both counts -- returns at its head
// once the call's stop word is set; for PT = LinParams lin_stopped() is the constant false and the gate compiles away.
template <int MODEL, bool ROBUST = false, typename PT = LinParams>
__global__ __launch_bounds__(256) void k_lin_relin(PT p, LinNonlin n, int mode, int *count, LinRobust r, int *rcount)
{
    if (lin_stopped(p)) return;                             // PT = LinParams: never
    const int f = blockIdx.x * 256 + threadIdx.x;
    bool flagged;
    const bool relin = lin_relin_one<MODEL, ROBUST>(p, n, r, mode, f, f < p.F, flagged);
    if (count) {
        const unsigned long long who = __ballot(relin);
        if ((threadIdx.x & 63) == 0 && who) atomicAdd(count, __popcll(who));
    }
    if constexpr (ROBUST) {
        if (rcount) {
            const unsigned long long who = __ballot(flagged);
            if ((threadIdx.x & 63) == 0 && who) atomicAdd(rcount, __popcll(who));
        }
    }
}

// The same stage over the factors [f0, f1) only, one lane per factor of the RANGE: what gbp_lin_extend_nonlinear runs in mode NL_INIT
// on the factors it appended (compute_factor on the new factors, gbp.py:267-294).  Work and traffic go by f1 - f0, not by F; lanes
// outside the range neither load nor store; no atomics.  `mode` stays a run-time argument so that the lane's code is k_lin_relin's.
template <int MODEL>
__global__ __launch_bounds__(256) void k_lin_relin_range(LinParams p, LinNonlin n, int mode, int f0, int f1)
{
    const int f = f0 + blockIdx.x * 256 + threadIdx.x;
    bool flagged;
    (void)lin_relin_one<MODEL>(p, n, LinRobust{}, mode, f, f < f1, flagged);
}

// sum_f 0.5 |h(mu) - diag(s) z|^2 at the current belief means (gbp.py:36-44, 251-265): one partial per block, the lanes of a wave and
// the four waves of a block added in a fixed order, exactly the shape of k_lin_energy (gbp_lin_sweep.hpp).  PT = LinGated: the energy
// pass of a sweep of gbp_lin_iterate_until_nonlinear, gated like the stage above, into the call's own partials.
template <int MODEL, typename PT = LinParams>
__global__ __launch_bounds__(256) void k_lin_energy_nl(PT p, LinNonlin n, double *out)
{
    if (lin_stopped(p)) return;                             // PT = LinParams: never
    constexpr int D = NonlinModel<MODEL>::D, M = NonlinModel<MODEL>::M, P = LinDims<D>::P, REC = LinDims<D>::REC;
    __shared__ double red[256 / 64];
    const int f = blockIdx.x * 256 + threadIdx.x;
    const size_t F = (size_t)p.F;
    double e = 0.0;
    if (f < p.F) {
        const double *ma = p.bel + (size_t)p.va[f] * REC + D + P, *mb = p.bel + (size_t)p.vb[f] * REC + D + P;
        double x[2 * D], z[M], s[M];
#pragma unroll
        for (int k = 0; k < D; ++k) { x[k] = ma[k]; x[D + k] = mb[k]; }
#pragma unroll
        for (int k = 0; k < M; ++k) { z[k] = n.meas[k * F + f]; s[k] = n.sinfo[k * F + f]; }
        e = nonlin_energy<MODEL>(x, z, s);
        if (p.w) e *= p.w[f];                               // the weighted form (gbp.py:43): sigma^2 / adaptive_gauss_noise_var, as k_lin_energy
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) e += __shfl_down(e, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

}  // namespace gbp
