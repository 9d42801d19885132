#!/usr/bin/env python3
"""Generate fixture G31 (the SE(3) and SE(2) relative-pose factor models of include/gbp_lin.h in exact arithmetic).

    python tests/golden/make_g31.py

Every value is computed with mpmath at DPS decimal digits from the DEFINITIONS, not from the engine's closed forms, and rounded to
double once at the end: R = mp.expm of the hat matrix; Log in the skew form (axis from the skew part, angle from atan2 of its norm and
the trace part), which at DPS digits is good up to pi - |phi| = 1e-8 and far beyond; the Jacobian by central differences with step
STEP, whose truncation error (STEP^2 times a third derivative) and cancellation (15 of DPS digits) both lie far below a double's last
bit.  From h and J, still in mp: eta_f = J^T (J x0 + diag(s) z - h), Lambda_f = J^T J, the energy 0.5 |h - diag(s) z|^2 and the squared
Mahalanobis distance |diag(s) z - h|^2.  Nothing of the reference project and none of the test twins' model functions is read; numpy
draws the seeded points and writes the file.

The points (x = [t_a, w_a, t_b, w_b], z, s; `cls` names the class of each, CLASSES the order):
  zero          w_a = w_b = 0 exactly
  wa0           w_a = 0, a relative rotation of 0.1 .. 2.5
  series        |w_a|, |phi| in 1e-9 .. 1e-4
  crossover     |w_a|, |phi| in 0.19 .. 0.21 (the engine's coefficients change from series to closed form at |w| = 0.2)
  ulp04         t = |w_a|^2, |w_b|^2 within a few ulp of 0.04, on both sides
  tiny          |w_a| = |w_b| = 1e-160 and 1e-200 (t is subnormal, then 0)
  pastpi        |w_a| in (pi, 4.5), |phi| <= 2.5, w_b continued past pi beside w_a
  general       |w_a| < 3, |phi| <= 2.5
  pi-G          pi - |phi| = G for G in GAPS: per G six axes of phi (random; along x, y, z; one component exactly 0; one component
                1e-9) times three w_a (0; |w_a| in (0.3, 3); |w_a| in (pi, 4.5)); w_b = the exact Log of R_a Exp(phi), rounded
  twopi         |w_a|, |w_b| within 1e-3 of 2 pi on both sides, and between 2 pi and 7: Jr(w) is near rank loss
  bigt          translations of size 1e4 with translation sqrt_info 1e-3 .. 1
  bigs          translations of size 1 with sqrt_info 20
and an SE(2) block under the keys `se2_*`: theta_a, theta_b in +-{0, 1e-9, 1, 9, 1e3, 1e6} (angles are never wrapped).

Stored, all rounded to double: x, z, s, cls; Ra, Rb (n, 3, 3); u, phi (n, 3); h (n, 6), J (n, 6, 12), eta (n, 12), lam (n, 12, 12),
energy, m2 (n,); and se2_x, se2_z, se2_s, se2_h (m, 3), se2_J (m, 3, 6), se2_eta (m, 6), se2_lam (m, 6, 6), se2_energy, se2_m2.
tests/test_linear_se3_exact_cpu.py recomputes every 16th point through exact_se3 / exact_se2 below and finds the file equal to the bit.
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DPS = 60
STEP = mp.mpf(10) ** -15
GAPS = (0.5, 1e-1, 1e-2, 1e-3, 1e-4, 1e-6, 1e-8)
CLASSES = ['zero', 'wa0', 'series', 'crossover', 'ulp04', 'tiny', 'pastpi', 'general'] + [f'pi-{g:g}' for g in GAPS] + ['twopi', 'bigt', 'bigs']
SE2_ANGLES = (0.0, 1e-9, 1.0, 9.0, 1e3, 1e6)
mp.mp.dps = DPS


# ---- the model, from its definitions ------------------------------------------------------------------------------------------------

def vec(a):
    return mp.matrix([mp.mpf(float(v)) if not isinstance(v, mp.mpf) else v for v in a])


def exp_so3(w):
    return mp.expm(mp.matrix([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]))


def log_so3(R):
    v = mp.matrix([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
    nv = mp.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
    if nv == 0:
        return v
    return v * (mp.atan2(nv, (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2) / nv)


def _se3_u_phi(ta, Ra, tb, Rb):
    Q = Ra.T
    return Q * (tb - ta), log_so3(Q * Rb)


def _finish(x, z, s, h, J):
    """eta_f, Lambda_f, energy, m2 in mp from the whitened h (M,) and J (M, 2 D) at x."""
    M, n = J.rows, J.cols
    sz = mp.matrix([s[k] * z[k] for k in range(M)])
    b = J * x + sz - h
    r = h - sz
    m2 = sum(r[k] ** 2 for k in range(M))
    return J.T * b, J.T * J, m2 / 2, m2


def _rounded(m, shape=None):
    a = np.array([float(v) for v in m], dtype=np.float64)
    return a.reshape(shape) if shape else a


def exact_se3(x, z, s):
    """One point: dict of Ra, Rb, u, phi, h, J, eta, lam, energy, m2, computed at DPS digits and rounded to double."""
    x, z, s = vec(x), vec(z), vec(s)

    def parts(y):
        return y[0:3], exp_so3(y[3:6]), y[6:9], exp_so3(y[9:12])

    def whitened(p):
        u, phi = _se3_u_phi(*p)
        return mp.matrix([s[k] * u[k] for k in range(3)] + [s[3 + k] * phi[k] for k in range(3)])

    base = parts(x)
    u, phi = _se3_u_phi(*base)
    h = whitened(base)
    J = mp.zeros(6, 12)
    for i in range(12):
        side = []
        for sign in (1, -1):
            y = x.copy()
            y[i] += sign * STEP
            p = list(base)                                   # only the part that x_i belongs to is made again
            k = i // 3
            p[k] = exp_so3(y[3 * k:3 * k + 3]) if k in (1, 3) else y[3 * k:3 * k + 3]
            side.append(whitened(p))
        d = (side[0] - side[1]) / (2 * STEP)
        for k in range(6):
            J[k, i] = d[k]
    eta, lam, energy, m2 = _finish(x, z, s, h, J)
    return dict(Ra=_rounded(base[1], (3, 3)), Rb=_rounded(base[3], (3, 3)), u=_rounded(u), phi=_rounded(phi), h=_rounded(h), J=_rounded(J, (6, 12)),
                eta=_rounded(eta), lam=_rounded(lam, (12, 12)), energy=float(energy), m2=float(m2))


def exact_se2(x, z, s):
    """One point of the SE(2) model (x = [xa, ya, theta_a, xb, yb, theta_b]): dict of h, J, eta, lam, energy, m2."""
    x, z, s = vec(x), vec(z), vec(s)

    def whitened(y):
        c, sn = mp.cos(y[2]), mp.sin(y[2])
        dx, dy = y[3] - y[0], y[4] - y[1]
        return mp.matrix([s[0] * (c * dx + sn * dy), s[1] * (-sn * dx + c * dy), s[2] * (y[5] - y[2])])

    h = whitened(x)
    J = mp.zeros(3, 6)
    for i in range(6):
        yp, ym = x.copy(), x.copy()
        yp[i] += STEP
        ym[i] -= STEP
        d = (whitened(yp) - whitened(ym)) / (2 * STEP)
        for k in range(3):
            J[k, i] = d[k]
    eta, lam, energy, m2 = _finish(x, z, s, h, J)
    return dict(h=_rounded(h), J=_rounded(J, (3, 6)), eta=_rounded(eta), lam=_rounded(lam, (6, 6)), energy=float(energy), m2=float(m2))


# ---- the points ---------------------------------------------------------------------------------------------------------------------------

def _unit(rs, n=1):
    v = rs.normal(0, 1, (n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _wb_of(wa, phi):
    """The exact Log of R_a Exp(phi), rounded: phi may be an mp vector."""
    return _rounded(log_so3(exp_so3(vec(wa)) * exp_so3(vec(phi))))


def se3_points():
    """x (n, 12), z (n, 6), s (n, 6), cls (n,) indices into CLASSES."""
    rs = np.random.RandomState(2031)
    rows = []

    def add(name, wa, wb, scale_t=3.0, s=None, zw=(0.0, 2.5)):
        x = np.concatenate([rs.normal(0, scale_t, 3), wa, rs.normal(0, scale_t, 3), wb])
        z = np.concatenate([rs.normal(0, 2, 3) * max(1.0, scale_t / 3.0), _unit(rs)[0] * rs.uniform(*zw)])
        rows.append((CLASSES.index(name), x, z, rs.uniform(0.5, 20.0, 6) if s is None else s))

    zero = np.zeros(3)
    for _ in range(4):
        add('zero', zero, zero)
    for _ in range(6):
        add('wa0', zero, _unit(rs)[0] * rs.uniform(0.1, 2.5))
    for _ in range(24):
        wa = _unit(rs)[0] * 10.0 ** rs.uniform(-9, -4)
        add('series', wa, _wb_of(wa, _unit(rs)[0] * 10.0 ** rs.uniform(-9, -4)))
    for _ in range(20):
        wa = _unit(rs)[0] * rs.uniform(0.19, 0.21)
        add('crossover', wa, _wb_of(wa, _unit(rs)[0] * rs.uniform(0.19, 0.21)))
    for k in range(12):                                      # |w|^2 a few ulp either side of 0.04 (one ulp of 0.04 is 6.9e-18)
        wa, wb = _unit(rs)[0] * 0.2 * (1.0 + (k % 3 - 1) * 2.0 ** -52), _unit(rs)[0] * 0.2 * (1.0 + (1 - k % 3) * 2.0 ** -52)
        add('ulp04', wa, wb)
    for mag in (1e-160, 1e-160, 1e-200, 1e-200):
        add('tiny', _unit(rs)[0] * mag, _unit(rs)[0] * mag)
    for _ in range(24):
        wa = _unit(rs)[0] * rs.uniform(np.pi, 4.5)
        phi = _unit(rs)[0] * rs.uniform(0.0, 2.5)
        wb = _wb_of(wa, phi)
        axis = wb / np.linalg.norm(wb)                       # the same rotation continued past pi: w_b + 2 pi k along its own axis
        cands = [wb + 2 * np.pi * k * axis for k in (-1, 0, 1)]
        add('pastpi', wa, min(cands, key=lambda c: np.linalg.norm(c - wa)))
    for _ in range(32):
        wa = _unit(rs)[0] * rs.uniform(0.0, 3.0)
        add('general', wa, _wb_of(wa, _unit(rs)[0] * rs.uniform(0.0, 2.5)))
    for gap in GAPS:
        for kind in range(6):
            for wa_kind in range(3):
                a = _unit(rs)[0]
                if 1 <= kind <= 3:
                    a = np.eye(3)[kind - 1] * rs.choice([-1.0, 1.0])
                elif kind == 4:
                    a[rs.randint(3)] = 0.0
                elif kind == 5:
                    a[rs.randint(3)] = 1e-9
                a = vec(a)
                phi = a * ((mp.pi - mp.mpf(gap)) / mp.sqrt(a[0] ** 2 + a[1] ** 2 + a[2] ** 2))
                wa = zero if wa_kind == 0 else _unit(rs)[0] * (rs.uniform(0.3, 3.0) if wa_kind == 1 else rs.uniform(np.pi, 4.5))
                add(f'pi-{gap:g}', wa, _rounded(phi) if wa_kind == 0 else _wb_of(wa, phi), zw=(2.5, 3.1))
    for k in range(24):
        def near():
            if k < 16:
                return 2 * np.pi + (1.0 if k % 2 else -1.0) * 10.0 ** rs.uniform(-9, -3)
            return rs.uniform(2 * np.pi, 7.0)
        add('twopi', _unit(rs)[0] * near(), _unit(rs)[0] * near())
    for _ in range(8):
        wa = _unit(rs)[0] * rs.uniform(0.0, 3.0)
        s = np.concatenate([10.0 ** rs.uniform(-3, 0, 3), rs.uniform(0.5, 20.0, 3)])
        add('bigt', wa, _wb_of(wa, _unit(rs)[0] * rs.uniform(0.0, 2.5)), scale_t=1e4, s=s)
    for _ in range(8):
        wa = _unit(rs)[0] * rs.uniform(0.0, 3.0)
        add('bigs', wa, _wb_of(wa, _unit(rs)[0] * rs.uniform(0.0, 2.5)), scale_t=1.0, s=np.full(6, 20.0))
    cls = np.array([r[0] for r in rows], dtype=np.int32)
    return np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]), np.stack([r[3] for r in rows]), cls


def se2_points():
    """x (m, 6), z (m, 3), s (m, 3): every signed angle of SE2_ANGLES as theta_a and as theta_b at least once."""
    rs = np.random.RandomState(2032)
    vals = [sg * v for v in SE2_ANGLES for sg in ((1.0,) if v == 0.0 else (1.0, -1.0))]
    pairs = [(a, vals[(i * 3 + 1) % len(vals)]) for i, a in enumerate(vals)] + [(vals[(i * 5 + 2) % len(vals)], b) for i, b in enumerate(vals)]
    while len(pairs) < 40:
        pairs.append((vals[rs.randint(len(vals))], vals[rs.randint(len(vals))]))
    m = len(pairs)
    x = rs.normal(0, 3, (m, 6))
    x[:, 2], x[:, 5] = [p[0] for p in pairs], [p[1] for p in pairs]
    return x, rs.normal(0, 2, (m, 3)), rs.uniform(0.5, 20.0, (m, 3))


def main():
    x, z, s, cls = se3_points()
    out = {}
    for i in range(x.shape[0]):
        for k, v in exact_se3(x[i], z[i], s[i]).items():
            out.setdefault(k, []).append(v)
        if i % 50 == 0:
            print(f'SE(3) point {i} / {x.shape[0]}', flush=True)
    arrays = dict(x=x, z=z, s=s, cls=cls, classes=np.array(CLASSES), **{k: np.array(v) for k, v in out.items()})
    x2, z2, s2 = se2_points()
    out = {}
    for i in range(x2.shape[0]):
        for k, v in exact_se2(x2[i], z2[i], s2[i]).items():
            out.setdefault(k, []).append(v)
    arrays.update(se2_x=x2, se2_z=z2, se2_s=s2, **{'se2_' + k: np.array(v) for k, v in out.items()})
    path = os.path.join(HERE, 'G31_se3_exact.npz')
    np.savez_compressed(path, **arrays)
    print(f'wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB): {x.shape[0]} SE(3) points, {x2.shape[0]} SE(2) points')


if __name__ == '__main__':
    sys.dont_write_bytecode = True
    main()
