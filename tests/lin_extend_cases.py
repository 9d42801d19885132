"""Shared by tests/test_linear_extend_cpu.py and tests/test_linear_extend_gpu.py: growing the numpy oracles of the linear engine the
way gbp_lin_extend grows a handle (include/gbp_lin.h), and the growth schedules the placement routines and the kernels are checked on."""
import numpy as np

from lin_map_cases import random_pairs, random_priors, star
from lin_robust_cases import RobustOracle, generic_jz
from oracle.linear_oracle import LinearOracleBatched

TOL = 1e-9


def grow(o, va, vb, fe=None, fl=None, pe=None, pl=None, fc=None, J=None, z=None, sigma=None, loss=None, threshold=2.0):
    """The oracle of the grown graph: `o`'s variables and factors followed by the new ones (priors pe / pl; factors (va, vb) as
    (fe, fl, fc) for a LinearOracleBatched, as (J, z, sigma, loss, threshold) for a RobustOracle), the messages -- and weights and
    flags -- of the old factors carried over, the new ones at zero / 1 / False, then update_all_beliefs() (gbp.py:56-58)."""
    D, F0 = o.D, o.F
    va, vb = np.asarray(va, dtype=np.int64).reshape(-1), np.asarray(vb, dtype=np.int64).reshape(-1)
    dF = va.shape[0]
    pe = np.zeros((0, D)) if pe is None else np.asarray(pe, dtype=float).reshape(-1, D)
    pl = np.zeros((0, D, D)) if pl is None else np.asarray(pl, dtype=float).reshape(-1, D, D)
    va1, vb1 = np.concatenate([o.va, va]), np.concatenate([o.vb, vb])
    pe1, pl1 = np.concatenate([o.pe, pe]), np.concatenate([o.pl, pl])
    if isinstance(o, RobustOracle):
        J = np.asarray(J, dtype=float).reshape((dF,) + o.J.shape[1:])
        z = np.asarray(z, dtype=float).reshape((dF,) + o.z.shape[1:])
        sigma = np.broadcast_to(np.asarray(sigma, dtype=float), (dF,))
        names = [loss] * dF if (loss is None or isinstance(loss, str)) else list(loss)
        thr = np.broadcast_to(np.asarray(threshold, dtype=float), (dF,))
        g = RobustOracle(va1, vb1, np.concatenate([o.J, J]), np.concatenate([o.z, z]), np.concatenate([o.sigma, sigma]), pe1, pl1,
                         list(o.loss) + names, np.concatenate([o.thr, thr]), eta_damping=o.damping)
        g.w[:F0], g.flag[:F0] = o.w, o.flag
        g.fe, g.fl = g.fe0 * g.w[:, None], g.fl0 * g.w[:, None, None]
    else:
        fe = np.asarray(fe, dtype=float).reshape(dF, 2 * D)
        fl = np.asarray(fl, dtype=float).reshape(dF, 2 * D, 2 * D)
        fc = np.zeros(dF) if fc is None else np.asarray(fc, dtype=float).reshape(dF)
        g = LinearOracleBatched(va1, vb1, np.concatenate([o.fe, fe]), np.concatenate([o.fl, fl]), pe1, pl1,
                                factor_const=np.concatenate([o.fc, fc]), eta_damping=o.damping)
    g.msg_eta[:F0], g.msg_lam[:F0] = o.msg_eta, o.msg_lam
    g.update_all_beliefs()
    return g


def generic_fc(rs, D, F):
    """Random linear factors over [a; b] with their constants: (eta (F, 2d), Lambda (F, 2d, 2d), const (F,)); J of d + 1 rows."""
    J = rs.randn(F, D + 1, 2 * D)
    z = rs.randn(F, D + 1)
    return np.einsum('fmi,fm->fi', J, z), np.einsum('fmi,fmj->fij', J, J), 0.5 * np.einsum('fm,fm->f', z, z)


def schedules():
    """(name, N0, (va0, vb0), [(dN, va, vb), ...], eta_damping): the structure of every growth the engine is checked on.  Ids of a
    step lie in [0, N + dN) of that step."""
    rs = np.random.RandomState(2300)
    out = []
    # F 63 -> 64 -> 65 -> 129: wave tails of the factor stage and of the re-stride; N' = 27 is a multiple of neither 32, 7 nor 2
    N0 = 23
    a0, b0 = random_pairs(rs, N0, 63)
    s1 = (0, *random_pairs(rs, N0, 1))
    s2 = (1, np.array([N0]), np.array([4]))
    a3, b3 = random_pairs(rs, N0 + 4, 64)
    tails = [s1, s2, (3, a3, b3)]
    out.append(('tails', N0, (a0, b0), tails, 0.0))
    out.append(('tails_damped', N0, (a0, b0), tails, 0.4))
    # an empty handle grown into a graph
    a1, b1 = random_pairs(rs, 5, 7)
    a2, b2 = random_pairs(rs, 7, 4)
    out.append(('empty', 0, (np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)), [(5, a1, b1), (2, a2, b2)], 0.0))
    # dN = 0: loop closures among old variables, one of them on a pair that is joined already (once each way)
    chain = (np.arange(11), np.arange(1, 12))
    out.append(('closures', 12, chain, [(0, np.array([0, 3, 1, 11, 5]), np.array([1, 9, 0, 0, 2]))], 0.4))
    # dF = 0: isolated new variables; then old-old, old-new and new-new factors in one step
    out.append(('isolated_mixed', 12, chain, [(3, np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)),
                                              (2, np.array([0, 13, 15, 16, 2, 12]), np.array([7, 4, 16, 15, 16, 13]))], 0.0))
    # the hub of degree 203 gains 35 edges to new variables, then 35 to old ones, on alternating sides
    N, sa, sb = star(rs)
    new_leaves = N + np.arange(35)
    old_leaves = 1 + np.arange(35)
    alt = np.arange(35) % 2 == 0
    out.append(('star', N, (sa, sb), [(35, np.where(alt, 0, new_leaves), np.where(alt, new_leaves, 0)),
                                      (0, np.where(alt, old_leaves, 0), np.where(alt, 0, old_leaves))], 0.0))
    return out


def full_graph(sched):
    """(N, va, vb) of a schedule after all its steps."""
    _, N, (va, vb), steps, _ = sched
    for dN, a, b in steps:
        N, va, vb = N + dN, np.concatenate([va, a]), np.concatenate([vb, b])
    return N, np.asarray(va, dtype=np.int64), np.asarray(vb, dtype=np.int64)


def csr(N, va, vb):
    """The CSR the engine holds for a graph: (vptr, vadj = factor << 1 | side, epos_a, epos_b), by np.lexsort((factor, variable))."""
    F = len(va)
    var = np.concatenate([va, vb]).astype(np.int64)
    fac = np.concatenate([np.arange(F), np.arange(F)])
    side = np.concatenate([np.zeros(F, dtype=np.int64), np.ones(F, dtype=np.int64)])
    order = np.lexsort((fac, var))
    vptr = np.concatenate([[0], np.cumsum(np.bincount(var, minlength=N))]).astype(np.int32)
    vadj = ((fac[order] << 1) | side[order]).astype(np.int32)
    pos = np.empty(2 * F, dtype=np.int64)
    pos[order] = np.arange(2 * F)
    return vptr, vadj, pos[:F].astype(np.int32), pos[F:].astype(np.int32)


def robust_parts(rs, D, F, losses=True):
    """(J, z, sigma, loss, threshold) of F random factors, a share of them outliers."""
    from lin_robust_cases import mixed_losses
    J, z, sigma = generic_jz(rs, D, F)
    return J, z, sigma, (mixed_losses(rs, F) if losses else [None] * F), 1.0 + 2.0 * rs.rand(F)


__all__ = ['TOL', 'grow', 'generic_fc', 'schedules', 'full_graph', 'csr', 'robust_parts', 'random_priors']
