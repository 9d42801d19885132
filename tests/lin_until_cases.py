"""Shared by tests/test_linear_until_cpu.py and tests/test_linear_until_gpu.py: a numpy model of gbp_lin_iterate_until's rule
(include/gbp_lin.h) over oracle/linear_oracle.py with the robust oracle of tests/lin_robust_cases.py -- step, energy and MAP distance
per sweep, the deciding sweep and the reason -- the graphs the GPU tests run on, and how a usable deciding sweep is chosen on them."""
import numpy as np

from lin_map_cases import dense_joint
from lin_robust_cases import RobustOracle
from oracle.linear_oracle import toy_posegraph

TOL = 1e-9
STOP_NONE, STOP_STEP, STOP_MAP = 0, 1, 2
TRACE_ENERGY, TRACE_MAP = 1, 2
FIN_THREADS = 1024                                           # UNTIL_FIN of gbp_amd/csrc/gbp_lin_until.hpp (the shim reports it)
MAX_S = 40


def displacement(name, va, vb, x_true, sigma, seed, outliers=0):
    """A displacement graph (h = x_b - x_a) as RobustOracle arguments; `outliers` of its measurements are 10 sigma off."""
    rs = np.random.RandomState(seed)
    va, vb = np.asarray(va, dtype=np.int64), np.asarray(vb, dtype=np.int64)
    N, D = x_true.shape
    F = va.shape[0]
    z = x_true[vb] - x_true[va] + rs.normal(0.0, sigma, (F, D))
    if outliers:
        z[rs.choice(F, outliers, replace=False)] += 10.0 * sigma
    J = np.broadcast_to(np.hstack([-np.eye(D), np.eye(D)]), (F, D, 2 * D)).copy()
    pl = np.ascontiguousarray(np.broadcast_to(np.eye(D) / 9.0, (N, D, D)))
    return dict(name=name, va=va, vb=vb, J=J, z=z, sigma=sigma, pe=(x_true + rs.normal(0.0, 1.0, (N, D))) @ pl[0].T, pl=pl)


def toy():
    va, vb, fe, _, _, pe, pl = toy_posegraph(100, 3, 10, 1.0, seed=0)
    D = 3
    J = np.broadcast_to(np.hstack([-np.eye(D), np.eye(D)]), (len(va), D, 2 * D)).copy()
    return dict(name='toy_d3', va=np.asarray(va, dtype=np.int64), vb=np.asarray(vb, dtype=np.int64), J=J, z=fe[:, D:].copy(), sigma=1.0, pe=pe, pl=pl)


def graphs():
    """toy_posegraph, a ring of d = 1 (each variable joined to its next two), a chain of d = 6 with skips."""
    rs = np.random.RandomState(91)
    n1, n6 = 37, 23
    ring = displacement('ring_d1', np.repeat(np.arange(n1), 2), (np.repeat(np.arange(n1), 2) + np.tile([1, 2], n1)) % n1, rs.rand(n1, 1) * 10, 0.5, 1, outliers=4)
    chain = displacement('chain_d6', np.concatenate([np.arange(n6 - 1), np.arange(n6 - 2)]), np.concatenate([np.arange(1, n6), np.arange(2, n6)]),
                         rs.rand(n6, 6) * 10, 0.5, 2, outliers=3)
    t = toy()
    rs.seed(5)
    t['z'][rs.choice(len(t['va']), 20, replace=False)] += 8.0
    t['name'] = 'toy_d3_outliers'
    return {g['name']: g for g in (toy(), ring, chain, t)}


def oracle(g, loss=None, threshold=2.0):
    o = RobustOracle(g['va'], g['vb'], g['J'], g['z'], g['sigma'], g['pe'], g['pl'], loss, threshold)
    o.update_all_beliefs()
    return o


def map_of(g):
    """The batch MAP of the nominal joint (what solve_map finds before any robustify), (N, d)."""
    o = RobustOracle(g['va'], g['vb'], g['J'], g['z'], g['sigma'], g['pe'], g['pl'], None, 2.0)
    eta, lam = dense_joint(o.va, o.vb, o.fe0, o.fl0, o.pe, o.pl)
    return np.linalg.solve(lam, eta).reshape(o.N, o.D)


def step_of(new, old):
    """max |mu_new - mu_old| over variables and coordinates; 0 without variables."""
    return float(np.max(np.abs(np.asarray(new) - np.asarray(old)))) if np.asarray(new).size else 0.0


def decide(step, dist, tol_step, tol_map):
    """The stop rule after one sweep: STEP is tested before MAP; a tolerance of 0 is off; dist None: the column is not traced."""
    if tol_step > 0.0 and step <= tol_step:
        return STOP_STEP
    if tol_map > 0.0 and dist is not None and dist <= tol_map:
        return STOP_MAP
    return STOP_NONE


def run_model(o, max_iters, tol_step=0.0, tol_map=0.0, x_map=None, robustify=False):
    """The call on an oracle: (rows (iters, 3) of step / energy / distance, iters, reason).  The oracle is left after the deciding sweep."""
    rows, reason = [], STOP_NONE
    for _ in range(max_iters):
        old = o.mu.copy()
        o.synchronous_iteration(robustify)
        step = step_of(o.mu, old)
        dist = None if x_map is None else float(np.linalg.norm(o.mu - x_map))
        rows.append((step, o.energy(), np.nan if dist is None else dist))
        reason = decide(step, dist, tol_step, tol_map)
        if reason != STOP_NONE:
            break
    return np.array(rows).reshape(-1, 3), len(rows), reason


def usable_sweep(*columns):
    """The first sweep s in 5 .. MAX_S (1-based) that is no multiple of 3 or 8 and at which every given column is strictly below all
    its earlier values (so that a tolerance equal to it stops exactly there, and no check_every of the tests lands on it); None if
    there is none."""
    for s in range(5, min([MAX_S] + [len(c) for c in columns]) + 1):
        if s % 3 and s % 8 and all(c[s - 1] < v for c in columns for v in c[:s - 1]):
            return s
    return None


def emulate_finish_sum(part):
    """The finishing block's sum of partials in its own order: per thread strided in index order, then slot t += slot t + s for
    s = FIN_THREADS / 2 .. 1."""
    part = np.asarray(part, dtype=float)
    rows = -(-max(part.size, 1) // FIN_THREADS)
    pad = np.zeros(rows * FIN_THREADS)
    pad[:part.size] = part
    a = np.zeros(FIN_THREADS)
    for r in pad.reshape(rows, FIN_THREADS):
        a = a + r
    s = FIN_THREADS // 2
    while s:
        a[:s] = a[:s] + a[s:2 * s]
        s //= 2
    return float(a[0])
