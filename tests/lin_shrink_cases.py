"""Shared by the tests of gbp_lin_shrink (include/gbp_lin.h): shrinking the numpy oracles of the linear engine the way the call shrinks
a handle -- retired variables and dropped factors leave, what a leaving factor last told its one surviving end is added to that end's
prior -- and the structural schedules the index routines and the kernels are checked on.  Host-only: numpy, nothing of the device."""
import numpy as np

from lin_extend_cases import TOL, csr, random_priors, robust_parts
from lin_map_cases import random_pairs, star
from lin_robust_cases import RobustOracle
from oracle.linear_oracle import LinearOracleBatched


def plan(N, va, vb, retire=(), drop=()):
    """What leaves: (vkeep (N,), fkeep (F,), listed (F,), var_map, factor_map); the maps hold the new id or -1 (monotone)."""
    va, vb = np.asarray(va, dtype=np.int64).reshape(-1), np.asarray(vb, dtype=np.int64).reshape(-1)
    vkeep, listed = np.ones(N, dtype=bool), np.zeros(len(va), dtype=bool)
    vkeep[np.asarray(retire, dtype=np.int64).reshape(-1)] = False
    listed[np.asarray(drop, dtype=np.int64).reshape(-1)] = True
    fkeep = ~listed & vkeep[va] & vkeep[vb]
    vmap = np.where(vkeep, np.cumsum(vkeep) - 1, -1).astype(np.int32)
    fmap = np.where(fkeep, np.cumsum(fkeep) - 1, -1).astype(np.int32)
    return vkeep, fkeep, listed, vmap, fmap


def fold_sides(N, va, vb, retire=(), drop=(), fold=True):
    """Per factor: 0 folds nothing, 1 folds towards a, 2 towards b."""
    vkeep, fkeep, listed, _, _ = plan(N, va, vb, retire, drop)
    va, vb = np.asarray(va, dtype=np.int64).reshape(-1), np.asarray(vb, dtype=np.int64).reshape(-1)
    side = np.zeros(len(va), dtype=np.int32)
    if fold:
        side[~listed & vkeep[va] & ~vkeep[vb]] = 1
        side[~listed & ~vkeep[va] & vkeep[vb]] = 2
    return side


def shrink(o, retire=(), drop=(), fold=True):
    """(oracle of the survivors, var_map, factor_map).  Priors: the old prior, then the folded messages in ascending factor id; the
    survivors' messages -- and weights and flags -- carried over; then update_all_beliefs() (gbp.py:56-58).  Mirrors
    lin_extend_cases.grow()."""
    vkeep, fkeep, listed, vmap, fmap = plan(o.N, o.va, o.vb, retire, drop)
    side = fold_sides(o.N, o.va, o.vb, retire, drop, fold)
    pe, pl = o.pe.copy(), o.pl.copy()
    for f in np.flatnonzero(side):                           # ascending factor id = adjacency order of every variable
        s = side[f] - 1
        v = (o.va, o.vb)[s][f]
        pe[v] = pe[v] + o.msg_eta[f, s]
        pl[v] = pl[v] + o.msg_lam[f, s]
    va1, vb1 = vmap[o.va[fkeep]].astype(np.int64), vmap[o.vb[fkeep]].astype(np.int64)
    if isinstance(o, RobustOracle):
        g = RobustOracle(va1, vb1, o.J[fkeep], o.z[fkeep], o.sigma[fkeep], pe[vkeep], pl[vkeep], [l for l, k in zip(o.loss, fkeep) if k],
                         o.thr[fkeep], eta_damping=o.damping)
        g.w, g.flag = o.w[fkeep].copy(), o.flag[fkeep].copy()
        g.fe, g.fl = g.fe0 * g.w[:, None], g.fl0 * g.w[:, None, None]
    else:
        g = LinearOracleBatched(va1, vb1, o.fe[fkeep], o.fl[fkeep], pe[vkeep], pl[vkeep], factor_const=o.fc[fkeep], eta_damping=o.damping)
    g.msg_eta, g.msg_lam = o.msg_eta[fkeep].copy(), o.msg_lam[fkeep].copy()
    g.update_all_beliefs()
    return g, vmap, fmap


def hub_edges(va, vb, hub=0):
    return np.flatnonzero((np.asarray(va) == hub) | (np.asarray(vb) == hub))


def schedules():
    """(name, N0, (va0, vb0), [(retire, drop, fold), ...], eta_damping): the structure of every shrink the engine is checked on.  The
    ids of a step are those of the graph that step finds."""
    rs = np.random.RandomState(2400)
    none = np.zeros(0, dtype=np.int64)
    out = []
    # F 65 -> 64 -> 63: the wave tails of the gather and of the factor stage (drop only)
    a, b = random_pairs(rs, 23, 65)
    out.append(('f65_64_63', 23, (a, b), [(none, [7], 1), (none, [0], 1)], 0.0))
    # F 257 -> 255: the block tail of the gather and of d_red
    a, b = random_pairs(rs, 40, 257)
    out.append(('f257_255', 40, (a, b), [(none, [3, 200], 1)], 0.4))
    # N 33 -> 31 (retire only, folded)
    a, b = random_pairs(rs, 33, 70)
    out.append(('n33_31', 33, (a, b), [([0, 17], none, 1)], 0.0))
    out.append(('n33_31_damped', 33, (a, b), [([0, 17], none, 1)], 0.4))
    # the hub of degree 203 loses every other edge, then is retired itself: 102 messages fold into 102 leaves
    N, sa, sb = star(rs)
    he = hub_edges(sa, sb)
    out.append(('star', N, (sa, sb), [(none, he[::2], 1), ([0], none, 1)], 0.0))
    # a chain with closures: retiring 1 and 2 leaves factor (1, 2) with both ends retired; 0 is left without a factor
    ca = np.array([0, 1, 2, 3, 4, 5, 6, 0, 2, 7, 3])
    cb = np.array([1, 2, 3, 4, 5, 6, 7, 1, 5, 4, 1])
    out.append(('both_ends', 9, (ca, cb), [([1, 2], none, 1)], 0.0))
    # drop and retire in one call; factor 2 = (2, 3) is listed AND has a retired end (no fold); then the same with fold = 0
    out.append(('mixed', 9, (ca, cb), [([3], [2, 5], 1), ([0], [1], 1)], 0.4))
    out.append(('mixed_nofold', 9, (ca, cb), [([3], [2, 5], 0), ([6, 2], none, 0)], 0.0))
    # variable 8 has no factor and is retired; 4's only factor (3, 4) leaves with 3, so 4 survives without one
    out.append(('isolated', 9, (np.array([0, 1, 3, 5]), np.array([1, 2, 4, 6])), [([8, 3], none, 1), (none, none, 1)], 0.0))
    # everything retired: N' = F' = 0 (the GPU test then extends the emptied handle)
    a, b = random_pairs(rs, 7, 12)
    out.append(('emptied', 7, (a, b), [([5, 1], [4], 1), ([4, 3, 2, 1, 0], none, 1)], 0.0))
    return out


def prefix_graphs():
    """(name, N, va, vb, retire): graphs built in pose order (factor ids ascend with the pose), the lowest-numbered variables retired,
    so that at every survivor the leaving factors are a prefix of its adjacency list."""
    n = 40
    chain = (np.arange(n - 1), np.arange(1, n))
    # a ring of neighbours built pose by pose: pose j is joined to j - 1, j - 2, j - 3 as it arrives (ndim_posegraph.py:76-88 order)
    a, b = [], []
    for j in range(1, n):
        for i in range(max(0, j - 3), j):
            a.append(i); b.append(j)
    return [('chain', n, chain[0], chain[1], np.arange(5)), ('ring', n, np.array(a), np.array(b), np.arange(6))]


def tree(rs, D, n=12):
    """The chain of n with two side leaves (on variables 6 and 9) as plain factors: (N, va, vb, fe, fl, fc, pe, pl, retire): a prefix
    of the chain plus one leaf are retired.  Every connected piece of what is retired has ONE surviving neighbour, so marginalising it
    joins no two survivors (no fill-in) and the fold is the whole of it."""
    from lin_extend_cases import generic_fc
    va = np.concatenate([np.arange(n - 1), [6, 9]])
    vb = np.concatenate([np.arange(1, n), [n, n + 1]])
    N = n + 2
    fe, fl, fc = generic_fc(rs, D, len(va))
    pe, pl = random_priors(rs, N, D)
    return N, va, vb, fe, fl, fc, pe, pl, np.array([0, 1, 2, 3, n + 1])


def robust_oracle(rs, D, N, va, vb, damping, losses):
    """A RobustOracle on a structure: losses 'on' (mixed) or not (all None).  Priors without a zero component."""
    J, z, sigma, loss, thr = robust_parts(rs, D, len(va), losses == 'on')
    pe, pl = random_priors(rs, N, D)
    pe = np.where(pe == 0.0, 1.0, pe)
    return RobustOracle(np.asarray(va, dtype=np.int64), np.asarray(vb, dtype=np.int64), J, z, sigma, pe, pl, loss, thr, eta_damping=damping)


__all__ = ['TOL', 'plan', 'fold_sides', 'shrink', 'schedules', 'prefix_graphs', 'tree', 'robust_oracle', 'csr', 'hub_edges']
