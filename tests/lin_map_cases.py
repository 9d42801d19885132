"""Shared by tests/test_linear_map_cpu.py and tests/test_linear_map_gpu.py: the graphs the batch-MAP solver of the linear engine is
checked on, the dense joint system built from the same arrays (gbp.py:94-126), a numpy block-Jacobi PCG, and the engine's device
layout for the host shim."""
import numpy as np

TOL = 1e-9
ITER_CAP = 200


def generic_factors(rs, D, F, rows=None):
    """Random linear factors over [a; b]: J rows x 2d (d + 1 rows by default: rank-deficient Lambda_f = J^T J for d > 1)."""
    rows = D + 1 if rows is None else rows
    J = rs.randn(F, rows, 2 * D)
    z = rs.randn(F, rows)
    return np.einsum('fmi,fm->fi', J, z), np.einsum('fmi,fmj->fij', J, J)


def random_priors(rs, N, D):
    A = rs.randn(N, D, D)
    return rs.randn(N, D), A @ A.transpose(0, 2, 1) + 2.0 * np.eye(D)


def random_pairs(rs, N, F):
    va = rs.randint(0, N, F)
    return va, (va + 1 + rs.randint(0, N - 1, F)) % N


def star(rs):
    """A hub of degree 203 (alternating sides), and variables of every degree 0..5."""
    pairs = [(0, l) if l % 2 else (l, 0) for l in range(1, 204)]
    nxt = 204
    for k in range(2, 6):                                   # u_k has degree k; its leaves get degree 2
        for j in range(k):
            leaf = 1 + 10 * k + j
            pairs.append((nxt, leaf) if j % 2 else (leaf, nxt))
        nxt += 1
    N = nxt + 1                                             # the last variable is isolated
    pairs = [pairs[i] for i in rs.permutation(len(pairs))]
    va, vb = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs])
    deg = np.bincount(np.concatenate([va, vb]), minlength=N)
    assert deg[0] == 203 and all(d in deg for d in range(6))
    return N, va, vb


def shapes(D):
    """(name, va, vb, factor_eta, factor_lam, prior_eta, prior_lam) for every shape the solver is checked on."""
    rs = np.random.RandomState(500 + D)
    out = []

    def add(name, N, va, vb, rows=None):
        va, vb = np.asarray(va, dtype=np.int64), np.asarray(vb, dtype=np.int64)
        fe, fl = generic_factors(rs, D, va.shape[0], rows)
        pe, pl = random_priors(rs, N, D)
        out.append((name, va, vb, fe, fl, pe, pl))
    add('n3_f0', 3, [], [])
    add('n2_f1', 2, [0], [1])
    for F in (63, 64, 65, 129):                             # wave tails of the factor stage
        N = 2 + F // 3
        add(f'f{F}', N, *random_pairs(rs, N, F))
    for N in (33, 67):                                      # not multiples of 64 / (d + P)
        add(f'n{N}', N, *random_pairs(rs, N, 2 * N + 3))
    N, va, vb = star(rs)
    add('star', N, va, vb)
    add('parallel', 4, [0, 1, 0, 2, 1], [1, 0, 1, 3, 2])    # one pair joined three times, both orientations
    add('rank1', 20, *random_pairs(rs, 20, 45), rows=1)     # J with one row, under SPD priors
    return out


def random_generic_graph(D):
    """The graph of test_linear_gpu.py::test_random_pairwise_graphs_all_sizes."""
    rs = np.random.RandomState(10 + D)
    N, F = 40, 150
    va = rs.randint(0, N, F)
    vb = (va + 1 + rs.randint(0, N - 1, F)) % N
    fe, fl = [], []
    for _ in range(F):
        J = rs.randn(D + 1, 2 * D)
        z = rs.randn(D + 1)
        fe.append(J.T @ z); fl.append(J.T @ J)
    A = rs.randn(N, D, D)
    pl = A @ A.transpose(0, 2, 1) + 2.0 * np.eye(D)
    pe = rs.randn(N, D)
    return va, vb, np.array(fe), np.array(fl), pe, pl


def scaled_displacement_graph():
    """A chain-with-skips displacement graph 1e6 from the origin whose joint has 1e3 <= cond <= 1e4 (checked by the CPU test):
    measurement sigma 0.1 against prior sigma 1.5."""
    from oracle.linear_oracle import displacement_graph
    rs = np.random.RandomState(77)
    N, D = 60, 3
    va = np.concatenate([np.arange(N - 1), np.arange(N - 3)])
    vb = np.concatenate([np.arange(1, N), np.arange(3, N)])
    _, _, fe, fl, _, pe, pl = displacement_graph(va, vb, 1e6 + rs.rand(N, D) * 10, 0.1, rs, prior_sigma=1.5)
    return va, vb, fe, fl, pe, pl


def dense_joint(va, vb, fe, fl, pe, pl):
    """(eta, Lambda) of the joint over all variables, assembled factor by factor as gbp.py:94-126 does."""
    N, D = pe.shape
    lam = np.zeros((N * D, N * D))
    eta = pe.reshape(-1).copy()
    for v in range(N):
        lam[v * D:(v + 1) * D, v * D:(v + 1) * D] += pl[v]
    for f in range(len(va)):
        idx = np.concatenate([np.arange(va[f] * D, (va[f] + 1) * D), np.arange(vb[f] * D, (vb[f] + 1) * D)])
        lam[np.ix_(idx, idx)] += fl[f]
        eta[idx] += fe[f]
    return eta, lam


def numpy_pcg(lam, eta, D, rel_tol=1e-12, max_iters=ITER_CAP):
    """Block-Jacobi PCG from x = 0 on the dense joint, the recurrence's residual tested every iteration: (x, iterations)."""
    n = eta.shape[0]
    N = n // D
    Minv = np.zeros_like(lam)
    for v in range(N):
        s = slice(v * D, (v + 1) * D)
        Minv[s, s] = np.linalg.inv(lam[s, s])
    x = np.zeros(n)
    en = np.linalg.norm(eta)
    if en == 0.0:
        return x, 0
    r = eta.copy()
    z = Minv @ r
    p = z.copy()
    rz = r @ z
    it = 0
    while np.linalg.norm(r) / en > rel_tol and it < max_iters:
        q = lam @ p
        alpha = rz / (p @ q)
        x += alpha * p
        r -= alpha * q
        z = Minv @ r
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
        it += 1
    return x, it


def pack(va, vb, fe, fl, pe, pl):
    """The engine's device layout (gbp_lin_handle.hpp LinParams): SoA factor rows [row][F], packed upper triangles, priors
    [N][d + P], CSR adjacency in ascending factor id with (factor << 1 | side), and the CSR position of every (factor, side)."""
    N, D = pe.shape
    F = len(va)
    va, vb = np.ascontiguousarray(va, dtype=np.int32), np.ascontiguousarray(vb, dtype=np.int32)
    up2 = [(i, j) for i in range(2 * D) for j in range(i, 2 * D)]
    up = [(i, j) for i in range(D) for j in range(i, D)]
    fl = np.asarray(fl, dtype=float).reshape(F, 2 * D, 2 * D)
    feta = np.ascontiguousarray(np.asarray(fe, dtype=float).reshape(F, 2 * D).T)
    flam = np.ascontiguousarray(np.stack([fl[:, i, j] for i, j in up2])) if F else np.zeros((len(up2), 0))
    prior = np.ascontiguousarray(np.concatenate([pe, np.stack([pl[:, i, j] for i, j in up], axis=1)], axis=1))
    vptr = np.zeros(N + 1, dtype=np.int32)
    np.add.at(vptr, va + 1, 1); np.add.at(vptr, vb + 1, 1)
    vptr = np.cumsum(vptr).astype(np.int32)
    vadj, ea, eb = np.zeros(max(2 * F, 1), dtype=np.int32), np.zeros(max(F, 1), dtype=np.int32), np.zeros(max(F, 1), dtype=np.int32)
    fill = vptr[:-1].copy()
    for f in range(F):
        ea[f] = fill[va[f]]; vadj[fill[va[f]]] = f << 1; fill[va[f]] += 1
        eb[f] = fill[vb[f]]; vadj[fill[vb[f]]] = (f << 1) | 1; fill[vb[f]] += 1
    return dict(D=D, N=N, F=F, va=va, vb=vb, feta=feta, flam=flam, prior=prior, vptr=vptr, vadj=vadj, epos_a=ea, epos_b=eb)


def rel(a, b):
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)) if b.size else 0.0
