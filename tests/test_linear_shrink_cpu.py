"""Shrinking a live linear graph (include/gbp_lin.h: gbp_lin_shrink) on a CPU: the C ABI boundary, the shrunk numpy oracle of
tests/lin_shrink_cases.py against the reference's own shrunk run (fixture G24) and against exact marginalisation on a tree, and the
engine's index routines (gbp_amd/csrc/gbp_lin_shrink.hpp) compiled for the host through tests/hostmath/lin_shrink_shim.hip against the
CSR numpy builds for the survivors' graph.  The GPU side is tests/test_linear_shrink_gpu.py."""
import ctypes as ct
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, golden
from lin_extend_cases import generic_fc, random_priors
from lin_map_cases import dense_joint, rel
from lin_shrink_cases import TOL, csr, fold_sides, plan, prefix_graphs, schedules, shrink, tree
from oracle.linear_oracle import LinearOracleBatched

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostmath', 'lin_shrink_shim.hip')
LIB = os.path.join(HERE, 'hostmath', 'liblin_shrink_shim.so')
CSRC = os.path.join(REPO, 'gbp_amd', 'csrc')
SCHEDULES = schedules()


def hipcc():
    return shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def capi():
    from gbp_amd import build, _capi
    build.build()
    return _capi


def test_shrink_symbol_is_declared_exported_and_bound(capi):
    lib = capi.load()
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(REPO, 'include', 'gbp_lin.h')).read(), flags=re.S)
    ip, vp = ct.POINTER(ct.c_int32), ct.c_void_p
    assert re.search(r'\bint\s+gbp_lin_shrink\s*\(', header), "gbp_lin_shrink is not declared in include/gbp_lin.h"
    assert hasattr(lib, 'gbp_lin_shrink'), "gbp_lin_shrink is not exported"
    assert capi.SIGNATURES['gbp_lin_shrink'] == (ct.c_int, [vp, vp])
    assert re.search(r'\}\s*gbp_lin_shrink_desc_t\s*;', header)
    assert [(n, t) for n, t in capi.LinShrink._fields_] == [
        ('n_retire_vars', ct.c_int32), ('retire_vars', ip), ('n_drop_factors', ct.c_int32), ('drop_factors', ip), ('fold', ct.c_int32),
        ('var_map', ip), ('factor_map', ip)]
    # the field order of the header's struct is the one bound
    body = re.search(r'typedef struct \{([^}]*)\}\s*gbp_lin_shrink_desc_t', header).group(1)
    names = re.findall(r'\*?\s*(\w+)\s*[;,]', body)
    assert names == [n for n, _ in capi.LinShrink._fields_]
    assert 'gbp_lin_capi_shrink.hip' in __import__('gbp_amd.build', fromlist=['SOURCES']).SOURCES


def test_shrink_refuses_a_null_handle(capi):
    lib = capi.load()
    d = capi.LinShrink()
    assert lib.gbp_lin_shrink(None, ct.byref(d)) == -1
    assert b'NULL handle' in lib.gbp_last_error()


def test_linear_engine_has_the_shrink_methods(capi):
    import inspect
    from gbp_amd.linear import LinearEngine
    for m in ('shrink', 'retire', 'cull'):
        assert callable(getattr(LinearEngine, m))
    par = inspect.signature(LinearEngine.shrink).parameters
    assert list(par)[1:] == ['retire_vars', 'drop_factors', 'fold']
    assert par['fold'].default is True and par['retire_vars'].default == () and par['drop_factors'].default == ()


# ---- the shrunk oracle against the reference ------------------------------------------------------------------------------------------

def test_shrunk_oracle_reproduces_the_reference_shrunk_run():
    """Fixture G24: ndim_posegraph.py's graph (n = 50, dim = 3, M = 5) built by the reference's classes, swept 10 times, variables 0..9
    and their factors removed with the removed factors' messages added to the kept variables' priors, update_all_beliefs(), 10 sweeps.
    Priors, means and beliefs right after the shrink and after its sweeps, and the energy, at the tolerance G23 is held to."""
    g = golden('G24_toy_linear_shrunk')
    va, vb, z, pe, pl = g['va'], g['vb'], g['meas'], g['prior_eta'], g['prior_lam']
    D = pe.shape[1]
    J = np.hstack([-np.eye(D), np.eye(D)])
    fe, fl, fc = z @ J, np.tile(J.T @ J, (len(va), 1, 1)), 0.5 * np.einsum('fd,fd->f', z, z)      # sigma = 1
    o = LinearOracleBatched(va, vb, fe, fl, pe, pl, factor_const=fc)
    o.update_all_beliefs()
    o.iterate(10)
    assert rel(o.get_means(), g['pre_means']) < TOL
    s, vmap, fmap = shrink(o, retire=g['retire'])
    assert (s.N, s.F) == (g['bel_eta'].shape[0], int((fmap >= 0).sum())) == (40, 100)
    assert np.array_equal(vmap, np.concatenate([np.full(10, -1), np.arange(40)]))
    assert rel(s.pe, g['shrunk_prior_eta']) < TOL and rel(s.pl, g['shrunk_prior_lam']) < TOL
    assert rel(s.get_means(), g['shrunk_means']) < TOL
    assert rel(s.beliefs()[0], g['shrunk_bel_eta']) < TOL and rel(s.beliefs()[1], g['shrunk_bel_lam']) < TOL
    s.iterate(10)
    assert rel(s.get_means(), g['means']) < TOL, f"means {rel(s.get_means(), g['means']):.3e}"
    assert rel(s.beliefs()[0], g['bel_eta']) < TOL and rel(s.beliefs()[1], g['bel_lam']) < TOL
    want = float(g['energy'])
    assert abs(s.energy() - want) <= TOL * abs(want), f"energy {s.energy()!r} vs {want!r}"


@pytest.mark.parametrize('D', [1, 3, 6])
def test_fold_is_exact_marginalisation_on_a_tree(D):
    """A chain of 12 with two side leaves, N + 2 undamped sweeps (messages converged: a tree), a prefix of the chain and one leaf retired
    with the fold: the dense MAP and the dense Lambda^-1 of the SHRUNK graph equal those of the FULL graph restricted to the survivors.
    Eight seeds; 1.1e-15 relative was seen at worst, TOL is asserted."""
    worst = 0.0
    for seed in range(8):
        rs = np.random.RandomState(2410 + 10 * seed + D)
        N, va, vb, fe, fl, fc, pe, pl, retire = tree(rs, D)
        o = LinearOracleBatched(va, vb, fe, fl, pe, pl, factor_const=fc)
        o.update_all_beliefs()
        o.iterate(N + 2)
        s, vmap, _ = shrink(o, retire=retire)
        eta, lam = dense_joint(va, vb, fe, fl, pe, pl)
        S = np.linalg.inv(lam)
        keep = np.flatnonzero(vmap >= 0)
        idx = np.concatenate([np.arange(v * D, (v + 1) * D) for v in keep])
        eta1, lam1 = dense_joint(s.va, s.vb, s.fe, s.fl, s.pe, s.pl)
        e1, e2 = rel(np.linalg.solve(lam1, eta1), (S @ eta)[idx]), rel(np.linalg.inv(lam1), S[np.ix_(idx, idx)])
        worst = max(worst, e1, e2)
        assert e1 < TOL and e2 < TOL, (seed, e1, e2)
    print(f"d = {D}: worst relative difference {worst:.3e}")


def test_shrink_keeps_prefix_beliefs_bit_identical():
    """The helper itself, not the engine: where the leaving factors are a prefix of a survivor's adjacency list, the shrunk oracle adds
    the same numbers in the same order -- checked per variable by a sequential sum, as numpy's own reduction order is not pinned.  (The
    engine's side of this is asserted in tests/test_linear_shrink_gpu.py.)"""
    for name, N, va, vb, retire in prefix_graphs():
        rs = np.random.RandomState(3)
        fe, fl, fc = generic_fc(rs, 3, len(va))
        o = LinearOracleBatched(va, vb, fe, fl, *random_priors(rs, N, 3), factor_const=fc, eta_damping=0.2)
        o.update_all_beliefs(); o.iterate(4)
        s, vmap, fmap = shrink(o, retire=retire)
        side = fold_sides(N, va, vb, retire)
        for v in np.flatnonzero(vmap >= 0):
            fs = [(f, 0) for f in np.flatnonzero(va == v)] + [(f, 1) for f in np.flatnonzero(vb == v)]
            fs.sort()
            gone = [fmap[f] < 0 for f, _ in fs]
            assert gone == sorted(gone, reverse=True), f"{name}: variable {v}: the leaving factors are not a prefix"
            assert all(side[f] == k + 1 for (f, k), g in zip(fs, gone) if g)
            full = o.pe[v].copy()
            for f, k in fs:
                full = full + o.msg_eta[f, k]
            part = s.pe[vmap[v]].copy()
            for (f, k), g in zip(fs, gone):
                if not g:
                    part = part + o.msg_eta[f, k]
            assert np.array_equal(full, part), f"{name}: variable {v}"


# ---- the engine's index routines on the host --------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def shim():
    deps = [SRC] + [os.path.join(CSRC, f) for f in ('gbp_lin_shrink.hpp', 'gbp_lin_handle.hpp', 'gbp_math.hpp')]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        tmp = f'{LIB}.{os.getpid()}.tmp'
        subprocess.check_call([hipcc(), '--offload-host-only', '-O1', '-std=c++17', '-shared', '-fPIC', '-o', tmp, SRC])
        os.replace(tmp, LIB)
    so = ct.CDLL(LIB)
    i, ip = ct.c_int, ct.POINTER(ct.c_int32)
    so.lin_shrink_place.argtypes = [i, i, ip, ip, ip, ip, i, ip, i, ip, i] + [ip] * 10
    so.lin_shrink_place.restype = None
    return so


def place(so, N, va, vb, retire, drop, fold):
    """The shim on one shrink of the graph (N, va, vb), whose CSR is the lexsort one: a dict of its outputs cut to their sizes."""
    ip = ct.POINTER(ct.c_int32)
    F = len(va)
    vptr, vadj, _, _ = csr(N, va, vb)
    arr = lambda x: np.ascontiguousarray(np.concatenate([np.asarray(x, dtype=np.int32).reshape(-1), np.zeros(1, dtype=np.int32)]))
    retire, drop = np.asarray(retire, dtype=np.int32).reshape(-1), np.asarray(drop, dtype=np.int32).reshape(-1)
    ins = [arr(va), arr(vb), arr(vptr), arr(vadj)]
    names = ('var_map', 'factor_map', 'edge_map', 'fold_side', 'fold_edge', 'sizes', 'vptr', 'vadj', 'epos_a', 'epos_b')
    outs = {k: np.full(n + 1, -1, dtype=np.int32) for k, n in zip(names, (N, F, 2 * F, F, 2 * F, 3, N + 1, 2 * F, F, F))}
    p = lambda x: x.ctypes.data_as(ip)
    so.lin_shrink_place(N, F, *[p(x) for x in ins], len(retire), p(arr(retire)), len(drop), p(arr(drop)), int(fold), *[p(outs[k]) for k in names])
    N1, F1, E1 = (int(x) for x in outs['sizes'][:3])
    cut = dict(var_map=N, factor_map=F, edge_map=2 * F, fold_side=F, fold_edge=2 * F, sizes=3, vptr=N1 + 1, vadj=E1, epos_a=F1, epos_b=F1)
    for k, n in cut.items():
        assert np.all(outs[k][n:] == -1), f"{k}: written past its end"
    return {k: outs[k][:n] for k, n in cut.items()}


def check_step(so, N, va, vb, retire, drop, fold):
    """One shrink: the shim's outputs against numpy.  Returns the survivors' graph."""
    got = place(so, N, va, vb, retire, drop, fold)
    vkeep, fkeep, listed, vmap, fmap = plan(N, va, vb, retire, drop)
    N1, F1 = int(vkeep.sum()), int(fkeep.sum())
    assert list(got['sizes']) == [N1, F1, 2 * F1]
    assert np.array_equal(got['var_map'], vmap) and np.array_equal(got['factor_map'], fmap)
    va1, vb1 = vmap[va[fkeep]].astype(np.int64), vmap[vb[fkeep]].astype(np.int64)
    wptr, wadj, wea, web = csr(N1, va1, vb1)
    assert np.array_equal(got['vptr'], wptr) and np.array_equal(got['vadj'], wadj)
    assert np.array_equal(got['epos_a'], wea) and np.array_equal(got['epos_b'], web)
    # every surviving edge -- the row of vmsg that moves with it -- at the position its (factor, side) has in the survivors' CSR
    _, old_adj, old_ea, old_eb = csr(N, va, vb)
    assert np.array_equal(got['edge_map'][old_ea[fkeep]], wea) and np.array_equal(got['edge_map'][old_eb[fkeep]], web)
    assert np.all(got['edge_map'][old_ea[~fkeep]] == -1) and np.all(got['edge_map'][old_eb[~fkeep]] == -1)
    # the fold decisions, per factor and per edge of a surviving variable
    side = fold_sides(N, va, vb, retire, drop, fold)
    assert np.array_equal(got['fold_side'], side)
    want = np.full(2 * len(va), -1, dtype=np.int32)          # edges of retired variables are not looked at
    want[old_ea[vkeep[va]]] = side[vkeep[va]] == 1
    want[old_eb[vkeep[vb]]] = side[vkeep[vb]] == 2
    assert np.array_equal(got['fold_edge'], want)
    return N1, va1, vb1


@pytest.mark.parametrize('sched', SCHEDULES, ids=[s[0] for s in SCHEDULES])
def test_host_index_routines_match_numpy_step_by_step(shim, sched):
    _, N, (va, vb), steps, _ = sched
    va, vb = np.asarray(va, dtype=np.int64), np.asarray(vb, dtype=np.int64)
    for retire, drop, fold in steps:
        N, va, vb = check_step(shim, N, va, vb, retire, drop, fold)
    if sched[0] == 'emptied':
        assert (N, len(va)) == (0, 0)


def test_host_index_routines_on_random_shrinks(shim):
    """A graph of 60 variables and 300 factors shrunk 40 times by random lists of either kind and either fold, to nothing."""
    rs = np.random.RandomState(24)
    N = 60
    va = rs.randint(0, N, 300)
    vb = (va + 1 + rs.randint(0, N - 1, 300)) % N
    for step in range(40):
        if not N:
            break
        retire = rs.permutation(N)[:int(rs.randint(0, 4))]
        drop = rs.permutation(len(va))[:int(rs.randint(0, 9))] if len(va) else np.zeros(0, dtype=np.int64)
        if step == 39:
            retire = np.arange(N)
        N, va, vb = check_step(shim, N, va, vb, retire, drop, int(rs.randint(0, 2)))
