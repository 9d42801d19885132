"""The host arithmetic of the graph build (gbp_amd/csrc/gbp_build_plan.hpp) on a CPU, compiled host-only through
tests/hostmath/build_plan_shim.hip: the arena's size is the formula build_graph has always reserved with, the arena covers every array
placed in it and every upload of the fused plan (an array that does not fit is no error on the device -- it gets its own allocation and
a sweep's working set leaves the one block), and bits_for gives the bit counts the build's hand-written loops gave."""
import ctypes as ct
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostmath', 'build_plan_shim.hip')
LIB = os.path.join(HERE, 'hostmath', 'libbuild_plan_shim.so')
CSRC = os.path.join(os.path.dirname(HERE), 'gbp_amd', 'csrc')
CONSTANTS = ['WTILE', 'LIN_ROWS', 'MSG_ROWS', 'XTRA_ROW', 'LREC', 'TROW', 'CAMREC', 'CBEL', 'PART_ROW', 'RELIN_RING', 'RELIN_LANES', 'BLOCK',
             'CSTAGE_ROW', 'CSTAGE_PLAIN', 'INT4', 'INT2']
TABLE = ['cstage', 'lin', 'msg', 'xtra', 'avar', 'cpos', 'lrec', 'parts', 'cbel', 'cprior', 'cbelief', 'd_partial', 'd_red', 'd_relin_ring',
         'd_count', 'd_varmax']
PAGE = 4096


@pytest.fixture(scope='module')
def lib():
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    deps = [SRC] + [os.path.join(CSRC, f) for f in ('gbp_build_plan.hpp', 'gbp_fused_plan.hpp', 'gbp_kernels.hpp', 'gbp_math.hpp')]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        tmp = f'{LIB}.{os.getpid()}.tmp'
        subprocess.check_call([hipcc, '--offload-host-only', '-O1', '-std=c++17', '-shared', '-fPIC', '-o', tmp, SRC])
        os.replace(tmp, LIB)
    so = ct.CDLL(LIB)
    ll, ull, i = ct.c_longlong, ct.c_ulonglong, ct.c_int
    v11, out = ct.POINTER(ll), ct.POINTER(ull)
    sigs = {'plan_bits_for': ([ll], i), 'plan_arena_need': ([v11], ull), 'plan_arena_table': ([v11, out], i),
            'plan_uploads': ([i, i, ll, i, out], i), 'plan_arena_span': ([v11], ull), 'plan_uploads_span': ([i, i, ll, i], ull),
            'plan_constants': ([ct.POINTER(i)], i)}
    for name, (args, res) in sigs.items():
        fn = getattr(so, name)
        fn.argtypes, fn.restype = args, res
    return so


@pytest.fixture(scope='module')
def K(lib):
    out = (ct.c_int * 32)()
    assert lib.plan_constants(out) == len(CONSTANTS)
    return dict(zip(CONSTANTS, out))


def shapes(K):
    """(F, L, C, T, rows, n_wg, crow, general, remainder, robust, pack_mode, windowed): sizes of 0 and 1, each boolean both ways, every
    pack mode, whole tables (rows = n_wg * C), a windowed sum far below them, and the headline graph"""
    out = []
    small = [(0, 0, 0, 0), (0, 1, 1, 0), (1, 1, 1, 1), (1, 0, 1, 0), (0, 5, 3, 0), (426, 149, 16, 9), (4097, 1000, 700, 70), (100000, 9, 3, 1563)]
    for (F, L, C, T), remainder, robust, general, pack_mode in itertools.product(small, (0, 1), (0, 1), (0, 1), (0, 1, 2)):
        for n_wg in sorted({1, max(1, min(T, 256))}):
            crow = K['CSTAGE_ROW'] if remainder else K['CSTAGE_PLAIN']
            out.append((F, L, C, T, n_wg * C, n_wg, crow, general, remainder, robust, pack_mode, 0))
            if C and T:
                out.append((F, L, C, T, min(n_wg * C, n_wg * 2 + 1), n_wg, crow, general, remainder, robust, pack_mode, 1))
                out.append((F, L, C, T, 0, n_wg, crow, general, remainder, robust, pack_mode, 1))
    # one million factors at 40 per landmark, 500 cameras, 256 workgroups: dense tiles, whole tables; and a sequence of 2 000 cameras with windows
    out.append((1000000, 25000, 500, 15625, 256 * 500, 256, K['CSTAGE_PLAIN'], 0, 0, 1, 2, 0))
    out.append((1000000, 25000, 2000, 15625, 256 * 40, 256, K['CSTAGE_PLAIN'], 0, 0, 1, 2, 1))
    out.append((1000000, 25000, 2000, 15625, 256 * 2000, 256, K['CSTAGE_ROW'], 1, 1, 0, 1, 0))
    return out


def vec(s):
    return (ct.c_longlong * 11)(*s[:11])


def need_before(K, s):
    """the sum build_graph reserved with before the table existed, term for term"""
    F, L, C, T, rows, n_wg, crow, general, remainder, robust, pack_mode = (int(x) for x in s[:11])
    D, I = 8, 4
    S = max(T * K['WTILE'], 1)
    grid = (S + K['BLOCK'] - 1) // K['BLOCK']
    need = (max(F, 1) * crow * D + (64 << 8) if general else 0) \
        + S * (K['LIN_ROWS'] + K['MSG_ROWS'] + (K['XTRA_ROW'] if remainder else 0) + (1 if robust else 0)) * D + S * I
    need += max(L, 1) * K['LREC'] * D + max(rows, 1) * (K['TROW'] * D + 2 * I) + n_wg * K['INT4'] + max(C, 1) * K['INT2'] + 4 * 4096
    need += max(C, 1) * (K['CAMREC'] + K['CBEL'] + 27 + 27 + 1) * D + max(L, 1) * D
    need += 2 * grid * D + K['RELIN_RING'] * K['RELIN_LANES'] * I
    need += (n_wg + 1) * I + (2 * max(T, 1) * K['PART_ROW'] * D if pack_mode else 0) + (64 << 12)
    return need


def test_constants_are_the_layouts(K):
    assert (K['WTILE'], K['BLOCK'], K['INT4'], K['INT2']) == (64, 256, 16, 8)
    assert K['RELIN_RING'] == 1024


def test_arena_need_is_the_formula_it_replaces(lib, K):
    for s in shapes(K):
        assert lib.plan_arena_need(vec(s)) == need_before(K, s), s


def test_table_lists_what_the_build_allocates(lib, K):
    """sizes and existence of every array, restated: the ones the sweeps stream, then the small ones"""
    for s in shapes(K):
        F, L, C, T, rows, n_wg, crow, general, remainder, robust, pack_mode = (int(x) for x in s[:11])
        S = max(T * 64, 1)
        want = dict(cstage=max(F, 1) * crow * 8 if general and F > 0 else 0, lin=S * K['LIN_ROWS'] * 8, msg=S * K['MSG_ROWS'] * 8,
                    xtra=S * K['XTRA_ROW'] * 8 if remainder else 0, avar=S * 8 if robust else 0, cpos=S * 4, lrec=max(L, 1) * K['LREC'] * 8,
                    parts=2 * max(T, 1) * K['PART_ROW'] * 8 if pack_mode else 0, cbel=max(C, 1) * K['CAMREC'] * 8, cprior=max(C, 1) * 27 * 8,
                    cbelief=max(C, 1) * K['CBEL'] * 8, d_partial=max(C, 1) * 27 * 8, d_red=2 * ((S + 255) // 256) * 8,
                    d_relin_ring=K['RELIN_RING'] * K['RELIN_LANES'] * 4, d_count=8, d_varmax=max(C + L, 1) * 8)
        out = (ct.c_ulonglong * 32)()
        assert lib.plan_arena_table(vec(s), out) == len(TABLE)
        assert dict(zip(TABLE, out)) == want, s


def test_plan_uploads_are_fused_plans(lib, K):
    """fused_plan's fused_upload calls: the tables always, the four window arrays with windows"""
    out = (ct.c_ulonglong * 8)()
    assert lib.plan_uploads(256, 500, 256 * 500, 0, out) == 5
    assert list(out[:5]) == [256 * 500 * K['TROW'] * 8, 0, 0, 0, 0]
    assert lib.plan_uploads(256, 2000, 9000, 1, out) == 5
    assert list(out[:5]) == [9000 * K['TROW'] * 8, 256 * 16, 9000 * 4, 9000 * 4, 2000 * 8]
    assert lib.plan_uploads(1, 1, 0, 1, out) == 5                 # empty arrays are one element
    assert list(out[:5]) == [8, 16, 4, 4, 8]


def test_arena_covers_its_arrays_and_the_plan(lib, K):
    """every array starts on a page: the arena holds the page-rounded sizes of the table's arrays, then of the plan's uploads"""
    rnd = lambda n: (n + PAGE - 1) // PAGE * PAGE
    for s in shapes(K):
        F, L, C, T, rows, n_wg = (int(x) for x in s[:6])
        windowed = s[11]
        a, u = (ct.c_ulonglong * 32)(), (ct.c_ulonglong * 8)()
        na, nu = lib.plan_arena_table(vec(s), a), lib.plan_uploads(n_wg, C, rows, windowed, u)
        span = sum(rnd(b) for b in a[:na] if b) + sum(rnd(b) for b in u[:nu] if b)
        assert span == lib.plan_arena_span(vec(s)) + lib.plan_uploads_span(n_wg, C, rows, windowed)
        assert lib.plan_arena_need(vec(s)) >= span, (s, lib.plan_arena_need(vec(s)), span)


def test_bits_for_is_the_four_loops(lib):
    """bits_c / bits_l started at 1 and compared 1 << b (32-bit) against C and L; bits_k1 / bits_k2 compared 1ll << b against C + 2 and
    2 L + 3.  Below 2^31 both loops are the same function of what they compare against; bits_for is that function."""
    def loop32(n):
        b = 1
        while np.int32(1) << np.int32(b) < n:
            b += 1
        return b

    def loop64(n):
        b = 1
        while (1 << b) < n:
            b += 1
        return b

    ns = {0, 1, 2, 3, 4}
    for k in range(2, 31):
        ns |= {2 ** k - 1, 2 ** k, 2 ** k + 1}
    ns.discard(2 ** 30 + 1)
    for n in sorted(ns):
        assert lib.plan_bits_for(n) == loop32(n) == loop64(n), n
        assert lib.plan_bits_for(n + 2) == loop64(n + 2) and lib.plan_bits_for(2 * n + 3) == loop64(2 * n + 3), n
