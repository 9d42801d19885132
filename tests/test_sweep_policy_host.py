"""The sweep policy (gbp_amd/csrc/gbp_policy.hpp) on a CPU: every rule that decides which sweep runs, and in which form, pinned on both
sides of each of its thresholds, every environment override set and unset, and the choices on named graphs.  The rules are compiled
host-only through tests/hostmath/policy_shim.hip; the GPU tests check that each forced path gives the right beliefs, this one that the
automatic choice falls where the measurements in gbp_policy.hpp put it."""
import ctypes as ct
import math
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostmath', 'policy_shim.hip')
LIB = os.path.join(HERE, 'hostmath', 'libpolicy_shim.so')
CSRC = os.path.join(os.path.dirname(HERE), 'gbp_amd', 'csrc')

MiB = 1024.0 * 1024.0
NO_PIN = 0x7fffffff
FIELDS = ['pack_dense', 'fused_blocks', 'windows', 'staged_below', 'rows_wave_max', 'fused_pin_mib', 'fused_nt', 'acc_single',
          'single_probe_fail', 'cam_block', 'xchg_blocks', 'peer_split', 'peer_timeout_ms', 'rccl_fail', 'plan_debug', 'build_timing',
          'debug_layout']
UNSET = dict({f: None for f in FIELDS}, cam_block=0, peer_split=0, peer_timeout_ms=20000.0, rccl_fail=0, plan_debug=0, build_timing=0,
             debug_layout=0)


@pytest.fixture(scope='module')
def lib():
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    deps = [SRC] + [os.path.join(CSRC, f) for f in ('gbp_policy.hpp', 'gbp_fused_plan.hpp', 'gbp_kernels.hpp', 'gbp_math.hpp')]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        tmp = f'{LIB}.{os.getpid()}.tmp'
        subprocess.check_call([hipcc, '--offload-host-only', '-O1', '-std=c++17', '-shared', '-fPIC', '-o', tmp, SRC])
        os.replace(tmp, LIB)
    so = ct.CDLL(LIB)
    ll, i, d = ct.c_longlong, ct.c_int, ct.c_double
    sigs = {'policy_setenv': ([ct.c_char_p, ct.c_char_p], None), 'policy_clearenv': ([], None),
            'policy_overrides': ([ct.POINTER(d)], i), 'policy_dense_packing': ([ll, i, i], i), 'policy_fused_workgroups': ([i, i], i),
            'policy_camera_windows': ([i, i, ll, ll], i), 'policy_staged': ([ll, ll], i), 'policy_general_sweep': ([i, i, i, i, i], i),
            'policy_rows_wave': ([ll, i], i), 'policy_keep_mib': ([d], d), 'policy_pinned_tiles': ([d, d, d, i], i),
            'policy_single': ([i, i], i), 'policy_probe_mask': ([i], i), 'policy_cam_block': ([ll, i], i), 'policy_xchg_blocks': ([i, i], i),
            'policy_merged_exchange': ([i, i], i), 'policy_xchg_cap_fused': ([], i), 'policy_xchg_cap_staged': ([], i),
            'policy_fused_max_cams': ([], i), 'policy_sweep_bytes': ([i, i, i, ll, ct.POINTER(d)], None)}
    for name, (args, res) in sigs.items():
        fn = getattr(so, name)
        fn.argtypes, fn.restype = args, res
    so.policy_clearenv()
    return so


@pytest.fixture
def P(lib):
    """the shim with an empty override table, and a helper that sets one"""
    lib.policy_clearenv()
    yield lib
    lib.policy_clearenv()


def env(lib, **kv):
    lib.policy_clearenv()
    for k, v in kv.items():
        lib.policy_setenv(('GBP_' + k).encode(), v.encode())


def overrides(lib):
    out = (ct.c_double * 32)()
    n = lib.policy_overrides(out)
    assert n == len(FIELDS)
    return {f: (None if math.isnan(out[k]) else out[k]) for k, f in enumerate(FIELDS)}


def sweep_bytes(lib, T, L, C, rows):
    out = (ct.c_double * 3)()
    lib.policy_sweep_bytes(T, L, C, rows, out)
    return tuple(out)


# ---- parsing ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,value,field,expect', [
    ('PACK', 'dense', 'pack_dense', 1), ('PACK', 'whole', 'pack_dense', 0), ('PACK', 'DENSE', 'pack_dense', 0), ('PACK', '', 'pack_dense', 0),
    ('FUSED_BLOCKS', '12', 'fused_blocks', 12), ('FUSED_BLOCKS', '12x', 'fused_blocks', 12), ('FUSED_BLOCKS', 'x', 'fused_blocks', 0),
    ('WINDOWS', '0', 'windows', 0), ('WINDOWS', '1', 'windows', 1), ('WINDOWS', '7', 'windows', 1), ('WINDOWS', 'yes', 'windows', 0),
    ('STAGED_BELOW', '0.5', 'staged_below', 0.5), ('STAGED_BELOW', '1e-1', 'staged_below', 0.1), ('STAGED_BELOW', '0', 'staged_below', 0.0),
    ('ROWS_WAVE_MAX', '0', 'rows_wave_max', 0), ('ROWS_WAVE_MAX', '40', 'rows_wave_max', 40),
    ('FUSED_PIN_MIB', '-1', 'fused_pin_mib', -1.0), ('FUSED_PIN_MIB', '180.5', 'fused_pin_mib', 180.5),
    ('FUSED_NT', '3', 'fused_nt', 3), ('ACC_SINGLE', '0', 'acc_single', 0), ('ACC_SINGLE', '1', 'acc_single', 1),
    ('SINGLE_PROBE_FAIL', '5', 'single_probe_fail', 5), ('SINGLE_PROBE_FAIL', '0', 'single_probe_fail', 0),
    ('CAM_BLOCK', '128', 'cam_block', 128), ('CAM_BLOCK', 'x', 'cam_block', 0), ('XCHG_BLOCKS', '16', 'xchg_blocks', 16),
    ('PEER_SPLIT', '1', 'peer_split', 1), ('PEER_SPLIT', '0', 'peer_split', 1), ('PEER_SPLIT', '', 'peer_split', 1),
    ('PEER_TIMEOUT_MS', '150', 'peer_timeout_ms', 150.0), ('PEER_TIMEOUT_MS', '2.5', 'peer_timeout_ms', 2.5),
    ('PEER_TIMEOUT_MS', '0.5', 'peer_timeout_ms', 1.0), ('PEER_TIMEOUT_MS', '0', 'peer_timeout_ms', 1.0),
    ('PEER_TIMEOUT_MS', '-5', 'peer_timeout_ms', 1.0), ('PEER_TIMEOUT_MS', 'soon', 'peer_timeout_ms', 1.0),
    ('RCCL_FAIL', '0', 'rccl_fail', 1), ('PLAN_DEBUG', '', 'plan_debug', 1), ('BUILD_TIMING', '1', 'build_timing', 1),
    ('DEBUG_LAYOUT', '1', 'debug_layout', 1)])
def test_override_parsing(P, name, value, field, expect):
    """atoi / atof as the library always parsed them; a flag is set by its presence, whatever its value; each variable sets its own
    field and no other."""
    env(P, **{name: value})
    assert overrides(P) == dict(UNSET, **{field: expect})


def test_overrides_unset(P):
    assert overrides(P) == UNSET
    env(P, TILE_KERNEL='1', NO_REVERSE='1', NO_ARENA='1', PRINT_PTRS='1', PEER_COARSE='1')      # removed switches: nothing reads them
    assert overrides(P) == UNSET


# ---- the graph build ----------------------------------------------------------------------------------------------------------------

def test_packing(P):
    T = 100                                                    # dense below 0.85 x 64 T factors, and only with three factors per landmark
    assert P.policy_dense_packing(5439, T, 3) and not P.policy_dense_packing(5440, T, 3)
    assert not P.policy_dense_packing(5439, T, 2)
    assert not P.policy_dense_packing(0, T, 3) and not P.policy_dense_packing(100, 0, 3)
    env(P, PACK='dense')
    assert P.policy_dense_packing(6000, T, 3) and not P.policy_dense_packing(6000, T, 2)
    env(P, PACK='whole')
    assert not P.policy_dense_packing(100, T, 3)


def test_workgroups(P):
    assert [P.policy_fused_workgroups(T, 256) for T in (0, 1, 100, 256, 1000)] == [1, 1, 100, 256, 256]
    env(P, FUSED_BLOCKS='12')
    assert [P.policy_fused_workgroups(T, 256) for T in (5, 100, 1000)] == [5, 12, 12]
    env(P, FUSED_BLOCKS='0')
    assert P.policy_fused_workgroups(1000, 256) == 1
    env(P, FUSED_BLOCKS='1000')
    assert P.policy_fused_workgroups(1000, 256) == 256


def test_fused_max_cams(P):
    assert P.policy_fused_max_cams() == 587


def test_camera_windows(P):
    cmax = P.policy_fused_max_cams()
    assert P.policy_camera_windows(500, cmax, 700, 1000) and not P.policy_camera_windows(500, cmax, 701, 1000)   # sets at 7/10 of the tables
    assert P.policy_camera_windows(cmax + 1, cmax, 1000, 1000) and not P.policy_camera_windows(cmax, cmax, 1000, 1000)
    env(P, WINDOWS='0')
    assert not P.policy_camera_windows(cmax + 1, cmax, 1, 1000)
    env(P, WINDOWS='1')
    assert P.policy_camera_windows(10, cmax, 1000, 1000)


def test_staged_for_sparseness(P):
    rows = 256 * 500                                           # 0.75 factors per (workgroup, camera)
    assert P.policy_staged(95_999, rows) and not P.policy_staged(96_000, rows)
    env(P, STAGED_BELOW='0')
    assert not P.policy_staged(1, rows)
    env(P, STAGED_BELOW='1')
    assert P.policy_staged(rows - 1, rows) and not P.policy_staged(rows, rows)


def test_general_sweep(P):
    cmax = P.policy_fused_max_cams()
    assert not P.policy_general_sweep(0, 0, cmax, cmax, 0)
    assert P.policy_general_sweep(1, 0, 10, cmax, 0) and P.policy_general_sweep(0, 1, 10, cmax, 1)
    assert P.policy_general_sweep(0, 0, cmax + 1, cmax, 0) and not P.policy_general_sweep(0, 0, cmax + 1, cmax, 1)


# ---- the fused plan -------------------------------------------------------------------------------------------------------------------

def test_rows_wave(P):
    assert P.policy_rows_wave(1600, 100) and not P.policy_rows_wave(1601, 100)          # 16 rows per camera
    # many cameras: C > 662 + 2.16e-3 R (R = 17 592.6 at C = 700), beyond 16 rows per camera
    assert P.policy_rows_wave(17_592, 700) and not P.policy_rows_wave(17_593, 700)
    env(P, ROWS_WAVE_MAX='16')                                  # set: its bound alone
    assert P.policy_rows_wave(11_200, 700) and not P.policy_rows_wave(17_592, 700)
    env(P, ROWS_WAVE_MAX='0')
    assert not P.policy_rows_wave(1, 100000)
    env(P, ROWS_WAVE_MAX='40')
    assert P.policy_rows_wave(4000, 100) and not P.policy_rows_wave(4001, 100)


def test_cache_keep(P):
    assert P.policy_keep_mib(256 * MiB) == -1.0 and P.policy_keep_mib(256 * MiB + 1) == 230.0
    assert P.policy_keep_mib(350 * MiB - 1) == 230.0 and P.policy_keep_mib(350 * MiB) == 200.0
    assert P.policy_keep_mib(10_000 * MiB) == 200.0
    env(P, FUSED_PIN_MIB='100')
    assert P.policy_keep_mib(100 * MiB) == 100.0 and P.policy_keep_mib(1000 * MiB) == 100.0
    env(P, FUSED_PIN_MIB='-1')
    assert P.policy_keep_mib(1000 * MiB) == -1.0


def test_pinned_tiles(P):
    assert P.policy_pinned_tiles(-1.0, 0.0, 1.0, 10) == NO_PIN
    assert P.policy_pinned_tiles(200.0, 0.0, MiB, 10) == 20 and P.policy_pinned_tiles(200.0, 100 * MiB, MiB, 10) == 10
    assert P.policy_pinned_tiles(200.0, 300 * MiB, MiB, 10) == 0
    assert P.policy_pinned_tiles(0.0, 0.0, MiB, 10) == 0


def test_single_accumulation(P):
    assert P.policy_single(350, 0) == 1 and P.policy_single(351, 0) == 0
    assert P.policy_single(200, 1) == 1 and P.policy_single(201, 1) == 0
    for v in ('0', '1', '2'):
        env(P, ACC_SINGLE=v)
        assert P.policy_single(10, 0) == int(v) and P.policy_single(5000, 1) == int(v)


def test_single_probe_mask(P):
    assert P.policy_probe_mask(0) == 0 and P.policy_probe_mask(3) == 3
    env(P, SINGLE_PROBE_FAIL='5')
    assert P.policy_probe_mask(0) == 5
    env(P, SINGLE_PROBE_FAIL='0')
    assert P.policy_probe_mask(3) == 0


# ---- the launches -----------------------------------------------------------------------------------------------------------------------

def test_cam_block(P):
    C = 100                                                     # 64 / 128 / 256 threads at 200 / 640 factors per camera
    assert [P.policy_cam_block(F, C) for F in (0, 19_999, 20_000, 63_999, 64_000, 10**7)] == [64, 64, 128, 128, 256, 256]
    env(P, CAM_BLOCK='128')
    assert P.policy_cam_block(1, C) == 128 and P.policy_cam_block(10**7, C) == 128
    env(P, CAM_BLOCK='64')
    assert P.policy_cam_block(10**7, C) == 64
    env(P, CAM_BLOCK='0')
    assert P.policy_cam_block(1, C) == 64


def test_xchg_blocks(P):
    fused, staged = P.policy_xchg_cap_fused(), P.policy_xchg_cap_staged()
    assert fused == 2048 and staged == 2**31 - 1
    assert P.policy_xchg_blocks(4096, fused) == 2048 and P.policy_xchg_blocks(2047, fused) == 2047
    assert P.policy_xchg_blocks(4096, staged) == 4096
    env(P, XCHG_BLOCKS='16')
    assert P.policy_xchg_blocks(4096, fused) == 16 and P.policy_xchg_blocks(4096, staged) == 16 and P.policy_xchg_blocks(8, staged) == 8
    env(P, XCHG_BLOCKS='0')
    assert P.policy_xchg_blocks(4096, fused) == 1
    env(P, XCHG_BLOCKS='100000')
    assert P.policy_xchg_blocks(4096, fused) == 2048 and P.policy_xchg_blocks(4096, staged) == 4096


def test_merged_exchange(P):
    assert P.policy_merged_exchange(0, 1)
    assert not P.policy_merged_exchange(1, 1) and not P.policy_merged_exchange(0, 0)
    env(P, PEER_SPLIT='0')
    assert not P.policy_merged_exchange(0, 1)


# ---- named graphs ------------------------------------------------------------------------------------------------------------------------

def plan(P, C, L, F, T, min_deg, n_cus=256, set_share=1.0):
    """the automatic choices build_graph and fused_plan make for a graph of T whole-landmark tiles whose workgroups' camera sets add up
    to `set_share` of the whole tables"""
    cmax = P.policy_fused_max_cams()
    assert not P.policy_dense_packing(F, T, min_deg)
    n_wg = P.policy_fused_workgroups(T, n_cus)
    rows = n_wg * C
    windows = bool(P.policy_camera_windows(C, cmax, int(set_share * rows), rows))
    staged = bool(P.policy_staged(F, rows))
    general = bool(P.policy_general_sweep(int(staged), 0, C, cmax, int(windows)))
    fixed, touched, per_tile = sweep_bytes(P, T, L, C, rows)
    pin = P.policy_pinned_tiles(P.policy_keep_mib(touched), fixed, per_tile, n_wg)
    return dict(n_wg=n_wg, windows=windows, general=general, pinned=pin != NO_PIN, pin=pin, touched=touched,
                single=P.policy_single(C, int(pin != NO_PIN)), per_pair=F / rows)


def test_headline_graph(P):
    """500 cameras x 100 000 landmarks x 1M factors (ten per landmark: six landmarks per tile) on 256 CUs; random cameras, so every
    workgroup's set is nearly all 500: fused, whole tables, inside the cache (the 243 MB of arena_reserve), one accumulation round per rank"""
    p = plan(P, 500, 100_000, 1_000_000, -(-100_000 // 6), 10)
    assert p['n_wg'] == 256 and not p['general'] and not p['windows'] and not p['pinned'] and p['single'] == 0, p
    # 64 T slots x (22 stream rows + cpos) x 8 bytes + 100 000 landmark records of 160 bytes + 256 x 500 table rows of 224 bytes + 500
    # camera rows of 87 doubles
    assert p['touched'] == 64 * 16_667 * 23 * 8 + 100_000 * 160 + 256 * 500 * 224 + 500 * 87 * 8 == 241_290_592, p


def test_fr1desk_graph(P):
    """fr1desk: 63 cameras, 2 869 landmarks, 13 298 factors in 221 tiles -- 0.96 factors per (workgroup, camera), above the staged threshold: fused, SINGLE"""
    p = plan(P, 63, 2_869, 13_298, 221, 3)
    assert p['n_wg'] == 221 and not p['general'] and not p['pinned'] and p['single'] == 1, p
    assert round(p['per_pair'], 2) == 0.96


def test_2m_factor_graph(P):
    """bench.py's larger graph, twice the headline's landmarks: beyond the cache, 200 MiB of it kept, the rest streams past it"""
    p = plan(P, 500, 200_000, 2_000_000, -(-200_000 // 6), 10)
    assert not p['general'] and p['pinned'] and 0 < p['pin'] < -(-200_000 // 6) // 256 and p['single'] == 0, p
    assert p['touched'] > 350 * MiB
