"""Landmark reordering (GBP_FLAG_REORDER_LMKS) on a CPU: the ordering rule of gbp_amd/csrc/gbp_policy.hpp, compiled host-only through
tests/hostmath/reorder_shim.hip, against its numpy restatement (tests/reorder_host.py); and the camera-set model the rule was chosen
against -- the landmarks in some order, cut into 256 equal runs, distinct cameras per run -- on shuffled sequences.

The caps of the model are set against the GENERATOR's order (landmarks by the centre they were drawn around), not against what the rule
gives: the largest set at most 1.5 x the generator's and at most the fused sweep's table (fused_max_cams, read from the policy
headers), the rows of all sets at most 1.25 x the generator's."""
import ctypes as ct
import os
import shutil
import subprocess

import numpy as np
import pytest

from gbp_amd.synthetic import make_synthetic
from reorder_host import (N_RUNS, camera_sets, relabel_landmarks, rule_order, sequence_lists, shuffle_landmarks, wide_span)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'hostmath', 'reorder_shim.hip')
LIB = os.path.join(HERE, 'hostmath', 'libreorder_shim.so')
CSRC = os.path.join(os.path.dirname(HERE), 'gbp_amd', 'csrc')
_ip = ct.POINTER(ct.c_int32)


@pytest.fixture(scope='module')
def lib():
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    deps = [SRC] + [os.path.join(CSRC, f) for f in ('gbp_policy.hpp', 'gbp_fused_plan.hpp', 'gbp_kernels.hpp', 'gbp_math.hpp')]
    if not os.path.exists(LIB) or any(os.path.getmtime(d) > os.path.getmtime(LIB) for d in deps):
        tmp = f'{LIB}.{os.getpid()}.tmp'
        subprocess.check_call([hipcc, '--offload-host-only', '-O1', '-std=c++17', '-shared', '-fPIC', '-o', tmp, SRC])
        os.replace(tmp, LIB)
    so = ct.CDLL(LIB)
    i = ct.c_int
    for name, args, res in [('reorder_wide_span_of', [i], i), ('reorder_class_key_of', [i, i, i, i], i), ('reorder_spread_key_of', [i, i, i], i),
                            ('reorder_fused_max_cams', [], i), ('reorder_order', [_ip, _ip, i, i, i, _ip], None)]:
        fn = getattr(so, name)
        fn.argtypes, fn.restype = args, res
    return so


def shim_order(lib, cam_idx, lmk_idx, C, L):
    cam, lmk = np.ascontiguousarray(cam_idx, np.int32), np.ascontiguousarray(lmk_idx, np.int32)
    out = np.full(L, -1, np.int32)
    lib.reorder_order(cam.ctypes.data_as(_ip), lmk.ctypes.data_as(_ip), cam.size, C, L, out.ctypes.data_as(_ip))
    return out


# ---- the rule ---------------------------------------------------------------------------------------------------------------------

def test_wide_span_and_class_key_thresholds(lib):
    assert [lib.reorder_wide_span_of(C) for C in (1, 128, 512, 516, 2000, 13682)] == [128, 128, 128, 129, 500, 3420]
    assert all(lib.reorder_wide_span_of(C) == wide_span(C) for C in range(1, 3000, 7))
    C = 2000
    assert lib.reorder_class_key_of(3, 40, 539, C) == 40          # span 500: local, keyed by its lowest camera
    assert lib.reorder_class_key_of(3, 40, 540, C) == C           # span 501: wide
    assert lib.reorder_class_key_of(0, 2 ** 31 - 1, -1, C) == C + 1   # no factor
    assert lib.reorder_class_key_of(1, 0, 0, 1) == 0              # one camera


def test_spread_key_deals_the_wide_ones_evenly(lib):
    n_local, n_wide = 1000, 10
    keys = [lib.reorder_spread_key_of(p, n_local, n_wide) for p in range(n_local + n_wide + 3)]
    assert keys[:n_local] == [2 * p + 1 for p in range(n_local)]
    assert keys[n_local:n_local + n_wide] == [2 * (50 + 100 * j) for j in range(n_wide)]     # in front of locals 50, 150, ..., 950
    assert keys[n_local + n_wide:] == [2 * n_local + 2] * 3
    assert lib.reorder_spread_key_of(0, 0, 5) == 0 and lib.reorder_spread_key_of(5, 0, 5) == 2
    big = 2 ** 30 - 1                                             # no 32-bit overflow on the way
    assert lib.reorder_spread_key_of(big - 1, 10, big - 10) == 2 * (((2 * (big - 11) + 1) * 10) // (2 * (big - 10)))


@pytest.mark.parametrize('seed', range(6))
def test_rule_matches_its_numpy_restatement_on_random_graphs(lib, seed):
    rng = np.random.default_rng(seed)
    C = int(rng.choice([1, 2, 7, 130, 600, 3000]))
    L = int(rng.integers(1, 4000))
    F = int(rng.integers(0, 6 * L))
    lmk = rng.integers(0, max(1, int(L * 0.8)), size=F).astype(np.int32)        # the last fifth (and more) without factors
    base = rng.integers(0, C, size=L)
    local = rng.uniform(size=F) < 0.9
    cam = np.where(local, np.clip(base[lmk] + rng.integers(0, 20, size=F), 0, C - 1), rng.integers(0, C, size=F)).astype(np.int32)   # many ties
    got, want = shim_order(lib, cam, lmk, C, L), rule_order(cam, lmk, C, L)
    assert np.array_equal(np.sort(got), np.arange(L))
    assert np.array_equal(got, want)
    deg = np.bincount(lmk, minlength=L)
    empty = np.flatnonzero(deg == 0)
    assert np.array_equal(got[empty], L - empty.size + np.arange(empty.size))      # without factors: last, in user order


def test_already_ordered_input_gives_the_identity(lib):
    cam, lmk = sequence_lists(300, 5000, 4, 20, 0.0, seed=2)
    ident = rule_order(cam, lmk, 300, 5000)                        # some graph in its rule order ...
    lmk2 = ident[lmk]
    for order in (shim_order(lib, cam, lmk2, 300, 5000), rule_order(cam, lmk2, 300, 5000)):
        assert np.array_equal(order, np.arange(5000))              # ... is left alone
    one = shim_order(lib, np.zeros(50, np.int32), np.arange(50, dtype=np.int32)[::-1].copy(), 1, 50)
    assert np.array_equal(one, np.arange(50))                      # one camera: every key ties, user order stays


def test_order_is_invariant_under_the_shuffle_up_to_ties(lib):
    """The rule is a pure function of the graph: the runs' camera sets of a shuffled graph are those of the graph itself in rule order."""
    cam, lmk = sequence_lists(500, 20000, 6, 24, 0.02, seed=5)
    perm = np.random.default_rng(1).permutation(20000)
    a = camera_sets(cam, lmk, rule_order(cam, lmk, 500, 20000), 20000)
    b = camera_sets(cam, perm[lmk], rule_order(cam, perm[lmk], 500, 20000), 20000)
    assert abs(a[0] - b[0]) <= 0.1 * a[0] and abs(a[1] - b[1]) <= 0.02 * a[1]


# ---- the model ----------------------------------------------------------------------------------------------------------------------

def check_caps(lib, cam, lmk, C, L, label):
    """generator order = the landmark ids as given; shuffled, then ordered by the rule"""
    gen = camera_sets(cam, lmk, np.arange(L), L)
    perm = np.random.default_rng(11).permutation(L)
    shuffled = perm[lmk]
    unordered = camera_sets(cam, shuffled, np.arange(L), L)
    rule = camera_sets(cam, shuffled, rule_order(cam, shuffled, C, L), L)
    cap = lib.reorder_fused_max_cams()
    print(f'{label}: generator order {gen[0]} / {gen[1]}, shuffled {unordered[0]} / {unordered[1]}, rule {rule[0]} / {rule[1]} '
          f'(largest set / rows over {N_RUNS} runs; table cap {cap})')
    assert unordered[0] > cap                                      # what the flag is for: shuffled, no workgroup's set fits a table
    assert rule[0] <= 1.5 * gen[0]
    assert rule[0] <= cap
    assert rule[1] <= 1.25 * gen[1]
    return gen, rule


@pytest.mark.parametrize('window,closures', [(30, 0.0), (30, 0.02), (100, 0.02)])
def test_model_on_shuffled_synthetic_sequences(lib, window, closures):
    p = make_synthetic(n_cams=2000, n_lmks=100_000, window=window, closures=closures)      # numbered by centre: generator order
    gen, rule = check_caps(lib, p.cam_idx, p.lmk_idx, 2000, 100_000, f'2000 cams, window {window}, closures {closures}')
    if closures == 0.0:
        assert rule[0] <= gen[0] + 2 and rule[1] <= 1.01 * gen[1]  # the lowest-camera key alone reaches the generator's order


def test_model_on_a_shuffled_13682_camera_sequence(lib):
    cam, lmk = sequence_lists(13682, 616_000, 5, 60, 0.02, seed=0)
    check_caps(lib, cam, lmk, 13682, 616_000, '13682 cams, 616k x 5, window 60, closures 0.02')


def test_shuffle_and_relabel_helpers_are_inverse():
    p = make_synthetic(n_cams=12, n_lmks=200, obs_per_lmk=3, window=6)
    q, new_of_old = shuffle_landmarks(p, seed=4)
    assert np.array_equal(q.lmk_means[new_of_old], p.lmk_means) and np.array_equal(q.lmk_idx, new_of_old[p.lmk_idx])
    back = relabel_landmarks(q, np.argsort(new_of_old).astype(np.int32))
    assert np.array_equal(back.lmk_idx, p.lmk_idx) and np.array_equal(back.lmk_means, p.lmk_means)
