"""Host helpers of the landmark-reordering tests (tests/test_reorder_cpu.py, tests/test_reorder_gpu.py): the numpy restatement of the
ordering rule of gbp_amd/csrc/gbp_policy.hpp (reorder_class_key / reorder_spread_key), the camera-set model the rule was chosen
against, sequence graphs given as camera lists, and the shuffle of a problem's landmark ids."""
import dataclasses

import numpy as np

WIDE_MIN = 128            # gbp_policy.hpp: REORDER_WIDE_MIN
N_RUNS = 256              # the model's workgroups: one per CU of an MI355X


def wide_span(C):
    return max(WIDE_MIN, C // 4)


def rule_order(cam_idx, lmk_idx, C, L):
    """internal_of_user (L,) int32 by the rule: landmarks whose cameras span at most wide_span(C) ids go along the trajectory by their
    lowest camera, the wide ones are spread evenly by rank through that order, landmarks without factors go last; ties keep user order."""
    cam_idx, lmk_idx = np.asarray(cam_idx, np.int64), np.asarray(lmk_idx, np.int64)
    deg = np.bincount(lmk_idx, minlength=L)
    lo, hi = np.full(L, C, np.int64), np.full(L, -1, np.int64)
    np.minimum.at(lo, lmk_idx, cam_idx)
    np.maximum.at(hi, lmk_idx, cam_idx)
    key1 = np.where(deg == 0, C + 1, np.where(hi - lo + 1 > wide_span(C), C, lo))
    first = np.argsort(key1, kind='stable')                  # locals by lowest camera | wide | without factors, user order inside each
    n_local, n_wide = int((key1 < C).sum()), int((key1 == C).sum())
    pos = np.arange(L, dtype=np.int64)
    j = pos - n_local
    key2 = np.where(pos < n_local, 2 * pos + 1,
                    np.where(pos < n_local + n_wide, 2 * (((2 * j + 1) * n_local) // max(2 * n_wide, 1)), 2 * n_local + 2))
    user_of_internal = first[np.argsort(key2, kind='stable')]
    internal_of_user = np.empty(L, np.int32)
    internal_of_user[user_of_internal] = np.arange(L, dtype=np.int32)
    return internal_of_user


def camera_sets(cam_idx, lmk_idx, internal_of_lmk, L, n_runs=N_RUNS):
    """The model: the landmarks in the given order, cut into n_runs equal runs; (largest number of distinct cameras of a run, the sum
    over the runs) -- what plan_info reports as max_window and table_rows when every tile holds the same number of landmarks."""
    run = (np.asarray(internal_of_lmk, np.int64)[np.asarray(lmk_idx)] * n_runs) // L
    C = int(np.max(cam_idx)) + 1
    pairs = np.unique(run * C + np.asarray(cam_idx, np.int64))
    per_run = np.bincount(pairs // C, minlength=n_runs)
    return int(per_run.max()), int(per_run.sum())


def sequence_lists(n_cams, n_lmks, obs, window, closures, seed=0):
    """A sequence graph as camera lists, without geometry: every landmark is drawn around a centre and seen from `obs` distinct cameras
    of the `window` consecutive ones around it, a fraction `closures` of them from anywhere instead; numbered by centre (generator
    order).  Returns (cam_idx, lmk_idx) landmark-major."""
    rng = np.random.default_rng(seed)
    ctr = np.sort(rng.uniform(window / 2.0, n_cams - window / 2.0, size=n_lmks))
    lo = np.clip(np.ceil(ctr - window / 2.0 - 0.5).astype(np.int64), 0, n_cams - window)
    wide = rng.uniform(size=n_lmks) < closures
    cams = np.empty((n_lmks, obs), np.int64)
    for start in range(0, n_lmks, 65536):
        s = slice(start, min(start + 65536, n_lmks))
        m = s.stop - s.start
        cams[s] = lo[s, None] + np.argsort(rng.uniform(size=(m, window)), axis=1)[:, :obs]
    w = np.flatnonzero(wide)
    for i in w:
        cams[i] = rng.choice(n_cams, size=obs, replace=False)
    return cams.reshape(-1).astype(np.int32), np.repeat(np.arange(n_lmks, dtype=np.int32), obs)


def shuffle_landmarks(problem, seed=0):
    """(problem with landmark ids permuted at random, new_of_old): lmk_idx and lmk_means relabelled, the file rows left in place."""
    L = problem.n_lmks
    new_of_old = np.random.default_rng(seed).permutation(L).astype(np.int32)
    lmk_means = np.empty_like(problem.lmk_means)
    lmk_means[new_of_old] = problem.lmk_means
    return dataclasses.replace(problem, lmk_means=lmk_means, lmk_idx=new_of_old[problem.lmk_idx].astype(np.int32)), new_of_old


def relabel_landmarks(problem, internal_of_user):
    """The problem in the numbering a reordered handle uses inside (BAEngine.landmark_order())."""
    m = np.asarray(internal_of_user, np.int32)
    lmk_means = np.empty_like(problem.lmk_means)
    lmk_means[m] = problem.lmk_means
    return dataclasses.replace(problem, lmk_means=lmk_means, lmk_idx=m[problem.lmk_idx].astype(np.int32))
