"""The smallest graphs that reach each path of the graph build (gbp_capi_build.hip), shared by tools/rebuild_digest.py (bit-for-bit
digests of what create leaves) and tests/test_build_stages_gpu.py (create under GBP_DEBUG_LAYOUT: nothing placed outside the arena).
A scenario: the problem, BAEngine's keyword arguments, environment overrides read at create, and `reached` -- a predicate on
plan_info() that says the scenario still takes the path it is named for."""
import collections
import dataclasses

import numpy as np

Scenario = collections.namedtuple('Scenario', 'problem kw env reached given_priors')


def _permuted(p, rows=None, lmks=None):
    """the same problem with its file rows in the order `rows` and / or landmark l renamed lmks[l]"""
    cam, lmk, meas, lm = p.cam_idx, p.lmk_idx, p.meas, p.lmk_means
    if lmks is not None:
        inv = np.empty_like(lmks)
        inv[lmks] = np.arange(lmks.size)
        lmk, lm = lmks[lmk].astype(np.int32), lm[inv]
    if rows is not None:
        cam, lmk, meas = cam[rows], lmk[rows], meas[rows]
    return dataclasses.replace(p, cam_idx=cam, lmk_idx=lmk, meas=meas, lmk_means=lm)


def build_scenarios():
    from gbp_amd.synthetic import make_synthetic
    from window_host import base_case, big_landmark_problem
    base = base_case().base                                      # 16 cameras, 149 landmarks, 430 factors, camera-major
    rng = np.random.default_rng(11)
    shuffled = _permuted(base, rows=rng.permutation(base.n_factors))
    assert not np.array_equal(shuffled.cam_idx, np.sort(shuffled.cam_idx))
    relabelled = _permuted(base, lmks=rng.permutation(base.n_lmks))
    dense = make_synthetic(n_cams=48, n_lmks=12, obs_per_lmk=40, seed=61)       # 40 of a tile's 64 slots: more than 15 % empty
    sequence = make_synthetic(n_cams=60, n_lmks=400, obs_per_lmk=4, seed=2, window=6)      # (every camera observed)
    none = lambda p: dataclasses.replace(p, meas=np.zeros((0, 2)), cam_idx=np.zeros(0, np.int32), lmk_idx=np.zeros(0, np.int32))
    assert np.unique(sequence.cam_idx).size == sequence.n_cams
    no_lmks = dataclasses.replace(none(base), lmk_means=np.zeros((0, 3)))
    S = lambda problem, kw=None, env=None, reached=lambda pi: True, given_priors=False: Scenario(problem, {'loss': 'huber', **(kw or {})}, env or {}, reached, given_priors)
    return {
        'file_order_not_camera_major': S(shuffled, reached=lambda pi: pi['fused'] and pi['pack_mode'] == 0),
        'chunk_tiles': S(big_landmark_problem(), reached=lambda pi: pi['pack_mode'] == 1),
        'dense_packing': S(dense, reached=lambda pi: pi['pack_mode'] == 2 and pi['n_tiles'] == (dense.n_factors + 63) // 64),
        'dense_remainder': S(base, dict(num_undamped_iters=0), reached=lambda pi: not pi['fused'] and not pi['staged_by_sparseness']),
        'loss_none': S(base, dict(loss=None), reached=lambda pi: pi['fused']),
        'reorder_landmarks': S(relabelled, dict(reorder_landmarks=True), reached=lambda pi: pi['fused']),
        'camera_windows': S(sequence, env=dict(GBP_WINDOWS='1'), reached=lambda pi: pi['fused'] and 0 < pi['max_window'] < 60 and pi['table_rows'] < pi['n_blocks'] * 60),
        'no_fused': S(base, dict(fused=False), reached=lambda pi: not pi['fused'] and not pi['staged_by_sparseness']),
        'no_factors': S(none(base), reached=lambda pi: not pi['fused'] and pi['n_tiles'] == 7, given_priors=True),
        'no_landmarks': S(no_lmks, reached=lambda pi: not pi['fused'] and pi['n_tiles'] == 0, given_priors=True),
    }


def create(s):
    """the scenario's engine with priors and beliefs (the environment overrides are set while create reads them, then put back)"""
    import os
    from gbp_amd.engine import BAEngine
    old = {k: os.environ.get(k) for k in s.env}
    os.environ.update(s.env)
    try:
        e = BAEngine.from_problem(s.problem, **s.kw)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if s.given_priors:                                          # the prior rule gives a variable without factors Lambda = 0
        e.set_priors_var([np.eye(6) * 1e-2] * s.problem.n_cams + [np.eye(3) * 1e-1] * s.problem.n_lmks)
    else:
        e.generate_priors_var(50.0)
    e.update_all_beliefs()
    return e
