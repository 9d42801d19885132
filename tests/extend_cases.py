"""Batches and graphs at the edges of BAEngine.extend, for tests/test_extend_gpu.py and tools/rebuild_digest.py: what a growth call meets
that window_host.base_case()'s batch does not -- new variables no batch factor names, a batch without new variables, the smallest graphs.
"""
import dataclasses

import numpy as np

LONE = np.array([[0.3, -0.2, 4.0]])                              # a landmark no observation sees


def _raw_batch():
    """base_case()'s split before filter_batch: the batch still has the late observations of camera 5 and of every landmark"""
    from gbp_amd.synthetic import make_synthetic, keyframe_batches
    return keyframe_batches(make_synthetic(n_cams=20, n_lmks=150, obs_per_lmk=4, window=6, seed=1), [16, 2], defer=0.3).batches[0]


def bare_new_batch(base):
    """Two new cameras and three new landmarks on base_case()'s base: camera C + 1 and landmark L + 2 are named by no batch factor; camera C,
    landmarks L and L + 1 and some old variables are.  Landmark L is the split's own new one; landmark L + 1 is a second point 1 cm from
    an old landmark the new camera sees, and takes the batch's observations of that one."""
    b, C, L = _raw_batch(), base.n_cams, base.n_lmks
    ok = b['cam_idx'] != C + 1
    ci, li, z = b['cam_idx'][ok], b['lmk_idx'][ok].copy(), b['meas'][ok]
    twin = int(li[(ci == C) & (li < L)][0])
    li[li == twin] = L + 1
    out = dict(cam_means=b['cam_means'], lmk_means=np.concatenate([b['lmk_means'], base.lmk_means[twin:twin + 1] + 0.01, LONE]), meas=z,
               cam_idx=ci.astype(np.int32), lmk_idx=li.astype(np.int32))
    assert out['cam_means'].shape[0] == 2 and out['lmk_means'].shape[0] == 3
    assert C + 1 not in out['cam_idx'] and L + 2 not in out['lmk_idx'] and (out['cam_idx'] < C).any() and out['lmk_idx'].max() == L + 1
    assert {C}.issubset(out['cam_idx']) and {L, L + 1}.issubset(out['lmk_idx'])
    return out


def old_only_batch(base):
    """No new variable: the late observations of base_case()'s split between OLD cameras and OLD landmarks, and (the split defers none
    of camera 0's) a second observation of camera 0's first landmark half a pixel beside the first, so that EVERY old factor id
    behind camera 0's moves (ref_file is not the identity)."""
    b, C, L = _raw_batch(), base.n_cams, base.n_lmks
    ok = (b['cam_idx'] < C) & (b['lmk_idx'] < L)
    assert base.cam_idx[0] == 0
    out = dict(cam_means=np.zeros((0, 6)), lmk_means=np.zeros((0, 3)), meas=np.concatenate([b['meas'][ok], base.meas[:1] + 0.5]),
               cam_idx=np.concatenate([b['cam_idx'][ok], [0]]).astype(np.int32),
               lmk_idx=np.concatenate([b['lmk_idx'][ok], base.lmk_idx[:1]]).astype(np.int32))
    assert (out['cam_idx'] == 0).any() and (out['cam_idx'] > 0).any()
    return out


def smallest_case():
    """(base, batch, bare base): one camera, one landmark and the observation between them; a batch of one more of each -- the new camera
    sees the OLD landmark, the new landmark nothing; and the base without its observation."""
    from gbp_amd.synthetic import make_synthetic
    p = make_synthetic(n_cams=2, n_lmks=2, obs_per_lmk=2, window=2, seed=2)
    at = lambda c, l: int(np.flatnonzero((p.cam_idx == c) & (p.lmk_idx == l))[0])
    cut = lambda rows: dataclasses.replace(p, cam_means=p.cam_means[:1], lmk_means=p.lmk_means[:1], meas=p.meas[rows], cam_idx=p.cam_idx[rows],
                                           lmk_idx=p.lmk_idx[rows])
    r = at(1, 0)
    batch = dict(cam_means=p.cam_means[1:], lmk_means=p.lmk_means[1:], meas=p.meas[r:r + 1], cam_idx=np.array([1], np.int32),
                 lmk_idx=np.array([0], np.int32))
    return cut([at(0, 0)]), batch, cut([])
