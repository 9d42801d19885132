"""One window step as the sequence of the four calls it stands for -- the oracle side of BAEngine.window_step in
tests/test_window_step_*.py.

four_calls drives anything that has extend / cull / retire / retire_landmarks (a BAEngine, or the reference's own object graph behind
HostOps: tests/extend_host.py, cull_host.py, retire_host.py, retire_lmk_host.py on a NumpyBA) with lists given in the numbering from
BEFORE the step, carries every id through the maps of the calls before it, and composes the six maps gbp_ba_window_step reports
(include/gbp_ba.h).  base_case builds the graph, the batch and the lists of the tests, and says what it promises about them.
"""
import collections

import numpy as np

WindowMaps = collections.namedtuple('WindowMaps', 'cam_map lmk_map factor_map new_cam_ids new_lmk_ids new_factor_ids')


def compose(first, then):
    """old id -> id after `first` -> id after `then`; -1 stays -1."""
    first = np.asarray(first, np.int64)
    out = np.full(first.shape, -1, np.int64)
    ok = first >= 0
    out[ok] = np.asarray(then, np.int64)[first[ok]]
    return out


def filter_batch(batch, retire, lmks):
    """The batch without the observations that name a camera the step retires or a landmark it lets go of (gbp_ba_window_step refuses
    them: a front end does not add an observation to a keyframe it is dropping)."""
    ci, li = np.asarray(batch['cam_idx']), np.asarray(batch['lmk_idx'])
    ok = ~np.isin(ci, np.asarray(retire, np.int64)) & ~np.isin(li, np.asarray(lmks, np.int64))
    return dict(batch, meas=np.asarray(batch['meas'])[ok], cam_idx=ci[ok].astype(np.int32), lmk_idx=li[ok].astype(np.int32))


def new_factor_ids_of_extend(o2n, batch_cam_idx):
    """Union ids of the batch's factors after extend: the ids the old factors left free, taken in batch order inside each camera."""
    ci = np.asarray(batch_cam_idx)
    free = np.setdiff1d(np.arange(len(o2n) + ci.size), np.asarray(o2n))
    out = np.empty(ci.size, np.int64)
    out[np.argsort(ci, kind='stable')] = free
    return out


class EngineOps:
    """A BAEngine behind the four names four_calls uses."""

    def __init__(self, e, **prior_kw):
        self.e, self.kw = e, prior_kw

    def sizes(self):
        return self.e.C, self.e.L, self.e.F

    def extend(self, b):
        return self.e.extend(b['cam_means'], b['lmk_means'], b['meas'], b['cam_idx'], b['lmk_idx'], **self.kw)

    def cull(self, ids):
        return self.e.cull(ids)

    def retire(self, ids):
        return self.e.retire(ids)

    def retire_landmarks(self, ids, fold):
        return self.e.retire_landmarks(ids, fold=fold)


class HostOps:
    """The reference's object graph (a NumpyBA made by extend_host.make_numpy_ba) behind the same names."""

    def __init__(self, nb, **prior_kw):
        self.nb, self.kw = nb, prior_kw

    def sizes(self):
        return self.nb.C, self.nb.L, len(self.nb.graph.factors)

    def extend(self, b):
        from extend_host import extend
        return extend(self.nb, b, **self.kw)

    def cull(self, ids):
        from cull_host import cull_numpy_ba
        return cull_numpy_ba(self.nb, ids)

    def retire(self, ids):
        from retire_host import retire_numpy_ba
        return retire_numpy_ba(self.nb, ids)

    def retire_landmarks(self, ids, fold):
        from retire_lmk_host import retire_landmarks_numpy_ba
        return retire_landmarks_numpy_ba(self.nb, ids, fold)


def four_calls(ops, batch=None, cull=(), retire=(), lmks=(), fold=True):
    """extend(batch), cull, retire, retire_landmarks on `ops`, every list in the numbering from BEFORE the step.  Returns the six maps."""
    C, L, F = ops.sizes()
    cur = dict(cam=np.arange(C), lmk=np.arange(L), fac=np.arange(F), ncam=np.zeros(0, np.int64), nlmk=np.zeros(0, np.int64),
               nfac=np.zeros(0, np.int64))
    if batch is not None:
        dC, dL = len(np.asarray(batch['cam_means']).reshape(-1, 6)), len(np.asarray(batch['lmk_means']).reshape(-1, 3))
        o2n = ops.extend(batch)
        cur.update(fac=np.asarray(o2n, np.int64), nfac=new_factor_ids_of_extend(o2n, batch['cam_idx']),
                   ncam=np.arange(C, C + dC), nlmk=np.arange(L, L + dL))

    def push(maps):
        cm, lm, fm = maps
        for key, m in (('cam', cm), ('ncam', cm), ('lmk', lm), ('nlmk', lm), ('fac', fm), ('nfac', fm)):
            cur[key] = compose(cur[key], m)

    def alive(ids, key):
        t = cur[key][np.asarray(ids, np.int64).reshape(-1)]
        return t[t >= 0].astype(np.int32)

    if len(cull):
        push(ops.cull(alive(cull, 'fac')))
    if len(retire):
        push(ops.retire(alive(retire, 'cam')))
    if len(lmks):
        push(ops.retire_landmarks(alive(lmks, 'lmk'), fold))
    return WindowMaps(*(cur[k].astype(np.int32) for k in ('cam', 'lmk', 'fac', 'ncam', 'nlmk', 'nfac')))


def window_step_numpy_ba(nb, batch=None, cull=(), retire=(), lmks=(), fold=True, **prior_kw):
    """One window step on the reference's object graph: the composition of extend_numpy_ba, cull_numpy_ba, retire_numpy_ba and
    retire_landmarks_numpy_ba."""
    return four_calls(HostOps(nb, **prior_kw), batch, cull, retire, lmks, fold)


def result_problem(K, cam_means, lmk_means, fac, batch, maps):
    """The BAProblem a window step leaves, from the old graph's reference-order arrays (means, fac = dict z / cam / lmk), the batch and
    the six maps: file order = the staying old factors in old order, then the batch."""
    from gbp_amd.synthetic import BAProblem
    cam_u, lmk_u = np.concatenate([maps.cam_map, maps.new_cam_ids]), np.concatenate([maps.lmk_map, maps.new_lmk_ids])
    cm, lm = np.asarray(cam_means), np.asarray(lmk_means)
    z, ci, li = np.asarray(fac['z']), np.asarray(fac['cam']), np.asarray(fac['lmk'])
    if batch is not None:
        cm, lm = np.concatenate([cm, np.asarray(batch['cam_means']).reshape(-1, 6)]), np.concatenate([lm, np.asarray(batch['lmk_means']).reshape(-1, 3)])
        z, ci, li = np.concatenate([z, batch['meas']]), np.concatenate([ci, batch['cam_idx']]), np.concatenate([li, batch['lmk_idx']])
    kf = np.concatenate([maps.factor_map, maps.new_factor_ids]) >= 0
    return BAProblem(K=K, cam_means=cm[cam_u >= 0], lmk_means=lm[lmk_u >= 0], meas=z[kf], cam_idx=cam_u[ci[kf]].astype(np.int32),
                     lmk_idx=lmk_u[li[kf]].astype(np.int32))


# ---- the base graph, the batch and the lists of tests/test_window_step_*.py ------------------------------------------------------------
Case = collections.namedtuple('Case', 'base batch cull retire lmks saved orphan')


def base_case():
    """make_synthetic(20 cameras, 150 landmarks, 4 observations each, window 6, seed 1) cut into a base of 16 cameras and one batch of 2
    with 30 % of the old cameras' observations arriving late (the batch brings factors of OLD cameras: old factor ids move).  The lists:
    retire cameras 0 and 5; let go of every landmark of camera 1 (the camera is orphaned) and of one landmark of camera 5; cull four
    factors, one of them of camera 5.  Camera 5 is the only old observer of landmark `saved`, which the batch observes from cameras that
    stay.  The batch is the split's without the observations that name a retired camera or a listed landmark (filter_batch)."""
    from gbp_amd.synthetic import make_synthetic, keyframe_batches
    split = keyframe_batches(make_synthetic(n_cams=20, n_lmks=150, obs_per_lmk=4, window=6, seed=1), [16, 2], defer=0.3)
    base, raw = split.base, split.batches[0]
    cam, lmk = base.cam_idx, base.lmk_idx
    assert np.array_equal(cam, np.sort(cam))                     # the base file is in reference order: factor id = file row
    retire = np.array([0, 5], np.int32)
    orphan, saved = 1, 40
    of5 = [int(l) for l in lmk[cam == 5] if l != saved and l not in set(lmk[cam == orphan])]
    lmks = np.array(sorted(set(int(l) for l in lmk[cam == orphan]) | set(int(l) for l in raw['lmk_idx'][raw['cam_idx'] == orphan]) | {of5[0]}), np.int32)
    cull = np.array([int(np.flatnonzero(cam == 5)[1]), 100, 250, 400], np.int32)
    return Case(base, filter_batch(raw, retire, lmks), cull, retire, lmks, saved, orphan)


def check_case(c):
    """What the tests rely on, from cam_idx / lmk_idx alone."""
    cam, lmk, C, L = c.base.cam_idx, c.base.lmk_idx, c.base.n_cams, c.base.n_lmks
    bc, bl = c.batch['cam_idx'], c.batch['lmk_idx']
    assert (bc < C).any() and (bc >= C).any()                    # late observations of old cameras: ref_file is not the identity
    assert not np.isin(bc, c.retire).any() and not np.isin(bl, c.lmks).any()
    # one landmark loses all its old observers to the camera list but is seen by the batch
    assert c.saved < L and np.isin(cam[lmk == c.saved], c.retire).all() and (lmk == c.saved).any() and (bl == c.saved).any()
    assert c.saved not in c.lmks and not np.isin(np.flatnonzero(lmk == c.saved), c.cull).any()
    # one culled factor belongs to a retired camera
    assert np.isin(cam[c.cull], c.retire).any() and not np.isin(cam[c.cull], c.retire).all()
    # one factor has both a retired camera and a listed landmark
    assert (np.isin(cam, c.retire) & np.isin(lmk, c.lmks)).any()
    # one camera has all its landmarks listed, so it is orphaned
    assert c.orphan not in c.retire and np.isin(lmk[cam == c.orphan], c.lmks).all() and not (bc == c.orphan).any()
    # landmark 0 and camera 15 stay
    goes = np.isin(cam, c.retire) | np.isin(lmk, c.lmks)
    goes[c.cull] = True
    assert 0 not in c.lmks and ((lmk == 0) & ~goes).any() and 15 not in c.retire and ((cam == 15) & ~goes).any()
    return goes


# ---- edge graphs (the constructions of tests/test_retire_lmk_gpu.py, kept here so that no test module imports another) -----------------
def three_chunk_problem():
    """6 cameras x 300 landmarks x 3 observations, every camera with exactly 150 factors: three chunks of the camera fold, the last one
    partial.  Landmarks 0..149 are seen by cameras {0, 1, 2}, landmarks 150..299 by {3, 4, 5}, but for two: landmark 149 by {0, 2, 3} and
    landmark 150 by {1, 4, 5}."""
    import dataclasses
    from gbp_amd.synthetic import make_synthetic
    p = make_synthetic(n_cams=6, n_lmks=300, obs_per_lmk=6, window=None, seed=3)
    sees = np.zeros((300, 6), bool)
    sees[:150, :3] = True
    sees[150:, 3:] = True
    sees[149] = [True, False, True, True, False, False]
    sees[150] = [False, True, False, False, True, True]
    keep = sees[p.lmk_idx, p.cam_idx]
    q = dataclasses.replace(p, meas=p.meas[keep], cam_idx=p.cam_idx[keep], lmk_idx=p.lmk_idx[keep])
    assert q.n_factors == 900 and (np.bincount(q.cam_idx) == 150).all()
    return q


def big_landmark_problem():
    """landmark 0 is seen by all 80 cameras (above a tile: chunk tiles), 60 landmarks by 2 cameras each, 10 by one camera only"""
    from gbp_amd.synthetic import make_synthetic, BAProblem
    big = make_synthetic(n_cams=80, n_lmks=1, obs_per_lmk=80, window=80, seed=4)
    few = make_synthetic(n_cams=80, n_lmks=60, obs_per_lmk=2, window=8, seed=5)
    one = make_synthetic(n_cams=80, n_lmks=10, obs_per_lmk=1, window=8, seed=6)
    parts = (big, few, one)
    off = np.cumsum([0] + [q.n_lmks for q in parts])
    cam = np.concatenate([q.cam_idx for q in parts])
    order = np.argsort(cam, kind='stable')                      # camera-major, as the reference orders a file
    p = BAProblem(K=big.K, cam_means=big.cam_means, lmk_means=np.concatenate([q.lmk_means for q in parts]),
                  meas=np.concatenate([q.meas for q in parts])[order], cam_idx=cam[order].astype(np.int32),
                  lmk_idx=np.concatenate([q.lmk_idx + o for q, o in zip(parts, off)])[order].astype(np.int32))
    deg = np.bincount(p.lmk_idx, minlength=p.n_lmks)
    assert deg[0] == 80 and (deg[1:61] == 2).all() and (deg[61:] == 1).all()
    return p


def hold_back(problem, rows):
    """(base, batch): the problem without the observations `rows` (file rows), and a batch without new variables that brings them late.
    Every variable must keep an observation in the base."""
    import dataclasses
    rows = np.asarray(rows, np.int64)
    keep = np.ones(problem.n_factors, bool)
    keep[rows] = False
    base = dataclasses.replace(problem, meas=problem.meas[keep], cam_idx=problem.cam_idx[keep], lmk_idx=problem.lmk_idx[keep])
    assert np.unique(base.cam_idx).size == problem.n_cams
    batch = dict(cam_means=np.zeros((0, 6)), lmk_means=np.zeros((0, 3)), meas=problem.meas[rows].copy(),
                 cam_idx=problem.cam_idx[rows].astype(np.int32), lmk_idx=problem.lmk_idx[rows].astype(np.int32))
    return base, batch


def bare_camera_problem(cam=8):
    """base_case()'s 16-camera base without every observation of camera `cam`: the camera is in the graph and has no factor; every other
    camera and every landmark keeps one.  gbp_ba_retire keeps such a camera (it drops what is on its list, nothing else), every other
    shrinking call drops it with the other variables no staying factor names."""
    import dataclasses
    p = base_case().base
    keep = p.cam_idx != cam
    q = dataclasses.replace(p, meas=p.meas[keep], cam_idx=p.cam_idx[keep], lmk_idx=p.lmk_idx[keep])
    assert 0 < cam < p.n_cams - 1 and np.array_equal(np.unique(q.cam_idx), np.delete(np.arange(p.n_cams), cam))
    assert np.unique(q.lmk_idx).size == p.n_lmks and (q.cam_idx == 0).sum() < q.n_factors
    return q
