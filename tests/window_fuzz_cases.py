"""Random window schedules for a live BA handle: the shared generator of tests/test_window_fuzz_cpu.py and tests/test_window_fuzz_gpu.py.

random_schedule(seed) draws a base graph and five window steps (a keyframe batch, a cull list, a camera list, a landmark list, a fold
flag, and whether the step is ONE gbp_ba_window_step or the four calls it stands for) from np.random.default_rng(seed).  A step's lists
are legal only for the graph the steps before it left, so the generator follows the graph itself -- as index arrays, by the rules of
include/gbp_ba.h (index_step below: which factor leaves, which variable survives, how the survivors are numbered).  The maps it predicts
are written from those rules directly, not composed from four calls: a second derivation beside tests/window_host.py's.  healthy() is
the health rule of tests/test_fuzz_gpu.py on the host graph alone; tally() says which of the shapes the hand-built cases single out a run
has met.  Host-only: numpy, nothing of the device."""
import collections

import numpy as np

from window_host import WindowMaps, filter_batch

N_STEPS = 5
# Default seeds: chosen so that (tests/test_window_fuzz_cpu.py proves each on the host model alone) every shape of SHAPES occurs, a camera
# folds more than 64 messages at least twice, every seed is healthy through its first step and at least 75 % of all steps are healthy.
SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15)
SHAPES = ('late_observations', 'batch_without_cameras', 'empty_cull', 'empty_retire', 'empty_landmarks', 'orphaned_camera',
          'saved_landmark', 'fold_above_64', 'retired_camera_and_listed_landmark', 'culled_factor_of_retired_camera', 'no_fold',
          'how_step', 'how_calls')
REFUSALS = ('repeated cull id', 'batch names a retired camera', 'landmark id equal to L', 'no factor left')

Step = collections.namedtuple('Step', 'sweeps batch cull retire lmks fold how pushes')
Graph = collections.namedtuple('Graph', 'C L cam lmk')            # sizes and the factors' (camera, landmark) in reference order
Schedule = collections.namedtuple('Schedule', 'seed base steps graphs maps refuse settings')


def _i32(a):
    return np.asarray(a, np.int64).reshape(-1).astype(np.int32)


def _renumber(keep):
    keep = np.asarray(keep, bool)
    return np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int64)


# ---- the header's rules on index arrays ------------------------------------------------------------------------------------------------
def index_step(g, step):
    """One window step on Graph g by rules b - d of gbp_ba_window_step (include/gbp_ba.h).  Returns (WindowMaps, Graph after the step)."""
    bt = step.batch
    dC, dL = len(bt['cam_means']), len(bt['lmk_means'])
    bc, bl = np.asarray(bt['cam_idx'], np.int64), np.asarray(bt['lmk_idx'], np.int64)
    F, dF = g.cam.size, bc.size
    if not (dC or dL or dF or len(step.cull) or len(step.retire) or len(step.lmks)):
        ident = lambda n: np.arange(n, dtype=np.int32)
        return WindowMaps(ident(g.C), ident(g.L), ident(F), ident(0), ident(0), ident(0)), g
    goes = np.isin(g.cam, step.retire) | np.isin(g.lmk, step.lmks)              # c. why an old factor leaves
    goes[np.asarray(step.cull, np.int64)] = True
    cam_u, lmk_u = np.concatenate([g.cam, bc]), np.concatenate([g.lmk, bl])
    stays = np.concatenate([~goes, np.ones(dF, bool)])                           # a batch factor never leaves
    keep_c = np.bincount(cam_u[stays], minlength=g.C + dC) > 0                    # b. a variable survives with a surviving factor
    keep_l = np.bincount(lmk_u[stays], minlength=g.L + dL) > 0
    assert not keep_c[np.asarray(step.retire, np.int64)].any() and not keep_l[np.asarray(step.lmks, np.int64)].any()
    cm, lm = _renumber(keep_c), _renumber(keep_l)
    kept = np.flatnonzero(stays)                                                 # old survivors in old order, then the batch
    order = kept[np.argsort(cm[cam_u[kept]], kind='stable')]                      # d. camera-major, old before new inside a camera
    fm = np.full(F + dF, -1, np.int64)
    fm[order] = np.arange(order.size)
    maps = WindowMaps(*(a.astype(np.int32) for a in (cm[:g.C], lm[:g.L], fm[:F], cm[g.C:], lm[g.L:], fm[F:])))
    return maps, Graph(int(keep_c.sum()), int(keep_l.sum()), cm[cam_u[order]].astype(np.int32), lm[lmk_u[order]].astype(np.int32))


def is_legal(g, step):
    """The header's rules for the arguments of one step, from the arrays alone: ids in range and distinct, a batch in the union numbering
    that names no retired camera and no listed landmark, at least one factor left.  Returns the first rule broken, or None."""
    bt = step.batch
    dC, dL = len(bt['cam_means']), len(bt['lmk_means'])
    for name, ids, n in (('cull', step.cull, g.cam.size), ('retire', step.retire, g.C), ('landmarks', step.lmks, g.L)):
        ids = np.asarray(ids, np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= n):
            return name + ': id out of range'
        if np.unique(ids).size != ids.size:
            return name + ': id repeated'
    bc, bl = np.asarray(bt['cam_idx'], np.int64), np.asarray(bt['lmk_idx'], np.int64)
    if not (bc.size == bl.size == len(bt['meas'])):
        return 'batch: lengths differ'
    if bc.size and (bc.min() < 0 or bc.max() >= g.C + dC or bl.min() < 0 or bl.max() >= g.L + dL):
        return 'batch: id beyond the union'
    if np.isin(bc, step.retire).any() or np.isin(bl, step.lmks).any():
        return 'batch: names a retired camera or a listed landmark'
    goes = np.isin(g.cam, step.retire) | np.isin(g.lmk, step.lmks)
    goes[np.asarray(step.cull, np.int64)] = True
    if bc.size + int((~goes).sum()) == 0:
        return 'no factor left'
    return None


# ---- carrying the ids of a split's batches through a window that also shrinks ----------------------------------------------------------
def carry_batch(raw, cam_now, lmk_now, C, L):
    """A batch of gbp_amd.synthetic.keyframe_batches (ids in the numbering of the GROWING graph) in the union numbering of the graph as it
    is now.  cam_now / lmk_now: split id -> current id, -1 for what has gone; the observations that name something gone are left out.
    Returns (batch, cam_u, lmk_u), the last two being cam_now / lmk_now extended by the batch's own variables (for carry_ids)."""
    dC, dL = len(raw['cam_means']), len(raw['lmk_means'])
    cam_u, lmk_u = np.concatenate([cam_now, C + np.arange(dC)]), np.concatenate([lmk_now, L + np.arange(dL)])
    ci, li = cam_u[raw['cam_idx']], lmk_u[raw['lmk_idx']]
    alive = (ci >= 0) & (li >= 0)
    return dict(raw, meas=raw['meas'][alive], cam_idx=ci[alive].astype(np.int32), lmk_idx=li[alive].astype(np.int32)), cam_u, lmk_u


def carry_ids(cam_u, lmk_u, maps):
    """cam_now / lmk_now after the step whose maps are `maps` (cam_u / lmk_u from carry_batch)."""
    full_c, full_l = np.concatenate([maps.cam_map, maps.new_cam_ids]), np.concatenate([maps.lmk_map, maps.new_lmk_ids])
    return np.where(cam_u >= 0, full_c[np.maximum(cam_u, 0)], -1), np.where(lmk_u >= 0, full_l[np.maximum(lmk_u, 0)], -1)


# ---- drawing ---------------------------------------------------------------------------------------------------------------------------
def _draw_base(rng):
    """(split, sizes): the graph of one schedule, or None when a base variable has no factor (the host graph is singular then)."""
    from gbp_amd.synthetic import make_synthetic, keyframe_batches
    sizes = [int(rng.integers(6, 13))] + [int(rng.integers(0, 4)) for _ in range(N_STEPS)]
    obs = int(rng.integers(3, 7))
    p = make_synthetic(n_cams=sum(sizes) + 1, n_lmks=int(rng.integers(60, 201)), obs_per_lmk=obs, window=obs + int(rng.integers(1, 5)),
                       seed=int(rng.integers(1 << 30)))
    split = keyframe_batches(p, sizes, defer=float(rng.choice([0.0, 0.3, 0.6])), seed=int(rng.integers(1 << 30)))
    b = split.base
    if b.n_factors == 0 or np.unique(b.cam_idx).size != b.n_cams or np.unique(b.lmk_idx).size != b.n_lmks:
        return None
    return split


def draw_step(rng, g, bt0):
    """One step for Graph g (the CURRENT graph: legality depends on it) and the carried batch bt0, or None when the draw cannot be made
    legal.  With probability 0.25 each the step is pushed towards an orphaned camera, a saved landmark, a camera fold of more than one
    chunk, and a cull that takes a camera's factors but one."""
    C, L, cam, lmk = g
    F = cam.size
    bc, bl = np.asarray(bt0['cam_idx'], np.int64), np.asarray(bt0['lmk_idx'], np.int64)
    sweeps, fold, how = int(rng.integers(1, 5)), bool(rng.random() < 0.7), ('step', 'calls')[int(rng.integers(2))]
    want = [name for name in ('orphan', 'saved', 'wide', 'heavy') if rng.random() < 0.25]
    pushes = []
    # cameras
    n_ret = min(int(rng.integers(0, 3)), max(C - 3, 0))
    retire = rng.choice(C, size=n_ret, replace=False)
    keep_lmk = -1
    if 'saved' in want:                                          # retire the only old observers of a landmark the batch observes
        for l in rng.permutation(np.unique(bl[bl < L])):
            obs = np.unique(cam[lmk == l])
            if 0 < obs.size <= 2 and C - obs.size >= 3 and (~np.isin(bc[bl == l], obs)).any():
                retire, keep_lmk = obs, int(l)
                pushes.append('saved')
                break
    stay_c = np.setdiff1d(np.arange(C), retire)
    per_cam = np.bincount(cam, minlength=C)
    # landmarks
    lmks = set(int(l) for l in rng.choice(L, size=int(rng.integers(0, L // 8 + 1)), replace=False))
    if 'orphan' in want:                                         # every landmark of one staying camera, its late observations' too
        ok = [c for c in stay_c if per_cam[c] and (bl[bc == c] < L).all() and keep_lmk not in lmk[cam == c] and keep_lmk not in bl[bc == c]]
        if ok:
            c = min(ok, key=lambda k: (per_cam[k], k))
            lmks |= set(int(l) for l in lmk[cam == c]) | set(int(l) for l in bl[bc == c])
            pushes.append('orphan')
    if 'wide' in want:                                           # more than 64 factors of one staying camera: two chunks of its fold
        ok = [c for c in stay_c if np.setdiff1d(lmk[cam == c], [keep_lmk]).size >= 70]
        if ok:                                                   # (one landmark at least stays: the camera is not orphaned by this push)
            c = int(rng.choice(ok))
            mine = np.setdiff1d(lmk[cam == c], [keep_lmk])
            lmks |= set(int(l) for l in rng.choice(mine, size=int(rng.integers(69, mine.size)), replace=False))
            fold = True
            pushes.append('wide')
    lmks.discard(keep_lmk)
    lmks = np.array(sorted(lmks), np.int64)
    bt = filter_batch(bt0, retire, lmks)
    # factors
    cull = set(int(f) for f in rng.choice(F, size=int(rng.integers(0, F // 10 + 1)), replace=False))
    if 'heavy' in want:                                          # a whole camera's factors but one
        ok = [c for c in stay_c if per_cam[c] >= 2]
        if ok:
            c = int(rng.choice(ok))
            cull |= set(int(f) for f in np.flatnonzero(cam == c)[:-1])
            pushes.append('heavy')
    if keep_lmk >= 0:
        cull -= set(int(f) for f in np.flatnonzero(lmk == keep_lmk))
    step = Step(sweeps, bt, _i32(sorted(cull)), _i32(np.sort(retire)), _i32(lmks), fold, how, tuple(pushes))
    if is_legal(g, step) is not None:
        return None
    maps, after = index_step(g, step)
    # A new variable the batch gives no factor is where one step and the four calls part BY THE HEADER (the step drops it, gbp_ba_extend
    # followed by gbp_ba_retire alone keeps it), and a window of fewer than three cameras is no window: neither is drawn.
    if (maps.new_cam_ids < 0).any() or (maps.new_lmk_ids < 0).any() or after.C < 3 or after.cam.size < 20:
        return None
    return step


def random_schedule(seed):
    """Base problem, N_STEPS steps, the graphs before each step (and after the last) and the maps index_step predicts, all drawn from
    np.random.default_rng([seed, sub]) with the first sub-seed whose draw is legal throughout.  refuse = (position, kind) of the one
    refused step of the seed (REFUSALS); settings = how the GPU test creates the engines of this seed."""
    for sub in range(64):
        rng = np.random.default_rng([int(seed), sub])
        split = _draw_base(rng)
        if split is None:
            continue
        b = split.base
        order = np.argsort(b.cam_idx, kind='stable')
        g = Graph(b.n_cams, b.n_lmks, b.cam_idx[order].astype(np.int32), b.lmk_idx[order].astype(np.int32))
        cam_now, lmk_now = np.arange(g.C), np.arange(g.L)
        steps, graphs, maps = [], [g], []
        for raw in split.batches:
            bt0, cam_u, lmk_u = carry_batch(raw, cam_now, lmk_now, g.C, g.L)
            step = draw_step(rng, g, bt0)
            if step is None:
                break
            m, g = index_step(g, step)
            cam_now, lmk_now = carry_ids(cam_u, lmk_u, m)
            steps.append(step)
            graphs.append(g)
            maps.append(m)
        if len(steps) < N_STEPS:
            continue
        refuse = (int(rng.integers(N_STEPS)), int(rng.integers(len(REFUSALS))))
        settings = dict(loss=[None, 'huber', 'constant'][seed % 3], reorder_landmarks=bool(seed % 2),
                        env={2: {'GBP_PACK': 'dense'}, 3: {'GBP_WINDOWS': '1'}}.get(seed % 4, {}))
        return Schedule(int(seed), b, steps, graphs, maps, refuse, settings)
    raise ValueError(f'seed {seed}: no legal schedule in 64 draws')


def refused_variant(g, step, kind):
    """Arguments (batch, cull, retire, lmks) of a step the header refuses with GBP_EINVAL, made from a legal one: REFUSALS[kind].  A
    kind the step has no material for (no batch observation to misname) falls back to the landmark id equal to L."""
    bt, cull, retire, lmks = step.batch, step.cull, step.retire, step.lmks
    name = REFUSALS[kind]
    if name == 'batch names a retired camera' and len(bt['cam_idx']):
        old = int(retire[0]) if len(retire) else 0
        ci = np.array(bt['cam_idx'])
        ci[len(ci) // 2] = old
        return name, (dict(bt, cam_idx=ci), cull, retire if len(retire) else _i32([old]), lmks)
    if name == 'repeated cull id':
        return name, (bt, _i32(list(cull) + [int(cull[len(cull) // 2])] if len(cull) else [0, 0]), retire, lmks)
    if name == 'no factor left':
        return name, (None, _i32(np.arange(g.cam.size)), retire, lmks)
    return REFUSALS[2], (bt, cull, retire, _i32(list(lmks) + [g.L]))


# ---- health, on the host graph alone ---------------------------------------------------------------------------------------------------
def make_host(problem, loss, weaker=50.0):
    """The reference's object graph of `problem` with priors and beliefs, and the ARE healthy() measures against."""
    from extend_host import make_numpy_ba
    nb = make_numpy_ba(problem, loss=loss)
    nb.generate_priors_var(weaker)
    nb.update_all_beliefs()
    nb.are0 = nb.are()
    return nb


def healthy(nb):
    """tests/test_fuzz_gpu.py::healthy on a NumpyBA: the comparison of two float64 implementations means something only while every
    cavity (belief minus own message) is positive definite with a condition below 1e7, no landmark sits closer to a camera's focal plane
    than a depth ratio of 0.2, and the ARE is below 1e3 x the initial one (nb.are0, at least 1)."""
    from gbp_amd.synthetic import rodrigues
    fs = nb.graph.factors
    ec = np.linalg.eigvalsh(np.array([f.adj_var_nodes[0].belief.lam - f.messages[0].lam for f in fs]))
    el = np.linalg.eigvalsh(np.array([f.adj_var_nodes[1].belief.lam - f.messages[1].lam for f in fs]))
    if not (ec.min() > 0 and el.min() > 0 and (ec[:, -1] / ec[:, 0]).max() < 1e7 and (el[:, -1] / el[:, 0]).max() < 1e7):
        return False
    cm, lm = np.array([f.adj_var_nodes[0].mu for f in fs]), np.array([f.adj_var_nodes[1].mu for f in fs])
    pc = np.einsum('fij,fj->fi', rodrigues(cm[:, 3:]), lm) + cm[:, :3]
    if not (np.abs(pc[:, 2]) / np.linalg.norm(pc, axis=1)).min() > 0.2:
        return False
    return bool(nb.are() < 1e3 * max(nb.are0, 1.0))


# ---- which shapes a run has met ----------------------------------------------------------------------------------------------------------
def tally(schedule_run):
    """schedule_run: one (Graph before the step, Step, WindowMaps of the step) per step, from whoever ran them (the index model, the host
    graph, an engine).  Returns {shape: number of steps that show it}, from the index arrays alone."""
    out = dict.fromkeys(SHAPES, 0)
    for g, s, m in schedule_run:
        bc = np.asarray(s.batch['cam_idx'], np.int64)
        culled = np.zeros(g.cam.size, bool)
        culled[np.asarray(s.cull, np.int64)] = True
        ret_f, lst_f = np.isin(g.cam, s.retire), np.isin(g.lmk, s.lmks)
        out['late_observations'] += bool((bc < g.C).any())
        out['batch_without_cameras'] += len(s.batch['cam_means']) == 0
        out['empty_cull'] += len(s.cull) == 0
        out['empty_retire'] += len(s.retire) == 0
        out['empty_landmarks'] += len(s.lmks) == 0
        gone_c = np.asarray(m.cam_map) < 0
        gone_c[np.asarray(s.retire, np.int64)] = False
        out['orphaned_camera'] += bool(gone_c.any())
        n_old, n_ret = np.bincount(g.lmk, minlength=g.L), np.bincount(g.lmk[ret_f], minlength=g.L)
        out['saved_landmark'] += bool(((n_old > 0) & (n_old == n_ret) & (np.asarray(m.lmk_map) >= 0)).any())
        folded = np.bincount(g.cam[lst_f & ~ret_f & ~culled], minlength=g.C)
        out['fold_above_64'] += bool(s.fold and (folded[np.asarray(m.cam_map) >= 0] > 64).any())
        out['retired_camera_and_listed_landmark'] += bool((ret_f & lst_f).any())
        out['culled_factor_of_retired_camera'] += bool((culled & ret_f).any())
        out['no_fold'] += bool(not s.fold and len(s.lmks))
        out['how_step'] += s.how == 'step'
        out['how_calls'] += s.how == 'calls'
    return {k: int(v) for k, v in out.items()}


def parts_of(step):
    """How many of the four calls a step stands for change something: what rebuild_count goes up by when it is taken as calls."""
    bt = step.batch
    return int(bool(len(bt['cam_means']) or len(bt['lmk_means']) or len(bt['meas']))) + int(len(step.cull) > 0) + int(len(step.retire) > 0) \
        + int(len(step.lmks) > 0)
