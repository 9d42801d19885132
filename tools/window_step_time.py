"""gbp_ba_window_step at the headline size, beside the four calls it stands for: on the 1M-factor, 2 000-camera sequence of
tools/retire_time.py (make_synthetic(window=30, n_cams=2000)) cut by keyframe_batches into a base of 1 998 cameras and one batch of 2,
one realistic step of a fixed-lag front end: append the 2 keyframes, cull the 0.1 % of the factors with the largest residual, retire the
2 oldest cameras, let go of the landmarks whose highest camera is below 50.

Prints one JSON line and writes it to profiles/window_step_time.json (--out PATH: elsewhere): medians of WINDOW_REPS (5) runs with
min - max, all in one process, each run on a fresh live handle in the same state -- the step as ONE window_step, and as extend, cull,
retire, retire_landmarks with the ids carried through the maps (the time of the four calls alone, each call's own median with min - max,
and with the id translation a front end then has to do on the host).  GBP_HIP_LIB (gbp_amd/_capi.py) names another build of the library
to time beside this one."""
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    from gbp_amd.engine import BAEngine
    from gbp_amd.synthetic import make_synthetic, keyframe_batches
    out = sys.argv[sys.argv.index('--out') + 1] if '--out' in sys.argv else os.path.join(REPO, 'profiles', 'window_step_time.json')
    reps = int(os.environ.get('WINDOW_REPS', '5'))
    n_cams = int(os.environ.get('WINDOW_CAMS', '2000'))
    kw = dict(n_cams=n_cams, window=30) if n_cams == 2000 else dict(n_cams=n_cams, window=30, n_lmks=50 * n_cams, obs_per_lmk=10)
    split = keyframe_batches(make_synthetic(**kw), [n_cams - 2, 2])
    p, bt = split.base, split.batches[0]
    retire = np.array([0, 1], np.int32)
    hi = np.full(p.n_lmks, -1, np.int64)
    np.maximum.at(hi, p.lmk_idx, p.cam_idx)
    np.maximum.at(hi, bt['lmk_idx'][bt['lmk_idx'] < p.n_lmks], bt['cam_idx'][bt['lmk_idx'] < p.n_lmks])
    lmks = np.flatnonzero((hi >= 0) & (hi < 50)).astype(np.int32)
    ok = ~np.isin(bt['cam_idx'], retire) & ~np.isin(bt['lmk_idx'], lmks)
    batch = (bt['cam_means'], bt['lmk_means'], bt['meas'][ok], bt['cam_idx'][ok], bt['lmk_idx'][ok])

    def live():
        e = BAEngine.from_problem(p)
        e.generate_priors_var(50.0)
        e.update_all_beliefs()
        e.iterate(3)
        e.sync()
        return e

    e = live()
    worst = np.argsort(e.residuals()[1])[-max(1, p.n_factors // 1000):].astype(np.int32)
    cull = np.sort(worst)
    e.close()

    def alive(ids, m):
        t = m[ids]
        return t[t >= 0]

    t_one, t_four, t_four_calls, parts = [], [], [], []
    sizes = counts = None
    for r in range(reps):
        e = live()
        n0 = e.rebuild_count()
        t = time.perf_counter()
        m = e.window_step(cull=cull, retire=retire, retire_landmarks=lmks, batch=batch)
        e.sync()
        t_one.append(time.perf_counter() - t)
        if r == 0:
            sizes = dict(cams=e.C, lmks=e.L, factors=e.F)
            counts = dict(rebuilds_window_step=e.rebuild_count() - n0, culled=int(cull.size), retired_cams=int(retire.size), listed_lmks=int(lmks.size),
                          new_cams=int(len(batch[0])), new_lmks=int(len(batch[1])), new_factors=int(len(batch[2])),
                          late_factors_of_old_cams=int((batch[3] < p.n_cams).sum()), factors_gone=int((m.factor_map < 0).sum()),
                          cams_gone=int((m.cam_map < 0).sum()), lmks_gone=int((m.lmk_map < 0).sum()), plan=e.plan_info())
        e.close()
        e = live()
        n0 = e.rebuild_count()
        t = time.perf_counter()
        in_calls, each = 0.0, []

        def call(fn, *a, **k):
            nonlocal in_calls
            t0 = time.perf_counter()
            res = fn(*a, **k)
            e.sync()
            each.append(time.perf_counter() - t0)
            in_calls += each[-1]
            return res
        o2n = call(e.extend, *batch)
        cm, lm, fm = call(e.cull, o2n[cull])
        cm2, lm2, fm2 = call(e.retire, alive(retire, cm))
        lm_now = np.where(lm[:p.n_lmks] >= 0, lm2[np.maximum(lm[:p.n_lmks], 0)], -1)
        call(e.retire_landmarks, alive(lmks, lm_now).astype(np.int32))
        t_four.append(time.perf_counter() - t)
        t_four_calls.append(in_calls)
        parts.append(each)
        if r == 0:
            counts['rebuilds_four_calls'] = e.rebuild_count() - n0
            assert (e.C, e.L, e.F) == (sizes['cams'], sizes['lmks'], sizes['factors'])
        e.close()
    ms = lambda v: dict(median=round(1e3 * float(np.median(v)), 3), min=round(1e3 * min(v), 3), max=round(1e3 * max(v), 3),
                        all=[round(1e3 * x, 3) for x in v])
    res = dict(before=dict(cams=int(p.n_cams), lmks=int(p.n_lmks), factors=int(p.n_factors)), after=sizes, step=counts, reps=reps,
               window_step_ms=ms(t_one), four_calls_ms=ms(t_four_calls), four_calls_with_id_translation_ms=ms(t_four),
               four_calls_each_ms=dict(zip(('extend', 'cull', 'retire', 'retire_landmarks'),
                                           [ms(c) for c in zip(*parts)])))
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
