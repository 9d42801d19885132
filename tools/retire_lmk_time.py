"""gbp_ba_retire_landmarks at the headline size, beside the calls it stands next to: on the 1M-factor, 2 000-camera sequence of
tools/retire_time.py (make_synthetic(window=30, n_cams=2000)) the landmarks whose highest camera is below 100 are retired.

Prints one JSON line, all times medians of RETIRE_REPS (5) calls in one session, each on a fresh live handle: the FOLD call, the DROP call
(the same work without the fold kernel: the difference is the fold), a device-input create of the FOLD call's survivors (the path it
replaces, which loses the state), and gbp_ba_retire of cameras 0..99 on the same graph."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from gbp_amd.engine import BAEngine
    from gbp_amd.synthetic import make_synthetic, BAProblem
    reps = int(os.environ.get('RETIRE_REPS', '5'))
    p = make_synthetic(n_cams=2000, window=30)
    hi = np.full(p.n_lmks, -1, np.int64)
    np.maximum.at(hi, p.lmk_idx, p.cam_idx)
    ids = np.flatnonzero((hi >= 0) & (hi < 100)).astype(np.int32)
    cams = np.arange(100, dtype=np.int32)

    def live():
        e = BAEngine.from_problem(p)
        e.generate_priors_var(50.0)
        e.update_all_beliefs()
        e.iterate(3)
        e.sync()
        return e

    def timed(call):
        e = live()
        t = time.perf_counter()
        maps = call(e)
        e.sync()
        return time.perf_counter() - t, e, maps

    t_fold, t_drop, t_cams, t_create = [], [], [], []
    sizes = gone = None
    for r in range(reps):
        if r == 0:
            e = live()
            fac, means = e.factors(dense=False), e.means()
            e.close()
        dt, e, (cm, lm, fm) = timed(lambda x: x.retire_landmarks(ids, fold=True))
        t_fold.append(dt)
        if r == 0:
            kf = fm >= 0
            s = BAProblem(K=p.K, cam_means=means[0][cm >= 0], lmk_means=means[1][lm >= 0], meas=fac['z'][kf],
                          cam_idx=cm[fac['cam'][kf]].astype(np.int32), lmk_idx=lm[fac['lmk'][kf]].astype(np.int32))
            dev = {k: torch.from_numpy(np.ascontiguousarray(getattr(s, k))).cuda() for k in ('cam_means', 'lmk_means', 'meas', 'cam_idx', 'lmk_idx')}
            torch.cuda.synchronize()
            sizes = (s.n_cams, s.n_lmks, s.n_factors)
            gone = dict(factors=int((~kf).sum()), cams=int((cm < 0).sum()), lmks=int((lm < 0).sum()),
                        cams_that_fold=int(np.unique(fac['cam'][~kf]).size), plan=e.plan_info())
        e.close()
        t = time.perf_counter()
        f = BAEngine(p.K, dev['cam_means'].data_ptr(), dev['lmk_means'].data_ptr(), dev['meas'].data_ptr(), dev['cam_idx'].data_ptr(),
                     dev['lmk_idx'].data_ptr(), device_pointers=sizes)
        f.sync()
        t_create.append(time.perf_counter() - t)
        f.close()
        dt, e, _ = timed(lambda x: x.retire_landmarks(ids, fold=False))
        t_drop.append(dt)
        e.close()
        dt, e, maps = timed(lambda x: x.retire(cams))
        t_cams.append(dt)
        if r == 0:
            gone_cams = dict(factors=int((maps[2] < 0).sum()), cams=int((maps[0] < 0).sum()), lmks=int((maps[1] < 0).sum()))
        e.close()
    med = lambda v: round(1e3 * float(np.median(v)), 3)
    allv = lambda v: [round(1e3 * x, 3) for x in v]
    print(json.dumps(dict(factors_before=int(p.n_factors), cams_before=int(p.n_cams), lmks_before=int(p.n_lmks), listed_lmks=int(ids.size),
                          gone=gone, survivors=dict(cams=sizes[0], lmks=sizes[1], factors=sizes[2]), gone_by_retire_of_100_cams=gone_cams,
                          retire_landmarks_fold_ms=med(t_fold), retire_landmarks_fold_ms_all=allv(t_fold),
                          retire_landmarks_drop_ms=med(t_drop), retire_landmarks_drop_ms_all=allv(t_drop),
                          fold_ms_by_difference=round(med(t_fold) - med(t_drop), 3),
                          create_survivors_ms_device_input=med(t_create), create_survivors_ms_all=allv(t_create),
                          retire_100_cams_ms=med(t_cams), retire_100_cams_ms_all=allv(t_cams))))


if __name__ == '__main__':
    main()
