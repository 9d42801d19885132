"""gbp_ba_retire at the headline size: the oldest 5 % of the cameras of a 1M-factor, 2 000-camera sequence (make_synthetic(window=30,
n_cams=2000)) are retired.

Prints one JSON line: the retire call's wall time against a device-input create of the survivors' problem (the path it replaces: what
rebuilding the handle costs WITHOUT the state) and against that create plus one state load, and the sweep rate before the call, right
after it and on a fresh handle of the survivors with the same state (same plan: same speed expected)."""
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
    sweeps = int(os.environ.get('RETIRE_SWEEPS', '200'))
    p = make_synthetic(n_cams=2000, window=30)
    gone = np.arange(p.n_cams // 20, dtype=np.int32)

    def sweep_rate(e):
        e.iterate(5)
        e.sync()
        t = time.perf_counter()
        e.iterate(sweeps)
        e.sync()
        return sweeps / (time.perf_counter() - t)

    def live():
        e = BAEngine.from_problem(p)
        e.generate_priors_var(50.0)
        e.update_all_beliefs()
        e.iterate(3)
        e.sync()
        return e

    t_ret, t_create, t_load = [], [], []
    rate_before = None
    for r in range(reps):
        e = live()
        if r == 0:
            rate_before = sweep_rate(e)
            fac, means = e.factors(dense=False), e.means()
        t = time.perf_counter()
        cm, lm, fm = e.retire(gone)
        e.sync()
        t_ret.append(time.perf_counter() - t)
        if r == 0:
            kf = fm >= 0
            s = BAProblem(K=p.K, cam_means=means[0][cm >= 0], lmk_means=means[1][lm >= 0], meas=fac['z'][kf],
                          cam_idx=cm[fac['cam'][kf]].astype(np.int32), lmk_idx=lm[fac['lmk'][kf]].astype(np.int32))
            dev = {k: torch.from_numpy(np.ascontiguousarray(getattr(s, k))).cuda() for k in ('cam_means', 'lmk_means', 'meas', 'cam_idx', 'lmk_idx')}
            torch.cuda.synchronize()
            sizes = (s.n_cams, s.n_lmks, s.n_factors)
        blob = e.save_state()
        t = time.perf_counter()
        f = BAEngine(p.K, dev['cam_means'].data_ptr(), dev['lmk_means'].data_ptr(), dev['meas'].data_ptr(), dev['cam_idx'].data_ptr(),
                     dev['lmk_idx'].data_ptr(), device_pointers=sizes)
        f.sync()
        t_create.append(time.perf_counter() - t)
        t = time.perf_counter()
        f.load_state(blob)
        f.sync()
        t_load.append(time.perf_counter() - t)
        if r == reps - 1:
            shrunk, fresh = e, f
        else:
            e.close()
            f.close()
    rates = [(sweep_rate(shrunk), sweep_rate(fresh)) for _ in range(3)]          # alternated: neither handle runs on a warmer GPU
    rate_shrunk, rate_fresh = (float(np.median([x[k] for x in rates])) for k in (0, 1))
    med = lambda v: 1e3 * float(np.median(v))
    print(json.dumps(dict(factors_before=int(p.n_factors), cams_before=int(p.n_cams), retired_cams=int(gone.size), factors_after=sizes[2],
                          lmks_before=int(p.n_lmks), lmks_after=sizes[1], plan_shrunk=shrunk.plan_info(), plan_fresh=fresh.plan_info(),
                          retire_ms=med(t_ret), retire_ms_all=[round(1e3 * x, 3) for x in t_ret],
                          create_survivors_ms_device_input=med(t_create), load_state_ms_host_blob=med(t_load),
                          sweeps_per_s_before=rate_before, sweeps_per_s_after_retire=rate_shrunk, sweeps_per_s_fresh_survivors=rate_fresh)))


if __name__ == '__main__':
    main()
