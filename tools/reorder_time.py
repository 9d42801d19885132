"""GBP_FLAG_REORDER_LMKS (BAEngine(reorder_landmarks=True)) at size: sequences whose landmark ids are shuffled, swept with and without the
flag, beside the same sequence in generator order; and what the flag costs gbp_ba_create.

Prints one JSON line.  Per graph: the plans and microseconds per sweep (median of REORDER_REPS timed runs of REORDER_SWEEPS sweeps each,
the three handles alternated inside every repetition so that none runs on a warmer GPU, five warm-up sweeps before every run) with the
spread (min .. max) of the repetitions.  create: device-input create of the 1M-factor shuffled sequence with and without the flag, ms."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))


def main():
    import torch
    from gbp_amd.engine import BAEngine
    from gbp_amd.synthetic import make_synthetic
    from reorder_host import shuffle_landmarks
    reps = int(os.environ.get('REORDER_REPS', '5'))
    sweeps = int(os.environ.get('REORDER_SWEEPS', '200'))
    graphs = [('2000 cams, window 30', dict(n_cams=2000, n_lmks=100_000, window=30)),
              ('2000 cams, window 30, closures 0.02', dict(n_cams=2000, n_lmks=100_000, window=30, closures=0.02)),
              ('2000 cams, window 100, closures 0.02', dict(n_cams=2000, n_lmks=100_000, window=100, closures=0.02))]
    only = os.environ.get('REORDER_GRAPHS')
    if only:
        graphs = [graphs[int(k)] for k in only.split(',')]

    def live(problem, **kw):
        e = BAEngine.from_problem(problem, **kw)
        e.generate_priors_var(50.0)
        e.update_all_beliefs()
        e.iterate(3)
        e.sync()
        return e

    def us_per_sweep(e):
        e.iterate(5)
        e.sync()
        t = time.perf_counter()
        e.iterate(sweeps)
        e.sync()
        return 1e6 * (time.perf_counter() - t) / sweeps

    stat = lambda v: dict(median=round(float(np.median(v)), 2), min=round(float(min(v)), 2), max=round(float(max(v)), 2))
    out = dict(sweeps_per_run=sweeps, reps=reps, graphs=[])
    shuffled_1m = None
    for label, kw in graphs:
        p = make_synthetic(**kw)
        q, _ = shuffle_landmarks(p, seed=6)
        shuffled_1m = shuffled_1m or q
        handles = dict(generator_order=live(p), shuffled=live(q), shuffled_reordered=live(q, reorder_landmarks=True))
        times = {k: [] for k in handles}
        for _ in range(reps):
            for k, e in handles.items():
                times[k].append(us_per_sweep(e))
        row = dict(graph=label, factors=int(p.n_factors))
        for k, e in handles.items():
            pi = e.plan_info()
            row[k] = dict(us_per_sweep=stat(times[k]), fused=pi['fused'], max_window=pi['max_window'], table_rows=pi['table_rows'])
            e.close()
        row['speedup_over_shuffled'] = round(row['shuffled']['us_per_sweep']['median'] / row['shuffled_reordered']['us_per_sweep']['median'], 3)
        row['ratio_to_generator_order'] = round(row['shuffled_reordered']['us_per_sweep']['median'] / row['generator_order']['us_per_sweep']['median'], 3)
        out['graphs'].append(row)

    q = shuffled_1m
    dev = {k: torch.from_numpy(np.ascontiguousarray(getattr(q, k))).cuda() for k in ('cam_means', 'lmk_means', 'meas', 'cam_idx', 'lmk_idx')}
    torch.cuda.synchronize()
    create = {False: [], True: []}
    for r in range(reps + 1):                                  # the first pair warms the allocator and the code objects up
        for flag in (False, True):
            t = time.perf_counter()
            e = BAEngine(q.K, dev['cam_means'].data_ptr(), dev['lmk_means'].data_ptr(), dev['meas'].data_ptr(), dev['cam_idx'].data_ptr(),
                         dev['lmk_idx'].data_ptr(), device_pointers=(q.n_cams, q.n_lmks, q.n_factors), reorder_landmarks=flag)
            e.sync()
            if r:
                create[flag].append(1e3 * (time.perf_counter() - t))
            e.close()
    out['create_ms_device_input'] = dict(factors=int(q.n_factors), plain=stat(create[False]), reordered=stat(create[True]))
    print(json.dumps(out))


if __name__ == '__main__':
    main()
