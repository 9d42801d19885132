"""gbp_ba_extend at the headline size: one keyframe appended to a 1M-factor sequence (make_synthetic(window=30, n_cams=2000)).

Prints one JSON line (--out PATH: also written there): the extend call's wall time (medians of EXTEND_REPS (5) runs with min - max, for a
device-input and a host-input batch, each on a fresh live handle) against a device-input create of the union (what rebuilding the
handle costs without the state), and the sweep rate right after extend against a fresh handle of the union (same plan: same speed
expected).  GBP_HIP_LIB (gbp_amd/_capi.py) names another build of the library to time beside this one.
Run the transplant alone under `rocprofv3 --kernel-trace --stats -- python tools/extend_time.py` for its kernel time."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    from gbp_amd.engine import BAEngine
    from gbp_amd.synthetic import make_synthetic, keyframe_batches
    reps = int(os.environ.get('EXTEND_REPS', '5'))
    sweeps = int(os.environ.get('EXTEND_SWEEPS', '200'))
    p = make_synthetic(n_cams=2000, window=30)
    sp = keyframe_batches(p, [1999, 1])
    b = sp.batches[0]
    cat = lambda k: np.concatenate([getattr(sp.base, k), b[k]])
    u = {k: cat(k) for k in ('cam_means', 'lmk_means', 'meas', 'cam_idx', 'lmk_idx')}
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in u.items()}
    bdev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in b.items()}
    torch.cuda.synchronize()
    sizes = (u['cam_means'].shape[0], u['lmk_means'].shape[0], u['meas'].shape[0])
    bsizes = (b['cam_means'].shape[0], b['lmk_means'].shape[0], b['meas'].shape[0])

    def create_union():
        e = BAEngine(p.K, dev['cam_means'].data_ptr(), dev['lmk_means'].data_ptr(), dev['meas'].data_ptr(), dev['cam_idx'].data_ptr(),
                     dev['lmk_idx'].data_ptr(), device_pointers=sizes)
        e.sync()
        return e

    def sweep_rate(e):
        e.iterate(5)
        e.sync()
        t = time.perf_counter()
        e.iterate(sweeps)
        e.sync()
        return sweeps / (time.perf_counter() - t)

    t_ext, t_host, t_create = [], [], []
    for _ in range(reps):
        e = BAEngine.from_problem(sp.base)
        e.generate_priors_var(50.0)
        e.update_all_beliefs()
        e.iterate(3)
        e.sync()
        t = time.perf_counter()
        e.extend(bdev['cam_means'].data_ptr(), bdev['lmk_means'].data_ptr(), bdev['meas'].data_ptr(), bdev['cam_idx'].data_ptr(),
                 bdev['lmk_idx'].data_ptr(), device_pointers=bsizes)
        e.sync()
        t_ext.append(time.perf_counter() - t)
        e.close()
        e = BAEngine.from_problem(sp.base)
        e.generate_priors_var(50.0)
        e.update_all_beliefs()
        e.iterate(3)
        e.sync()
        t = time.perf_counter()
        e.extend(b['cam_means'], b['lmk_means'], b['meas'], b['cam_idx'], b['lmk_idx'])
        e.sync()
        t_host.append(time.perf_counter() - t)
        if _ == reps - 1:
            grown = e
        else:
            e.close()
        t = time.perf_counter()
        f = create_union()
        t_create.append(time.perf_counter() - t)
        if _ != reps - 1:
            f.close()
    f.load_state(grown.save_state())          # the same state: both handles run the same sweeps (relinearisation waves included)
    rates = [(sweep_rate(grown), sweep_rate(f)) for _ in range(3)]          # alternated: neither handle runs on a warmer GPU
    rate_grown, rate_fresh = (float(np.median([r[k] for r in rates])) for k in (0, 1))
    spread = lambda v: dict(min=round(1e3 * min(v), 3), max=round(1e3 * max(v), 3), all=[round(1e3 * x, 3) for x in v])
    line = json.dumps(dict(factors=sizes[2], cams=sizes[0], new_factors=bsizes[2], plan_grown=grown.plan_info(), plan_fresh=f.plan_info(),
                           extend_ms_device_input=1e3 * float(np.median(t_ext)), extend_ms_host_input=1e3 * float(np.median(t_host)),
                           extend_ms_device_input_spread=spread(t_ext), extend_ms_host_input_spread=spread(t_host),
                           create_union_ms_device_input=1e3 * float(np.median(t_create)),
                           sweeps_per_s_after_extend=rate_grown, sweeps_per_s_fresh_union=rate_fresh,
                           # k_transplant_slots per old factor: 22 doubles of lin + msg read and written, the 16-byte row pair of the new
                           # meta | state word read, cpos / ref_file / cadj / old_to_new (divide by its rocprofv3 kernel time)
                           transplant_bytes=int(sp.base.n_factors) * (2 * 22 * 8 + 16 + 16)))
    print(line)
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as out:
            out.write(line + '\n')


if __name__ == '__main__':
    main()
