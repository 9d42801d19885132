"""sha256 digests of what every graph-changing call of a live BA handle leaves, for comparing two builds of the library bit for bit
(GBP_HIP_LIB names the library, gbp_amd/_capi.py; run once per library, each in a fresh process, and compare the outputs).

Prints one JSON object per scenario (--out PATH: also written there, one per line): the maps the call returned, save_state() directly
after it and save_state() after three more sweeps.  The graph, the batch and the lists are tests/window_host.py's base_case(); the calls:
cull, retire, retire_landmarks (fold / drop), the full window_step, extend, and extend by tests/extend_cases.py's batches (extend_bare_new:
new variables no batch factor names, priors from scalars; extend_old_only: late factors of old cameras and no new variable); each on a
default handle (loss='huber', 6 sweeps), on a handle created with landmark reordering, and on one whose dense remainder is on
(num_undamped_iters=0, 9 sweeps); and retire([0]) and extend on bare_camera_problem(), where a camera has no factor.

Then the create-only scenarios of tests/build_cases.py, one per path of the graph build (gbp_capi_build.hip) the live calls' small graph
does not reach: create, priors, update_all_beliefs, three sweeps; save_state(), plan_info() and check_layout() are hashed, and `reached`
says whether the scenario still takes the path it is named for (read from plan_info()).  --create-only runs these alone."""
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]
W = 50.0


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    from gbp_amd import _capi
    from gbp_amd.engine import BAEngine
    from build_cases import build_scenarios, create
    from extend_cases import bare_new_batch, old_only_batch
    from window_host import bare_camera_problem, base_case
    c = base_case()
    five = lambda b: (b['cam_means'], b['lmk_means'], b['meas'], b['cam_idx'], b['lmk_idx'])
    bare_new, old_only = five(bare_new_batch(c.base)), five(old_only_batch(c.base))
    bt = (c.batch['cam_means'], c.batch['lmk_means'], c.batch['meas'], c.batch['cam_idx'], c.batch['lmk_idx'])
    calls = {
        'cull': lambda e: e.cull(c.cull),
        'retire': lambda e: e.retire(c.retire),
        'retire_landmarks_fold': lambda e: e.retire_landmarks(c.lmks),
        'retire_landmarks_drop': lambda e: e.retire_landmarks(c.lmks, fold=False),
        'window_step': lambda e: e.window_step(cull=c.cull, retire=c.retire, retire_landmarks=c.lmks, batch=bt, prior_weaker_factor=W),
        'extend': lambda e: (e.extend(*bt, prior_weaker_factor=W),),
        'extend_bare_new': lambda e: (e.extend(*bare_new, cam_prior_lambda=[2.0, 5.0], lmk_prior_lambda=[1.0, 1.5, 3.0]),),
        'extend_old_only': lambda e: (e.extend(*old_only, prior_weaker_factor=W),),
    }
    handles = {'default': (dict(loss='huber'), 6), 'reordered': (dict(loss='huber', reorder_landmarks=True), 6),
               'dense_remainder': (dict(num_undamped_iters=0), 9)}

    def live(problem, kw, sweeps, bare=None):
        e = BAEngine.from_problem(problem, **kw)
        e.generate_priors_var(W)
        if bare is not None:                                    # the prior rule leaves a camera without a factor at Lambda = 0
            pr = e.priors()
            lam = pr[1][:, 0, 0].max()
            pr[1][bare], pr[0][bare] = lam * np.eye(6), lam * problem.cam_means[bare]
            e.set_priors(*pr)
        e.update_all_beliefs()
        e.iterate(sweeps)
        return e

    def record(name, e, call):
        maps = call(e)
        rec = dict(scenario=name, sizes=[e.C, e.L, e.F], maps=[sha(m) for m in maps], state=sha(e.save_state()))
        e.iterate(3)
        rec['state_after_3_sweeps'] = sha(e.save_state())
        e.close()
        return json.dumps(rec)

    def created(name, s):
        e = create(s)
        e.iterate(3)
        pi = e.plan_info()
        rec = dict(scenario='create/' + name, sizes=[e.C, e.L, e.F], reached=bool(s.reached(pi)), plan_info=pi, bad_slots=e.check_layout(),
                   state_after_3_sweeps=sha(e.save_state()))
        e.close()
        return json.dumps(rec)

    lines = [json.dumps(dict(library=os.path.basename(os.path.dirname(os.path.abspath(_capi.LIB_PATH))) + '/' + os.path.basename(_capi.LIB_PATH)))]
    if '--create-only' not in sys.argv:
        for hname, (kw, sweeps) in handles.items():
            for cname, call in calls.items():
                lines.append(record(f'{hname}/{cname}', live(c.base, kw, sweeps), call))
        lines.append(record('bare_camera/retire', live(bare_camera_problem(), dict(loss='huber'), 6, bare=8), lambda e: e.retire([0])))
        lines.append(record('bare_camera/extend', live(bare_camera_problem(), dict(loss='huber'), 6, bare=8), calls['extend']))
    for name, s in build_scenarios().items():
        lines.append(created(name, s))
    print('\n'.join(lines))
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
