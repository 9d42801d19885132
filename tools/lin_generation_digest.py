"""sha256 digests of what every rebuild of a live linear handle leaves, for comparing two builds of the library bit for bit (GBP_HIP_LIB
names the library, gbp_amd/_capi.py; run once per library, each in a fresh process, and compare the outputs line for line).

Plays the schedules of tests/lin_generation_cases.py -- plain with factor_const, robust, losses set and cleared, plain with F over 256
and back, SE(2) nonlinear: create, 3 sweeps, extend, 3 sweeps, shrink, 3 sweeps, extend, shrink -- and prints one JSON object per step
(--out PATH: also written there, one per line): the sizes, the number of device allocations, the maps a shrink returned, and a digest of
the raw bytes of every getter of the kind (messages, beliefs, means, energy; weights where losses are set; linearisation on SE(2))."""
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'tests')]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    from lin_generation_cases import KINDS, Player, engine_of, schedule
    lines = []

    def record(kind, p, what, maps=()):
        lines.append(json.dumps(dict(kind=kind, step=what, sizes=list(p.e.sizes()), allocs=p.e.alloc_count(), maps=[sha(m) for m in maps],
                                     state=[sha(a) for a in p.observables()])))

    for kind in KINDS:
        start, steps = schedule(kind)
        model = start()
        p = Player(kind, engine_of(model, kind))                # the engine alone: the model only supplies the starting graph
        record(kind, p, 'create')
        for i, step in enumerate(steps):
            record(kind, p, f'{i}:{step[0]}', p.play(step) or ())
        p.e.close()
    print('\n'.join(lines))
    if '--out' in sys.argv:
        with open(sys.argv[sys.argv.index('--out') + 1], 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
