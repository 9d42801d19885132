"""The graph build (gbp_capi_build.hip) under GBP_DEBUG_LAYOUT: besides decoding the layout, build_graph then refuses a graph of which
an array of build_arena_table or an upload of the fused plan was placed outside the arena (gbp_build_plan.hpp) -- without the override
such an array silently gets an allocation of its own and the sweep's working set leaves the one block.  The overrides are read at
create, so a fresh child process runs with the variable set: create on every scenario of tests/build_cases.py (one per path of the
build), and the full window step of tests/window_host.py's base_case(), whose rebuild runs the same check."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

CHILD = r'''
import json, sys
sys.path[:0] = [%r, %r]
import numpy as np
from build_cases import build_scenarios, create
from window_host import base_case
from gbp_amd.engine import BAEngine
out = {}
for name, s in build_scenarios().items():
    e = create(s)
    e.iterate(2)
    pi = e.plan_info()
    out[name] = dict(reached=bool(s.reached(pi)), bad_slots=e.check_layout(), finite=bool(all(np.isfinite(b).all() for b in e.beliefs())), plan_info=pi)
    e.close()
c = base_case()
e = BAEngine.from_problem(c.base, loss='huber')
e.generate_priors_var(50.0); e.update_all_beliefs(); e.iterate(4)
bt = (c.batch['cam_means'], c.batch['lmk_means'], c.batch['meas'], c.batch['cam_idx'], c.batch['lmk_idx'])
r = e.window_step(cull=c.cull, retire=c.retire, retire_landmarks=c.lmks, batch=bt, prior_weaker_factor=50.0)
e.iterate(2)
out['window_step'] = dict(sizes=[e.C, e.L, e.F], bad_slots=e.check_layout(), fused=e.plan_info()['fused'],
                          finite=bool(all(np.isfinite(b).all() for b in e.beliefs())))
e.close()
print('RESULT ' + json.dumps(out))
''' % (REPO, HERE)


@pytest.fixture(scope='module')
def child():
    env = dict(os.environ, GBP_DEBUG_LAYOUT='1', PYTHONDONTWRITEBYTECODE='1')
    r = subprocess.run([sys.executable, '-c', CHILD], cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('RESULT ')]
    assert line, r.stdout[-2000:]
    return json.loads(line[-1][len('RESULT '):])


def test_create_places_everything_in_the_arena_on_every_path(child):
    from build_cases import build_scenarios
    names = list(build_scenarios())
    assert len(names) == 10 and all(n in child for n in names)
    for n in names:
        assert child[n]['reached'], (n, child[n]['plan_info'])          # the scenario still takes the path it is named for
        assert child[n]['bad_slots'] == 0 and child[n]['finite'], (n, child[n])


def test_window_step_rebuild_places_everything_in_the_arena(child):
    w = child['window_step']
    assert w['bad_slots'] == 0 and w['finite'] and w['fused'], w
    assert w['sizes'] != [16, 149, 430] and min(w['sizes']) > 0, w     # the step really changed base_case()'s graph
