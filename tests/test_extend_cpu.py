"""CPU side of graph growth (gbp_ba_extend): the ABI struct and its binding, keyframe_batches, and the host oracle of growth
(tests/extend_host.py) against the reference's create order."""
import ctypes as ct
import os
import re

import numpy as np
import pytest

from conftest import REPO
from extend_host import make_numpy_ba, extend as host_extend


def _header_fields(struct):
    text = open(os.path.join(REPO, 'include', 'gbp_ba.h')).read()
    body = re.search(r'typedef struct %s \{(.*?)\} %s_t;' % (struct, struct), text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = []
    for decl in body.split(';'):
        decl = decl.strip()
        if decl:
            names += [re.sub(r'[*\s]', '', n.split()[-1] if ' ' in n.strip() else n) for n in decl.split(',')]
    return names


def test_ext_struct_matches_header_layout():
    from gbp_amd import _capi
    assert [f[0] for f in _capi.Ext._fields_] == _header_fields('gbp_ba_ext')
    # 4 int32, 5 pointers, 1 double, 2 pointers on LP64
    assert ct.sizeof(_capi.Ext) == 16 + 40 + 8 + 16
    assert _capi.Ext.cam_means.offset == 16 and _capi.Ext.lmk_idx.offset == 48
    assert _capi.Ext.prior_weaker_factor.offset == 56 and _capi.Ext.lmk_prior_lambda.offset == 72


def test_extend_symbol_is_bound():
    from gbp_amd import build, _capi
    build.build()
    assert 'gbp_ba_extend' in _capi.SIGNATURES
    assert hasattr(_capi.load(), 'gbp_ba_extend')


def _problem(**kw):
    from gbp_amd.synthetic import make_synthetic
    return make_synthetic(**dict(dict(n_cams=40, n_lmks=600, obs_per_lmk=4, window=8, seed=2), **kw))


@pytest.mark.parametrize('defer', [0.0, 0.2])
def test_keyframe_batches_rebuild_the_problem(defer):
    from gbp_amd.synthetic import keyframe_batches
    p = _problem()
    sp = keyframe_batches(p, [10, 10, 5, 15], defer=defer, seed=4)
    assert (sp.deferred > 0) == (defer > 0)
    parts = [dict(cam_means=sp.base.cam_means, lmk_means=sp.base.lmk_means, meas=sp.base.meas, cam_idx=sp.base.cam_idx,
                  lmk_idx=sp.base.lmk_idx)] + sp.batches
    C = L = 0
    seen = []
    for b in parts:
        C += b['cam_means'].shape[0]
        L += b['lmk_means'].shape[0]
        assert (b['cam_idx'] < C).all() and (b['lmk_idx'] < L).all()          # union numbering: only what exists by then
        seen.append(np.stack([b['cam_idx'], sp.lmk_order[b['lmk_idx']]], 1))
    assert (C, L) == (p.n_cams, p.n_lmks)
    np.testing.assert_array_equal(np.concatenate([b['cam_means'] for b in parts]), p.cam_means)
    np.testing.assert_array_equal(np.concatenate([b['lmk_means'] for b in parts]), p.lmk_means[sp.lmk_order])
    got = np.concatenate(seen)
    z = np.concatenate([b['meas'] for b in parts])
    key = lambda ids, m: np.lexsort((m[:, 1], m[:, 0], ids[:, 1], ids[:, 0]))
    want = np.stack([p.cam_idx, p.lmk_idx], 1)
    i, j = key(got, z), key(want, p.meas)
    np.testing.assert_array_equal(got[i], want[j])
    np.testing.assert_array_equal(z[i], p.meas[j])
    # each landmark joins with the first camera that observes it
    first_cam = np.full(p.n_lmks, 1 << 30)
    np.minimum.at(first_cam, p.lmk_idx, p.cam_idx)
    bounds = np.cumsum([0, 10, 10, 5, 15])
    lmk_part = np.concatenate([np.full(b['lmk_means'].shape[0], k) for k, b in enumerate(parts)])
    np.testing.assert_array_equal(lmk_part, np.searchsorted(bounds, first_cam[sp.lmk_order], side='right') - 1)


def test_deferred_observations_shift_old_ids_by_the_stated_formula():
    from gbp_amd.synthetic import keyframe_batches
    sp = keyframe_batches(_problem(), [12, 12, 16], defer=0.25, seed=1)
    cam = np.sort(sp.base.cam_idx, kind='stable')                          # reference order: camera-major
    for b in sp.batches:
        union = np.concatenate([cam, b['cam_idx']])
        order = np.argsort(union, kind='stable')
        pos = np.empty_like(order)
        pos[order] = np.arange(order.size)
        old_to_new = pos[:cam.size]
        formula = np.arange(cam.size) + np.array([(b['cam_idx'] < c).sum() for c in cam])
        np.testing.assert_array_equal(old_to_new, formula)
        assert (old_to_new != np.arange(cam.size)).any() or not (b['cam_idx'] < cam.max()).any()
        cam = union[order]


def test_host_growth_equals_the_union_built_at_once():
    """Growing the reference's object graph by a batch with no sweep in between gives the graph create_ba_graph builds from the
    union (same factor order, linearisation points and beliefs up to rounding: an old variable's mean is its belief mean), once the old variables' priors are the same."""
    from gbp_amd.synthetic import keyframe_batches, BAProblem
    from oracle.numpy_ba import NumpyBA
    p = _problem(n_cams=14, n_lmks=200, window=6)
    sp = keyframe_batches(p, [8, 6], defer=0.2, seed=3)
    nb = make_numpy_ba(sp.base)
    nb.generate_priors_var(50.0)
    nb.update_all_beliefs()
    b = sp.batches[0]
    o2n = host_extend(nb, b, prior_weaker_factor=50.0)
    cat = lambda k: np.concatenate([getattr(sp.base, k), b[k]])
    u = NumpyBA(BAProblem(K=p.K, cam_means=cat('cam_means'), lmk_means=cat('lmk_means'), meas=cat('meas'), cam_idx=cat('cam_idx'),
                          lmk_idx=cat('lmk_idx')))
    for v, w in zip(nb.graph.var_nodes, u.graph.var_nodes):
        w.prior.eta, w.prior.lam = v.prior.eta.copy(), v.prior.lam.copy()
    u.update_all_beliefs()
    assert len(u.graph.factors) == len(nb.graph.factors)
    for f, g in zip(nb.graph.factors, u.graph.factors):
        np.testing.assert_array_equal(f.measurement, g.measurement)
        np.testing.assert_allclose(f.linpoint, g.linpoint, rtol=1e-12, atol=1e-15)    # (old means: the belief's, not the initial ones)
    assert (o2n != np.arange(o2n.size)).any()
    for x, y in zip(nb.beliefs(), u.beliefs()):
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=1e-9)


@pytest.mark.parametrize('tag', ['small', 'vsmall_huber'])
def test_host_growth_replays_reference_fixture_g17(tag):
    """tests/extend_host.py grows the reference's object graph the way the reference's own classes grew it in make_g17.py: the whole
    G17 trajectory (extends with insertions, ba.py's schedule) agrees to ~1e-8 -- up to G17_HOLD on the non-robust run (extend_host.py)."""
    from conftest import golden
    from extend_host import HostGraph, g17_inputs, g17_replay, G17_HOLD
    g = golden(f'G17_grow_{tag}')
    base, _ = g17_inputs(g)
    worst = g17_replay(g, HostGraph(base, None if str(g['loss']) == 'None' else str(g['loss'])), belief_tol=1e-8, msg_tol=1e-8,
                       are_rtol=1e-8, energy_rtol=1e-8, hold=G17_HOLD[tag])
    assert worst < 1e-8
