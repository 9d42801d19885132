"""Landmark reordering (GBP_FLAG_REORDER_LMKS, BAEngine(reorder_landmarks=True)) on the device.

A reordered handle of a problem is, inside, a plain handle of the problem relabelled by landmark_order(): the first group of tests
holds it to that BITWISE (same plan, same beliefs / means / covariances / priors through the map, same messages and relinearisation
state directly: factor order does not change).  The rest: the order is the rule's (tests/reorder_host.py restates it), the reference's
own 20 sweeps of the 700-camera sequence with shuffled landmark ids, the point of it all (a shuffled sequence gets camera windows
back), every landmark-indexed boundary, checkpoints, and a live graph grown and shrunk."""
import hashlib
import os

import numpy as np
import pytest

from conftest import DATA, belief_gap, golden, rel_err_rows
from gbp_amd.balio import read_bal
from gbp_amd.synthetic import BAProblem, keyframe_batches, make_synthetic
from reorder_host import relabel_landmarks, rule_order, shuffle_landmarks

pytestmark = pytest.mark.gpu

W = 50.0
BELIEF_TOL = 1e-6          # tests/test_hip_parity.py: beliefs against the reference / the C oracle
MSG_TOL = 1e-5             # tests/test_hip_parity.py: messages against the reference
LIVE_TOL = 1e-7            # tests/test_extend_gpu.py, tests/test_retire_gpu.py: beliefs against a second run of the same graph
# sha256 of save_state() of a plain (flag-less) handle of _small() after priors, beliefs and 3 sweeps, measured on the parent commit:
# the blobs of handles without the flag are byte for byte what they were (version 7, same header, same digest).
PLAIN_BLOB_SHA256 = '5cb51c7d7489c169ee4593314b35f162ed8570a9b0930aa4a9a34a777b7597c2'


@pytest.fixture(scope='module')
def eng():
    from gbp_amd import build
    build.build()
    from gbp_amd import engine
    return engine


def _start(e):
    e.generate_priors_var(W)
    e.update_all_beliefs()
    return e


def _bitwise(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _small(seed=1, **kw):
    return make_synthetic(n_cams=16, n_lmks=150, obs_per_lmk=4, window=6, seed=seed, **kw)


def _through(arrays, order):
    """landmark halves of a (cam_eta, cam_lam, lmk_eta, lmk_lam)-like tuple of a relabelled handle, gathered into user order"""
    return tuple(a if i < len(arrays) // 2 else a[order] for i, a in enumerate(arrays))


def _assert_same_inside(a, b, order, where):
    """a: reordered handle; b: plain handle of the relabelled problem; everything bitwise"""
    assert a.plan_info() == b.plan_info() and a.info() == b.info(), (where, a.plan_info(), b.plan_info())
    for name in ('beliefs', 'priors', 'means', 'covariances'):
        for x, y in zip(getattr(a, name)(), _through(getattr(b, name)(), order)):
            assert _bitwise(x, y), (where, name)
    for x, y in zip(a.messages(), b.messages()):
        assert _bitwise(x, y), (where, 'messages')
    ra, rb = a.relin_state(), b.relin_state()
    for key in ra:
        assert _bitwise(ra[key], rb[key]), (where, key)
    fa, fb = a.factors(dense=False), b.factors(dense=False)
    assert _bitwise(fa['linpoint'], fb['linpoint']) and _bitwise(fa['cam'], fb['cam']) and _bitwise(order[fa['lmk']], fb['lmk']), where


# ---- 3. exactness: a reordered handle is a plain handle of the relabelled problem ---------------------------------------------------

def _exact_cases():
    seq700 = read_bal(os.path.join(DATA, 'synth_seq700.txt'))
    yield 'seq700', seq700, dict()
    yield 'seq700_huber', seq700, dict(loss='huber')
    yield 'synthetic_2000', make_synthetic(n_cams=2000, n_lmks=20_000, window=30, closures=0.02, seed=2), dict(loss='constant')
    # landmarks of 40 factors: the dense packing (plan_info pack_mode 2); of 70 and 6: chunk tiles (pack_mode 1)
    yield 'dense', make_synthetic(n_cams=60, n_lmks=600, obs_per_lmk=40, window=50, seed=3), dict()
    big = make_synthetic(n_cams=90, n_lmks=40, obs_per_lmk=70, window=80, seed=4)
    few = make_synthetic(n_cams=90, n_lmks=400, obs_per_lmk=2, window=8, seed=5)
    yield 'chunks', BAProblem(K=big.K, cam_means=big.cam_means, lmk_means=np.concatenate([big.lmk_means, few.lmk_means]),
                              meas=np.concatenate([big.meas, few.meas]), cam_idx=np.concatenate([big.cam_idx, few.cam_idx]),
                              lmk_idx=np.concatenate([big.lmk_idx, few.lmk_idx + 40]).astype(np.int32)), dict(loss='huber')


@pytest.mark.parametrize('case', ['seq700', 'seq700_huber', 'synthetic_2000', 'dense', 'chunks'])
def test_reordered_handle_equals_plain_handle_of_the_relabelled_problem(eng, oracle_mod, case):
    p, kw = next((p, kw) for name, p, kw in _exact_cases() if name == case)
    q, _ = shuffle_landmarks(p, seed=7)
    a = eng.BAEngine.from_problem(q, reorder_landmarks=True, **kw)
    order = a.landmark_order()
    assert np.array_equal(np.sort(order), np.arange(q.n_lmks)) and not np.array_equal(order, np.arange(q.n_lmks))
    b = eng.BAEngine.from_problem(relabel_landmarks(q, order), **kw)
    assert a.check_layout() == 0 and b.check_layout() == 0
    if case == 'dense':
        assert a.plan_info()['pack_mode'] == 2
    if case == 'chunks':
        assert a.plan_info()['pack_mode'] == 1
    for e in (a, b):
        _start(e)
    _assert_same_inside(a, b, order, (case, 'start'))
    for e in (a, b):
        oracle_mod.replay_ba(e, 12)
    _assert_same_inside(a, b, order, (case, 'after 12 sweeps'))
    assert a.are() == b.are() and a.energy() == b.energy()
    a.close(); b.close()


# ---- 4. the order is the rule's -----------------------------------------------------------------------------------------------------

def test_landmark_order_is_the_rule(eng):
    p = make_synthetic(n_cams=700, n_lmks=6000, obs_per_lmk=5, window=20, closures=0.05, seed=9)
    q, _ = shuffle_landmarks(p, seed=1)
    keep = q.lmk_idx < 5900                                        # the last hundred landmarks lose their factors
    q = BAProblem(K=q.K, cam_means=q.cam_means, lmk_means=q.lmk_means, meas=q.meas[keep], cam_idx=q.cam_idx[keep], lmk_idx=q.lmk_idx[keep])
    a = eng.BAEngine.from_problem(q, reorder_landmarks=True)
    want = rule_order(q.cam_idx, q.lmk_idx, q.n_cams, q.n_lmks)
    assert np.array_equal(a.landmark_order(), want)
    assert np.array_equal(want[5900:], np.arange(5900, 6000))      # without factors: last, in user order
    plain = eng.BAEngine.from_problem(q)
    assert np.array_equal(plain.landmark_order(), np.arange(q.n_lmks))
    ordered = eng.BAEngine.from_problem(relabel_landmarks(q, want), reorder_landmarks=True)
    assert np.array_equal(ordered.landmark_order(), np.arange(q.n_lmks))      # already in key order: the identity
    for e in (a, plain, ordered):
        e.close()


# ---- 5. against the reference itself ------------------------------------------------------------------------------------------------

def test_g16_with_shuffled_landmark_ids_against_the_reference(eng, oracle_mod):
    """Fixture G16 (the reference's 20 sweeps of the 700-camera sequence) with the landmark ids of the file permuted at random: the
    reference's result does not depend on landmark ids, so the fixture holds as it is, landmark arrays taken back through the shuffle."""
    from test_hip_parity import replay_with_snaps
    g = golden('G16_seq700_20it')
    p = read_bal(os.path.join(DATA, 'synth_seq700.txt'))
    q, new_of_old = shuffle_landmarks(p, seed=16)
    e = _start(eng.BAEngine.from_problem(q, reorder_landmarks=True))
    pi = e.plan_info()
    assert pi['fused'] and pi['max_window'] > 0, pi
    ares, energies, relin, snaps = replay_with_snaps(oracle_mod, e, 20, (4, 12, 20))
    assert np.array_equal(relin, g['n_relin']) and relin.max() == 7200
    assert np.allclose(ares, g['are'], rtol=1e-6) and np.allclose(energies, g['energy'], rtol=1e-5)
    for k in (4, 12, 20):
        ce, cl, le, ll = snaps[k]['bel']
        gap = belief_gap((ce, cl, le[new_of_old], ll[new_of_old]), g, f'it{k}_')
        print(f'G16 shuffled + reordered, sweep {k}: belief gap {gap:.3e}')
        assert gap < BELIEF_TOL, (k, gap)
    s = snaps[20]
    for arr, name in zip(s['msg'], ('msg_cam_eta', 'msg_cam_lam', 'msg_lmk_eta', 'msg_lmk_lam')):
        err = rel_err_rows(arr, g[f'it20_{name}'])
        assert err < MSG_TOL, (name, err)
    assert np.array_equal(s['st']['iters_since_relin'], g['it20_iters_since_relin'])
    assert np.array_equal(s['st']['eta_damping'], g['it20_eta_damping'])
    e.close()


# ---- 6. the point of it -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('closures', [0.0, 0.02])
def test_shuffled_sequence_gets_camera_windows_back(eng, oracle_mod, closures):
    """2 000 cameras, 40 000 landmarks x 10, window 30, landmark ids shuffled.  Without the flag every workgroup meets about 1 130 of the
    cameras (the model of tests/test_reorder_cpu.py) against a table of gbp_ba_fused_max_cams() = 587 and the plan is the general sweep:
    confirmed on the commit before this option existed (both graphs: fused 0, no windows; in generator order 40 / 9 598 and 113 / 17 389
    largest table / rows), where this test cannot pass at all -- BAEngine has no reorder_landmarks there.  With the flag: the fused sweep with windows, its largest table and its rows within the caps the model
    is held to, against the plan of the generator-ordered problem; and 20 sweeps agree with the C oracle."""
    from gbp_amd import _capi
    p = make_synthetic(n_cams=2000, n_lmks=40_000, window=30, closures=closures)
    q, new_of_old = shuffle_landmarks(p, seed=6)
    gen = eng.BAEngine.from_problem(p).plan_info()
    plain = eng.BAEngine.from_problem(q)
    e = eng.BAEngine.from_problem(q, reorder_landmarks=True)
    pi, cap = e.plan_info(), _capi.load().gbp_ba_fused_max_cams()
    print(f'closures {closures}: generator order {gen["max_window"]} / {gen["table_rows"]}, shuffled plain fused={plain.plan_info()["fused"]}, '
          f'reordered {pi["max_window"]} / {pi["table_rows"]} (largest table / rows; cap {cap})')
    assert gen['fused'] and gen['max_window'] > 0, gen
    assert not plain.plan_info()['fused'], plain.plan_info()
    assert pi['fused'] and pi['max_window'] > 0, pi
    assert pi['max_window'] <= 1.5 * gen['max_window'] and pi['max_window'] <= cap, (pi, gen)
    assert pi['table_rows'] <= 1.25 * gen['table_rows'], (pi, gen)
    plain.close()
    o = oracle_mod.OracleBA.from_problem(q, threads=8)
    for g in (o, e):
        _start(g)
        oracle_mod.replay_ba(g, 20)
    gap = max(rel_err_rows(x, y) for x, y in zip(e.beliefs(), o.beliefs()))
    print(f'closures {closures}: belief gap against the C oracle after 20 sweeps {gap:.3e}')
    assert gap < BELIEF_TOL, gap
    assert np.array_equal(o.relin_state()['iters_since_relin'], e.relin_state()['iters_since_relin'])
    e.close()


# ---- 7. boundaries ------------------------------------------------------------------------------------------------------------------

def test_landmark_indexed_boundaries_speak_user_ids(eng):
    p = make_synthetic(n_cams=40, n_lmks=900, obs_per_lmk=4, window=8, seed=12)
    q, _ = shuffle_landmarks(p, seed=3)
    e = _start(eng.BAEngine.from_problem(q, reorder_landmarks=True))
    plain = _start(eng.BAEngine.from_problem(q))
    assert not np.array_equal(e.landmark_order(), np.arange(q.n_lmks))
    C, L = q.n_cams, q.n_lmks
    rng = np.random.default_rng(0)
    f = e.factors(dense=False)                                     # the factor-id view: the caller's ids, reference order
    order = np.argsort(q.cam_idx, kind='stable')
    assert np.array_equal(f['lmk'], q.lmk_idx[order]) and np.array_equal(f['cam'], q.cam_idx[order])
    assert np.allclose(f['linpoint'][:, 6:], q.lmk_means[f['lmk']], rtol=0, atol=0)
    assert _bitwise(e.factor_lambda_max()[1], plain.factor_lambda_max()[1])
    for x, y in zip(e.priors(), plain.priors()):                   # generate_priors_var: per-landmark maxima
        assert _bitwise(x, y)
    # set_priors
    ce, le = rng.normal(size=(C, 6)), rng.normal(size=(L, 3))
    cl = np.einsum('nij,nkj->nik', *(2 * [rng.normal(size=(C, 6, 6))])) + np.eye(6)
    ll = np.einsum('nij,nkj->nik', *(2 * [rng.normal(size=(L, 3, 3))])) + np.eye(3)
    e.set_priors(ce, cl, le, ll)
    got = e.priors()
    assert _bitwise(got[0], ce) and _bitwise(got[2], le) and np.allclose(got[1], cl, rtol=1e-15) and np.allclose(got[3], ll, rtol=1e-15)
    # set_prior_scalars: Lambda = l I, eta = l mu
    lc, lmk_l = rng.uniform(1, 2, size=C), rng.uniform(1, 2, size=L)
    e.set_prior_scalars(lc, lmk_l)
    got, (_, lm) = e.priors(), e.means()
    assert _bitwise(got[3], lmk_l[:, None, None] * np.eye(3)[None]) and _bitwise(got[2], lmk_l[:, None] * lm)
    # set_priors_var
    cov = [np.eye(6) * (1.0 + 0.01 * v) for v in range(C)] + [np.eye(3) * (2.0 + 0.001 * v) for v in range(L)]
    e.set_priors_var(cov)
    got = e.priors()
    assert np.allclose(got[3], np.array([np.linalg.inv(c) for c in cov[C:]]), rtol=1e-14)
    assert np.allclose(got[2], np.einsum('nij,nj->ni', got[3], lm), rtol=1e-14)
    # streaming means
    plain.set_priors_var(cov)
    for g in (e, plain):
        g.update_all_beliefs()
        g.iterate(3)
    e.means_snapshot()
    for x, y in zip(e.means_fetch(wait=True), e.means()):
        assert _bitwise(x, y)
    for x, y in zip(e.means(), plain.means()):                     # against a handle without the flag: summation order differs
        assert rel_err_rows(x, y) < LIVE_TOL
    assert e.check_layout() == 0
    e.close(); plain.close()


def test_compat_graph_keeps_file_order(eng, tmp_path):
    import sys
    from conftest import REPO
    from gbp_amd.synthetic import write_bal
    sys.path.insert(0, os.path.join(REPO, 'gbp_amd', 'compat'))
    try:
        from gbp import gbp_ba
    finally:
        sys.path.remove(os.path.join(REPO, 'gbp_amd', 'compat'))
    q, _ = shuffle_landmarks(make_synthetic(n_cams=20, n_lmks=300, obs_per_lmk=3, window=6, seed=8), seed=2)
    path = str(tmp_path / 'shuffled.txt')
    write_bal(q, path)
    configs = dict(gauss_noise_std=2, loss=None, Nstds=3.0, beta=0.01, num_undamped_iters=6, min_linear_iters=8, eta_damping=0.4,
                   prior_std_weaker_factor=50.0, reorder_landmarks=True)
    graph = gbp_ba.create_ba_graph(path, configs)
    direct = eng.BAEngine.from_problem(read_bal(path), reorder_landmarks=True)
    assert not np.array_equal(direct.landmark_order(), np.arange(q.n_lmks))
    for g in (graph, direct):
        g.generate_priors_var(weaker_factor=50.0)
        g.update_all_beliefs()
    for _ in range(4):
        graph.synchronous_iteration()
        direct.synchronous_iteration()
    ce, cl, le, ll = direct.beliefs()
    _, lm = direct.means()
    for l in (0, 1, 57, q.n_lmks - 1):
        node = graph.var_nodes[q.n_cams + l]
        assert node.variableID == q.n_cams + l
        assert _bitwise(np.asarray(node.belief.eta), le[l]) and _bitwise(np.asarray(node.belief.lam), ll[l]) and _bitwise(np.asarray(node.mu), lm[l])
    assert _bitwise(np.asarray(graph.var_nodes[3].belief.eta), ce[3])
    direct.close()


# ---- 8. checkpoints -----------------------------------------------------------------------------------------------------------------

def test_checkpoints_of_reordered_and_plain_handles_do_not_mix(eng):
    q, _ = shuffle_landmarks(_small(), seed=5)
    a = _start(eng.BAEngine.from_problem(q, reorder_landmarks=True))
    plain = _start(eng.BAEngine.from_problem(q))
    for e in (a, plain):
        e.iterate(3)
    blob, plain_blob = a.save_state(), plain.save_state()
    twin = eng.BAEngine.from_problem(q, reorder_landmarks=True)
    twin.load_state(blob)
    for e in (a, twin):
        e.iterate(5)
    assert _bitwise(a.save_state(), twin.save_state())
    for x, y in zip(a.beliefs(), twin.beliefs()):
        assert _bitwise(x, y)
    # the two kinds refuse each other's blobs, untouched
    before_a, before_p = a.save_state(), plain.save_state()
    with pytest.raises(Exception, match='different graph'):
        plain.load_state(blob)
    with pytest.raises(Exception, match='different graph'):
        a.load_state(plain_blob)
    assert _bitwise(a.save_state(), before_a) and _bitwise(plain.save_state(), before_p)
    # ... also when the order happens to be the identity
    ordered = relabel_landmarks(q, a.landmark_order())
    ia, ip = _start(eng.BAEngine.from_problem(ordered, reorder_landmarks=True)), _start(eng.BAEngine.from_problem(ordered))
    assert np.array_equal(ia.landmark_order(), np.arange(q.n_lmks))
    with pytest.raises(Exception, match='different graph'):
        ip.load_state(ia.save_state())
    with pytest.raises(Exception, match='different graph'):
        ia.load_state(ip.save_state())
    for e in (a, plain, twin, ia, ip):
        e.close()


def test_plain_blob_is_byte_identical_to_the_parents(eng):
    e = _start(eng.BAEngine.from_problem(_small()))
    e.iterate(3)
    digest = hashlib.sha256(e.save_state().tobytes()).hexdigest()
    print('sha256 of the plain blob:', digest)
    assert digest == PLAIN_BLOB_SHA256
    e.close()


# ---- 9. live graph ------------------------------------------------------------------------------------------------------------------

def _drive(eng, sp, k, reorder, **kw):
    """base + every batch (two sweeps after each), then the first 2 k cameras retired, two more sweeps"""
    e = _start(eng.BAEngine.from_problem(sp.base, reorder_landmarks=reorder, **kw))
    e.iterate(2)
    for b in sp.batches:
        e.extend(b['cam_means'], b['lmk_means'], b['meas'], b['cam_idx'], b['lmk_idx'], prior_weaker_factor=W)
        e.iterate(2)
    maps = e.retire(np.arange(2 * k))
    e.iterate(2)
    return e, maps


@pytest.mark.parametrize('loss,defer', [(None, 0.0), ('huber', 0.2)])
def test_live_graph_extend_and_retire_through_the_maps(eng, loss, defer):
    k = 4
    p = make_synthetic(n_cams=40, n_lmks=700, obs_per_lmk=4, window=8, closures=0.03, seed=21)
    q, _ = shuffle_landmarks(p, seed=9)
    sp = keyframe_batches(q, [16] + [k] * 6, defer=defer, seed=1)
    sp_shuffled = []
    # keyframe_batches numbers the landmarks in joining order -- along the trajectory; shuffle inside every batch so that they are not
    rng = np.random.default_rng(4)
    L0 = sp.base.n_lmks
    perm_parts, start = [rng.permutation(L0)], L0
    for b in sp.batches:
        n = b['lmk_means'].shape[0]
        perm_parts.append(start + rng.permutation(n)); start += n
    new_of_old = np.concatenate(perm_parts).astype(np.int32)

    def relabel_part(part, lo, hi):
        means = np.empty_like(part['lmk_means'])
        means[new_of_old[lo:hi] - lo] = part['lmk_means']
        return dict(part, lmk_means=means, lmk_idx=new_of_old[part['lmk_idx']].astype(np.int32))
    base = relabel_part(dict(cam_means=sp.base.cam_means, lmk_means=sp.base.lmk_means, meas=sp.base.meas, cam_idx=sp.base.cam_idx,
                             lmk_idx=sp.base.lmk_idx), 0, L0)
    sp.base = BAProblem(K=q.K, cam_means=base['cam_means'], lmk_means=base['lmk_means'], meas=base['meas'], cam_idx=base['cam_idx'],
                        lmk_idx=base['lmk_idx'])
    lo = L0
    for i, b in enumerate(sp.batches):
        n = b['lmk_means'].shape[0]
        sp.batches[i] = relabel_part(b, lo, lo + n); lo += n

    a, maps = _drive(eng, sp, k, True, loss=loss)
    a2, maps2 = _drive(eng, sp, k, True, loss=loss)
    plain, maps_p = _drive(eng, sp, k, False, loss=loss)
    for m, m2, mp in zip(maps, maps2, maps_p):
        assert np.array_equal(m, m2) and np.array_equal(m, mp)     # the maps are the caller's numbering, flag or no flag
    assert _bitwise(a.save_state(), a2.save_state())               # reproducible run to run
    assert not np.array_equal(a.landmark_order(), np.arange(a.L)) and a.check_layout() == 0
    # user-order beliefs agree with a handle without the flag driven the same way
    for x, y in zip(a.beliefs(), plain.beliefs()):
        gap = rel_err_rows(x, y)
        assert gap < LIVE_TOL, gap
    assert np.array_equal(a.iters_since_relin(), plain.iters_since_relin())
    # a fresh reordered handle of the same final problem takes the state blob and continues bitwise
    f, (cm, lm) = a.factors(dense=False), a.means()
    final = BAProblem(K=q.K, cam_means=cm, lmk_means=lm, meas=f['z'], cam_idx=f['cam'], lmk_idx=f['lmk'])
    fresh = _start(eng.BAEngine.from_problem(final, reorder_landmarks=True, loss=loss))
    assert np.array_equal(fresh.landmark_order(), a.landmark_order())
    assert np.array_equal(a.landmark_order(), rule_order(f['cam'], f['lmk'], a.C, a.L))
    assert a.plan_info() == fresh.plan_info()
    fresh.load_state(a.save_state())
    for e in (a, fresh):
        e.iterate(6)
    assert _bitwise(a.save_state(), fresh.save_state())
    for name in ('beliefs', 'priors', 'messages'):
        for x, y in zip(getattr(a, name)(), getattr(fresh, name)()):
            assert _bitwise(x, y), name
    # a failing extend (landmark id out of range) leaves the reordered handle as it was
    blob, order = a.save_state(), a.landmark_order()
    with pytest.raises(Exception):
        a.extend(np.zeros((1, 6)), np.zeros((0, 3)), np.zeros((1, 2)), np.array([a.C], np.int32), np.array([a.L + 5], np.int32))
    assert _bitwise(a.save_state(), blob) and np.array_equal(a.landmark_order(), order)
    a.iterate(1); fresh.iterate(1)
    assert _bitwise(a.save_state(), fresh.save_state())
    for e in (a, a2, plain, fresh):
        e.close()
