"""Randomised shapes through the landmark-sharded driver at world sizes 2-4 (thread ranks on one GPU, tests/test_sharded_gpu.py)
against ONE engine on the same graph: ragged partitions, ranks that own a single landmark or none, cameras a rank never sees,
over-sized landmarks, every loss, random sweep flags, both sweeps, both loops, both in-library exchanges (callback / peer stores).  The graphs are those of test_fuzz_gpu.py."""
import os
import threading

import numpy as np
import pytest

from conftest import rel_err_rows
from test_fuzz_gpu import random_problem
from test_sharded_gpu import LockstepDist, LockstepWorld

pytestmark = pytest.mark.gpu
N_SEEDS = int(os.environ.get('GBP_FUZZ_SEEDS', 18))
SWEEPS_COMPARED = {}      # seed -> (sweeps compared, sweeps of the schedule)


def sharded_run(p, world, fused, library_loop, cfg, flags, exchange='auto'):
    from gbp_amd.sharded import ShardedBA
    shared = LockstepWorld(world)
    out, errors = [None] * world, []

    def rank_main(r):
        try:
            import torch
            torch.cuda.set_device(0)
            g = ShardedBA(p, device=0, fused=fused, dist=LockstepDist(shared, r), library_loop=library_loop, exchange=exchange, **cfg)
            assert not library_loop or g.exchange == ('callback' if exchange == 'auto' else exchange)
            g.generate_priors_var(30.0)
            g.update_all_beliefs()
            for rob, rel in flags:
                g.synchronous_iteration(robustify=rob, local_relin=rel)
            ce, cl = g.camera_beliefs()
            rng, le, ll = g.local_landmark_beliefs()
            out[r] = dict(ce=ce, cl=cl, le=le, ll=ll, rng=rng, are=g.are(), energy=g.energy(), n_relin=g.count_relinearising())
        except BaseException as e:                           # noqa: BLE001 -- surface it in the main thread
            errors.append(e)
            shared.barrier.abort()

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    if errors:
        raise errors[0]
    return out


@pytest.mark.parametrize('seed', range(N_SEEDS))
def test_sharded_random_shapes(oracle_mod, seed):
    from gbp_amd.engine import BAEngine
    rng = np.random.default_rng(5000 + seed)
    p = random_problem(seed)
    world = 2 + seed % 3
    fused, library_loop = seed % 4 != 3, seed % 5 != 4
    cfg = dict(loss=[None, 'huber', 'constant'][seed % 3], Nstds=float(rng.uniform(1.0, 3.0)), beta=float(rng.choice([0.005, 0.01, 0.05])),
               num_undamped_iters=int(rng.choice([1, 2, 6])), min_linear_iters=int(rng.choice([2, 4, 8])),
               eta_damping=float(rng.choice([0.3, 0.4, 0.7])), gauss_noise_std=float(rng.uniform(1.5, 3.0)))
    flags = [(bool(rng.integers(0, 2)), bool(rng.random() < 0.8)) for _ in range(6)]
    # How far are two correct implementations apart on this run?  Aggressive settings can make a tiny graph ill-conditioned or blow it up
    # (test_fuzz_gpu.healthy) -- from there on there is nothing to hold the sharded sums against.  Such a run is CUT SHORT at its last sane
    # sweep, not skipped (seed 0 blew up on the single engine too and skipped on every run -- a seed that always skips tests
    # nothing): first pass = single engine and oracle sweep by sweep, the schedule ends in front of the first sweep after which the two are
    # more than 1e-4 apart (or not finite); the comparison below runs on that schedule.
    probe = BAEngine.from_problem(p, fused=fused, **cfg)
    o = oracle_mod.OracleBA.from_problem(p, threads=4, **cfg)
    for g in (probe, o):
        g.generate_priors_var(30.0)
        g.update_all_beliefs()
    cut = 0
    for rob, rel in flags:
        for g in (probe, o):
            g.synchronous_iteration(robustify=rob, local_relin=rel)
        pb = probe.beliefs()
        gap = max(rel_err_rows(a, b) for a, b in zip(pb, o.beliefs()))
        if not (np.isfinite(gap) and gap <= 1e-4 and all(np.isfinite(x).all() for x in pb)):
            break
        cut += 1
    probe.close()
    SWEEPS_COMPARED[seed] = (cut, len(flags))
    flags = flags[:cut]
    ref = BAEngine.from_problem(p, fused=fused, **cfg)
    o = oracle_mod.OracleBA.from_problem(p, threads=4, **cfg)
    for g in (ref, o):
        g.generate_priors_var(30.0)
        g.update_all_beliefs()
        for rob, rel in flags:
            g.synchronous_iteration(robustify=rob, local_relin=rel)
    rb = ref.beliefs()
    spread = max(rel_err_rows(a, b) for a, b in zip(rb, o.beliefs()))
    assert np.isfinite(spread) and spread <= 1e-4, (seed, cut, spread)      # by construction of the cut; never a skip
    tol = max(1e-7, 4.0 * spread)
    # odd seeds: the peer-store exchange (mailboxes + tags; fused and general sweeps, camera groups, every loss), even seeds: the
    # plugged-in all-gather
    ranks = sharded_run(p, world, fused, library_loop, cfg, flags, exchange='peer' if (seed % 2 and library_loop) else 'auto')
    rce, rcl, rle, rll = rb
    lo = 0
    for r in ranks:
        assert np.array_equal(r['ce'], ranks[0]['ce']) and np.array_equal(r['cl'], ranks[0]['cl'])   # identical on every rank
        assert rel_err_rows(r['ce'], rce) < tol and rel_err_rows(r['cl'], rcl) < tol, (seed, world, tol)
        a, b = r['rng']
        assert a == lo
        lo = b
        if b > a:
            assert rel_err_rows(r['le'], rle[a:b]) < tol and rel_err_rows(r['ll'], rll[a:b]) < tol, (seed, world, tol)
        assert r['are'] == pytest.approx(ref.are(), rel=max(1e-7, 100 * tol), abs=1e-9)
        assert r['n_relin'] == ranks[0]['n_relin']
    assert lo == p.n_lmks
    if spread < 1e-9:                                        # (a threshold decision can flip on the last bits otherwise)
        assert ranks[0]['n_relin'] == ref.count_relinearising()


def test_no_seed_was_skipped_and_most_ran_their_whole_schedule(request):
    """(runs after the parametrised test above: same module, file order)  Every seed was compared -- none skipped, none cut down to no
    sweep at all -- and cutting a schedule short stays the exception: if most seeds lost sweeps, the fuzz would no longer be testing
    relinearisation waves."""
    if os.environ.get('PYTEST_XDIST_WORKER'):
        pytest.skip('the seeds are spread over xdist workers (soak runs): the tally lives in the other processes')
    if request.config.getoption('keyword'):
        pytest.skip('-k selected a subset: the tally is incomplete by construction')
    counted = sorted(k for k, (cut, _) in SWEEPS_COMPARED.items() if cut >= 1)      # a schedule cut to 0 sweeps compared nothing
    assert counted == list(range(N_SEEDS)), f"seeds that did not reach the comparison: {sorted(set(range(N_SEEDS)) - set(counted))}"
    whole = sum(1 for c, n in SWEEPS_COMPARED.values() if c == n)
    assert whole >= (3 * N_SEEDS) // 4, SWEEPS_COMPARED
    print("sharded fuzz, sweeps compared per seed:", {k: v[0] for k, v in sorted(SWEEPS_COMPARED.items()) if v[0] != v[1]} or "all whole")
