#!/usr/bin/env python3
"""Generate fixture G19 (a BA graph from which single OBSERVATIONS are culled) by driving the reference's own classes.

    python tests/golden/make_g19.py --reference PATH_TO_THE_REFERENCE [--only small,vsmall_huber]

Like make_g18.py this runs where the reference is available read-only and copies nothing of it: the graph comes from the reference's
create_ba_graph on the shipped BAL file, and every cull is done on the reference's own objects by tests/cull_host.cull_graph (the steps
of include/gbp_ba.h gbp_ba_cull: the listed factors leave with their messages, nothing is added to any prior, cameras and landmarks left
without a factor leave too, renumber, update_all_beliefs).
Schedule: ba.py's (prior_std_weaker_factor 50, iters_since_relin reset to 1 before sweeps 3 and 8) for 10 sweeps, then cull, 10 plain
sweeps, cull, 10 plain sweeps.  The FIRST list holds the interesting cases by construction, not by luck -- the union of
  * all factors of camera 3 (a camera goes: the camera renumbering is not the identity),
  * all factors of the landmark with the most observations (a landmark goes),
  * the 5 % of the remaining factors with the largest reprojection_err() by the reference's own numbers;
the second is the 5 % largest only.  Asserted here: a camera is dropped, a landmark is dropped, a surviving landmark lost some but not
all of its factors, and the run stays finite.

Stored (the GPU tests never read the reference and cull the STORED lists, never a selection of their own): the problem as the reference
read it; per cull the list, the three maps, the reference's per-factor residuals just before it, and all priors and all beliefs right
after it; after every sweep ARE, energy and the number of factors that relinearised; after each batch's last sweep beliefs,
iters_since_relin, eta_damping (and adaptive variances with huber); messages after the last sweep.  Packing as make_g18.py's, to keep
each file below 1 MiB: symmetric matrices as upper triangles, messages for every 6th factor, float64 only, no dense copies, no means.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

from make_golden import default_configs, save      # noqa: E402

SWEEPS = 10
SHARE = 0.05
CAMERA = 3
RUNS = dict(small=('fr1desk_small.txt', {}), vsmall_huber=('fr1desk_vsmall.txt', dict(loss='huber')))
N_CULLS = 2
SAMPLE_MSG = 6
U6, U3 = np.triu_indices(6), np.triu_indices(3)


def four(graph, what):
    return dict(cam_eta=np.array([getattr(n, what).eta for n in graph.cam_nodes]), cam_lam=np.array([getattr(n, what).lam[U6] for n in graph.cam_nodes]),
                lmk_eta=np.array([getattr(n, what).eta for n in graph.lmk_nodes]), lmk_lam=np.array([getattr(n, what).lam[U3] for n in graph.lmk_nodes]))


def cull_list(graph, first):
    """(list, residuals): the ids to cull now, by the reference's own residuals."""
    from cull_host import residuals_of, largest_residuals
    res = residuals_of(graph)
    err = np.array([f.reprojection_err() for f in graph.factors])
    assert np.allclose(err, np.linalg.norm(res, axis=1), rtol=1e-14, atol=0)
    F = len(graph.factors)
    fixed = np.zeros(F, bool)
    if first:
        cam = graph.cam_nodes[CAMERA]
        big = max(graph.lmk_nodes, key=lambda n: len(n.adj_factors))
        for i, f in enumerate(graph.factors):
            fixed[i] = f.adj_var_nodes[0] is cam or f.adj_var_nodes[1] is big
    worst = largest_residuals(res, np.flatnonzero(~fixed), SHARE)
    return np.union1d(np.flatnonzero(fixed), worst).astype(np.int32), res


def run(tag):
    from gbp import gbp_ba
    from cull_host import cull_graph
    fname, over = RUNS[tag]
    cfg = default_configs(**over)
    from gbp_amd.balio import read_bal
    path = os.path.join(HERE, 'data', fname)
    graph = gbp_ba.create_ba_graph(path, cfg)
    K = np.asarray(read_bal(path).K, np.float64)
    out = dict(bal=np.array(fname), loss=np.array(str(over.get('loss'))), n_culls=np.array(N_CULLS), sweeps=np.array(SWEEPS),
               base_K=K, base_cam_means=np.array([n.mu for n in graph.cam_nodes], np.float64),
               base_lmk_means=np.array([n.mu for n in graph.lmk_nodes], np.float64),
               base_meas=np.array([f.measurement for f in graph.factors], np.float64),
               base_cam_idx=np.array([f.adj_var_nodes[0].c_id for f in graph.factors], np.int32),
               base_lmk_idx=np.array([f.adj_var_nodes[1].l_id for f in graph.factors], np.int32))
    graph.generate_priors_var(weaker_factor=cfg['prior_std_weaker_factor'])
    graph.update_all_beliefs()
    are, energy, relins = [], [], []
    for b in range(N_CULLS + 1):
        if b:
            ids, res = cull_list(graph, first=b == 1)
            C_old, L_old, F_old = len(graph.cam_nodes), len(graph.lmk_nodes), len(graph.factors)
            deg = {id(n): len(n.adj_factors) for n in graph.lmk_nodes}
            cams, lmks, cm, lm, fm = cull_graph(graph, graph.cam_nodes, graph.lmk_nodes, ids)
            graph.cam_nodes[:], graph.lmk_nodes[:] = cams, lmks
            partial = sum(1 for n in lmks if 0 < len(n.adj_factors) < deg[id(n)])
            print(f'{tag} cull {b}: {ids.size} of {F_old} factors culled, {C_old - len(cams)} cameras and {L_old - len(lmks)} landmarks dropped, '
                  f'{partial} surviving landmarks lost some of their factors')
            if b == 1:
                assert C_old - len(cams) >= 1 and cm[CAMERA] == -1 and not np.array_equal(cm[cm >= 0], np.flatnonzero(cm >= 0))
                assert L_old - len(lmks) >= 1
            assert partial >= 1
            out[f'c{b}_factor_ids'], out[f'c{b}_cam_map'], out[f'c{b}_lmk_map'], out[f'c{b}_factor_map'] = ids, cm, lm, fm
            out[f'c{b}_residuals'] = res
            for name, arr in four(graph, 'prior').items():
                out[f'c{b}_prior_{name}'] = arr
            for name, arr in four(graph, 'belief').items():
                out[f'c{b}_cull_{name}'] = arr
        for i in range(SWEEPS):
            if b == 0 and i in (3, 8):                         # ba.py:91-93
                for f in graph.factors:
                    f.iters_since_relin = 1
            graph.synchronous_iteration(robustify=True, local_relin=True)
            are.append(graph.are())
            energy.append(graph.energy())
            relins.append(sum(1 for f in graph.factors if f.iters_since_relin == 0))
        print(f'{tag} batch {b}: ARE {are[-1]:.2f}')
        for name, arr in four(graph, 'belief').items():
            out[f'c{b}_end_{name}'] = arr
        out[f'c{b}_end_iters_since_relin'] = np.array([f.iters_since_relin for f in graph.factors], np.int32)
        out[f'c{b}_end_eta_damping'] = np.array([f.eta_damping for f in graph.factors], np.float64)
        if over.get('loss'):
            out[f'c{b}_end_adaptive_var'] = np.array([f.adaptive_gauss_noise_var for f in graph.factors], np.float64)
    fs = graph.factors[::SAMPLE_MSG]
    out['msg_cam_eta'] = np.array([f.messages[0].eta for f in fs])
    out['msg_cam_lam'] = np.array([f.messages[0].lam[U6] for f in fs])
    out['msg_lmk_eta'] = np.array([f.messages[1].eta for f in fs])
    out['msg_lmk_lam'] = np.array([f.messages[1].lam[U3] for f in fs])
    out['are'], out['energy'], out['n_relin'] = np.array(are), np.array(energy), np.array(relins, np.int32)
    assert all(np.isfinite(v).all() for v in out.values() if v.dtype.kind == 'f'), 'the run did not stay finite'
    save(f'G19_cull_{tag}', **out)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True)
    ap.add_argument('--only', default='')
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import warnings
    warnings.simplefilter('ignore', SyntaxWarning)
    for t in [s for s in args.only.split(',') if s] or list(RUNS):
        run(t)
