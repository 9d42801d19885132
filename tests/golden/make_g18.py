#!/usr/bin/env python3
"""Generate fixture G18 (a BA graph that SHRINKS: cameras are retired from a fixed-lag window) by driving the reference's own classes.

    python tests/golden/make_g18.py --reference PATH_TO_THE_REFERENCE [--only small,vsmall_huber]

Like make_g17.py this runs where the reference is available read-only and copies nothing of it: the graph comes from the reference's
create_ba_graph on the shipped BAL file, and every retirement is done on the reference's own objects by tests/retire_host.retire_graph
(the steps of include/gbp_ba.h gbp_ba_retire: fold the retired factors' messages to their landmarks into the landmarks' priors in
adj_factors order, drop the cameras, their factors and the orphaned landmarks, renumber, update_all_beliefs).
Schedule: ba.py's (prior_std_weaker_factor 50, iters_since_relin reset to 1 before sweeps 3 and 8) for 10 sweeps, then a fixed-lag run:
retire cameras, 10 plain sweeps, retire again, 10 plain sweeps.  The FIRST retirement takes a non-prefix set (cameras 3 and 0, in that
order), so renumbering is not a shift; the second the oldest cameras of what is left.

Stored (the GPU tests never read the reference): the problem as the reference read it; per retirement the camera list, the three maps,
the surviving landmarks' priors and all beliefs right after it; after every sweep ARE, energy and the number of factors that
relinearised; after each batch's last sweep beliefs, iters_since_relin, eta_damping (and adaptive variances with huber); messages after
the last sweep.  To keep each file below 1 MiB: symmetric matrices as upper triangles, messages for every 6th factor, and the records that
are per landmark (priors and beliefs after a retirement, beliefs at batch ends) in float64 only -- no dense copies, no means.
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
RUNS = dict(small=('fr1desk_small.txt', ((3, 0), (0, 1, 2)), {}),                        # 20 keyframes -> 18 -> 15
            vsmall_huber=('fr1desk_vsmall.txt', ((3, 0), (0, 1)), dict(loss='huber')))   # 10 keyframes -> 8 -> 6
SAMPLE_MSG = 6
U6, U3 = np.triu_indices(6), np.triu_indices(3)


def beliefs(graph):
    return dict(cam_eta=np.array([n.belief.eta for n in graph.cam_nodes]), cam_lam=np.array([n.belief.lam[U6] for n in graph.cam_nodes]),
                lmk_eta=np.array([n.belief.eta for n in graph.lmk_nodes]), lmk_lam=np.array([n.belief.lam[U3] for n in graph.lmk_nodes]))


def run(tag):
    from gbp import gbp_ba
    from retire_host import retire_graph
    fname, retirements, over = RUNS[tag]
    cfg = default_configs(**over)
    from gbp_amd.balio import read_bal
    path = os.path.join(HERE, 'data', fname)
    graph = gbp_ba.create_ba_graph(path, cfg)
    K = np.asarray(read_bal(path).K, np.float64)
    out = dict(bal=np.array(fname), loss=np.array(str(over.get('loss'))), n_retirements=np.array(len(retirements)), sweeps=np.array(SWEEPS),
               base_K=K, base_cam_means=np.array([n.mu for n in graph.cam_nodes], np.float64),
               base_lmk_means=np.array([n.mu for n in graph.lmk_nodes], np.float64),
               base_meas=np.array([f.measurement for f in graph.factors], np.float64),
               base_cam_idx=np.array([f.adj_var_nodes[0].c_id for f in graph.factors], np.int32),
               base_lmk_idx=np.array([f.adj_var_nodes[1].l_id for f in graph.factors], np.int32))
    graph.generate_priors_var(weaker_factor=cfg['prior_std_weaker_factor'])
    graph.update_all_beliefs()
    are, energy, relins = [], [], []
    for b in range(len(retirements) + 1):
        if b:
            ids = np.array(retirements[b - 1], np.int32)
            before = {id(n): (n.belief.eta.copy(), n.belief.lam.copy()) for n in graph.cam_nodes + graph.lmk_nodes}
            L_old = len(graph.lmk_nodes)
            cams, lmks, cm, lm, fm = retire_graph(graph, graph.cam_nodes, graph.lmk_nodes, ids)
            graph.cam_nodes[:], graph.lmk_nodes[:] = cams, lmks
            gap = max(max(np.abs(n.belief.eta - before[id(n)][0]).max() / np.abs(before[id(n)][0]).max(),
                          np.abs(n.belief.lam - before[id(n)][1]).max() / np.abs(before[id(n)][1]).max()) for n in cams + lmks)
            deg1 = sum(1 for n in lmks if len(n.adj_factors) == 1)
            print(f'{tag} retirement {b}: cameras {list(ids)}, {int((fm < 0).sum())} factors and {L_old - len(lmks)} orphan landmarks dropped, '
                  f'{deg1} landmarks of degree 1 remain, surviving beliefs moved by {gap:.1e} (relative)')
            out[f'r{b}_cam_ids'], out[f'r{b}_cam_map'], out[f'r{b}_lmk_map'], out[f'r{b}_factor_map'] = ids, cm, lm, fm
            out[f'r{b}_lmk_prior_eta'] = np.array([n.prior.eta for n in lmks])
            out[f'r{b}_lmk_prior_lam'] = np.array([n.prior.lam[U3] for n in lmks])
            for name, arr in beliefs(graph).items():
                out[f'r{b}_ret_{name}'] = arr
        for i in range(SWEEPS):
            if b == 0 and i in (3, 8):                         # ba.py:91-93
                for f in graph.factors:
                    f.iters_since_relin = 1
            graph.synchronous_iteration(robustify=True, local_relin=True)
            are.append(graph.are())
            energy.append(graph.energy())
            relins.append(sum(1 for f in graph.factors if f.iters_since_relin == 0))
        print(f'{tag} batch {b}: ARE {are[-1]:.2f}')
        for name, arr in beliefs(graph).items():
            out[f'r{b}_end_{name}'] = arr
        out[f'r{b}_end_iters_since_relin'] = np.array([f.iters_since_relin for f in graph.factors], np.int32)
        out[f'r{b}_end_eta_damping'] = np.array([f.eta_damping for f in graph.factors], np.float64)
        if over.get('loss'):
            out[f'r{b}_end_adaptive_var'] = np.array([f.adaptive_gauss_noise_var for f in graph.factors], np.float64)
    fs = graph.factors[::SAMPLE_MSG]
    out['msg_cam_eta'] = np.array([f.messages[0].eta for f in fs])
    out['msg_cam_lam'] = np.array([f.messages[0].lam[U6] for f in fs])
    out['msg_lmk_eta'] = np.array([f.messages[1].eta for f in fs])
    out['msg_lmk_lam'] = np.array([f.messages[1].lam[U3] for f in fs])
    out['are'], out['energy'], out['n_relin'] = np.array(are), np.array(energy), np.array(relins, np.int32)
    save(f'G18_retire_{tag}', **out)


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
