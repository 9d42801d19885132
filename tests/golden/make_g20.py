#!/usr/bin/env python3
"""Generate fixture G20 (a BA graph that lets go of LANDMARKS: map points are retired by name) by driving the reference's own classes.

    python tests/golden/make_g20.py --reference PATH_TO_THE_REFERENCE [--only small,vsmall_huber]

Like make_g18.py this runs where the reference is available read-only and copies nothing of it: the graph comes from the reference's
create_ba_graph on the shipped BAL file, and every retirement is done on the reference's own objects by
tests/retire_lmk_host.retire_landmarks_graph (the steps of include/gbp_ba.h gbp_ba_retire_landmarks: fold the departing factors' messages
to their cameras into the cameras' priors in adj_factors order -- or drop them --, remove the landmarks, their factors and the orphaned
cameras and landmarks, renumber, update_all_beliefs).
Schedule: ba.py's (prior_std_weaker_factor 50, iters_since_relin reset to 1 before sweeps 3 and 8) for 10 sweeps, then retire landmarks
with FOLD, 10 plain sweeps, retire landmarks with DROP, 10 plain sweeps.  The FIRST list (retire_lmk_host.pick_first_list) is no prefix of
the ids, so renumbering is not a shift; it holds ALL the landmarks of one camera, so that camera is orphaned and the camera map is not a
shift either; and it holds landmarks of the lowest degree there is -- 2 in both files: the shipped BAL files have no landmark of
degree 1, and none can arise here (a camera is orphaned only when ALL its landmarks go, so no surviving landmark ever loses a factor);
degree 1 is covered by the synthetic graphs of tests/test_retire_lmk_gpu.py.  The second list is every 7th of the surviving landmarks from 3 on.

Stored (the GPU tests never read the reference): the problem as the reference read it; per retirement the landmark list, the mode, the
three maps, the surviving cameras' priors and all beliefs right after it; after every sweep ARE, energy and the number of factors that
relinearised; after each batch's last sweep beliefs, iters_since_relin, eta_damping (and adaptive variances with huber); messages after
the last sweep.  To keep each file below 1 MiB: symmetric matrices as upper triangles, messages for every 6th factor -- no dense copies,
no means.
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
RUNS = dict(small=('fr1desk_small.txt', {}), vsmall_huber=('fr1desk_vsmall.txt', dict(loss='huber')))
MODES = (True, False)                                           # fold, then drop
SAMPLE_MSG = 6
U6, U3 = np.triu_indices(6), np.triu_indices(3)


def beliefs(graph):
    return dict(cam_eta=np.array([n.belief.eta for n in graph.cam_nodes]), cam_lam=np.array([n.belief.lam[U6] for n in graph.cam_nodes]),
                lmk_eta=np.array([n.belief.eta for n in graph.lmk_nodes]), lmk_lam=np.array([n.belief.lam[U3] for n in graph.lmk_nodes]))


def run(tag):
    from gbp import gbp_ba
    from retire_lmk_host import retire_landmarks_graph, pick_first_list
    fname, over = RUNS[tag]
    cfg = default_configs(**over)
    from gbp_amd.balio import read_bal
    path = os.path.join(HERE, 'data', fname)
    graph = gbp_ba.create_ba_graph(path, cfg)
    K = np.asarray(read_bal(path).K, np.float64)
    out = dict(bal=np.array(fname), loss=np.array(str(over.get('loss'))), n_retirements=np.array(len(MODES)), sweeps=np.array(SWEEPS),
               base_K=K, base_cam_means=np.array([n.mu for n in graph.cam_nodes], np.float64),
               base_lmk_means=np.array([n.mu for n in graph.lmk_nodes], np.float64),
               base_meas=np.array([f.measurement for f in graph.factors], np.float64),
               base_cam_idx=np.array([f.adj_var_nodes[0].c_id for f in graph.factors], np.int32),
               base_lmk_idx=np.array([f.adj_var_nodes[1].l_id for f in graph.factors], np.int32))
    graph.generate_priors_var(weaker_factor=cfg['prior_std_weaker_factor'])
    graph.update_all_beliefs()
    are, energy, relins = [], [], []
    for b in range(len(MODES) + 1):
        if b:
            fold = MODES[b - 1]
            deg = np.array([len(n.adj_factors) for n in graph.lmk_nodes])
            if b == 1:
                ids, orphan = pick_first_list(out['base_cam_idx'], out['base_lmk_idx'], len(graph.cam_nodes), len(graph.lmk_nodes))
                assert 0 not in ids and (deg[ids] == deg.min()).any() and len(ids) < len(graph.lmk_nodes)
            else:
                ids, orphan = np.arange(3, len(graph.lmk_nodes), 7, dtype=np.int32), None
            before = {id(n): (n.belief.eta.copy(), n.belief.lam.copy()) for n in graph.cam_nodes + graph.lmk_nodes}
            C_old, L_old = len(graph.cam_nodes), len(graph.lmk_nodes)
            cams, lmks, cm, lm, fm = retire_landmarks_graph(graph, graph.cam_nodes, graph.lmk_nodes, ids, fold)
            graph.cam_nodes[:], graph.lmk_nodes[:] = cams, lmks
            if orphan is not None:
                assert cm[orphan] == -1 and (cm >= 0).sum() == C_old - 1 and orphan != C_old - 1
            gap = max(max(np.abs(n.belief.eta - before[id(n)][0]).max() / np.abs(before[id(n)][0]).max(),
                          np.abs(n.belief.lam - before[id(n)][1]).max() / np.abs(before[id(n)][1]).max()) for n in cams + lmks)
            print(f'{tag} retirement {b} ({"fold" if fold else "drop"}): {len(ids)} landmarks listed ({int((deg[ids] == deg.min()).sum())} of the lowest degree, {int(deg.min())}), '
                  f'{int((fm < 0).sum())} factors, {C_old - len(cams)} cameras and {L_old - len(lmks)} landmarks gone, '
                  f'surviving beliefs moved by {gap:.1e} (relative)')
            out[f'r{b}_lmk_ids'], out[f'r{b}_fold'] = ids, np.array(int(fold))
            out[f'r{b}_cam_map'], out[f'r{b}_lmk_map'], out[f'r{b}_factor_map'] = cm, lm, fm
            out[f'r{b}_cam_prior_eta'] = np.array([n.prior.eta for n in cams])
            out[f'r{b}_cam_prior_lam'] = np.array([n.prior.lam[U6] for n in cams])
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
    save(f'G20_retire_lmk_{tag}', **out)


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
