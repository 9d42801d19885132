#!/usr/bin/env python3
"""Generate fixture G17 (a BA graph that GROWS by keyframes) by driving the reference's own classes.

    python tests/golden/make_g17.py [--reference /root/reference] [--only small,vsmall_huber]

Like make_golden.py this runs where the reference is mounted read-only and copies nothing of it: the base graph comes from the
reference's create_ba_graph on a BAL file written here, and every growth step is done with the reference's classes the way a SLAM
front end would grow the graph (gbp_ba.py:114-141):
  FrameVariableNode / LandmarkVariableNode with mu set; per observation a ReprojectionFactor and
  compute_factor(linpoint = concat(cam.mu, lmk.mu)); appends to both nodes' adj_factors; graph.factors kept in create_ba_graph's
  order of the union (camera-major, old factors before new ones inside a camera); generate_priors_var's loop (gbp_ba.py:20-34) over
  the NEW nodes only; update_all_beliefs().
Schedule: the base follows ba.py (prior_std_weaker_factor 50, iters_since_relin reset to 1 before sweeps 3 and 8) for 10 sweeps, then
every batch is followed by 10 plain sweeps.  Batch 2 also carries about 5 % of the base cameras' observations that were held back from
the base (observations of old cameras arrive late: old factor ids move).

Stored (the GPU tests never read the reference): the base problem and every batch (union numbering); after each extend all beliefs,
old_to_new and the new factors' eta_f / Lambda_f / linpoint; after every sweep ARE, energy and the number of factors that relinearised;
after each batch's last sweep beliefs, iters_since_relin, eta_damping (and adaptive variances with huber); messages after the last sweep.
To keep each file below 1 MiB: symmetric matrices as upper triangles, landmark Lambda after an extend for the new landmarks only, eta_f /
Lambda_f for every 16th new factor, messages for every 6th factor.
"""
import argparse
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

from make_golden import default_configs, save      # noqa: E402

SWEEPS = 10
RUNS = dict(small=('fr1desk_small.txt', (8, 3, 3, 3, 3), {}),          # 20 keyframes: base 0-7, four batches of 3
            vsmall_huber=('fr1desk_vsmall.txt', (4, 2, 2, 2), dict(loss='huber')))     # 10 keyframes: base 0-3, three batches of 2
HOLD_BACK = 0.05
SAMPLE_NEW, SAMPLE_MSG = 16, 6      # every 16th new factor's eta_f / Lambda_f, every 6th factor's messages (one file stays below 1 MiB)
U6, U3, U9 = np.triu_indices(6), np.triu_indices(3), np.triu_indices(9)     # symmetric matrices: upper triangles, row-major


def beliefs(graph, lmk_lam_from=0):
    """eta and packed Lambda of every camera and landmark (landmark Lambda only from landmark `lmk_lam_from` on)."""
    return dict(cam_eta=np.array([n.belief.eta for n in graph.cam_nodes]), cam_lam=np.array([n.belief.lam[U6] for n in graph.cam_nodes]),
                lmk_eta=np.array([n.belief.eta for n in graph.lmk_nodes]),
                lmk_lam=np.array([n.belief.lam[U3] for n in graph.lmk_nodes[lmk_lam_from:]]).reshape(-1, 6))


def split(path, sizes, seed=17):
    """Base problem and batches (gbp_amd.synthetic.keyframe_batches); then ~5 % of the base cameras' observations -- never a landmark's
    first one -- are moved from the base to the end of batch 2."""
    from gbp_amd.balio import read_bal
    from gbp_amd.synthetic import keyframe_batches, BAProblem
    sp = keyframe_batches(read_bal(path), list(sizes))
    base, batches = sp.base, [dict(b) for b in sp.batches]
    rng = np.random.default_rng(seed)
    first = np.zeros(base.n_factors, bool)
    first[np.unique(base.lmk_idx, return_index=True)[1]] = True
    hold = (~first) & (rng.random(base.n_factors) < HOLD_BACK)
    b2 = batches[1]
    for k, src in (('meas', base.meas), ('cam_idx', base.cam_idx), ('lmk_idx', base.lmk_idx)):
        b2[k] = np.concatenate([b2[k], src[hold]])
    base = BAProblem(K=base.K, cam_means=base.cam_means, lmk_means=base.lmk_means, meas=base.meas[~hold], cam_idx=base.cam_idx[~hold],
                     lmk_idx=base.lmk_idx[~hold])
    return base, batches, int(hold.sum())


def grow(gbp_ba, graph, batch, cfg, K):
    """The reference graph after the batch's appends, the new nodes' priors and update_all_beliefs.  Returns old_to_new."""
    vid = 1 + max(v.variableID for v in graph.cam_nodes + graph.lmk_nodes)
    new_nodes = []
    for mu in batch['cam_means']:
        n = gbp_ba.FrameVariableNode(vid, 6, len(graph.cam_nodes))
        n.mu = np.array(mu, dtype=np.float64)
        graph.cam_nodes.append(n)
        new_nodes.append(n)
        vid += 1
    for mu in batch['lmk_means']:
        n = gbp_ba.LandmarkVariableNode(vid, 3, len(graph.lmk_nodes))
        n.mu = np.array(mu, dtype=np.float64)
        graph.lmk_nodes.append(n)
        new_nodes.append(n)
        vid += 1
    new = []
    for z, c, l in zip(batch['meas'], batch['cam_idx'], batch['lmk_idx']):
        cam_node, lmk_node = graph.cam_nodes[int(c)], graph.lmk_nodes[int(l)]
        f = gbp_ba.ReprojectionFactor(-1, [cam_node, lmk_node], np.array(z, dtype=np.float64), cfg['gauss_noise_std'], cfg['loss'],
                                      cfg['Nstds'], K)
        f.compute_factor(np.concatenate((cam_node.mu, lmk_node.mu)))
        cam_node.adj_factors.append(f)
        lmk_node.adj_factors.append(f)
        new.append(f)
    old = list(graph.factors)
    cam_of = np.array([f.adj_var_nodes[0].c_id for f in old + new])
    order = np.argsort(cam_of, kind='stable')                 # create_ba_graph's order of the union (gbp_ba.py:128-130)
    allf = old + new
    graph.factors[:] = [allf[k] for k in order]
    for fid, f in enumerate(graph.factors):
        f.factorID = fid
    pos = np.empty(order.size, np.int64)
    pos[order] = np.arange(order.size)
    for var_node in new_nodes:                                # generate_priors_var's loop body, new nodes only
        max_factor_lam = 0.
        for factor in var_node.adj_factors:
            max_factor_lam = max(max_factor_lam, np.max(factor.factor.lam))
        lam_prior = np.eye(var_node.dofs) * max_factor_lam / (cfg['prior_std_weaker_factor'] ** 2)
        var_node.prior.lam = lam_prior
        var_node.prior.eta = lam_prior @ var_node.mu
    graph.var_nodes = graph.cam_nodes + graph.lmk_nodes
    graph.n_var_nodes, graph.n_factor_nodes, graph.n_edges = len(graph.var_nodes), len(graph.factors), 2 * len(graph.factors)
    graph.update_all_beliefs()
    return pos[:len(old)].astype(np.int32), np.sort(pos[len(old):]).astype(np.int32)


def run(tag):
    from gbp import gbp_ba
    from gbp_amd.synthetic import write_bal
    fname, sizes, over = RUNS[tag]
    cfg = default_configs(**over)
    base, batches, held = split(os.path.join(HERE, 'data', fname), sizes)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'base.txt')
        write_bal(base, path, header='G17 base')
        graph = gbp_ba.create_ba_graph(path, cfg)
    K = np.array([[base.K[0], 0.0, base.K[2]], [0.0, base.K[1], base.K[3]], [0.0, 0.0, 1.0]])
    out = dict(bal=np.array(fname), loss=np.array(str(over.get('loss'))), n_batches=np.array(len(batches)), sweeps=np.array(SWEEPS),
               held_back=np.array(held), base_K=np.asarray(base.K, np.float64),                # the base as the reference read it:
               base_cam_means=np.array([n.mu for n in graph.cam_nodes], np.float64),            # (reference order = file order here)
               base_lmk_means=np.array([n.mu for n in graph.lmk_nodes], np.float64),
               base_meas=np.array([f.measurement for f in graph.factors], np.float64),
               base_cam_idx=np.array([f.adj_var_nodes[0].c_id for f in graph.factors], np.int32),
               base_lmk_idx=np.array([f.adj_var_nodes[1].l_id for f in graph.factors], np.int32))
    graph.generate_priors_var(weaker_factor=cfg['prior_std_weaker_factor'])
    graph.update_all_beliefs()
    are, energy, relins = [], [], []
    for b in range(len(batches) + 1):
        if b:
            batch = batches[b - 1]
            for k in ('cam_means', 'lmk_means', 'meas'):
                out[f'b{b}_{k}'] = np.asarray(batch[k], np.float64)
            for k in ('cam_idx', 'lmk_idx'):
                out[f'b{b}_{k}'] = np.asarray(batch[k], np.int32)
            L_old = len(graph.lmk_nodes)
            o2n, new_ids = grow(gbp_ba, graph, batch, cfg, K)
            out[f'b{b}_old_to_new'] = o2n
            out[f'b{b}_new_ids'] = new_ids
            out[f'b{b}_new_linpoint'] = np.array([np.asarray(graph.factors[i].linpoint, np.float64) for i in new_ids])
            some = new_ids[::SAMPLE_NEW]
            out[f'b{b}_sampled_ids'] = some
            out[f'b{b}_new_factor_eta'] = np.array([graph.factors[i].factor.eta for i in some])
            out[f'b{b}_new_factor_lam'] = np.array([graph.factors[i].factor.lam[U9] for i in some])
            for name, arr in beliefs(graph, lmk_lam_from=L_old).items():       # (landmark Lambda: the new landmarks only)
                out[f'b{b}_ext_{name}'] = arr
        for i in range(SWEEPS):
            if b == 0 and i in (3, 8):                         # ba.py:91-93
                for f in graph.factors:
                    f.iters_since_relin = 1
            graph.synchronous_iteration(robustify=True, local_relin=True)
            are.append(graph.are())
            energy.append(graph.energy())
            relins.append(sum(1 for f in graph.factors if f.iters_since_relin == 0))
        for name, arr in beliefs(graph).items():
            out[f'b{b}_end_{name}'] = arr
        out[f'b{b}_end_iters_since_relin'] = np.array([f.iters_since_relin for f in graph.factors], np.int32)
        out[f'b{b}_end_eta_damping'] = np.array([f.eta_damping for f in graph.factors], np.float64)
        if over.get('loss'):
            out[f'b{b}_end_adaptive_var'] = np.array([f.adaptive_gauss_noise_var for f in graph.factors], np.float64)
    fs = graph.factors[::SAMPLE_MSG]
    out['msg_cam_eta'] = np.array([f.messages[0].eta for f in fs])
    out['msg_cam_lam'] = np.array([f.messages[0].lam[U6] for f in fs])
    out['msg_lmk_eta'] = np.array([f.messages[1].eta for f in fs])
    out['msg_lmk_lam'] = np.array([f.messages[1].lam[U3] for f in fs])
    out['are'], out['energy'], out['n_relin'] = np.array(are), np.array(energy), np.array(relins, np.int32)
    save(f'G17_grow_{tag}', **out)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default='/root/reference')
    ap.add_argument('--only', default='')
    args = ap.parse_args()
    sys.path.insert(0, args.reference)
    import warnings
    warnings.simplefilter('ignore', SyntaxWarning)
    for t in [s for s in args.only.split(',') if s] or list(RUNS):
        run(t)
