#!/usr/bin/env python3
"""Throughput of the linear pairwise GBP engine (include/gbp_lin.h) on a large synthetic pose graph (secondary path;
the headline benchmark is bench.py).  Variables on a ring, each joined to its next `k` neighbours by a
linear_displacement factor (gbp/factors/linear_displacement.py:8-14).  Prints one JSON line.

Algorithmic bytes per sweep (fp64, packed symmetric, P = d(d+1)/2): per factor read Lambda_f d(2d+1) + eta_f 2d +
two belief records 2(d+P) + two old messages 2(d+P), write two messages 2(d+P), and the belief stage reads them again
2(d+P); per variable prior d+P read, d+P+d written."""
import argparse, json, os, statistics, sys, time
import numpy as np
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from gbp_amd.linear import LinearEngine

ap = argparse.ArgumentParser()
ap.add_argument('--vars', type=int, default=200_000)
ap.add_argument('--dofs', type=int, default=3)
ap.add_argument('--k', type=int, default=5)
ap.add_argument('--steps', type=int, default=100)
ap.add_argument('--warmup', type=int, default=10)
ap.add_argument('--no-cpu-baseline', action='store_true')
ap.add_argument('--map', action='store_true', help='after the timed sweeps, solve the batch MAP (cold) and report the distance of the means from it')
ap.add_argument('--marginals', action='store_true',
                help='instead of the run above: on the two 1M-factor graphs (the defaults, and --vars 1000000 --k 1) time one multi-column CG iteration '
                     'of gbp_lin_solve_marginals (8 columns) against one of gbp_lin_solve_map, and the sweeps, in one session; writes profiles/linear_marginals.json')
ap.add_argument('--robust', action='store_true',
                help='instead of the run above: on the same two graphs with 10 %% outlier measurements time iterate(n, robustify=True) (huber, threshold 2) '
                     'against the plain iterate(n) of a handle without losses, alternating; writes profiles/linear_robust.json')
ap.add_argument('--extend', action='store_true',
                help='instead of the run above: on the 200k x 3 ring (k = 5, 1M factors) time one extend by 1000 variables and 5000 factors against '
                     'gbp_lin_create of the grown graph, alternating, and the sweeps of the grown handle against one created whole; writes profiles/linear_extend.json')
ap.add_argument('--shrink', action='store_true',
                help='instead of the run above: on the 200k x 3 ring (k = 5, 1M factors) time one shrink retiring the 1000 lowest-numbered variables (folded) '
                     "against gbp_lin_create of the survivors' graph, alternating, and the sweeps of the shrunk handle against the created one; writes profiles/linear_shrink.json")
ap.add_argument('--until', action='store_true',
                help='instead of the run above: on the same two graphs time iterate_until(n) (tolerances off; no column, the energy column, both columns) '
                     'against iterate(n) on the same handle and against the host loop iterate(1); energy(); map_distance(), alternating; writes profiles/linear_until.json')
ap.add_argument('--nonlinear', action='store_true',
                help='instead of the run above: the same two graphs re-posed as SE(2) pose graphs; time iterate(n, relinearise=True) with beta = +inf and with '
                     'beta = 0 against iterate(n) on the same handle, and one host relinearisation + gbp_lin_create against iterate(1, relinearise=True); '
                     'writes profiles/linear_nonlinear.json')
ap.add_argument('--nonlinear-live', action='store_true',
                help='time gbp_lin_extend_nonlinear (+1000 poses, +5000 factors) and gbp_lin_shrink_nonlinear (the 1000 oldest poses, folded) against '
                     're-creating the handle (gbp_lin_create + gbp_lin_set_nonlinear) and against the linear extend / shrink, and the nonlinear sweep '
                     'against --parent-lib; writes profiles/linear_nonlinear_live.json')
ap.add_argument('--nonlinear-robust', action='store_true',
                help='time the robust relinearising sweep (gbp_lin_iterate_nonlinear_robust) against gbp_lin_iterate_nonlinear on the two graphs of '
                     '--nonlinear, fused and with robustify as a launch of its own, and the sweeps without losses against --parent-lib; writes '
                     'profiles/linear_nonlinear_robust.json')
ap.add_argument('--nonlinear-until', action='store_true',
                help='ms per sweep of iterate_until_nonlinear (plain, with the energy column, with both columns) against iterate_nonlinear and the host '
                     'loop iterate(1, relinearise=True); energy(), at beta = +inf and beta = 0; with --parent-lib the older sweeps against the parent '
                     "commit's library; writes profiles/linear_nonlinear_until.json")
ap.add_argument('--nonlinear-se3', action='store_true',
                help='ms per sweep of the SE(3) relinearising sweeps (beta = +inf, beta = 0, robust) against the plain d = 6 gbp_lin_iterate on the same '
                     'handle, on a 100k x 6 ring (k = 5) and a 500k-pose chain (k = 1) re-posed as SE(3), and the SE(2) nonlinear sweep against '
                     '--parent-lib; writes profiles/linear_nonlinear_se3.json')
ap.add_argument('--nonlinear-map', action='store_true',
                help='time per outer iteration of gbp_lin_solve_map_nonlinear (Levenberg-Marquardt on the device) on the SE(3) ring and chain, beside its counted '
                     'bytes and its two nearest existing pieces: the relinearise kernel of an all-relinearising sweep and a gbp_lin_solve_map of the same CG '
                     'iteration count; writes profiles/linear_nonlinear_map.json')
ap.add_argument('--nonlinear-map-robust', action='store_true',
                help='gbp_lin_solve_map_nonlinear_robust on the graphs of --nonlinear-map: one reweight launch against the linearise launch of the parent '
                     "commit's gbp_lin_solve_map_nonlinear, a full robust solve with 5 %% of the closures corrupted, and the existing paths against "
                     '--parent-lib (required); writes profiles/linear_nonlinear_map_robust.json')
ap.add_argument('--model-cost', action='store_true',
                help='the kernels that evaluate the SE(3) / SE(2) models (relinearise, energy, the Gauss-Newton linearise and reweight calls, a sweep) '
                     'of this library against --parent-lib (required), alternating; prints one JSON line')
ap.add_argument('--parent-lib', default=None, help="--nonlinear-live / --nonlinear-robust / --nonlinear-until: the parent commit's libgbp_hip.so, loaded beside this one for the yardsticks")
ap.add_argument('--parent-results', default=None,
                help="--extend / --shrink / --until / --nonlinear: a file of lines 'parent {json}' / 'here {json}', each the JSON line of a plain run of this tool from the parent "
                     "commit's tree or from this one (run alternating, in the same session); summarised per workload under sweeps_per_s_vs_parent")
ap.add_argument('--repeats', type=int, default=5, help='--marginals / --robust / --extend: repeats per timing (the median is reported)')
a = ap.parse_args()


def ring(N, D, k, rs):
    mu0 = rs.rand(N, D) * 10
    va = np.repeat(np.arange(N), k)
    vb = (va + np.tile(np.arange(1, k + 1), N)) % N
    z = mu0[vb] - mu0[va] + rs.normal(0, 1.0, (va.shape[0], D))
    J = np.hstack([-np.eye(D), np.eye(D)])
    return (va, vb, z @ J, np.ascontiguousarray(np.broadcast_to(J.T @ J, (va.shape[0], 2 * D, 2 * D))), mu0 / 3.0,
            np.ascontiguousarray(np.broadcast_to(np.eye(D) / 3.0, (N, D, D)))), 0.5 * np.einsum('fd,fd->f', z, z)


def marginals_profile():
    """Host clock around DIRECT calls of the two C entry points, each of which ends in a stream synchronise (no device events in the
    ABI); every figure is the median of --repeats calls after a warm-up call of the same shape, the two solvers alternating.
    gbp_lin_solve_map is timed by itself: no download of the solution.  gbp_lin_solve_marginals is one batch (2 ids x 3 dofs = 6 live
    columns and 2 zero ones, which run the same instructions) and brings back 18 doubles; its staging buffer exists after the warm-up,
    so a timed call allocates nothing.
    Two figures per solver.  per_iter: the difference between a solve cut at max_iters = 40 and one cut at 8, over 32 -- four kernels
    per iteration and one read-back of the partial |r|^2 every 8, and nothing else: what both calls do once (the memset of x, the
    first residual, the true-residual product at the end, and for the marginals the gather and the 18-double copy) cancels.
    whole_solve: a solve to rel_tol 1e-12 over its iterations, with all of that in."""
    import ctypes as ct
    from gbp_amd import _capi
    D, runs = 3, []
    lo, hi = 8, 40
    for N, k in ((200_000, 5), (1_000_000, 1)):
        g, fc = ring(N, D, k, np.random.RandomState(0))
        F = g[0].shape[0]
        e = LinearEngine(*g, factor_const=fc)
        e.update_all_beliefs()
        e.iterate(a.warmup); e.sync()
        ids, sigma = _capi.i32([N // 3, 7]), np.zeros((2, D, D))

        def sweeps():
            t = time.perf_counter(); e.iterate(a.steps); e.sync()
            return (time.perf_counter() - t) / a.steps

        def single(max_iters):
            o, i = _capi.LinMapOpts(1e-12, max_iters, 8, 0), _capi.LinMapInfo()
            t = time.perf_counter(); rc = e._lib.gbp_lin_solve_map(e._h, ct.byref(o), ct.byref(i)); t = time.perf_counter() - t
            _capi.check(rc)
            return t, i

        def multi(max_iters):
            o, i = _capi.LinMapOpts(1e-12, max_iters, 8, 0), _capi.LinMargInfo()
            t = time.perf_counter()
            rc = e._lib.gbp_lin_solve_marginals(e._h, _capi.iptr(ids), 2, ct.byref(o), _capi.dptr(sigma), None, ct.byref(i))
            t = time.perf_counter() - t
            _capi.check(rc)
            return t, i
        single(10000); multi(10000)                         # workspaces, LDL^T, staging, code objects
        sw0 = [sweeps() for _ in range(a.repeats)]
        rec = {key: [] for key in ('s_lo', 's_hi', 's_full', 'm_lo', 'm_hi', 'm_full')}
        for _ in range(a.repeats):                          # alternating
            for key, fn, n in (('s_lo', single, lo), ('m_lo', multi, lo), ('s_hi', single, hi), ('m_hi', multi, hi),
                               ('s_full', single, 10000), ('m_full', multi, 10000)):
                t, i = fn(n)
                assert i.iters == n or n == 10000, (key, i.iters)
                rec[key].append((t, i.iters))
            i1, i8 = rec['s_full'][-1][1], rec['m_full'][-1][1]
        conv = single(10000)[1].converged, multi(10000)[1]
        med = {key: statistics.median(t for t, _ in v) for key, v in rec.items()}
        t_single, t_multi = (med['s_hi'] - med['s_lo']) / (hi - lo), (med['m_hi'] - med['m_lo']) / (hi - lo)
        w_single, w_multi = med['s_full'] / i1, med['m_full'] / i8
        sw1 = [sweeps() for _ in range(a.repeats)]
        runs.append({"vars": N, "dofs": D, "k": k, "factors": F,
                     "per_iter": {"ms_map": 1e3 * t_single, "ms_marginals_8_columns": 1e3 * t_multi, "ratio_per_column": t_multi / (8.0 * t_single),
                                  "cut_at_iterations": [lo, hi],
                                  "ms_solve_map_cut": {str(lo): [1e3 * t for t, _ in rec['s_lo']], str(hi): [1e3 * t for t, _ in rec['s_hi']]},
                                  "ms_solve_marginals_cut": {str(lo): [1e3 * t for t, _ in rec['m_lo']], str(hi): [1e3 * t for t, _ in rec['m_hi']]}},
                     "whole_solve": {"ms_map_per_iter": 1e3 * w_single, "map_iters": i1, "map_converged": bool(conv[0]),
                                     "ms_marginals_per_iter_8_columns": 1e3 * w_multi, "marginals_iters": i8, "marginals_converged": bool(conv[1].converged),
                                     "marginals_rel_residual": conv[1].rel_residual, "ratio_per_column": w_multi / (8.0 * w_single),
                                     "ms_solve_map": [1e3 * t for t, _ in rec['s_full']], "ms_solve_marginals": [1e3 * t for t, _ in rec['m_full']]},
                     "ratio_derived_from_factor_traffic": traffic_ratio(D, 0.0), "ratio_derived_with_variable_traffic": traffic_ratio(D, 1.0 / k),
                     "sweeps_per_s_before": 1.0 / statistics.median(sw0), "sweeps_per_s_after": 1.0 / statistics.median(sw1),
                     "sweeps_per_s_all": [1.0 / t for t in sw0 + sw1]})
        e.close()
    out = {"what": "tools/bench_linear.py --marginals on one MI355X: one iteration of gbp_lin_solve_marginals (8 columns at a time) against one of "
                   "gbp_lin_solve_map, and gbp_lin_iterate before and after, in one session; ratio_per_column = t_multi / (8 t_single)",
           "method": " ".join(marginals_profile.__doc__.split()), "traffic": " ".join(traffic_ratio.__doc__.split()),
           "repeats": a.repeats, "sweep_steps": a.steps, "runs": runs}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'linear_marginals.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


def traffic_ratio(D, vars_per_factor):
    """Doubles moved per factor and iteration, 8 columns together over 8 single solves.  Per factor: Lambda_f d(2d+1), read once by
    either; per column the gather of p 2d, the edge buffer written and read 4d.  Per variable (vars_per_factor = N / F; 0 leaves this
    part out, which is the bound of the design): per column p, q in the product, x, r, p, q read and x, r, z written in the step, z, p
    read and p written in the direction: 12d; shared by the columns: the prior block d(d+1)/2 and the LDL^T d(d+1)/2 + d."""
    P = D * (D + 1) // 2
    lam, col = D * (2 * D + 1), 6 * D + vars_per_factor * 12 * D
    shared = vars_per_factor * (2 * P + D)
    return (lam + shared + 8 * col) / (8.0 * (lam + shared + col))


def sweep_doubles(D, vars_per_factor, robust):
    """Doubles moved per factor and sweep (the module docstring's count).  A robust sweep adds k_lin_robustify, which re-reads Lambda_f
    d(2d+1), eta_f 2d and the two means 2d, reads const_f, the threshold and the noise variance 3 and the loss code (4 bytes), writes
    the weight 1 and the flag (4 bytes); and k_lin_factor<D, true> reads the weight 1."""
    P = D * (D + 1) // 2
    plain = D * (2 * D + 1) + 2 * D + 8 * (D + P) + vars_per_factor * (2 * (D + P) + D)
    return plain + (D * (2 * D + 1) + 4 * D + 3 + 0.5 + 1 + 0.5 + 1 if robust else 0)


def robust_profile():
    """Host clock around iterate(steps) + sync on two handles of the same graph (one without losses: k_lin_factor<D, false>; one with the
    huber loss, threshold 2, on every factor: k_lin_robustify + k_lin_factor<D, true> per sweep), after a warm-up of both; --repeats
    alternating runs, medians reported.  Every tenth measurement is 20 sigma off, so that the robust branch of the weight is taken."""
    D, runs = 3, []
    for N, k in ((200_000, 5), (1_000_000, 1)):
        rs = np.random.RandomState(0)
        (va, vb, fe, fl, pe, pl), _ = ring(N, D, k, rs)
        F = va.shape[0]
        J = np.hstack([-np.eye(D), np.eye(D)])
        z = fe @ J.T / 2.0                                  # J J^T = 2 I: the measurements back from eta_f = J^T z
        z[::10] += 20.0
        fe, fc = z @ J, 0.5 * np.einsum('fd,fd->f', z, z)
        plain, rob = LinearEngine(va, vb, fe, fl, pe, pl, factor_const=fc), LinearEngine(va, vb, fe, fl, pe, pl, factor_const=fc)
        rob.set_robust('huber', 2.0)
        for e, r in ((plain, False), (rob, True)):
            e.update_all_beliefs()
            e.iterate(a.warmup, robustify=r); e.sync()

        def timed(e, r):
            t = time.perf_counter(); e.iterate(a.steps, robustify=r); e.sync()
            return 1e3 * (time.perf_counter() - t) / a.steps
        tp, tr = [], []
        for _ in range(a.repeats):                          # alternating
            tp.append(timed(plain, False)); tr.append(timed(rob, True))
        w, flag = rob.weights()
        bp, br = sweep_doubles(D, 1.0 / k, False), sweep_doubles(D, 1.0 / k, True)
        mp, mr = statistics.median(tp), statistics.median(tr)
        runs.append({"vars": N, "dofs": D, "k": k, "factors": F, "ms_per_plain_sweep": mp, "ms_per_robust_sweep": mr, "ratio_measured": mr / mp,
                     "doubles_per_factor_plain": bp, "doubles_per_factor_robust": br, "ratio_counted_bytes": br / bp,
                     "plain_sweeps_per_s": 1e3 / mp, "robust_factors": int(flag.sum()), "min_weight": float(w.min()),
                     "ms_plain_all": tp, "ms_robust_all": tr})
        plain.close(); rob.close()
    out = {"what": "tools/bench_linear.py --robust on one MI355X: ms per sweep of iterate(n, robustify=True) against iterate(n) of a handle without "
                   "losses, on the 200k x 3 ring (k = 5) and the 1M-variable chain (k = 1)",
           "method": " ".join(robust_profile.__doc__.split()), "traffic": " ".join(sweep_doubles.__doc__.split()),
           "repeats": a.repeats, "sweep_steps": a.steps, "runs": runs}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'linear_robust.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


def extend_profile():
    """Host clock, call to gbp_lin_sync.  extend: on a handle of the 200k x 3 ring (k = 5) that has beliefs and 10 sweeps behind it,
    LinearEngine.extend by 1000 variables, each joined to the 5 variables before it (5000 factors), then sync.  re-create: what the
    parent commit offers for the same step, LinearEngine(...) of the grown graph from host arrays already in the ABI's types
    (contiguous float64 / int32), then sync; its messages start at zero again, which is not charged.  --repeats alternating pairs
    after one warm-up pair, medians reported; the base handle of every extend is made outside the clock.  Then iterate(steps) of the
    last grown handle against a handle created at the final size after it and one created at the final size before anything else in the process, alternating, with the spread of each.  --parent-results adds plain runs of this tool from the parent commit's tree and this one."""
    from gbp_amd import _capi
    D, N, k, dN = 3, 200_000, 5, 1000
    rs = np.random.RandomState(0)
    (va, vb, fe, fl, pe, pl), fc = ring(N, D, k, rs)
    mu1 = rs.rand(dN, D) * 10
    na = np.repeat(np.arange(N, N + dN), k)
    nb = na - np.tile(np.arange(1, k + 1), dN)
    mu = np.concatenate([pe * 3.0, mu1])
    z = mu[nb] - mu[na] + rs.normal(0, 1.0, (na.shape[0], D))
    J = np.hstack([-np.eye(D), np.eye(D)])
    nfe, nfl, nfc = z @ J, np.ascontiguousarray(np.broadcast_to(J.T @ J, (na.shape[0], 2 * D, 2 * D))), 0.5 * np.einsum('fd,fd->f', z, z)
    npe, npl = mu1 / 3.0, np.ascontiguousarray(np.broadcast_to(np.eye(D) / 3.0, (dN, D, D)))
    va, vb, na, nb = _capi.i32(va), _capi.i32(vb), _capi.i32(na), _capi.i32(nb)
    whole_args = (np.concatenate([va, na]), np.concatenate([vb, nb]), np.concatenate([fe, nfe]), np.concatenate([fl, nfl]),
                  np.concatenate([pe, npe]), np.concatenate([pl, npl]))
    whole_fc = np.concatenate([fc, nfc])

    first = LinearEngine(*whole_args, factor_const=whole_fc)   # created whole before anything else exists in the process
    first.update_all_beliefs(); first.iterate(a.warmup); first.sync()

    def base():
        e = LinearEngine(va, vb, fe, fl, pe, pl, factor_const=fc)
        e.update_all_beliefs(); e.iterate(a.warmup); e.sync()
        return e

    def timed_extend(e):
        t = time.perf_counter(); e.extend(na, nb, nfe, nfl, npe, npl, factor_const=nfc); e.sync()
        return 1e3 * (time.perf_counter() - t)

    def timed_create():
        t = time.perf_counter(); e = LinearEngine(*whole_args, factor_const=whole_fc); e.sync()
        return 1e3 * (time.perf_counter() - t), e
    t_ext, t_new, grown, whole = [], [], None, None
    for r in range(a.repeats + 1):                          # alternating; the first pair warms up
        e = base()
        te = timed_extend(e)
        tc, w = timed_create()
        if r:
            t_ext.append(te); t_new.append(tc)
        if r == a.repeats:
            grown, whole = e, w
        else:
            e.close(); w.close()
    assert grown.sizes() == (N + dN, va.shape[0] + na.shape[0])
    whole.update_all_beliefs(); whole.iterate(a.warmup); whole.sync()
    grown.iterate(a.warmup); grown.sync()

    def sweeps(e):
        t = time.perf_counter(); e.iterate(a.steps); e.sync()
        return a.steps / (time.perf_counter() - t)
    sg, sw, sf = [], [], []
    for _ in range(a.repeats):
        sg.append(sweeps(grown)); sw.append(sweeps(whole)); sf.append(sweeps(first))
    vs_parent = None
    if a.parent_results:
        runs = {}
        for ln in open(a.parent_results):
            who, js = ln.split(' ', 1)
            r = json.loads(js)
            runs.setdefault(r['config']['workload'], {'parent': [], 'here': []})[who].append(r['value'])
        vs_parent = [{"workload": w, "parent": v['parent'], "here": v['here'], "median_parent": statistics.median(v['parent']),
                      "median_here": statistics.median(v['here']),
                      "spread_parent": (max(v['parent']) - min(v['parent'])) / statistics.median(v['parent']),
                      "spread_here": (max(v['here']) - min(v['here'])) / statistics.median(v['here'])} for w, v in runs.items()]
    me, mc = statistics.median(t_ext), statistics.median(t_new)
    out = {"what": "tools/bench_linear.py --extend on one MI355X: one gbp_lin_extend of the 200k x 3 ring (1M factors) by 1000 variables and 5000 "
                   "factors against gbp_lin_create of the grown graph, and the sweeps of the grown handle against a handle created whole",
           "method": " ".join(extend_profile.__doc__.split()), "repeats": a.repeats, "sweep_steps": a.steps,
           "vars": N, "dofs": D, "factors": int(va.shape[0]), "new_vars": dN, "new_factors": int(na.shape[0]),
           "ms_extend": me, "ms_recreate": mc, "ratio_recreate_over_extend": mc / me, "ms_extend_all": t_ext, "ms_recreate_all": t_new,
           "sweeps_per_s_grown": statistics.median(sg), "sweeps_per_s_created_whole": statistics.median(sw),
           "ratio_grown_over_whole": statistics.median(sg) / statistics.median(sw),
           "spread_grown": (max(sg) - min(sg)) / statistics.median(sg), "spread_whole": (max(sw) - min(sw)) / statistics.median(sw),
           "sweeps_per_s_created_whole_first_in_process": statistics.median(sf), "spread_whole_first": (max(sf) - min(sf)) / statistics.median(sf),
           "sweeps_per_s_grown_all": sg, "sweeps_per_s_whole_all": sw, "sweeps_per_s_whole_first_all": sf,
           "sweeps_per_s_vs_parent": vs_parent}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'linear_extend.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


def shrink_profile():
    """Host clock, call to gbp_lin_sync.  shrink: on a handle of the 200k x 3 ring (k = 5, 1M factors) that has beliefs and 10 sweeps
    behind it, LinearEngine.shrink retiring the 1000 lowest-numbered variables with the fold (the maps are asked for), then sync.
    re-create: what the parent commit offers for the same step, LinearEngine(...) of the survivors' graph from host arrays already in
    the ABI's types, then sync; it loses every message, which is not charged.  --repeats alternating pairs after one warm-up pair,
    medians reported; the base handle of every shrink is made outside the clock.  Then iterate(steps) of the last shrunk handle against
    the handle created at the survivors' size after it, alternating, with the spread of each.  --parent-results adds plain runs of this
    tool from the parent commit's tree and this one."""
    from gbp_amd import _capi
    D, N, k, gone = 3, 200_000, 5, 1000
    rs = np.random.RandomState(0)
    (va, vb, fe, fl, pe, pl), fc = ring(N, D, k, rs)
    va, vb = _capi.i32(va), _capi.i32(vb)
    retire = np.arange(gone, dtype=np.int32)
    keep = (va >= gone) & (vb >= gone)
    surv_args = (_capi.i32(va[keep] - gone), _capi.i32(vb[keep] - gone), np.ascontiguousarray(fe[keep]), np.ascontiguousarray(fl[keep]),
                 np.ascontiguousarray(pe[gone:]), np.ascontiguousarray(pl[gone:]))
    surv_fc = np.ascontiguousarray(fc[keep])

    def base():
        e = LinearEngine(va, vb, fe, fl, pe, pl, factor_const=fc)
        e.update_all_beliefs(); e.iterate(a.warmup); e.sync()
        return e

    def timed_shrink(e):
        t = time.perf_counter(); e.shrink(retire_vars=retire, fold=True); e.sync()
        return 1e3 * (time.perf_counter() - t)

    def timed_create():
        t = time.perf_counter(); e = LinearEngine(*surv_args, factor_const=surv_fc); e.sync()
        return 1e3 * (time.perf_counter() - t), e
    t_shr, t_new, shrunk, created = [], [], None, None
    for r in range(a.repeats + 1):                          # alternating; the first pair warms up
        e = base()
        ts = timed_shrink(e)
        tc, w = timed_create()
        if r:
            t_shr.append(ts); t_new.append(tc)
        if r == a.repeats:
            shrunk, created = e, w
        else:
            e.close(); w.close()
    assert shrunk.sizes() == created.sizes() == (N - gone, int(keep.sum()))
    created.update_all_beliefs(); created.iterate(a.warmup); created.sync()
    shrunk.iterate(a.warmup); shrunk.sync()

    def sweeps(e):
        t = time.perf_counter(); e.iterate(a.steps); e.sync()
        return a.steps / (time.perf_counter() - t)
    ss, sc = [], []
    for _ in range(a.repeats):
        ss.append(sweeps(shrunk)); sc.append(sweeps(created))
    vs_parent = None
    if a.parent_results:
        runs = {}
        for ln in open(a.parent_results):
            who, js = ln.split(' ', 1)
            r = json.loads(js)
            runs.setdefault(r['config']['workload'], {'parent': [], 'here': []})[who].append(r['value'])
        vs_parent = [{"workload": w, "parent": v['parent'], "here": v['here'], "median_parent": statistics.median(v['parent']),
                      "median_here": statistics.median(v['here']),
                      "spread_parent": (max(v['parent']) - min(v['parent'])) / statistics.median(v['parent']),
                      "spread_here": (max(v['here']) - min(v['here'])) / statistics.median(v['here'])} for w, v in runs.items()]
    ms, mc = statistics.median(t_shr), statistics.median(t_new)
    out = {"what": "tools/bench_linear.py --shrink on one MI355X: one gbp_lin_shrink of the 200k x 3 ring (1M factors) retiring its 1000 "
                   "lowest-numbered variables with the fold against gbp_lin_create of the survivors' graph, and the sweeps of the shrunk "
                   "handle against a handle created at the survivors' size",
           "method": " ".join(shrink_profile.__doc__.split()), "repeats": a.repeats, "sweep_steps": a.steps,
           "vars": N, "dofs": D, "factors": int(va.shape[0]), "retired_vars": gone, "factors_left": int(keep.sum()),
           "ms_shrink": ms, "ms_recreate": mc, "ratio_recreate_over_shrink": mc / ms, "ms_shrink_all": t_shr, "ms_recreate_all": t_new,
           "spread_shrink": (max(t_shr) - min(t_shr)) / ms, "spread_recreate": (max(t_new) - min(t_new)) / mc,
           "sweeps_per_s_shrunk": statistics.median(ss), "sweeps_per_s_created": statistics.median(sc),
           "ratio_shrunk_over_created": statistics.median(ss) / statistics.median(sc),
           "spread_shrunk": (max(ss) - min(ss)) / statistics.median(ss), "spread_created": (max(sc) - min(sc)) / statistics.median(sc),
           "sweeps_per_s_shrunk_all": ss, "sweeps_per_s_created_all": sc, "sweeps_per_s_vs_parent": vs_parent}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'linear_shrink.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


def until_profile():
    """Host clock around whole calls on ONE handle per graph, each ending in a stream synchronise, after a warm-up of every form (and a
    solve_map, which the distance column needs); --repeats alternating rounds, medians reported, per sweep.  plain: iterate(steps) +
    sync.  until: iterate_until(steps) with both tolerances off (so all `steps` sweeps run) and check_every = steps (one read of the stop
    word), with no column, with the energy column, and with both.  host_loop: iterate(1); energy(); map_distance() from Python, `steps`
    times, on this same handle and library -- the calls the parent commit offers for the same trace (their device code is unchanged; it
    has no step column, which would add a get_means download per sweep); it was NOT timed on a build of the parent commit.
    Counted, beside each ratio: a traced sweep reads the old mean (d doubles per variable) and writes one partial per belief block
    (1 / VPW doubles per variable, VPW = 64 / (d + P)), and adds one kernel boundary (the finishing kernel) priced at 3.2 us; the energy
    column adds one pass over the factors (Lambda_f d(2d+1), eta_f 2d, const 1, two means 2d doubles per factor) and one more boundary;
    the distance column adds the MAP iterate (d doubles per variable) and one more partial."""
    D, runs, boundary_ms = 3, [], 3.2e-3
    P = D * (D + 1) // 2
    for N, k in ((200_000, 5), (1_000_000, 1)):
        g, fc = ring(N, D, k, np.random.RandomState(0))
        F = g[0].shape[0]
        e = LinearEngine(*g, factor_const=fc)
        e.update_all_beliefs()
        e.iterate(a.warmup); e.sync()
        e.solve_map()
        n = a.steps

        def plain():
            t = time.perf_counter(); e.iterate(n); e.sync()
            return 1e3 * (time.perf_counter() - t) / n

        def until(energy, dist):
            t = time.perf_counter(); r = e.iterate_until(n, energy=energy, map_distance=dist, check_every=n); t = time.perf_counter() - t
            assert r.iters == n and not r.converged
            return 1e3 * t / n

        def host_loop():
            t = time.perf_counter()
            for _ in range(n):
                e.iterate(1); e.energy(); e.map_distance()
            return 1e3 * (time.perf_counter() - t) / n
        plain(); until(False, False); until(True, True); host_loop()
        rec = {key: [] for key in ('plain', 'until', 'until_energy', 'until_both', 'host_loop')}
        for _ in range(a.repeats):                          # alternating
            rec['plain'].append(plain()); rec['until'].append(until(False, False)); rec['until_energy'].append(until(True, False))
            rec['until_both'].append(until(True, True)); rec['host_loop'].append(host_loop())
        med = {key: statistics.median(v) for key, v in rec.items()}
        spread = {key: (max(v) - min(v)) / med[key] for key, v in rec.items()}
        per_f = sweep_doubles(D, 1.0 / k, False)
        vpw = 64 // (D + P)
        extra_trace = (D + 1.0 / vpw) / k                   # doubles per factor
        extra_energy = D * (2 * D + 1) + 2 * D + 1 + 2 * D
        extra_dist = (D + 1.0 / vpw) / k
        counted = lambda extra, boundaries: (per_f + extra) / per_f + boundaries * boundary_ms / med['plain']
        runs.append({"vars": N, "dofs": D, "k": k, "factors": F, "ms_per_sweep": med, "spread": spread, "ms_all": rec,
                     "ratio_until_over_plain": med['until'] / med['plain'], "ratio_counted": counted(extra_trace, 1),
                     "ratio_until_energy_over_plain": med['until_energy'] / med['plain'], "ratio_energy_counted": counted(extra_trace + extra_energy, 2),
                     "ratio_until_both_over_plain": med['until_both'] / med['plain'], "ratio_both_counted": counted(extra_trace + extra_energy + extra_dist, 2),
                     "ratio_host_loop_over_until_both": med['host_loop'] / med['until_both'],
                     "doubles_per_factor_plain": per_f, "extra_doubles_per_factor": {"trace": extra_trace, "energy": extra_energy, "distance": extra_dist},
                     "kernel_boundary_ms_assumed": boundary_ms})
        e.close()
    vs_parent = None
    if a.parent_results:
        by = {}
        for ln in open(a.parent_results):
            who, js = ln.split(' ', 1)
            r = json.loads(js)
            by.setdefault(r['config']['workload'], {'parent': [], 'here': []})[who].append(r['value'])
        vs_parent = [{"workload": w, "parent": v['parent'], "here": v['here'], "median_parent": statistics.median(v['parent']),
                      "median_here": statistics.median(v['here']),
                      "spread_parent": (max(v['parent']) - min(v['parent'])) / statistics.median(v['parent']),
                      "spread_here": (max(v['here']) - min(v['here'])) / statistics.median(v['here'])} for w, v in by.items()]
    out = {"what": "tools/bench_linear.py --until on one MI355X: ms per sweep of gbp_lin_iterate_until (tolerances off) against gbp_lin_iterate on the same "
                   "handle and against the host loop it replaces, on the 200k x 3 ring (k = 5) and the 1M-variable chain (k = 1)",
           "method": " ".join(until_profile.__doc__.split()), "repeats": a.repeats, "sweep_steps": a.steps, "runs": runs,
           "sweeps_per_s_vs_parent": vs_parent}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'linear_until.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


def se2_graph(N, k, rs):
    """N poses on a circle of radius N / 20 (about 0.3 between neighbours), headings unwrapped over one turn, each joined to its next k
    neighbours (the closing ones measure minus a turn of heading: nothing is wrapped); sqrt information (10, 10, 20), noise to match;
    priors sigma (1, 1, 0.5) at truth + N(0, (0.1, 0.1, 0.03))."""
    th = np.arange(N) * 2 * np.pi / N
    R = N / 20.0
    truth = np.stack([R * np.cos(th), R * np.sin(th), th + np.pi / 2], 1)
    va = np.repeat(np.arange(N), k)
    vb = (va + np.tile(np.arange(1, k + 1), N)) % N
    s = np.tile(np.array([10.0, 10.0, 20.0]), (va.shape[0], 1))
    z = se2_h(np.concatenate([truth[va], truth[vb]], 1), np.ones_like(s)) + rs.normal(0, 1, s.shape) / s
    pl = np.ascontiguousarray(np.broadcast_to(np.diag([1.0, 1.0, 4.0]), (N, 3, 3)))
    pe = np.einsum('nij,nj->ni', pl, truth + rs.normal(0, 1, (N, 3)) * np.array([0.1, 0.1, 0.03]))
    return va.astype(np.int32), vb.astype(np.int32), z, s, pe, pl


def se2_h(x, s):
    c, sn = np.cos(x[:, 2]), np.sin(x[:, 2])
    dx, dy = x[:, 3] - x[:, 0], x[:, 4] - x[:, 1]
    return s * np.stack([c * dx + sn * dy, -sn * dx + c * dy, x[:, 5] - x[:, 2]], 1)


def se2_host_factors(x, z, s):
    """What a caller does today: eta_f, Lambda_f of every factor at x (F, 6), vectorised numpy (gbp.py:280-289)."""
    c, sn = np.cos(x[:, 2]), np.sin(x[:, 2])
    dx, dy = x[:, 3] - x[:, 0], x[:, 4] - x[:, 1]
    o, l = np.zeros_like(c), np.ones_like(c)
    J = s[:, :, None] * np.stack([np.stack([-c, -sn, -sn * dx + c * dy, c, sn, o], 1), np.stack([sn, -c, -c * dx - sn * dy, -sn, c, o], 1),
                                  np.stack([o, o, -l, o, o, l], 1)], 1)
    b = np.einsum('fki,fi->fk', J, x) + s * z - se2_h(x, s)
    return np.einsum('fki,fk->fi', J, b), np.einsum('fki,fkj->fij', J, J)


def nonlinear_profile():
    """Host clock around whole calls, each ending in a stream synchronise, after a warm-up of every form; --repeats alternating rounds of
    --steps sweeps, medians reported per sweep, spread = (max - min) / median.  (a) on ONE handle with beta = +inf: iterate(n) against
    iterate(n, relinearise=True), where the relinearise stage runs and relinearises nothing.  (b) a second handle with beta = 0 and
    min_linear_iters = 0, where every factor relinearises in every sweep.  (c) what a caller has without this path: the means downloaded,
    every factor re-made on the host in vectorised numpy, gbp_lin_create of the graph and the belief stage -- against
    iterate(1, relinearise=True) on the handle of (b); the host figure loses every message besides.
    Counted beside (a): per factor the stage gathers two means (6 doubles), reads the linpoint (6) and iters (0.5), writes iters (0.5), and
    the factor stage reads the factor's damping (1): 14 doubles on top of the plain sweep's count, plus one kernel boundary priced at
    3.2 us.  (b) adds the measurement and square-root information read (6) and eta_f, Lambda_f and the linpoint written (33).  The counts
    are of algorithmic bytes, not of what the caches fetch (gathers fetch whole lines): an excess of the measured ratio over the counted
    one is UNEXPLAINED here -- no counters were collected."""
    D, runs, boundary_ms = 3, [], 3.2e-3
    for N, k in ((200_000, 5), (1_000_000, 1)):
        va, vb, z, s, pe, pl = se2_graph(N, k, np.random.RandomState(0))
        F = va.shape[0]
        e = LinearEngine.se2_pose_graph(va, vb, z, s, pe, pl, float('inf'), 4, 2, eta_damping=0.4)
        e0 = LinearEngine.se2_pose_graph(va, vb, z, s, pe, pl, 0.0, 4, 0, eta_damping=0.4)
        n = a.steps

        def plain():
            t = time.perf_counter(); e.iterate(n); e.sync()
            return 1e3 * (time.perf_counter() - t) / n

        def relin(h):
            t = time.perf_counter(); c = h.iterate(n, relinearise=True); t = time.perf_counter() - t
            return 1e3 * t / n, c

        def one_device():
            t = time.perf_counter(); e0.iterate(1, relinearise=True); e0.sync()
            return 1e3 * (time.perf_counter() - t)

        def one_host():
            t = time.perf_counter()
            mu = e0.get_means().reshape(N, 3)
            fe, fl = se2_host_factors(np.concatenate([mu[va], mu[vb]], 1), z, s)
            h = LinearEngine(va, vb, fe, fl, pe, pl, eta_damping=0.4)
            h.update_all_beliefs(); h.sync()
            t = 1e3 * (time.perf_counter() - t)
            h.close()
            return t
        e.iterate(a.warmup); e.sync(); relin(e); relin(e0); one_device(); one_host()
        rec = {key: [] for key in ('plain', 'relin_none', 'relin_all', 'one_device', 'one_host')}
        least = F
        for _ in range(a.repeats):                          # alternating
            rec['plain'].append(plain())
            t, c = relin(e); assert not c.any(); rec['relin_none'].append(t)
            t, c = relin(e0); least = min(least, int(c.min())); rec['relin_all'].append(t)
            rec['one_device'].append(one_device()); rec['one_host'].append(one_host())
        med = {key: statistics.median(v) for key, v in rec.items()}
        spread = {key: (max(v) - min(v)) / med[key] for key, v in rec.items()}
        per_f = sweep_doubles(D, 1.0 / k, False)
        runs.append({"vars": N, "dofs": D, "k": k, "factors": F, "ms_per_sweep": med, "spread": spread, "ms_all": rec,
                     "ratio_relin_none_over_plain": med['relin_none'] / med['plain'], "ratio_none_counted": (per_f + 14) / per_f + boundary_ms / med['plain'],
                     "ratio_relin_all_over_plain": med['relin_all'] / med['plain'], "ratio_all_counted": (per_f + 14 + 39) / per_f + boundary_ms / med['plain'],
                     "ratio_host_over_device_one_relinearising_sweep": med['one_host'] / med['one_device'],
                     "doubles_per_factor_plain": per_f, "kernel_boundary_ms_assumed": boundary_ms, "counters_collected": False,
                     "fewest_relinearised_in_a_beta_0_sweep": least,
                     "energy_after": {"beta_inf": e.energy(), "beta_0": e0.energy()}})
        e.close(); e0.close()
    vs_parent = None
    if a.parent_results:
        by = {}
        for ln in open(a.parent_results):
            who, js = ln.split(' ', 1)
            r = json.loads(js)
            by.setdefault(r['config']['workload'], {'parent': [], 'here': []})[who].append(r['value'])
        vs_parent = [{"workload": w, "parent": v['parent'], "here": v['here'], "median_parent": statistics.median(v['parent']),
                      "median_here": statistics.median(v['here']),
                      "spread_parent": (max(v['parent']) - min(v['parent'])) / statistics.median(v['parent']),
                      "spread_here": (max(v['here']) - min(v['here'])) / statistics.median(v['here'])} for w, v in by.items()]
    out = {"what": "tools/bench_linear.py --nonlinear on one MI355X: ms per sweep of gbp_lin_iterate_nonlinear against gbp_lin_iterate on the same handle, and "
                   "against a host relinearisation + gbp_lin_create, on the 200k x 3 ring (k = 5) and the 1M-variable chain (k = 1) re-posed as SE(2)",
           "method": " ".join(nonlinear_profile.__doc__.split()), "repeats": a.repeats, "sweep_steps": a.steps, "runs": runs,
           "sweeps_per_s_vs_parent": vs_parent}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'linear_nonlinear.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


class RawSE2:
    """gbp_lin_create + gbp_lin_set_nonlinear through the C ABI of ANY build of the library (this one or --parent-lib)."""

    def __init__(self, lib, va, vb, z, s, pe, pl, beta, minlin, model=1):
        import ctypes as ct
        from gbp_amd import _capi
        self.lib, self.ct = lib, ct
        F, N = va.shape[0], pe.shape[0]
        D = 3 if model == 1 else 6                           # GBP_LIN_MODEL_SE2_BETWEEN / _SE3_BETWEEN
        fe, fl = np.zeros((F, 2 * D)), np.zeros((F, 2 * D, 2 * D))
        d = _capi.LinDesc()
        d.n_vars, d.dofs, d.n_factors, d.device = N, D, F, 0
        d.var_a, d.var_b = _capi.iptr(va), _capi.iptr(vb)
        d.factor_eta, d.factor_lam, d.factor_const = _capi.dptr(fe), _capi.dptr(fl), None
        d.prior_eta, d.prior_lam, d.eta_damping = _capi.dptr(pe), _capi.dptr(pl), 0.4
        self.h = ct.c_void_p()
        for name in ('gbp_lin_create', 'gbp_lin_set_nonlinear', 'gbp_lin_iterate_nonlinear', 'gbp_lin_sync'):
            getattr(lib, name).restype = ct.c_int
        lib.gbp_lin_destroy.restype = None
        assert lib.gbp_lin_create(ct.byref(self.h), ct.byref(d)) == 0
        nd = _capi.LinNonlinear(int(model), 4, int(minlin), 0, float(beta), _capi.dptr(z), _capi.dptr(s))
        assert lib.gbp_lin_set_nonlinear(self.h, ct.byref(nd)) == 0
        assert lib.gbp_lin_sync(self.h) == 0

    def sweeps(self, n):
        t = time.perf_counter()
        assert self.lib.gbp_lin_iterate_nonlinear(self.h, self.ct.c_int32(n), None) == 0 and self.lib.gbp_lin_sync(self.h) == 0
        return 1e3 * (time.perf_counter() - t) / n

    def close(self):
        self.lib.gbp_lin_destroy(self.h)


def nonlinear_live_profile():
    """Host clock around whole calls, each ending in gbp_lin_sync, after one untimed warm-up round; --repeats alternating rounds, medians
    reported, spread = (max - min) / median.  Per round and graph, on a handle that has run 4 relinearising sweeps: (a) extend_se2 by 1000
    poses and 5000 factors (each new pose joined to the pose before it and to 4 random older poses); (b) on the grown handle, shrink
    retiring the 1000 oldest poses with the fold; (c) the yardstick for each: gbp_lin_create + gbp_lin_set_nonlinear of the grown / the
    surviving graph from host arrays that are already packed, through --parent-lib where given (else this library: the same code) -- it
    loses every message, linearisation point, iters and damping besides; (d) the linear gbp_lin_extend / gbp_lin_shrink of the same sizes
    on a linear handle of the same graph.  Counted: a linear extend / shrink moves per factor the sweep's arrays (2 ends, 6 + 21 factor
    doubles, 18 message doubles, 18 of vmsg, 2 edge slots); the nonlinear calls move 16 more values per factor (3 + 3 + 6 + iters +
    damping), and the extend adds one linearise launch over the new factors.  (e) the sweep of gbp_lin_iterate_nonlinear at beta = +inf
    and at beta = 0 (min_linear_iters 0), this library against --parent-lib on handles of the same graph, alternating, once with the
    parent's handle created first and once with this library's."""
    import ctypes as ct
    from gbp_amd import _capi
    here = _capi.load()
    parent = ct.CDLL(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    dN, per = 1000, 5
    runs = []
    for N, k in ((200_000, 5), (1_000_000, 1)):
        rs = np.random.RandomState(0)
        va, vb, z, s, pe, pl = se2_graph(N, k, rs)
        F = va.shape[0]
        # the appended part: pose N + i hangs on the pose before it and on 4 random older ones
        na = np.concatenate([np.arange(N - 1, N + dN - 1)[:, None], rs.randint(0, N, (dN, per - 1))], 1).reshape(-1).astype(np.int32)
        nb = np.repeat(np.arange(N, N + dN), per).astype(np.int32)
        nz, ns = rs.normal(0, 0.3, (dN * per, 3)), np.tile(np.array([10.0, 10.0, 20.0]), (dN * per, 1))
        npl = np.ascontiguousarray(np.broadcast_to(np.diag([1.0, 1.0, 4.0]), (dN, 3, 3)))
        npe = rs.normal(0, 1, (dN, 3))
        ga, gb, gz, gs = np.concatenate([va, na]), np.concatenate([vb, nb]), np.concatenate([z, nz]), np.concatenate([s, ns])
        gpe, gpl = np.concatenate([pe, npe]), np.concatenate([pl, npl])
        keep = (ga >= dN) & (gb >= dN)                       # what survives retiring poses 0 .. 999
        sa, sb, sz, ss = ga[keep] - dN, gb[keep] - dN, np.ascontiguousarray(gz[keep]), np.ascontiguousarray(gs[keep])
        spe, spl = np.ascontiguousarray(gpe[dN:]), np.ascontiguousarray(gpl[dN:])
        sa, sb = np.ascontiguousarray(sa.astype(np.int32)), np.ascontiguousarray(sb.astype(np.int32))
        lfe, lfl = np.zeros((dN * per, 6)), np.ascontiguousarray(np.broadcast_to(np.eye(6), (dN * per, 6, 6)))
        ylib = parent or here

        def timed(fn, sync):
            t = time.perf_counter(); fn(); sync()
            return 1e3 * (time.perf_counter() - t)

        def recreate(args):
            t = time.perf_counter()
            h = RawSE2(ylib, *args, 0.05, 2)
            t = 1e3 * (time.perf_counter() - t)
            h.close()
            return t

        rec = {key: [] for key in ('extend_se2', 'shrink_nonlinear', 'recreate_grown', 'recreate_survivors', 'extend_linear', 'shrink_linear')}
        for rnd in range(a.repeats + 1):                    # round 0 is the warm-up
            e = LinearEngine.se2_pose_graph(va, vb, z, s, pe, pl, 0.05, 4, 2, eta_damping=0.4)
            e.iterate(4, relinearise=True); e.sync()
            row = {'extend_se2': timed(lambda: e.extend_se2(na, nb, nz, ns, npe, npl), e.sync)}
            row['shrink_nonlinear'] = timed(lambda: e.retire(np.arange(dN)), e.sync)
            assert e.sizes() == (N, int(keep.sum()))
            e.close()
            row['recreate_grown'] = recreate((ga, gb, gz, gs, gpe, gpl))
            row['recreate_survivors'] = recreate((sa, sb, sz, ss, spe, spl))
            l = LinearEngine(va, vb, np.zeros((F, 6)), np.ascontiguousarray(np.broadcast_to(np.eye(6), (F, 6, 6))), pe, pl, eta_damping=0.4)
            l.update_all_beliefs(); l.iterate(4); l.sync()
            row['extend_linear'] = timed(lambda: l.extend(na, nb, lfe, lfl, npe, npl), l.sync)
            row['shrink_linear'] = timed(lambda: l.retire(np.arange(dN)), l.sync)
            l.close()
            if rnd:
                for key, v in row.items():
                    rec[key].append(v)
        med = {key: statistics.median(v) for key, v in rec.items()}
        spread = {key: (max(v) - min(v)) / med[key] for key, v in rec.items()}
        lin_values = 2 + 27 + 18 + 18 + 2                     # per factor, moved by the linear calls
        sweeps = None
        if parent:
            sweeps = {}
            # both orders of creation: which handle's arrays are allocated first moves a handle's sweep by more than its rounds differ
            for tag, beta, minlin in (('beta_inf', float('inf'), 2), ('beta_0', 0.0, 0)):
                for order in ('parent_created_first', 'here_created_first'):
                    first, second = (parent, here) if order == 'parent_created_first' else (here, parent)
                    h1 = RawSE2(first, va, vb, z, s, pe, pl, beta, minlin)
                    h2 = RawSE2(second, va, vb, z, s, pe, pl, beta, minlin)
                    hp, hh = (h1, h2) if order == 'parent_created_first' else (h2, h1)
                    hp.sweeps(a.warmup); hh.sweeps(a.warmup)
                    tp, th = [], []
                    for _ in range(a.repeats):
                        tp.append(hp.sweeps(a.steps)); th.append(hh.sweeps(a.steps))
                    hp.close(); hh.close()
                    mp, mh = statistics.median(tp), statistics.median(th)
                    sweeps[tag + '_' + order] = {"ms_per_sweep_parent": mp, "ms_per_sweep_here": mh, "ratio_here_over_parent": mh / mp,
                                                 "spread_parent": (max(tp) - min(tp)) / mp, "spread_here": (max(th) - min(th)) / mh, "ms_all_parent": tp, "ms_all_here": th}
        runs.append({"vars": N, "k": k, "factors": F, "new_vars": dN, "new_factors": dN * per, "retired_vars": dN, "surviving_factors": int(keep.sum()),
                     "ms": med, "spread": spread, "ms_all": rec, "yardstick_library": "parent" if parent else "this library (no --parent-lib given)",
                     "ratio_recreate_over_extend_se2": med['recreate_grown'] / med['extend_se2'],
                     "ratio_recreate_over_shrink_nonlinear": med['recreate_survivors'] / med['shrink_nonlinear'],
                     "ratio_extend_se2_over_linear": med['extend_se2'] / med['extend_linear'], "ratio_shrink_nonlinear_over_linear": med['shrink_nonlinear'] / med['shrink_linear'],
                     "ratio_counted_values": (lin_values + 16) / lin_values, "counters_collected": False, "nonlinear_sweep_vs_parent": sweeps})
    out = {"what": "tools/bench_linear.py --nonlinear-live on one MI355X: gbp_lin_extend_nonlinear and gbp_lin_shrink_nonlinear against re-creating the handle and "
                   "against the linear calls, and the nonlinear sweep against the parent commit's library, on the 200k x 3 ring (k = 5) and the 1M-variable "
                   "chain (k = 1) re-posed as SE(2)",
           "method": " ".join(nonlinear_live_profile.__doc__.split()), "repeats": a.repeats, "sweep_steps": a.steps, "runs": runs}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'linear_nonlinear_live.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


def nonlinear_robust_profile():
    """Host clock around whole calls, each ending in gbp_lin_sync, after a warm-up of every form; --repeats alternating rounds of --steps
    sweeps, medians reported per sweep, spread = (max - min) / median.  On the two graphs of --nonlinear, beta = +inf (nothing
    relinearises, so the robustify cost stands alone), every factor with the Huber loss at threshold 2 (every lane takes the loss's
    path).  (a) one handle WITHOUT losses: gbp_lin_iterate_nonlinear (`plain`).  (b) one handle WITH losses: gbp_lin_iterate_nonlinear
    at the weights as they stand (`weighted`: the factor stage reads w), gbp_lin_iterate_nonlinear_robust (`robust`: the fused lane),
    and the alternative the fusion is measured against, robustify as a launch of its own -- gbp_lin_robustify_nonlinear +
    gbp_lin_iterate_nonlinear(1) per sweep, four launches (`separate`; that is the same lane code run in its robustify-only mode: no
    separate kernel is kept; its robustify launch does not count the flagged factors).  (b') a third handle whose threshold is never
    reached: the same lane, loads and stores as `robust`, but no wave adds to the sweep's flag count (`robust_nothing_flagged`) -- on
    the handle of (b) two waves in three do, all to one address.  Counted beside robust / plain, per factor on top of the relinearising sweep's count: z and s now read
    every sweep (6 doubles), loss (0.5), threshold (1), w written (1), flag written (0.5), w read by the factor stage (1) = 10.  An
    excess of the measured ratio over the counted one is UNEXPLAINED here -- no counters were collected.  (c) with --parent-lib: sweeps
    of gbp_lin_iterate_nonlinear and of gbp_lin_iterate on handles WITHOUT losses, this library against the parent commit's, alternating,
    once with the parent's handle created first and once with this library's; the margin is the larger of the two spreads."""
    import ctypes as ct
    from gbp_amd import _capi
    here = _capi.load()
    parent = ct.CDLL(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    D, runs, n = 3, [], a.steps
    for N, k in ((200_000, 5), (1_000_000, 1)):
        va, vb, z, s, pe, pl = se2_graph(N, k, np.random.RandomState(0))
        F = va.shape[0]
        e = LinearEngine.se2_pose_graph(va, vb, z, s, pe, pl, float('inf'), 4, 2, eta_damping=0.4)
        r = LinearEngine.se2_pose_graph(va, vb, z, s, pe, pl, float('inf'), 4, 2, eta_damping=0.4)
        r.set_robust('huber', 2.0)
        r0 = LinearEngine.se2_pose_graph(va, vb, z, s, pe, pl, float('inf'), 4, 2, eta_damping=0.4)
        r0.set_robust('huber', 1e9)                           # the same lane and traffic, nothing flagged: no wave adds to the count

        def timed(fn, h):
            t = time.perf_counter(); fn(); h.sync()
            return 1e3 * (time.perf_counter() - t) / n

        def separate():
            for _ in range(n):
                r.robustify_all_factors(); r._lib.gbp_lin_iterate_nonlinear(r._h, 1, None)
        forms = {'plain': lambda: timed(lambda: e._lib.gbp_lin_iterate_nonlinear(e._h, n, None), e),
                 'weighted': lambda: timed(lambda: r._lib.gbp_lin_iterate_nonlinear(r._h, n, None), r),
                 'robust': lambda: timed(lambda: r._lib.gbp_lin_iterate_nonlinear_robust(r._h, n, None, None), r),
                 'robust_nothing_flagged': lambda: timed(lambda: r0._lib.gbp_lin_iterate_nonlinear_robust(r0._h, n, None, None), r0),
                 'separate': lambda: timed(separate, r)}
        for fn in forms.values():
            fn()
        rec = {key: [] for key in forms}
        for _ in range(a.repeats):                          # alternating
            for key, fn in forms.items():
                rec[key].append(fn())
        flagged = int(r.weights()[1].sum())
        assert not r0.weights()[1].any()
        med = {key: statistics.median(v) for key, v in rec.items()}
        spread = {key: (max(v) - min(v)) / med[key] for key, v in rec.items()}
        per_f = sweep_doubles(D, 1.0 / k, False) + 14           # the relinearising sweep at beta = +inf (--nonlinear)
        vs_parent = None
        if parent:
            vs_parent = {}
            for order in ('parent_created_first', 'here_created_first'):
                first, second = (parent, here) if order == 'parent_created_first' else (here, parent)
                h1 = RawSE2(first, va, vb, z, s, pe, pl, float('inf'), 2)
                h2 = RawSE2(second, va, vb, z, s, pe, pl, float('inf'), 2)
                hp, hh = (h1, h2) if order == 'parent_created_first' else (h2, h1)
                for call in ('gbp_lin_iterate_nonlinear', 'gbp_lin_iterate'):
                    def sweeps(h):
                        t = time.perf_counter()
                        rc = h.lib.gbp_lin_iterate_nonlinear(h.h, ct.c_int32(n), None) if call == 'gbp_lin_iterate_nonlinear' else h.lib.gbp_lin_iterate(h.h, ct.c_int32(n))
                        assert rc == 0 and h.lib.gbp_lin_sync(h.h) == 0
                        return n / (time.perf_counter() - t)
                    sweeps(hp); sweeps(hh)
                    tp, th = [], []
                    for _ in range(a.repeats):
                        tp.append(sweeps(hp)); th.append(sweeps(hh))
                    mp, mh = statistics.median(tp), statistics.median(th)
                    sp, sh = (max(tp) - min(tp)) / mp, (max(th) - min(th)) / mh
                    vs_parent[call + '_' + order] = {"sweeps_per_s_parent": mp, "sweeps_per_s_here": mh, "ratio_here_over_parent": mh / mp, "spread_parent": sp,
                                                     "spread_here": sh, "margin": max(sp, sh), "beyond_margin": abs(mh / mp - 1.0) > max(sp, sh),
                                                     "all_parent": tp, "all_here": th}
                hp.close(); hh.close()
        runs.append({"vars": N, "dofs": D, "k": k, "factors": F, "ms_per_sweep": med, "spread": spread, "ms_all": rec, "flagged_at_the_end": flagged,
                     "ratio_robust_over_plain": med['robust'] / med['plain'], "ratio_robust_over_plain_counted": (per_f + 10) / per_f,
                     "ratio_robust_over_weighted": med['robust'] / med['weighted'], "ratio_robust_over_weighted_counted": (per_f + 10) / (per_f + 1),
                     "ratio_separate_over_robust": med['separate'] / med['robust'],
                     "ratio_robust_nothing_flagged_over_plain": med['robust_nothing_flagged'] / med['plain'], "doubles_per_factor_relinearising_sweep": per_f,
                     "counters_collected": False, "sweeps_per_s_vs_parent_without_losses": vs_parent})
        e.close(); r.close(); r0.close()
    out = {"what": "tools/bench_linear.py --nonlinear-robust on one MI355X: ms per sweep of gbp_lin_iterate_nonlinear_robust against gbp_lin_iterate_nonlinear, "
                   "with robustify fused into the relinearise lane and as a launch of its own, and the sweeps of handles without losses against the parent "
                   "commit's library, on the 200k x 3 ring (k = 5) and the 1M-variable chain (k = 1) re-posed as SE(2)",
           "method": " ".join(nonlinear_robust_profile.__doc__.split()), "repeats": a.repeats, "sweep_steps": a.steps, "runs": runs}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'linear_nonlinear_robust.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


def nonlinear_until_profile():
    """Host clock around whole calls, each ending in a stream synchronise, after a warm-up of every form; --repeats alternating rounds of
    --steps sweeps, medians reported per sweep, spread = (max - min) / median.  On the two graphs of --nonlinear, once with beta = +inf
    (the relinearise stage runs and relinearises nothing) and once with beta = 0, min_linear_iters = 0 (every factor relinearises in every
    sweep), tolerances off so that every form runs --steps sweeps: `iterate_nonlinear` (gbp_lin_iterate_nonlinear), `until`
    (gbp_lin_iterate_until_nonlinear, no column asked for), `until_energy`, `until_both` (energy and MAP distance, after one solve_map),
    and `host_loop`, the loop the call replaces: iterate(1, relinearise=True); energy() per sweep -- three calls that run the same
    device code as before this call existed, timed on this library.  Counted beside each ratio over iterate_nonlinear, in doubles per
    factor on top of the relinearising sweep's count (--nonlinear: the plain sweep + 14 at beta = +inf, + 53 at beta = 0): the trace
    reads the old mean per variable (3) and writes one partial per 7 variables, and with the distance reads x (3) and writes a second
    partial, times variables per factor; the energy pass gathers two means (6) and reads z and s (6) and one partial per 256 factors.
    Each adds kernel boundaries priced at 3.2 us: the finishing kernel (1), the energy pass (1).  The counts are of algorithmic bytes;
    an excess of a measured ratio over its count by more than the spread is UNEXPLAINED here -- no counters were collected.  With
    --parent-lib: gbp_lin_iterate_nonlinear and gbp_lin_iterate, this library against the parent commit's in one process, alternating,
    once with the parent's handle created first and once with this library's; the margin is the larger of the two spreads."""
    import ctypes as ct
    from gbp_amd import _capi
    here = _capi.load()
    parent = ct.CDLL(os.path.abspath(a.parent_lib)) if a.parent_lib else None
    D, runs, n, boundary_ms = 3, [], a.steps, 3.2e-3
    for N, k in ((200_000, 5), (1_000_000, 1)):
        va, vb, z, s, pe, pl = se2_graph(N, k, np.random.RandomState(0))
        F = va.shape[0]
        for tag, beta, minlin, extra in (('beta_inf', float('inf'), 2, 14), ('beta_0', 0.0, 0, 53)):
            e = LinearEngine.se2_pose_graph(va, vb, z, s, pe, pl, beta, 4, minlin, eta_damping=0.4)
            e.solve_map()

            def timed(fn):
                t = time.perf_counter(); fn(); e.sync()
                return 1e3 * (time.perf_counter() - t) / n

            def until(want):
                o = _capi.LinUntilOpts(n, 8, 0, want, 0.0, 0.0)
                i = _capi.LinUntilInfo()
                assert e._lib.gbp_lin_iterate_until_nonlinear(e._h, ct.byref(o), None, None, None, ct.byref(i)) == 0 and i.iters == n

            def host_loop():
                for _ in range(n):
                    e.iterate(1, relinearise=True); e.energy()
            forms = {'iterate_nonlinear': lambda: timed(lambda: e._lib.gbp_lin_iterate_nonlinear(e._h, n, None)),
                     'until': lambda: timed(lambda: until(0)),
                     'until_energy': lambda: timed(lambda: until(_capi.LIN_TRACE_ENERGY)),
                     'until_both': lambda: timed(lambda: until(_capi.LIN_TRACE_ENERGY | _capi.LIN_TRACE_MAP)),
                     'host_loop': lambda: timed(host_loop)}
            for fn in forms.values():
                fn()
            rec = {key: [] for key in forms}
            for _ in range(a.repeats):                      # alternating
                for key, fn in forms.items():
                    rec[key].append(fn())
            med = {key: statistics.median(v) for key, v in rec.items()}
            spread = {key: (max(v) - min(v)) / med[key] for key, v in rec.items()}
            vpf = 1.0 / k
            per_f = sweep_doubles(D, vpf, False) + extra
            add = {'until': vpf * (3 + 1 / 7.0), 'until_energy': vpf * (3 + 1 / 7.0) + 12 + 1 / 256.0,
                   'until_both': vpf * (6 + 2 / 7.0) + 12 + 1 / 256.0, 'host_loop': 12 + 1 / 256.0}
            bounds = {'until': 1, 'until_energy': 2, 'until_both': 2, 'host_loop': 1}
            ratios = {}
            for key in add:
                measured, base = med[key] / med['iterate_nonlinear'], med['iterate_nonlinear']
                counted = (per_f + add[key]) / per_f + bounds[key] * boundary_ms / base
                margin = max(spread[key], spread['iterate_nonlinear'])
                ratios[key] = {"measured": measured, "counted": counted, "doubles_added_per_factor": add[key], "kernel_boundaries_added": bounds[key],
                               "margin": margin, "unexplained_excess": bool(measured - counted > margin)}
            runs.append({"vars": N, "dofs": D, "k": k, "factors": F, "beta": tag, "ms_per_sweep": med, "spread": spread, "ms_all": rec,
                         "doubles_per_factor_relinearising_sweep": per_f, "ratio_over_iterate_nonlinear": ratios,
                         "ratio_host_loop_over_until_energy": med['host_loop'] / med['until_energy'], "counters_collected": False})
            e.close()
        if parent:
            vs_parent = {}
            for order in ('parent_created_first', 'here_created_first'):
                first, second = (parent, here) if order == 'parent_created_first' else (here, parent)
                h1 = RawSE2(first, va, vb, z, s, pe, pl, float('inf'), 2)
                h2 = RawSE2(second, va, vb, z, s, pe, pl, float('inf'), 2)
                hp, hh = (h1, h2) if order == 'parent_created_first' else (h2, h1)
                for call in ('gbp_lin_iterate_nonlinear', 'gbp_lin_iterate'):
                    def sweeps(h):
                        t = time.perf_counter()
                        rc = h.lib.gbp_lin_iterate_nonlinear(h.h, ct.c_int32(n), None) if call == 'gbp_lin_iterate_nonlinear' else h.lib.gbp_lin_iterate(h.h, ct.c_int32(n))
                        assert rc == 0 and h.lib.gbp_lin_sync(h.h) == 0
                        return n / (time.perf_counter() - t)
                    sweeps(hp); sweeps(hh)
                    tp, th = [], []
                    for _ in range(a.repeats):
                        tp.append(sweeps(hp)); th.append(sweeps(hh))
                    mp, mh = statistics.median(tp), statistics.median(th)
                    sp, sh = (max(tp) - min(tp)) / mp, (max(th) - min(th)) / mh
                    vs_parent[call + '_' + order] = {"sweeps_per_s_parent": mp, "sweeps_per_s_here": mh, "ratio_here_over_parent": mh / mp, "spread_parent": sp,
                                                     "spread_here": sh, "margin": max(sp, sh), "beyond_margin": abs(mh / mp - 1.0) > max(sp, sh),
                                                     "all_parent": tp, "all_here": th}
                hp.close(); hh.close()
            runs.append({"vars": N, "dofs": D, "k": k, "factors": F, "sweeps_per_s_vs_parent": vs_parent})
    out = {"what": "tools/bench_linear.py --nonlinear-until on one MI355X: ms per sweep of gbp_lin_iterate_until_nonlinear against gbp_lin_iterate_nonlinear and "
                   "the host loop it replaces, and the older sweeps against the parent commit's library, on the 200k x 3 ring (k = 5) and the 1M-variable "
                   "chain (k = 1) re-posed as SE(2)",
           "method": " ".join(nonlinear_until_profile.__doc__.split()), "repeats": a.repeats, "sweep_steps": a.steps, "runs": runs}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'linear_nonlinear_until.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


def se3_graph(N, k, rs):
    """N poses on a circle of radius N / 20, the rotation vector angle * (1, 2, 2) / 3 with the angle rising to 4.5 rad (past pi) half way
    round and falling back, so that it is continuous and every relative rotation small; each pose joined to its next k neighbours;
    sqrt information (10, 10, 10, 20, 20, 20), noise to match; priors sigma (1, 1, 1, 0.5, 0.5, 0.5) at truth + N(0, (0.1 x 3, 0.03 x 3))."""
    th = np.arange(N) * 2 * np.pi / N
    R = N / 20.0
    axis = np.array([1.0, 2.0, 2.0]) / 3.0
    ang = 4.5 * (1.0 - np.abs(2.0 * np.arange(N) / N - 1.0))
    truth = np.concatenate([np.stack([R * np.cos(th), R * np.sin(th), 0.3 * np.sin(2 * th)], 1), ang[:, None] * axis], 1)
    va = np.repeat(np.arange(N), k)
    vb = (va + np.tile(np.arange(1, k + 1), N)) % N

    def rot(w):                                             # Rodrigues, |w| > 0 or the identity
        t = np.linalg.norm(w, axis=1)
        u = w / np.where(t > 0, t, 1.0)[:, None]
        K = np.zeros((w.shape[0], 3, 3))
        K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -u[:, 2], u[:, 1], u[:, 2], -u[:, 0], -u[:, 1], u[:, 0]
        return np.eye(3)[None] + np.sin(t)[:, None, None] * K + (1 - np.cos(t))[:, None, None] * (K @ K)
    Ra, Rb = rot(truth[va, 3:]), rot(truth[vb, 3:])
    E = np.swapaxes(Ra, 1, 2) @ Rb
    v = 0.5 * np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], 1)
    nv = np.linalg.norm(v, axis=1)
    phi = (np.arctan2(nv, 0.5 * (np.trace(E, axis1=1, axis2=2) - 1.0)) / np.where(nv > 0, nv, 1.0))[:, None] * v
    s = np.tile(np.array([10.0, 10.0, 10.0, 20.0, 20.0, 20.0]), (va.shape[0], 1))
    z = np.concatenate([np.einsum('fji,fj->fi', Ra, truth[vb, :3] - truth[va, :3]), phi], 1) + rs.normal(0, 1, s.shape) / s
    pl = np.ascontiguousarray(np.broadcast_to(np.diag([1.0, 1.0, 1.0, 4.0, 4.0, 4.0]), (N, 6, 6)))
    pe = np.einsum('nij,nj->ni', pl, truth + rs.normal(0, 1, (N, 6)) * np.array([0.1, 0.1, 0.1, 0.03, 0.03, 0.03]))
    return va.astype(np.int32), vb.astype(np.int32), z, s, pe, pl


def nonlinear_se3_profile():
    """Host clock around whole calls, each ending in a stream synchronise, after a warm-up of every form; --repeats alternating rounds of
    --steps sweeps, medians reported per sweep, spread = (max - min) / median.  On a 100k-pose ring with k = 5 (500k factors) and a
    500k-pose chain with k = 1, d = 6, re-posed as SE(3) (se3_graph).  One handle with beta = +inf: `plain` (gbp_lin_iterate) against
    `relin_none` (gbp_lin_iterate_nonlinear, the relinearise stage runs and relinearises nothing); on the same handle with the Huber
    loss on every factor, `robust` (gbp_lin_iterate_nonlinear_robust, beta = +inf still, after `plain_weighted`, gbp_lin_iterate with the
    losses set, was timed).  A second handle with beta = 0 and min_linear_iters = 0: `relin_all`, every factor re-made in every sweep,
    against ITS plain sweep (`plain_b0`).  Counted beside each ratio, in doubles per factor on top of the plain d = 6 sweep's count: at
    beta = +inf the stage gathers two means (12), reads the linpoint (12) and iters (0.5), writes iters (0.5), and the factor stage reads
    the factor's damping (1): 26, plus one kernel boundary priced at 3.2 us; beta = 0 adds the measurement and square-root information
    read (12) and eta_f, Lambda_f and the linpoint written (12 + 78 + 12): 114 more; the robust lane adds z and s (12), loss, threshold,
    weight written and read, flag (4): 16.  The counts are of algorithmic bytes, not of what the caches fetch; the beta = 0 lane also does
    the arithmetic of the model (two Rodrigues, a Log, five 3 x 3 products, 78 entries of Lambda_f), which a count of doubles does not
    see: an excess of a measured ratio over its count is UNEXPLAINED here -- no counters were collected, and no split of the relinearise
    kernel's time into arithmetic and traffic was measured.  With --parent-lib: the SE(2) sweeps (gbp_lin_iterate_nonlinear at
    beta = +inf and gbp_lin_iterate on the 200k x 3 ring, k = 5) of this library against the parent commit's, alternating in one session,
    once with either library's handle created first."""
    import ctypes as ct
    from gbp_amd import _capi
    D, runs, boundary_ms = 6, [], 3.2e-3
    n = a.steps
    for N, k in ((100_000, 5), (500_000, 1)):
        va, vb, z, s, pe, pl = se3_graph(N, k, np.random.RandomState(0))
        F = va.shape[0]
        e = LinearEngine.se3_pose_graph(va, vb, z, s, pe, pl, float('inf'), 4, 2, eta_damping=0.4)
        e0 = LinearEngine.se3_pose_graph(va, vb, z, s, pe, pl, 0.0, 4, 0, eta_damping=0.4)

        def timed(fn, h):
            t = time.perf_counter(); fn(); h.sync()
            return 1e3 * (time.perf_counter() - t) / n
        forms = {'plain': lambda: timed(lambda: e.iterate(n), e),
                 'relin_none': lambda: timed(lambda: e._lib.gbp_lin_iterate_nonlinear(e._h, n, None), e),
                 'plain_b0': lambda: timed(lambda: e0.iterate(n), e0),
                 'relin_all': lambda: timed(lambda: e0._lib.gbp_lin_iterate_nonlinear(e0._h, n, None), e0)}
        e.iterate(a.warmup); e.sync()
        rec = {key: [] for key in list(forms) + ['plain_weighted', 'robust']}
        for fn in forms.values():
            fn()
        for _ in range(a.repeats):                          # alternating
            for key, fn in forms.items():
                rec[key].append(fn())
        counts = e0.iterate(2, relinearise=True)
        energy = {"beta_inf": e.energy(), "beta_0": e0.energy()}
        e.set_robust('huber', 4.0)
        rforms = {'plain_weighted': lambda: timed(lambda: e.iterate(n), e),
                  'robust': lambda: timed(lambda: e._lib.gbp_lin_iterate_nonlinear_robust(e._h, n, None, None), e)}
        for fn in rforms.values():
            fn()
        for _ in range(a.repeats):
            for key, fn in rforms.items():
                rec[key].append(fn())
        flagged = int(e.weights()[1].sum())
        med = {key: statistics.median(v) for key, v in rec.items()}
        spread = {key: (max(v) - min(v)) / med[key] for key, v in rec.items()}
        per_f = sweep_doubles(D, 1.0 / k, False)
        runs.append({"vars": N, "dofs": D, "k": k, "factors": F, "ms_per_sweep": med, "spread": spread, "ms_all": rec,
                     "ratio_relin_none_over_plain": med['relin_none'] / med['plain'], "ratio_none_counted": (per_f + 26) / per_f + boundary_ms / med['plain'],
                     "ratio_relin_all_over_plain": med['relin_all'] / med['plain_b0'], "ratio_all_counted": (per_f + 26 + 114) / per_f + boundary_ms / med['plain_b0'],
                     "ratio_robust_over_plain": med['robust'] / med['plain'], "ratio_robust_counted": (per_f + 26 + 16) / per_f + boundary_ms / med['plain'],
                     "ratio_robust_over_plain_weighted": med['robust'] / med['plain_weighted'],
                     "doubles_per_factor_plain": per_f, "kernel_boundary_ms_assumed": boundary_ms, "counters_collected": False,
                     "relinearised_in_two_more_beta_0_sweeps": counts.tolist(), "flagged_at_the_end": flagged, "energy_after": energy})
        e.close(); e0.close()
    vs_parent = None
    if a.parent_lib:
        here, parent = _capi.load(), ct.CDLL(os.path.abspath(a.parent_lib))
        va, vb, z, s, pe, pl = se2_graph(200_000, 5, np.random.RandomState(0))
        vs_parent = {}
        for order in ('parent_created_first', 'here_created_first'):
            first, second = (parent, here) if order == 'parent_created_first' else (here, parent)
            h1 = RawSE2(first, va, vb, z, s, pe, pl, float('inf'), 2)
            h2 = RawSE2(second, va, vb, z, s, pe, pl, float('inf'), 2)
            hp, hh = (h1, h2) if order == 'parent_created_first' else (h2, h1)
            for call in ('gbp_lin_iterate_nonlinear', 'gbp_lin_iterate'):
                def sweeps(h):
                    t = time.perf_counter()
                    rc = h.lib.gbp_lin_iterate_nonlinear(h.h, ct.c_int32(n), None) if call == 'gbp_lin_iterate_nonlinear' else h.lib.gbp_lin_iterate(h.h, ct.c_int32(n))
                    assert rc == 0 and h.lib.gbp_lin_sync(h.h) == 0
                    return n / (time.perf_counter() - t)
                sweeps(hp); sweeps(hh)
                tp, th = [], []
                for _ in range(a.repeats):
                    tp.append(sweeps(hp)); th.append(sweeps(hh))
                mp, mh = statistics.median(tp), statistics.median(th)
                sp, sh = (max(tp) - min(tp)) / mp, (max(th) - min(th)) / mh
                vs_parent[call + '_' + order] = {"sweeps_per_s_parent": mp, "sweeps_per_s_here": mh, "ratio_here_over_parent": mh / mp, "spread_parent": sp,
                                                 "spread_here": sh, "margin": max(sp, sh), "beyond_margin": abs(mh / mp - 1.0) > max(sp, sh),
                                                 "all_parent": tp, "all_here": th}
            hp.close(); hh.close()
    out = {"what": "tools/bench_linear.py --nonlinear-se3 on one MI355X: ms per sweep of the SE(3) relinearising sweeps against the plain d = 6 gbp_lin_iterate on "
                   "the same handle, on a 100k x 6 ring (k = 5) and a 500k-pose chain (k = 1) re-posed as SE(3); and the SE(2) sweeps against the parent "
                   "commit's library on the 200k x 3 ring (k = 5)",
           "method": " ".join(nonlinear_se3_profile.__doc__.split()), "repeats": a.repeats, "sweep_steps": a.steps, "runs": runs,
           "se2_sweeps_per_s_vs_parent": vs_parent}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'linear_nonlinear_se3.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


def nonlinear_map_profile():
    """Host clock around whole calls, each ending in a stream synchronise, after a warm-up of every form; --repeats alternating rounds,
    medians reported, spread = (max - min) / median.  On the 100k-pose SE(3) ring with k = 5 (500k factors) and the 500k-pose chain with
    k = 1 (se3_graph).  `lm_per_outer`: gbp_lin_solve_map_nonlinear from the belief means with max_outer = 4, tolerances off, lambda0 =
    1e-3, inner solves of at most --steps CG iterations (rel_tol 1e-30, so every inner solve runs exactly that many, after the product
    of its start and before the product of its true residual): ms = call / outer.  Its two nearest existing pieces run on a handle of
    the PARENT commit's library (--parent-lib, required; loaded beside this one) with beta = 0 and min_linear_iters = 0, in the same
    alternating rounds: `relin_all`, gbp_lin_relinearise after a sweep has moved the means (the relinearise kernel of an all-
    relinearising sweep, alone: its count is checked to be F), and `solve_map`, gbp_lin_solve_map with the same max_iters and rel_tol and
    warm_start = 1 -- started at the means, so that it too forms the product of its start, as every inner solve of `lm` does.  Counted
    per outer iteration, in doubles, on top of that solve's own count: the linearise lane gathers x (12), reads z and s (12) and writes
    eta_f, Lambda_f (12 + 78) per factor (the parent's relinearise lane moves 12 + 12 + 12 + 90 + 12 + 2: counted with relin_all, so the
    two nearly cancel); the damping lane reads the prior (27), the factors' diagonal (6 per edge, 2 edges per factor), x (6) and writes
    the damped prior (27) per variable; the set-up of the diagonal blocks is run per outer iteration (27 + 6 per variable read, the 42-
    entry factor blocks per edge, 27 + 6 written), where solve_map's is made once and is outside its timed call; the energy-only lane
    reads 24 per factor; the difference lane 27 + 12 per variable; three copies of x (12 per variable each).  An excess of `lm` over
    relin_all + solve_map beyond that count is UNEXPLAINED here: no counters were collected.
    The existing paths against the parent, both libraries in one session, alternating, once with either library's handle created first
    (balanced = the geometric mean of the two orders): gbp_lin_iterate_nonlinear (beta = +inf) and gbp_lin_iterate on the 200k x 3 SE(2)
    ring (k = 5), --steps sweeps per call; and gbp_lin_solve_map (cold, max_iters = --steps, rel_tol 1e-30) on the same handles, whose
    host path this commit rewrote."""
    import ctypes as ct
    from gbp_amd import _capi
    if not a.parent_lib:
        raise SystemExit("--nonlinear-map needs --parent-lib: its yardsticks are measured on the parent commit's library")
    here, parent = _capi.load(), ct.CDLL(os.path.abspath(a.parent_lib))
    for lib in (here, parent):
        for name in ('gbp_lin_relinearise', 'gbp_lin_solve_map', 'gbp_lin_iterate', 'gbp_lin_iterate_nonlinear', 'gbp_lin_sync'):
            getattr(lib, name).restype = ct.c_int
    D, runs = 6, []

    def raw_solve(h, warm):
        o, i = _capi.LinMapOpts(1e-30, int(a.steps), 8, int(warm)), _capi.LinMapInfo()
        t = time.perf_counter()
        assert h.lib.gbp_lin_solve_map(h.h, ct.byref(o), ct.byref(i)) == 0     # ends in a stream synchronise
        return 1e3 * (time.perf_counter() - t), i.iters

    for N, k in ((100_000, 5), (500_000, 1)):
        va, vb, z, s, pe, pl = se3_graph(N, k, np.random.RandomState(0))
        F = va.shape[0]
        e = LinearEngine.se3_pose_graph(va, vb, z, s, pe, pl, float('inf'), 4, 2, eta_damping=0.4)
        hp = RawSE2(parent, va, vb, z, s, pe, pl, 0.0, 0, model=2)
        assert hp.lib.gbp_lin_iterate_nonlinear(hp.h, ct.c_int32(2), None) == 0 and hp.lib.gbp_lin_sync(hp.h) == 0
        outer = 4
        res = {}

        def lm():
            t = time.perf_counter()
            r = e.solve_map_nonlinear(max_outer=outer, tol_step=0.0, tol_grad=0.0, lambda0=1e-3, rel_tol=1e-30, max_iters=a.steps)
            res['r'] = r
            return 1e3 * (time.perf_counter() - t) / max(r.outer, 1)

        def relin_all():
            assert hp.lib.gbp_lin_iterate(hp.h, ct.c_int32(1)) == 0 and hp.lib.gbp_lin_sync(hp.h) == 0   # moves the means: untimed
            n = ct.c_int32()
            t = time.perf_counter()
            assert hp.lib.gbp_lin_relinearise(hp.h, ct.byref(n)) == 0           # downloads its count: ends in a stream synchronise
            dt = 1e3 * (time.perf_counter() - t)
            res['relin'] = n.value
            return dt

        def solve_map():
            hp_solve = raw_solve(hp, 1)
            res['cg'] = hp_solve[1]
            return hp_solve[0]
        raw_solve(hp, 1)                                    # makes the parent handle's workspace and diagonal blocks, outside the timing
        forms = {'lm_per_outer': lm, 'relin_all': relin_all, 'solve_map': solve_map}
        rec = {key: [] for key in forms}
        for fn in forms.values():
            fn()
        for _ in range(a.repeats):                          # alternating
            for key, fn in forms.items():
                rec[key].append(fn())
        assert res['relin'] == F, res
        med = {key: statistics.median(v) for key, v in rec.items()}
        spread = {key: (max(v) - min(v)) / med[key] for key, v in rec.items()}
        r = res['r']
        extra_doubles = F * (12 + 12 + 90 + 24 + 12 + 2 * 42) + N * (27 + 6 + 27 + 33 + 33 + 27 + 12 + 36)
        parent_relin_doubles = F * (12 + 12 + 12 + 90 + 12 + 2)
        counted = 8 * (extra_doubles - parent_relin_doubles)
        runs.append({"vars": N, "dofs": D, "k": k, "factors": F, "ms": med, "spread": spread, "ms_all": rec, "yardsticks_on": "the parent commit's library",
                     "outer": r.outer, "accepted": r.accepted, "rejected": r.rejected, "cg_iters_per_outer": r.cg_iters / max(r.outer, 1),
                     "solve_map_cg_iters": res['cg'], "solve_map_warm_start": True, "relinearised": res['relin'],
                     "energy0": r.energy0, "energy": r.energy, "sum_of_pieces_ms": med['relin_all'] + med['solve_map'],
                     "lm_over_sum_of_pieces": med['lm_per_outer'] / (med['relin_all'] + med['solve_map']),
                     "counted_bytes_per_outer_beyond_the_pieces": counted, "counted_ms_at_8TBps": counted / 8e12 * 1e3,
                     "excess_over_pieces_ms": med['lm_per_outer'] - med['relin_all'] - med['solve_map'],
                     "excess_is": "measured; whatever of it exceeds the counted bytes is unexplained: no counters collected", "counters_collected": False})
        e.close(); hp.close()

    # the existing paths, this library against the parent's
    n = a.steps
    va, vb, z, s, pe, pl = se2_graph(200_000, 5, np.random.RandomState(0))
    vs_parent = {}
    for order in ('parent_created_first', 'here_created_first'):
        first, second = (parent, here) if order == 'parent_created_first' else (here, parent)
        h1 = RawSE2(first, va, vb, z, s, pe, pl, float('inf'), 2)
        h2 = RawSE2(second, va, vb, z, s, pe, pl, float('inf'), 2)
        hp, hh = (h1, h2) if order == 'parent_created_first' else (h2, h1)
        for call in ('gbp_lin_iterate_nonlinear', 'gbp_lin_iterate', 'gbp_lin_solve_map'):
            def run(h):
                if call == 'gbp_lin_solve_map':
                    ms, it = raw_solve(h, 0)
                    assert it == n
                    return n / (1e-3 * ms)                  # CG iterations per second
                t = time.perf_counter()
                rc = h.lib.gbp_lin_iterate_nonlinear(h.h, ct.c_int32(n), None) if call == 'gbp_lin_iterate_nonlinear' else h.lib.gbp_lin_iterate(h.h, ct.c_int32(n))
                assert rc == 0 and h.lib.gbp_lin_sync(h.h) == 0
                return n / (time.perf_counter() - t)
            run(hp); run(hh)
            tp, th = [], []
            for _ in range(a.repeats):
                tp.append(run(hp)); th.append(run(hh))
            mp, mh = statistics.median(tp), statistics.median(th)
            sp, sh = (max(tp) - min(tp)) / mp, (max(th) - min(th)) / mh
            vs_parent[call + '_' + order] = {"per_s_parent": mp, "per_s_here": mh, "ratio_here_over_parent": mh / mp, "spread_parent": sp, "spread_here": sh,
                                             "margin": max(sp, sh), "beyond_margin": abs(mh / mp - 1.0) > max(sp, sh), "all_parent": tp, "all_here": th}
        hp.close(); hh.close()
    for call in ('gbp_lin_iterate_nonlinear', 'gbp_lin_iterate', 'gbp_lin_solve_map'):
        r1, r2 = (vs_parent[call + '_' + o]["ratio_here_over_parent"] for o in ('parent_created_first', 'here_created_first'))
        vs_parent[call + '_balanced'] = (r1 * r2) ** 0.5
    out = {"what": "tools/bench_linear.py --nonlinear-map on one MI355X: ms per outer Levenberg-Marquardt iteration of gbp_lin_solve_map_nonlinear on the 100k x 6 SE(3) "
                   "ring (k = 5) and the 500k-pose chain (k = 1), beside the relinearise kernel of an all-relinearising sweep plus a warm-started gbp_lin_solve_map of "
                   "the same CG iteration count, both on the parent commit's library; and the existing sweeps and gbp_lin_solve_map against the parent's",
           "method": " ".join(nonlinear_map_profile.__doc__.split()), "repeats": a.repeats, "cg_iters_cap": a.steps, "runs": runs,
           "existing_paths_vs_parent": vs_parent}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'linear_nonlinear_map.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


def nonlinear_map_robust_profile():
    """Host clock around whole calls, each ending in a stream synchronise, after a warm-up of every form; --repeats alternating rounds,
    medians reported, spread = (max - min) / median.  On the 100k-pose SE(3) ring with k = 5 (500k factors) and the 500k-pose chain with
    k = 1 (se3_graph), the Huber loss at threshold 4 on every factor that is no odometry (the ring) / on every factor (the chain), and
    5 % of those factors' measurements corrupted by (1.5, -1, 0.8, 0.3, -0.2, 0.25).  `reweight`: gbp_lin_solve_map_nonlinear_robust with
    max_rounds = 0 and no weights / flags asked for -- the means gathered, ONE k_gn_reweight launch, its finish, four doubles downloaded, x
    copied; `reweight_with_report`: the same with the weights (F doubles) and flags (F int32) brought back.  `linearise_parent`:
    gbp_lin_solve_map_nonlinear with max_outer = 0 on a handle of the PARENT commit's library (--parent-lib, loaded beside this one) --
    the means gathered, ONE k_gn_factor<MODEL, true> launch, its finish, four doubles downloaded, x copied: the same call shape around
    the kernel the reweight lane extends.  `lm_here` / `lm_parent`: gbp_lin_solve_map_nonlinear (max_outer 4, tolerances off, lambda0
    1e-3, --steps CG iterations per inner solve at rel_tol 1e-30) on a handle WITHOUT losses of either library -- the loop both entry
    points now share.  `robust_solve`: one full gbp_lin_solve_map_nonlinear_robust from the belief means (max_rounds 10, the rounds at
    tol_grad 1e-3, tol_step 0, inner solves to 1e-10 in at most 2000 iterations), timed once per repeat: rounds, LM iterations, ms.
    The existing sweeps and gbp_lin_solve_map against the parent: both libraries in one session on the 200k x 3 SE(2) ring (k = 5),
    alternating, once with either library's handle created first (balanced = the geometric mean of the two orders)."""
    import ctypes as ct
    from gbp_amd import _capi
    if not a.parent_lib:
        raise SystemExit("--nonlinear-map-robust needs --parent-lib: its yardsticks are measured on the parent commit's library")
    here, parent = _capi.load(), ct.CDLL(os.path.abspath(a.parent_lib))
    for lib in (here, parent):
        for name in ('gbp_lin_solve_map_nonlinear', 'gbp_lin_solve_map', 'gbp_lin_iterate', 'gbp_lin_iterate_nonlinear', 'gbp_lin_sync'):
            getattr(lib, name).restype = ct.c_int
    runs = []

    def raw_lm(h, outer):
        o = _capi.LinNlmapOpts(outer, 0, 1e-3, 10.0, 0.1, 1e-12, 1e8, 0.0, 0.0, _capi.LinMapOpts(1e-30, int(a.steps), 8, 0))
        i = _capi.LinNlmapInfo()
        t = time.perf_counter()
        assert h.lib.gbp_lin_solve_map_nonlinear(h.h, ct.byref(o), None, ct.byref(i)) == 0
        return 1e3 * (time.perf_counter() - t), i.outer

    for N, k in ((100_000, 5), (500_000, 1)):
        rs = np.random.RandomState(0)
        va, vb, z, s, pe, pl = se3_graph(N, k, rs)
        F = va.shape[0]
        lossy = np.ones(F, bool) if k == 1 else (np.abs(vb - va) != 1) & (np.abs(vb - va) != N - 1)
        bad = lossy & (rs.uniform(size=F) < 0.05)
        z = z.copy()
        z[bad] += np.array([1.5, -1.0, 0.8, 0.3, -0.2, 0.25])
        e = LinearEngine.se3_pose_graph(va, vb, z, s, pe, pl, float('inf'), 4, 2, eta_damping=0.4)
        e.set_robust(['huber' if l else None for l in lossy], np.full(F, 4.0))
        hh = RawSE2(here, va, vb, z, s, pe, pl, float('inf'), 2, model=2)
        hp = RawSE2(parent, va, vb, z, s, pe, pl, float('inf'), 2, model=2)
        res = {}

        def reweight():                                     # through the C ABI with no weights / flags asked for: nothing but four doubles comes back
            o = _capi.LinIrlsOpts(0, 0, 1e-9, 1e-10, _capi.LinNlmapOpts(4, 0, 1e-3, 10.0, 0.1, 1e-12, 1e8, 0.0, 0.0, _capi.LinMapOpts(1e-30, int(a.steps), 8, 0)))
            i = _capi.LinIrlsInfo()
            t = time.perf_counter()
            assert e._lib.gbp_lin_solve_map_nonlinear_robust(e._h, ct.byref(o), None, None, None, None, ct.byref(i)) == 0
            return 1e3 * (time.perf_counter() - t)

        def reweight_with_report():                         # the same with weights (F doubles) and flags (F int32) downloaded
            t = time.perf_counter()
            res['rw'] = e.solve_map_nonlinear_robust(max_rounds=0)
            return 1e3 * (time.perf_counter() - t)

        def robust_solve():
            t = time.perf_counter()
            res['full'] = e.solve_map_nonlinear_robust(max_rounds=10, tol_grad=1e-3, tol_step=0.0, rel_tol=1e-10, max_iters=2000)
            return 1e3 * (time.perf_counter() - t)
        forms = {'reweight': reweight, 'reweight_with_report': reweight_with_report, 'linearise_parent': lambda: raw_lm(hp, 0)[0], 'lm_here': lambda: raw_lm(hh, 4)[0] / 4, 'lm_parent': lambda: raw_lm(hp, 4)[0] / 4,
                 'robust_solve': robust_solve}
        rec = {key: [] for key in forms}
        for fn_ in forms.values():
            fn_()
        for i in range(a.repeats):                          # alternating, the order turned round every other round
            for key in (list(forms) if i % 2 == 0 else list(forms)[::-1]):
                rec[key].append(forms[key]())
        med = {key: statistics.median(v) for key, v in rec.items()}
        spread = {key: (max(v) - min(v)) / med[key] for key, v in rec.items()}
        full = res['full']
        runs.append({"vars": N, "dofs": 6, "k": k, "factors": F, "lossy_factors": int(lossy.sum()), "corrupted": int(bad.sum()), "ms": med, "spread": spread,
                     "ms_all": rec, "reweight_over_parent_linearise": med['reweight'] / med['linearise_parent'],
                     "lm_here_over_parent": med['lm_here'] / med['lm_parent'], "flagged_at_x0": int(res['rw'].flagged),
                     "robust_solve": {"rounds": full.rounds, "lm_iterations": full.outer, "rejected": full.rejected, "cg_iters": full.cg_iters,
                                      "reason": full.reason, "converged": full.converged, "flagged": int(full.flagged), "energy0": full.energy0,
                                      "energy": full.energy, "ms": med['robust_solve']},
                     "counters_collected": False})
        e.close(); hh.close(); hp.close()

    n = a.steps
    va, vb, z, s, pe, pl = se2_graph(200_000, 5, np.random.RandomState(0))
    vs_parent = {}
    for order in ('parent_created_first', 'here_created_first'):
        first, second = (parent, here) if order == 'parent_created_first' else (here, parent)
        h1 = RawSE2(first, va, vb, z, s, pe, pl, float('inf'), 2)
        h2 = RawSE2(second, va, vb, z, s, pe, pl, float('inf'), 2)
        hp, hh = (h1, h2) if order == 'parent_created_first' else (h2, h1)
        for call in ('gbp_lin_iterate_nonlinear', 'gbp_lin_iterate', 'gbp_lin_solve_map'):
            def run(h):
                t = time.perf_counter()
                if call == 'gbp_lin_solve_map':
                    o, i = _capi.LinMapOpts(1e-30, int(n), 8, 0), _capi.LinMapInfo()
                    assert h.lib.gbp_lin_solve_map(h.h, ct.byref(o), ct.byref(i)) == 0 and i.iters == n
                else:
                    rc = h.lib.gbp_lin_iterate_nonlinear(h.h, ct.c_int32(n), None) if call == 'gbp_lin_iterate_nonlinear' else h.lib.gbp_lin_iterate(h.h, ct.c_int32(n))
                    assert rc == 0 and h.lib.gbp_lin_sync(h.h) == 0
                return n / (time.perf_counter() - t)
            run(hp); run(hh)
            tp, th = [], []
            for _ in range(a.repeats):
                tp.append(run(hp)); th.append(run(hh))
            mp, mh = statistics.median(tp), statistics.median(th)
            sp, sh = (max(tp) - min(tp)) / mp, (max(th) - min(th)) / mh
            vs_parent[call + '_' + order] = {"per_s_parent": mp, "per_s_here": mh, "ratio_here_over_parent": mh / mp, "spread_parent": sp, "spread_here": sh,
                                             "margin": max(sp, sh), "beyond_margin": abs(mh / mp - 1.0) > max(sp, sh)}
        hp.close(); hh.close()
    for call in ('gbp_lin_iterate_nonlinear', 'gbp_lin_iterate', 'gbp_lin_solve_map'):
        r1, r2 = (vs_parent[call + '_' + o]["ratio_here_over_parent"] for o in ('parent_created_first', 'here_created_first'))
        vs_parent[call + '_balanced'] = (r1 * r2) ** 0.5
    out = {"what": "tools/bench_linear.py --nonlinear-map-robust on one MI355X: gbp_lin_solve_map_nonlinear_robust on the 100k x 6 SE(3) ring (k = 5) and the "
                   "500k-pose chain (k = 1) with 5 % of the lossy factors corrupted",
           "method": " ".join(nonlinear_map_robust_profile.__doc__.split()), "repeats": a.repeats, "cg_iters_cap": a.steps, "runs": runs,
           "existing_paths_vs_parent": vs_parent}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'profiles', 'linear_nonlinear_map_robust.json')
    with open(path, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    print(json.dumps(out))


def model_cost_profile():
    """Every kernel that evaluates the pose models, this library against the PARENT commit's (--parent-lib, required, loaded beside
    this one), through the C ABI on handles of the same graph.  Host clock around whole calls, each ending in a stream synchronise, after
    a warm-up of every form; --repeats alternating rounds, the order of the two libraries turned round every other round; medians,
    ratio = here / parent in time, spread = (max - min) / median; all of it once with the parent's handles created first and once with
    this library's (ratio_balanced: the geometric mean of the two).  On the 100k-pose SE(3) ring with k = 5 (se3_graph: no relative
    rotation comes near the branch for the neighbourhood of pi, as in every graph the benchmarks run): `relin_all` --steps sweeps of
    gbp_lin_iterate_nonlinear at beta = 0, min_linear_iters = 0, where k_lin_relin<SE3> re-makes every factor in every sweep;
    `relin_none` the same at beta = +inf: an SE(3) sweep in which nothing relinearises; `energy` gbp_lin_energy (k_lin_energy_nl<SE3>);
    `linearise` gbp_lin_solve_map_nonlinear with max_outer = 0 (one k_gn_factor<SE3, true> launch); `reweight`
    gbp_lin_solve_map_nonlinear_robust with max_rounds = 0 and the Huber loss at 4 on every factor (one k_gn_reweight<SE3> launch).
    `se2_relin_all`: the first form on the 200k-pose SE(2) ring with k = 5 (se2_graph)."""
    import ctypes as ct
    from gbp_amd import _capi
    if not a.parent_lib:
        raise SystemExit("--model-cost needs --parent-lib")
    libs = {'here': _capi.load(), 'parent': ct.CDLL(os.path.abspath(a.parent_lib))}
    for lib in libs.values():
        for name in ('gbp_lin_solve_map_nonlinear', 'gbp_lin_solve_map_nonlinear_robust', 'gbp_lin_set_robust_nonlinear', 'gbp_lin_energy'):
            getattr(lib, name).restype = ct.c_int
    n = a.steps

    def lm0(h):
        o = _capi.LinNlmapOpts(0, 0, 1e-3, 10.0, 0.1, 1e-12, 1e8, 0.0, 0.0, _capi.LinMapOpts(1e-30, 8, 8, 0))
        t = time.perf_counter()
        assert h.lib.gbp_lin_solve_map_nonlinear(h.h, ct.byref(o), None, ct.byref(_capi.LinNlmapInfo())) == 0
        return 1e3 * (time.perf_counter() - t)

    def irls0(h):
        o = _capi.LinIrlsOpts(0, 0, 1e-9, 1e-10, _capi.LinNlmapOpts(4, 0, 1e-3, 10.0, 0.1, 1e-12, 1e8, 0.0, 0.0, _capi.LinMapOpts(1e-30, 8, 8, 0)))
        t = time.perf_counter()
        assert h.lib.gbp_lin_solve_map_nonlinear_robust(h.h, ct.byref(o), None, None, None, None, ct.byref(_capi.LinIrlsInfo())) == 0
        return 1e3 * (time.perf_counter() - t)

    def energy(h):
        out = ct.c_double()
        t = time.perf_counter()
        assert h.lib.gbp_lin_energy(h.h, ct.byref(out)) == 0
        return 1e3 * (time.perf_counter() - t)

    rec = {}

    def measure(order, forms):
        """forms: {name: (fn, handles by library)}"""
        for name, (fn, hs) in forms.items():
            for who in ('parent', 'here'):
                fn(hs[who])
        for i in range(a.repeats):
            for name, (fn, hs) in forms.items():
                for who in (('parent', 'here') if i % 2 == 0 else ('here', 'parent')):
                    rec.setdefault(name, {}).setdefault(order, {'parent': [], 'here': []})[who].append(fn(hs[who]))

    g3, g2 = se3_graph(100_000, 5, np.random.RandomState(0)), se2_graph(200_000, 5, np.random.RandomState(0))
    F3 = g3[0].shape[0]
    codes, thr = _capi.i32(np.ones(F3)), np.full(F3, 4.0)
    # where a handle's arrays land moves a sweep by several per cent: every form is measured with either library's handle created first
    for first in ('parent', 'here'):
        who = (first, 'here' if first == 'parent' else 'parent')
        order = first + '_created_first'
        all3 = {w: RawSE2(libs[w], *g3, 0.0, 0, model=2) for w in who}
        none3 = {w: RawSE2(libs[w], *g3, float('inf'), 2, model=2) for w in who}
        lossy3 = {w: RawSE2(libs[w], *g3, float('inf'), 2, model=2) for w in who}
        for h in lossy3.values():
            assert h.lib.gbp_lin_set_robust_nonlinear(h.h, 0, F3, _capi.iptr(codes), _capi.dptr(thr)) == 0
        measure(order, {'relin_all': (lambda h: h.sweeps(n), all3), 'relin_none': (lambda h: h.sweeps(n), none3), 'energy': (energy, none3),
                        'linearise': (lm0, none3), 'reweight': (irls0, lossy3)})
        for hs in (all3, none3, lossy3):
            for h in hs.values():
                h.close()
        all2 = {w: RawSE2(libs[w], *g2, 0.0, 0) for w in who}
        measure(order, {'se2_relin_all': (lambda h: h.sweeps(n), all2)})
        for h in all2.values():
            h.close()
    res = {}
    for name, by in rec.items():
        res[name] = {}
        for order, v in by.items():
            mp, mh = statistics.median(v['parent']), statistics.median(v['here'])
            res[name][order] = {"ms_parent": mp, "ms_here": mh, "ratio_here_over_parent": mh / mp, "spread_parent": (max(v['parent']) - min(v['parent'])) / mp,
                                "spread_here": (max(v['here']) - min(v['here'])) / mh, "ms_all_parent": v['parent'], "ms_all_here": v['here']}
        r1, r2 = (res[name][o]["ratio_here_over_parent"] for o in ('parent_created_first', 'here_created_first'))
        res[name]["ratio_balanced"] = (r1 * r2) ** 0.5
    print(json.dumps({"what": "tools/bench_linear.py --model-cost on one MI355X: the kernels that evaluate the SE(3) / SE(2) models, this library "
                              "against the parent commit's", "method": " ".join(model_cost_profile.__doc__.split()), "repeats": a.repeats,
                      "sweeps_per_call": n, "se3_factors": F3, "se2_factors": int(g2[0].shape[0]), "counters_collected": False, "results": res}))


if a.model_cost:
    model_cost_profile()
    sys.exit(0)
if a.nonlinear_map_robust:
    nonlinear_map_robust_profile()
    sys.exit(0)
if a.nonlinear_map:
    nonlinear_map_profile()
    sys.exit(0)
if a.nonlinear_se3:
    nonlinear_se3_profile()
    sys.exit(0)
if a.nonlinear_until:
    nonlinear_until_profile()
    sys.exit(0)
if a.nonlinear_robust:
    nonlinear_robust_profile()
    sys.exit(0)
if a.nonlinear_live:
    nonlinear_live_profile()
    sys.exit(0)
if a.nonlinear:
    nonlinear_profile()
    sys.exit(0)
if a.until:
    until_profile()
    sys.exit(0)
if a.shrink:
    shrink_profile()
    sys.exit(0)
if a.marginals:
    marginals_profile()
    sys.exit(0)
if a.extend:
    extend_profile()
    sys.exit(0)
if a.robust:
    robust_profile()
    sys.exit(0)
N, D, k = a.vars, a.dofs, a.k
(va, vb, fe, fl, pe, pl), fc = ring(N, D, k, np.random.RandomState(0))
F = va.shape[0]
e = LinearEngine(va, vb, fe, fl, pe, pl, factor_const=fc)
e.update_all_beliefs()
e.iterate(a.warmup); e.sync()
t0 = time.perf_counter(); e.iterate(a.steps); e.sync(); dt = time.perf_counter() - t0
map_res = None
if a.map:
    # the batch MAP by block-Jacobi CG (gbp_lin_solve_map), cold; the first call also makes the workspace and the diagonal-block
    # factors, so that is done by a product beforehand and kept out of the time per iteration
    e.joint_eta()
    tm = time.perf_counter(); _, info = e.solve_map(); tm = time.perf_counter() - tm
    ms_cg = 1e3 * tm / max(info['iters'], 1)
    map_res = {"cg_iters": info['iters'], "converged": info['converged'], "rel_residual": info['rel_residual'], "ms_per_cg_iter": ms_cg,
               "map_distance": e.map_distance(), "sweeps_before_distance": a.warmup + a.steps,
               "cg_iter_over_sweep": ms_cg / (1e3 * dt / a.steps)}
P = D * (D + 1) // 2
bytes_sweep = 8 * (F * (D * (2 * D + 1) + 2 * D + 6 * (D + P) + 2 * (D + P)) + N * (2 * (D + P) + D))
cpu = None
if not a.no_cpu_baseline:
    # bounded sample of the same workload for the numpy oracle (dense per-factor loops, one thread): the first 400 variables
    # of the ring with their factors, 3 sweeps; reported per factor-sweep and scaled to this graph
    from oracle.linear_oracle import LinearOracle
    n_s = 400
    sel = (va < n_s - k)
    o = LinearOracle(va[sel], vb[sel], fe[sel], np.ascontiguousarray(fl[sel]), pe[:n_s], np.ascontiguousarray(pl[:n_s]), factor_const=fc[sel])
    o.update_all_beliefs(); o.synchronous_iteration()
    tc = time.perf_counter(); o.iterate(3); tc = (time.perf_counter() - tc) / 3
    us_per_factor = 1e6 * tc / int(sel.sum())
    cpu = {"value": 1.0 / (us_per_factor * 1e-6 * F), "unit": "iter/s", "cores": 1, "kind": "port",
           "sample": f"numpy oracle (oracle/linear_oracle.py) on the first {n_s} variables / {int(sel.sum())} factors of the same ring, "
                     f"3 sweeps, {us_per_factor:.1f} us per factor-sweep, scaled to {F} factors"}
print(json.dumps({"metric": "linear GBP sweeps/s", "value": a.steps / dt, "unit": "iter/s", "ms_per_step": 1e3 * dt / a.steps,
                  "config": {"workload": f"ring pose graph {N} vars x {D} dofs, {F} linear_displacement factors"},
                  "dtype": "f64", "roofline": {"bound": "hbm", "achieved": bytes_sweep * a.steps / dt / 1e9, "peak": 8000.0,
                                               "unit": "GB/s", "frac": bytes_sweep * a.steps / dt / 1e9 / 8000.0, "traffic": None},
                  "energy_after": e.energy(), "map": map_res, "cpu_baseline": cpu}))
