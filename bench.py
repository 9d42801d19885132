#!/usr/bin/env python3
"""bench.py -- GBP iterations/s on the synthetic 500-cam x 100k-landmark x 1M-factor BA graph.

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]

A "step" is one FactorGraph.synchronous_iteration(robustify=True, local_relin=True) (gbp/gbp.py:86-92) over the whole
graph, inputs resident in HBM.  N > 1 shards the graph by landmark across N ranks, one process per GPU, one exchange of the
camera partial sums per iteration inside the library (gbp_ba_iterate_sharded): an RCCL all-gather, or peer stores straight into
the ranks' mailboxes over xGMI with no collective call (--exchange; the default measures both and reports the faster as `value`,
the other beside it); the total work is fixed, so scaling is "strong".  Started without torchrun, `--gpus N` spawns its own N ranks (re-exec under
torch.distributed.run on 127.0.0.1); started under torchrun it uses the ranks it is given.  Rank 0 prints ONE JSON line.

A plain run does only what its headline figure needs: it sets up the graph (generate_priors_var + update_all_beliefs), brings the
GPU's clocks up with ~SPIN_UP_S of throw-away replays, restores the state, runs W untimed sweeps, then EXACTLY K timed sweeps
bracketed by a barrier + device synchronisation on both sides (max over ranks), and prints the line: `value` = K / that time,
`ms_per_step` = that time / K.  `--dump-outputs DIR` writes what the last timed sweep left (timed_outputs(): beliefs, means and ARE,
float64) as DIR/<name>.npy; the inputs are seeded, so two builds can be compared array by array.
Everything below -- the repeated batches, the instrumented replays, the parity check, the CPU baselines, the HBM-bound size and, for
N > 1, the prediction and the secondary workload -- runs with `--full` only.

Timing protocol of --full.  Every batch starts from the same state -- the graph right after generate_priors_var +
update_all_beliefs, restored from a device-resident checkpoint -- runs W untimed sweeps and then EXACTLY K timed sweeps bracketed by a
barrier + device synchronisation on both sides (max over ranks).  Batches are repeated until >= 0.5 s have been timed;
`value` = K / median batch time, the minimum is reported beside it.  One extra, untimed replay of the same batch is
instrumented: workgroup 0 of every kernel of every sweep stores the device's constant-rate clock when it starts (consecutive start
stamps tile the stream's timeline the way rocprofv3's kernel durations do); a further replay brackets every 7th launch of the
dominant kernel with HIP events as a cross-check (an event pair also times the dispatch behind its barrier packet), and the device counts the factors that relinearise in each
sweep: steady sweeps (fewer than 1 factor in 1000 relinearises: the case SURVEY 8d's byte count describes) and relinearising
sweeps are reported separately.  N > 1 also prints per-rank device times (sweep / reduce + exchange / finish / step) and the
rank count the exchange itself reports.

Roofline bookkeeping.  `roofline.achieved` = the bytes the engine's data layout MUST move per launch of the dominant
kernel (`layout_bytes` below: F (21 read + 10 written doubles + 8 B of meta | state words) + L (a 20-double
record read + 9 doubles of mean | covariance written) + one 28-double table row per camera and workgroup) / the mean launch time over the timed region (all K launches; the steady subset is reported beside
it as `kernel_steady_ms`); `frac` = achieved / 8 TB/s, never above 1.  `traffic` = HBM
bytes per launch from the rocprofv3 PMC passes committed under profiles/ (not measured by this run).  The survey's 1072 B/factor model of a dense
two-pass implementation is kept only as `survey_equivalent_*`: this engine does that work in fewer bytes.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak, /opt/skills/guides/MI355X_MICROARCH.md:35
COPY_CEILING_GBS = 6290.0      # measured float4 copy on MI355X, same line of the guide: what a pure streaming kernel reaches
MIN_TIMED_S = 0.5
SPIN_UP_S = 0.3               # plain run: throw-away replays ahead of its one timed batch (clocks up after the host-side set-up)
STAMPS = 1 << 30              # gbp_ba_set_kernel_timing(STAMPS): device-clock stamps in every launch, HIP events around the first one only
EVENT_EVERY = 7               # HIP events bracket every 7th launch of the dominant kernel in the instrumented replay (cross-check)
CLK_RING = 4096               # sweeps the library keeps stamps for (gbp_capi.hip)
MAX_BATCHES = 2000          # (a 20-step batch of a 15 us sweep is 0.3 ms: the cap only bounds degenerate cases)


def survey_bytes(F, L, C):
    """fp64, packed-symmetric dense messages, two passes, steady-state iteration."""
    return F * 1072 + L * 168 + C * 480


def layout_bytes(F, L, C, n_blocks, fused, table_rows=None):
    """Bytes one launch of the dominant kernel must move in THIS engine's layout."""
    per_factor = (21 + 10) * 8 + 8        # x0 9 z 2 | messages 10 in, 10 out | meta 4 B + state 4 B in (a factor that only ages writes no state:
                                          # the word holds the clock value of its last relinearisation; PMC write traffic 138 -> 119 MB)
    per_lmk = 20 * 8 + 9 * 8              # record (mean 3 | covariance 6 | rows | prior 9 | pad) in, mean | covariance out
    if fused:                             # k_sweep_wat: + one table row (27 sums + 1 pad double) per camera and workgroup out (camera windows:
        return F * per_factor + L * per_lmk + (table_rows if table_rows else n_blocks * C) * 28 * 8      # per camera of the workgroup's window)
    # k_factor_tile: the same per-factor / per-landmark streams + what rebuilds the camera message, staged camera-major
    # (x0 9 | q_C 2 | W 3 in one whole 128-byte line, + cpos)
    return F * (per_factor + 16 * 8 + 4) + L * per_lmk


DUMP_LIMIT_BYTES = 64 << 20    # --dump-outputs writes at most this much


def timed_outputs(graph, limit=DUMP_LIMIT_BYTES):
    """(collective for N > 1: the ARE is summed over ranks) What a caller of the timed path holds after its last sweep, as float64
    arrays: the beliefs (information form) and means of every camera and landmark -- for N > 1 the landmarks of this rank's shard,
    `lmk_range` -- and the average reprojection error.  When they would exceed `limit` bytes, the landmark rows are a fixed sample
    (seed 0, ascending, listed in `lmk_sample_rows`); the cameras are always complete."""
    are = graph.are()
    eng = getattr(graph, 'engine', graph)
    ce, cl, le, ll = eng.beliefs()
    cm, lm = eng.means()
    out = dict(cam_eta=ce, cam_lam=cl, cam_mean=cm, lmk_eta=le, lmk_lam=ll, lmk_mean=lm, are=np.array([are]))
    if hasattr(graph, 'lmk_range'):
        out['lmk_range'] = np.array(graph.lmk_range, dtype=np.float64)
    lmk = ('lmk_eta', 'lmk_lam', 'lmk_mean')
    if sum(a.nbytes for a in out.values()) > limit:
        fixed = sum(a.nbytes for k, a in out.items() if k not in lmk)
        per_row = sum(out[k][:1].nbytes for k in lmk) + 8                  # (+ its entry in lmk_sample_rows)
        n = int(max(1, min(le.shape[0], (limit - fixed) // per_row)))
        rows = np.sort(np.random.default_rng(0).choice(le.shape[0], size=n, replace=False))
        out.update({k: out[k][rows] for k in lmk}, lmk_sample_rows=rows.astype(np.float64))
    return {k: np.ascontiguousarray(a, dtype=np.float64) for k, a in out.items()}


def library_fingerprint():
    """sha256 (16 hex digits) of the libgbp_hip.so this process runs: committed counter passes are tied to the binary they measured."""
    import hashlib
    from gbp_amd import _capi
    try:
        return hashlib.sha256(open(_capi.LIB_PATH, 'rb').read()).hexdigest()[:16]
    except OSError:
        return None


def host_cores():
    """Cores this process may really use: affinity mask, capped by the cgroup CPU quota when there is one."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else (os.cpu_count() or 1)
    try:
        quota, period = open('/sys/fs/cgroup/cpu.max').read().split()[:2]
        if quota != 'max':
            n = max(1, min(n, int(float(quota) / float(period))))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(problem, budget_s=20.0, engine=None):
    """Time the CPU oracle (oracle/gbp_oracle.c, a port of the reference's algorithm) on the same workload,
    bounded to ~budget_s of wall time: a few whole sweeps of the same graph at 1 thread and at several OpenMP widths.
    With `engine` (the measured graph, snapshot of its initial state taken): the engine replays as many sweeps as the oracle
    has done by then and the two average reprojection errors must agree to 1e-8 -- the checker's only other use here."""
    from oracle import oracle
    o = oracle.OracleBA.from_problem(problem, threads=1)
    o.generate_priors_var(50.0)
    o.update_all_beliefs()
    t0 = time.perf_counter()
    o.iterate(1)                                              # also the warm-up sweep
    dt1 = time.perf_counter() - t0
    best = (dt1, 1, 1)
    spent, sweeps = dt1, 1
    for threads in sorted({min(host_cores(), t) for t in (8, 32, 64, host_cores())}):
        if threads == 1 or spent > budget_s:
            continue
        o.set_threads(threads)
        o.iterate(1)
        n = int(max(1, min(10, (budget_s - spent) / 4 // max(best[0], 1e-3))))
        t0 = time.perf_counter()
        o.iterate(n)
        dt = (time.perf_counter() - t0) / n
        spent += dt * (n + 1)
        sweeps += n + 1
        if dt < best[0]:
            best = (dt, threads, n)
    out = {"value": 1.0 / best[0], "unit": "iter/s", "cores": best[1], "kind": "port",
           "sample": f"{best[2]} whole sweeps of the same {problem.n_factors}-factor graph (after warm-up), C oracle with "
                     f"OpenMP over factors/variables, best of several thread counts on {host_cores()} usable cores",
           "value_1thread": 1.0 / dt1, "us_per_factor_iter_1thread": dt1 / problem.n_factors * 1e6}
    if engine is not None:
        while sweeps < 10 and spent < 2 * budget_s:          # through the first relinearising sweep (sweep 8) when the budget allows
            t0 = time.perf_counter(); o.iterate(1); spent += time.perf_counter() - t0; sweeps += 1
        engine.restore_snapshot()
        engine.iterate(sweeps)
        a_e, a_o = engine.are(), o.are()
        gap = abs(a_e - a_o) / abs(a_o)
        out["are_check"] = {"sweeps": sweeps, "engine": a_e, "oracle": a_o, "rel_gap": gap, "ok": bool(gap < 1e-8)}
        if gap >= 1e-8:
            print(f"[bench] WARNING: ARE after {sweeps} sweeps: engine {a_e!r} vs oracle {a_o!r} (rel {gap:.2e})", file=sys.stderr)
    return out


def cpu_baseline_numpy(problem, budget_s=15.0):
    """the numpy restatement with the reference's cost model (one Python object per factor, ~40 numpy calls per
    factor and sweep) at 1 thread -- only sensible on the small graphs of BASELINE configs 2-3."""
    from oracle.numpy_ba import NumpyBA
    n = NumpyBA(problem)
    n.generate_priors_var(50.0)
    n.update_all_beliefs()
    t0 = time.perf_counter()
    n.iterate(1)
    dt = time.perf_counter() - t0
    k = int(max(0, min(5, (budget_s - dt) // max(dt, 1e-3))))
    if k:
        t0 = time.perf_counter()
        n.iterate(k)
        dt = (time.perf_counter() - t0) / k
    return {"value": 1.0 / dt, "unit": "iter/s", "cores": 1, "kind": "port",
            "sample": f"{max(k, 1)} whole sweeps of the same {problem.n_factors}-factor graph, object-per-factor numpy graph (oracle/numpy_ba.py)",
            "us_per_factor_iter": dt / problem.n_factors * 1e6}


def measured_traffic():
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 PMC passes (profiles/rNN_hbm_traffic.json), but only
    when they were taken on THIS binary (the file records the library's sha256): a stale counter file is reported as such, not used."""
    import glob
    files = sorted(glob.glob(os.path.join(REPO, 'profiles', 'r*_hbm_traffic.json')))
    if not files:
        return None, "no committed counter pass"
    try:
        d = json.load(open(files[-1]))
    except (OSError, ValueError):
        return None, "unreadable counter file"
    name = os.path.basename(files[-1])
    if d.get('library_sha256_16') != library_fingerprint():
        return None, f"profiles/{name} was measured on another build of libgbp_hip.so ({d.get('library_sha256_16')}): not applicable to this binary"
    return d.get('traffic_bytes_per_launch'), name


PEER_NOTE = {}            # why the peer-store exchange was not measured (rank-local: whatever THIS rank saw)


def try_peer_exchange(args, problem, local_rank, dist, torch, measure, rccl_graph, side_dev='cuda', per_rank_of=None):
    """N > 1: the same job once more with the peer-store exchange (gbp_ba_peer_connect: the reduce kernels store the camera partial
    sums straight into every rank's mailbox over xGMI, the finish kernels poll arrival words; no collective call).  Every step
    is agreed on by all ranks; any failure (IPC handles, a time-out in the two-sweep probe) just returns None.  Returns the
    measure() dict + `matches_rccl`: camera beliefs after two sweeps from the same start are bitwise those of the RCCL path."""
    from gbp_amd.sharded import ShardedBA
    os.environ.setdefault('GBP_PEER_TIMEOUT_MS', '3000')

    def agreed(ok):
        t = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64, device=side_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(t.item() > 0.5)

    g = None
    try:
        g = ShardedBA(problem, device=local_rank, fused=False if args.no_fused else None, exchange='peer')
        ok = g.exchange == 'peer'
        if not ok:
            PEER_NOTE['reason'] = f"peer-store exchange not available, ShardedBA used {g.exchange!r} instead ({g.exchange_fallback})"
    except Exception as e:                                     # noqa: BLE001
        print(f"[bench] peer-store exchange unavailable: {e}", file=sys.stderr)
        PEER_NOTE['reason'] = f"peer-store exchange unavailable: {e}"
        ok = False
    if not agreed(ok):
        if g is not None:
            g.close()
        return None
    try:
        g.generate_priors_var(50.0)
        g.update_all_beliefs()
        g.iterate(2)
        g.sync()                                               # reports a finish kernel that gave up waiting
        ok = True
    except Exception as e:                                     # noqa: BLE001
        print(f"[bench] peer-store exchange probe failed: {e}", file=sys.stderr)
        PEER_NOTE['reason'] = f"two-sweep probe of the peer-store exchange failed: {e}"
        ok = False
    if not agreed(ok):
        g.close()
        return None
    rccl_graph.restore_snapshot()
    rccl_graph.iterate(2)
    a, b = rccl_graph.camera_beliefs(), g.camera_beliefs()
    match = agreed(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]))
    try:
        m = measure(g, min_timed_s=MIN_TIMED_S / 2)
        m['matches_rccl'] = match
    except Exception as e:                                     # noqa: BLE001
        print(f"[bench] peer-store exchange run failed: {e}", file=sys.stderr)
        PEER_NOTE['reason'] = f"the timed run with the peer-store exchange failed: {e}"
        m = None
    ok = agreed(m is not None)
    if ok and per_rank_of is not None:
        m['per_rank'] = per_rank_of(m, g)                      # (collective: every rank has a measurement at this point)
    g.close()
    return m if ok else None


G9B = os.path.join(REPO, 'tests', 'golden', 'G9b_synthetic_full_1000000.npz')


def parity_check(graph, problem, dist, torch, side_dev, world, local_rank, n_sweeps=10, default_graph=True):
    """Outside the timed region, every rank: the first ten sweeps of the batch schedule once more, against fixture G9b -- the
    REFERENCE's own run of this very graph (tests/golden/make_g9b.py: 500 camera beliefs after sweep 10, the ARE after every sweep).
    Makes a multi-GPU line self-proving: (i) camera beliefs bitwise equal on all ranks, (ii) < 1e-6 from the reference's at sweep 10,
    (iii) the ARE trace, (iv) how many ranks the exchange itself reports and how many distinct devices they sit on."""
    out = {"fixture": None, "ok": None}
    is_headline = (default_graph and problem.n_factors == 1_000_000 and problem.n_cams == 500 and problem.n_lmks == 100_000 and os.path.exists(G9B))
    g = np.load(G9B) if is_headline else None
    graph.restore_snapshot()
    ares = [graph.are()]
    for _ in range(n_sweeps):
        graph.iterate(1)
        ares.append(graph.are())
    graph.sync()
    ce, cl = (graph.camera_beliefs() if hasattr(graph, 'camera_beliefs') else graph.beliefs()[:2])
    flat = np.concatenate([np.asarray(ce, dtype=np.float64).ravel(), np.asarray(cl, dtype=np.float64).ravel()])
    if dist is not None and world > 1:
        lo = torch.tensor(flat, dtype=torch.float64, device=side_dev)
        hi = lo.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        out["camera_beliefs_bitwise_equal_across_ranks"] = bool(torch.equal(lo, hi))
        ids = [None] * world
        try:
            pr = torch.cuda.get_device_properties(local_rank)
            me = str(getattr(pr, 'uuid', None) or (getattr(pr, 'pci_domain_id', 0), getattr(pr, 'pci_bus_id', local_rank), getattr(pr, 'pci_device_id', 0)))
        except Exception:                                        # noqa: BLE001
            me = f"unknown-{local_rank}"
        dist.all_gather_object(ids, me)
        out["distinct_devices"] = len(set(ids))
        out["one_rank_per_device"] = len(set(ids)) == world
    in_library = getattr(graph, 'library_loop', True)            # (the Python-driven loop exchanges through torch.distributed: the library has no rank count to report)
    if hasattr(graph, 'comm_info') and in_library:
        try:
            out["ranks_reported_by_exchange"] = int(graph.comm_info()['n_ranks'])
        except Exception:                                        # noqa: BLE001
            pass
    out["sweeps"] = n_sweeps
    out["are_trace"] = [float(a) for a in ares]
    if g is not None:
        def gap(a, b):
            a, b = np.asarray(a).reshape(a.shape[0], -1), np.asarray(b).reshape(b.shape[0], -1)
            return float((np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)).max())
        out["fixture"] = "tests/golden/G9b_synthetic_full_1000000.npz (the reference's own ten sweeps of this graph)"
        out["camera_belief_gap_vs_reference"] = max(gap(ce, g[f'it{n_sweeps}_cam_eta']), gap(cl, g[f'it{n_sweeps}_cam_lam']))
        ref = np.asarray(g['are_trace'], dtype=np.float64)[:n_sweeps + 1]
        out["are_trace_max_rel_err"] = float(np.max(np.abs(np.asarray(ares) - ref) / np.abs(ref)))
        ok = out["camera_belief_gap_vs_reference"] < 1e-6 and out["are_trace_max_rel_err"] < 1e-6
        if world > 1:
            ok = ok and out.get("camera_beliefs_bitwise_equal_across_ranks", False) and (not in_library or out.get("ranks_reported_by_exchange") == world)
        out["ok"] = bool(ok)
        out["tolerance"] = "camera beliefs (eta, Lambda) 1e-6 relative per camera, ARE 1e-6 relative per sweep (BASELINE north_star: 1e-4)"
    return out


def free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    return port


class Preflight(Exception):
    """A multi-GPU run cannot start on this node as asked; the message says exactly why."""


def preflight(n, device_count, can_access_peer, device_name=lambda i: None, share_gpu=False):
    """`--gpus N`, before anything is spawned or initialised: are there N devices, and can every pair reach each other (the peer-store
    exchange writes into the other ranks' memory; RCCL falls back to host staging without it, at a fraction of the xGMI rate)?  Pure
    logic over three callables (torch.cuda.device_count / can_device_access_peer / get_device_name in bench.py itself;
    tests/test_bench_launch.py passes doubles).  Returns the topology that goes into the JSON line (`config.topology`); raises Preflight.
    share_gpu (GBP_BENCH_SHARE_GPU, one-GPU test boxes): every rank sits on device 0, nothing to check between devices."""
    have = int(device_count())
    if share_gpu:
        if have < 1:
            raise Preflight("no GPU visible (GBP_BENCH_SHARE_GPU puts every rank on device 0)")
        return {"devices": 1, "ranks": n, "shared_gpu": True, "names": [device_name(0)], "peer_access": None}
    if have < n:
        raise Preflight(f"--gpus {n} but only {have} device(s) visible to this process "
                        f"(HIP_VISIBLE_DEVICES={os.environ.get('HIP_VISIBLE_DEVICES')!r}, ROCR_VISIBLE_DEVICES={os.environ.get('ROCR_VISIBLE_DEVICES')!r})")
    missing = [(i, j) for i in range(n) for j in range(n) if i != j and not can_access_peer(i, j)]
    topo = {"devices": have, "ranks": n, "shared_gpu": False, "names": [device_name(i) for i in range(n)],
            "peer_access": "all pairs" if not missing else {"missing": missing}}
    if missing:
        raise Preflight(f"devices {missing[0][0]} and {missing[0][1]} cannot access each other's memory (hipDeviceCanAccessPeer; "
                        f"{len(missing)} of {n * (n - 1)} ordered pairs fail): the landmark-sharded sweep needs peer access between all ranks")
    return topo


def torch_preflight(n):
    import torch
    share = bool(os.environ.get('GBP_BENCH_SHARE_GPU'))
    if not torch.cuda.is_available():
        raise Preflight("no GPU visible: bench.py times the HIP engine on MI355X and has no CPU fallback")
    return preflight(n, torch.cuda.device_count, torch.cuda.can_device_access_peer, torch.cuda.get_device_name, share)


def error_line(args, msg, fd=1):
    """A run that cannot start still prints ONE JSON line -- with "error" and no value -- and exits non-zero: a driver's record then
    says why, instead of holding the traceback of whichever rank died first."""
    out = {"metric": "GBP iterations/sec (whole node), 1M-factor BA graph", "value": None, "unit": "iter/s", "n_gpus": args.gpus, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": None, "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
           "data": "synthetic", "error": msg}
    os.write(fd, (json.dumps(out) + '\n').encode())
    print(f"[bench] {msg}", file=sys.stderr)


EXIT_PREFLIGHT = 3


def spawn_ranks(n, script=None):
    """`python bench.py --gpus N` outside torchrun: become the launcher of N ranks of this very command line."""
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.setdefault('OMP_NUM_THREADS', str(max(1, host_cores() // n)))
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={n}', '--master-addr', '127.0.0.1',
           '--master-port', str(free_port()), os.path.abspath(script or __file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def main(shard_factory=None, script=None):
    """shard_factory / script: NOT reachable from the command line.  tests/tools/bench_dry_launch.py -- test infrastructure, run in the
    build container where there is no GPU -- passes a double for a rank's engine and its own path, so that the launch path (spawning
    the ranks, rendezvous, the one JSON line) can be exercised without a device; such a line is marked "dry_run" and measures nothing."""
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--cams', type=int, default=500)
    ap.add_argument('--lmks', type=int, default=100_000)
    ap.add_argument('--obs', type=int, default=10)
    ap.add_argument('--window', type=int, default=None, help='a SEQUENCE instead of the headline graph: every landmark is seen from --obs of this many '
                    'consecutive cameras (make_synthetic(window=...)); the fused sweep then runs with per-workgroup camera windows')
    ap.add_argument('--bal', default=None, help='BAL text file instead of the synthetic graph (BASELINE configs 2-3, e.g. '
                                                'tests/golden/data/fr1desk.txt); not the headline workload')
    ap.add_argument('--closures', type=float, default=0.0, help='with --window: this fraction of the landmarks is seen from anywhere along the trajectory')
    ap.add_argument('--no-fused', action='store_true')
    ap.add_argument('--full', action='store_true',
                    help='everything beside the headline figure: batches repeated until >= 0.5 s are timed, the instrumented replays behind '
                         '`roofline` and `per_rank`, the parity check against fixture G9b, the CPU baselines, the 2M-factor HBM-bound replay, '
                         'and for N > 1 the prediction and the secondary workload.  Without it: set up, W warm-up sweeps, K timed sweeps, one line')
    ap.add_argument('--dump-outputs', default=None, metavar='DIR',
                    help='after the timed sweeps, write what the last timed sweep left (beliefs, means, ARE) as DIR/<name>.npy (float64)')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='(--full) skip the CPU baselines')
    ap.add_argument('--no-hbm-size', action='store_true', help='(--full) skip the 2M-factor replay behind roofline.frac_hbm_bound')
    ap.add_argument('--single-batch', action='store_true', help='(--full) one timed batch only (profiling runs)')
    ap.add_argument('--sharded', action='store_true', help='take the N > 1 code path (process group, ShardedBA, RCCL exchange forced) even with one rank')
    ap.add_argument('--exchange', default='auto', choices=['auto', 'rccl', 'peer'],
                    help='N > 1: how the camera partial sums travel.  rccl = one ncclAllGather per sweep on the library\'s communicator; peer = '
                         'direct stores into the ranks\' mailboxes, no collective; auto = measure rccl, then peer, report the faster as `value` '
                         'and the other beside it')
    ap.add_argument('--python-loop', action='store_true', help='N > 1: drive the sweeps from Python (shard_begin / all_gather / shard_end)')
    ap.add_argument('--dump-sweeps', default=None, help='(--full) write the per-sweep kernel times (ms) and relinearisation counts of the instrumented replay to this .npz')
    ap.add_argument('--backend', default='nccl', help='torch.distributed backend of the side channel (tests: gloo)')
    ap.add_argument('--secondary-lmks', type=int, default=800_000, help='(--full) N > 1: landmarks of the SECONDARY, bandwidth-bound workload timed after the headline '
                    'one (default 800 000 = 8M factors: 1M per rank at N = 8; every rank makes its own share against the shared cameras); 0 = skip')
    args = ap.parse_args()
    if args.dump_sweeps and not args.full:
        ap.error('--dump-sweeps writes what the instrumented replay of --full recorded: give --full as well')

    dry = shard_factory is not None
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        if not dry:                                               # the launcher itself looks at the node first: nothing is spawned onto a node that cannot run the job
            try:
                torch_preflight(args.gpus)
            except Preflight as e:
                error_line(args, str(e))
                raise SystemExit(EXIT_PREFLIGHT)
        raise SystemExit(spawn_ranks(args.gpus, script))

    # Only the JSON line may reach stdout: native libraries (RCCL prints a version banner at communicator creation) write to
    # file descriptor 1 directly, so the descriptor itself is pointed at stderr and the result goes out through a saved copy.
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    import torch
    rank = int(os.environ.get('RANK', '0'))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    side_dev = 'cpu' if (dry or args.backend == 'gloo') else 'cuda'      # where the side channel's few scalars live
    if os.environ.get('GBP_BENCH_SHARE_GPU'):                             # tests on a one-GPU box: every rank on device 0 (gloo + peer exchange)
        local_rank = 0
    topology = None
    if not dry:
        # Every rank of a torchrun launch looks at the node before the process group exists (all ranks see the same devices, so all
        # take the same way out: no rank is left waiting in a rendezvous); rank 0 prints the line.
        try:
            topology = torch_preflight(world)
        except Preflight as e:
            if rank == 0:
                error_line(args, str(e), json_fd)
            raise SystemExit(EXIT_PREFLIGHT)
        torch.cuda.set_device(local_rank)

    if args.bal:
        from gbp_amd.balio import read_bal
        problem = read_bal(args.bal)
        workload = f"BAL file {os.path.basename(args.bal)}"
    else:
        from gbp_amd.synthetic import make_synthetic
        problem = make_synthetic(n_cams=args.cams, n_lmks=args.lmks, obs_per_lmk=args.obs, seed=0, window=args.window, closures=args.closures)
        workload = "synthetic BAL" if args.window is None else f"synthetic sequence (window {args.window}, closures {args.closures})"
    F, L, C = problem.n_factors, problem.n_lmks, problem.n_cams

    # one node: the collectives' bootstrap sockets need no NIC and no resolvable hostname (the data path is xGMI either way)
    os.environ.setdefault('NCCL_SOCKET_IFNAME', 'lo')
    dist = None
    if world > 1 or dry or args.sharded:
        import torch.distributed as dist
        from gbp_amd.sharded import ShardedBA
        if dry:
            dist.init_process_group(args.backend)
            graph = ShardedBA(problem, engine_factory=shard_factory)
        else:
            if 'MASTER_ADDR' not in os.environ:                     # --sharded without torchrun: a one-rank group of our own
                os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(free_port()), RANK='0', WORLD_SIZE='1', LOCAL_RANK='0')
            dist.init_process_group(args.backend, **({} if args.backend == 'gloo' else {'device_id': torch.device('cuda', local_rank)}))
            graph = ShardedBA(problem, device=local_rank, fused=False if args.no_fused else None, library_loop=not args.python_loop,
                              always_exchange=args.sharded, exchange='peer' if args.exchange == 'peer' else 'rccl')
    else:
        from gbp_amd.engine import BAEngine
        graph = BAEngine.from_problem(problem, device=local_rank, fused=False if args.no_fused else None)      # None: the library picks the sweep, as for any user

    def fence():
        if dist is not None:
            dist.barrier()
        if not dry:
            torch.cuda.synchronize()

    def measure(graph, min_timed_s=MIN_TIMED_S, dump=True):
        """The timing protocol on one graph object: returns batch times (+ with --full the kernel-level picture of one instrumented
        replay; + with --dump-outputs what the last timed batch left in the graph, taken before anything else runs on it)."""
        graph.generate_priors_var(50.0)
        graph.update_all_beliefs()
        graph.sync()
        if not dry:
            graph.snapshot_state()                             # device-resident: restoring it leaves no idle gap before the sweeps

        spin = [0]                                             # throw-away sweeps ahead of an instrumented replay (set below)

        def batch(timing=0):
            """Restore the initial state, W untimed sweeps, then K sweeps between two fences.  Returns wall seconds (max over ranks)."""
            stamps = timing == STAMPS
            if stamps:                                             # before the warm-up: switching the stamps on costs host time
                graph.set_kernel_timing(timing)
            if timing and not dry:
                # The host work around an instrumented replay (switching the stamps on, reading them back, numpy) leaves the GPU idle
                # for milliseconds; it drops its clocks, and a 20-sweep batch is over before they are back: such replays measured
                # sweeps 4-9 % longer than the timed batches they stand for.  About 25 ms of throw-away sweeps put the clocks where the
                # back-to-back timed batches find them.  They are whole replays of the batch (restore, W + K sweeps), so that every launch
                # of the process is one of the schedule's sweeps and rocprofv3's average over ALL launches of this command is an average
                # of the same sweeps `value` times (sweeps that simply ran on from wherever the state was sat deep in the regime where
                # factors relinearise every sweep, and pulled that average 6 % above the timed one).
                for _ in range(spin[0] // (args.warmup + args.steps)):
                    graph.restore_snapshot()
                    graph.iterate(args.warmup + args.steps)
            if not dry:
                graph.restore_snapshot()
            graph.iterate(args.warmup)
            graph.sync()
            if timing and not stamps:
                graph.set_kernel_timing(timing)
            fence()
            t0 = time.perf_counter()
            graph.iterate(args.steps)
            graph.sync()
            fence()
            dt = time.perf_counter() - t0
            if dist is not None:
                t = torch.tensor([dt], dtype=torch.float64, device=side_dev)
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                dt = float(t.item())
            return dt

        if args.full:
            batch()                                           # untimed: page in code, caches, clocks
            times = [batch()]
            while not args.single_batch and sum(times) < min_timed_s and len(times) < MAX_BATCHES:
                times.append(batch())
        else:
            # The host-side set-up leaves the GPU idle long enough to drop its clocks, and W warm-up sweeps (1.4 ms at W = 20) do not bring
            # them back: a cold K = 200 batch measured 13 % above the median of --full.  ~SPIN_UP_S of throw-away replays (restore + at most
            # 200 sweeps each) go first, as the untimed batch of --full does; batch() restores the state, so the timed sweeps are the same.
            if not dry:
                t_end = time.perf_counter() + SPIN_UP_S
                while True:
                    graph.restore_snapshot()
                    graph.iterate(min(args.warmup + args.steps, 200))
                    graph.sync()
                    done = time.perf_counter() >= t_end
                    if dist is not None:                       # (every rank runs the same number of replays: they contain exchanges)
                        t = torch.tensor([0.0 if done else 1.0], dtype=torch.float64, device=side_dev)
                        dist.all_reduce(t, op=dist.ReduceOp.MAX)
                        done = float(t.item()) < 0.5
                    if done:
                        break
            times = [batch()]                                 # W warm-up sweeps, then exactly K timed
        m = dict(times=np.array(times), ev_ms=np.zeros(0), clk=np.zeros((0, 6)), relin=np.zeros(0, np.int64), k_name='')
        if dump and args.dump_outputs:
            m['outputs'] = timed_outputs(graph)
        if args.full and not dry:
            # One more, untimed replay of the same batch, instrumented: every kernel of every sweep stamps the device's
            # constant-rate clock (first workgroup in, last workgroup out), and HIP events bracket every EVENT_EVERY-th launch of
            # the dominant kernel as a cross-check (an event pair around a launch also times the dispatch behind the event's
            # barrier packet and serialises the stream, so it is neither put around every launch nor used for the roofline).
            # (A single replay can land on a slow patch -- one in a few is 5 % off the median batch -- so the replay is repeated and the
            #  one whose device step is closest to the median batch time is the one reported: the picture of a TYPICAL batch.)
            want_us = float(np.median(times)) / args.steps * 1e6
            per = args.warmup + args.steps                     # (whole batches, and what the stamp ring holds besides the measured one)
            spin[0] = per * int(min(max(1, -(-25e3 // (want_us * per))), max(0, (CLK_RING - per) // per)))
            for rep in range(3):
                batch(timing=STAMPS)                           # stamps only (events around the first launch alone)
                clk = graph.sweep_clocks()[spin[0] + args.warmup:spin[0] + args.warmup + args.steps]      # (the throw-away and warm-up sweeps are stamped too)
                graph.set_kernel_timing(0)
                step_us = float(np.nanmean(np.diff(clk[:, 0]))) if clk.shape[0] > 1 else want_us
                if rep == 0 or abs(step_us - want_us) < abs(best_us - want_us):
                    m['clk'], best_us = clk, step_us
                done = abs(best_us - want_us) <= 0.015 * want_us
                if dist is not None:                           # (every rank runs the same number of replays: they contain barriers)
                    t = torch.tensor([0.0 if done else 1.0], dtype=torch.float64, device=side_dev)
                    dist.all_reduce(t, op=dist.ReduceOp.MAX)
                    done = float(t.item()) < 0.5
                if done:
                    break
            batch(timing=EVENT_EVERY)
            m['ev_ms'] = graph.kernel_times()
            _, _, m['k_name'] = graph.kernel_timing()
            graph.set_kernel_timing(0)
            if args.steps <= 512:
                m['relin'] = np.asarray(graph.relin_counts(args.steps), dtype=np.int64)
        m['are'] = graph.are() if args.full else None
        return m

    def kernel_picture(m, F_total):
        """Per-sweep device times (ms) from the clock stamps, split into steady and relinearising sweeps."""
        clk, relin = m['clk'], m['relin']
        n = clk.shape[0]
        pic = dict(n=n)
        if not n:
            return pic
        # START stamps tile the timeline like rocprofv3's kernel durations do: a kernel's interval runs from its workgroup 0 to
        # workgroup 0 of the next kernel (its own drain and the next dispatch included).
        step = np.diff(clk[:, 0]) * 1e-3                          # sweep start to next sweep start
        nxt = np.append(clk[1:, 0], np.nan)                      # start of the next sweep
        sweep = (clk[:, 2] - clk[:, 0]) * 1e-3
        sharded_step = np.isfinite(clk[:, 4])
        reduce_ = (np.where(sharded_step, clk[:, 4], nxt) - clk[:, 2]) * 1e-3     # (with an exchange in between: reduce + exchange, see xch)
        finish = (nxt - clk[:, 4]) * 1e-3
        xch = np.full(n, np.nan)                                  # not separable from the reduce by start stamps alone: reported together
        steady = relin * 1000 < F_total if relin.size == n else np.ones(n, bool)   # fewer than 1 factor in 1000 relinearises
        if not steady.any():
            steady = np.ones(n, bool)
        ok = steady & np.isfinite(sweep)
        pic.update(sweep=sweep, reduce=reduce_, finish=finish, xch=xch, step=step, steady=steady, ok=ok,
                   ev_idx=np.arange(0, n, EVENT_EVERY)[:m['ev_ms'].size])
        return pic

    def mean_ms(x, mask=None):
        x = np.asarray(x, dtype=float)
        if mask is not None:
            x = x[mask[:x.size]]
        x = x[np.isfinite(x)]
        return float(x.mean()) if x.size else None

    def gather_per_rank(m, g=None):
        """(collective) per-rank device times of the instrumented replay, and each rank's own roofline: the bytes ITS shard's layout must
        move per launch of the sweep kernel / that rank's mean launch time (the N > 1 counterpart of `roofline`: judgeable per device)"""
        g = graph if g is None else g
        pic = kernel_picture(m, F)
        if dist is None or dry or not pic['n']:
            return None
        info = g.info()
        fused = bool(info.get('fused'))
        pl = getattr(g, 'engine', g).plan_info()
        lay = layout_bytes(g.F, g.L, C, info.get('n_blocks', 0), fused, pl.get('table_rows') if pl.get('max_window') else None)
        mine = [mean_ms(pic[k], pic['ok']) or 0.0 for k in ('sweep', 'reduce', 'finish')] + [mean_ms(pic['step'], pic['ok'][:-1]) or 0.0,
                float(g.F), float(g.comm_info()['n_ranks']), float(g.L), float(lay), 1.0 if fused else 0.0,
                mean_ms(pic['sweep'], np.isfinite(pic['sweep'])) or 0.0]
        t = torch.tensor(mine, dtype=torch.float64, device=side_dev)
        allr = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(allr, t)
        out = []
        for r, v in enumerate(x.cpu().tolist() for x in allr):
            k_ms = v[9]                                           # all timed launches of this rank's sweep kernel (like roofline.kernel_avg_ms)
            gbs = v[7] / (k_ms * 1e-3) / 1e9 if k_ms > 0 else 0.0
            out.append(dict(rank=r, sweep_ms=v[0], reduce_and_exchange_ms=v[1], finish_ms=v[2], step_ms_device=v[3], n_factors=int(v[4]),
                            ranks_reported_by_exchange=int(v[5]), n_lmks=int(v[6]), sweep="fused" if v[8] > 0.5 else "general",
                            roofline={"bound": "hbm", "kernel_avg_ms": k_ms, "bytes_per_launch": int(v[7]), "achieved": gbs, "peak": HBM_PEAK_GBS,
                                      "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS}))
        return out

    def hbm_bound_size():
        """The headline graph's working set (~240 MB) sits inside the MI355X's 256 MiB memory-side cache, and the counters behind
        `traffic` sit in front of it.  The same sweep on twice the landmarks (2M factors, ~480 MB per sweep: all of it HBM) is timed
        beside it -- one short instrumented batch, outside the timed region -- so that the cache-assisted and the HBM-bound fraction
        travel together in one line."""
        from gbp_amd.engine import BAEngine
        from gbp_amd.synthetic import make_synthetic
        big = make_synthetic(n_cams=args.cams, n_lmks=2 * args.lmks, obs_per_lmk=args.obs, seed=0, window=args.window, closures=args.closures)
        g = BAEngine.from_problem(big, device=local_rank)
        try:
            g.generate_priors_var(50.0); g.update_all_beliefs(); g.sync(); g.snapshot_state()
            # Five replays, median reported with the range beside it (a best-of-three is optimistic by construction on
            # a quantity that lands in one of two modes ~6 % apart from process to process, EXPERIMENTS.md round 5).
            REPLAYS = 5
            ks_all, ks_steady = [], []
            n_steady = 0
            for rep in range(REPLAYS):
                g.set_kernel_timing(STAMPS)                        # (before the warm-up, as in batch())
                for _ in range(6):                                 # (clocks up with whole replays of the batch: see batch())
                    g.restore_snapshot(); g.iterate(25)
                g.restore_snapshot(); g.iterate(5); g.sync()
                g.iterate(20); g.sync()
                clk = g.sweep_clocks()[155:175]
                relin = np.asarray(g.relin_counts(20), dtype=np.int64)
                g.set_kernel_timing(0)
                sw = (clk[:, 2] - clk[:, 0]) * 1e-3
                ks_all.append(float(np.nanmean(sw)))
                steady = (relin * 1000 < big.n_factors) & np.isfinite(sw)          # the sweeps SURVEY 8d's byte count describes: nobody relinearises
                if steady.any():
                    ks_steady.append(float(sw[steady].mean()))
                    n_steady = int(steady.sum())
            # the bytes of the sweep that RAN: the plan says whether it was the fused sweep and how many table rows it wrote
            info, plan = g.info(), g.plan_info()
            fused_big = bool(info.get('fused'))
            lay = layout_bytes(big.n_factors, big.n_lmks, big.n_cams, info.get('n_blocks', 0), fused_big,
                               plan.get('table_rows') if plan.get('max_window') else None)

            def frac_of(ms, peak=HBM_PEAK_GBS):
                return lay / (ms * 1e-3) / 1e9 / peak
            k_med, k_min, k_max = float(np.median(ks_all)), min(ks_all), max(ks_all)
            # Rounds 4-5: two modes ~6 % apart (0.455-0.48 | 0.50-0.51 at 2M factors) by where the driver had put the pages.  Since round 6 the
            # sweep of these sizes walks its tiles strided and every placement measured lands at 0.53-0.55: "slow" would be a regression.
            mode = "fast" if frac_of(k_med) >= 0.49 else "slow"
            out = {"n_factors": int(big.n_factors), "n_lmks": int(big.n_lmks), "sweep": "fused" if fused_big else "general",
                   "kernel_avg_ms": k_med, "kernel_avg_ms_range": [k_min, k_max], "replays": REPLAYS, "bytes_per_launch": lay,
                   "achieved": lay / (k_med * 1e-3) / 1e9, "frac": frac_of(k_med), "frac_range": [frac_of(k_max), frac_of(k_min)],
                   "frac_of_copy_ceiling": frac_of(k_med, COPY_CEILING_GBS), "mode": mode,
                   "note": "same kernel, sweeps 6-25 of the batch schedule (two of them relinearise every factor and move 72 B per factor more than "
                           f"bytes_per_launch counts), MEDIAN of {REPLAYS} replays with min / max beside it; state >> the 256 MiB memory-side cache; "
                           "`mode`: rounds 4-5 landed in one of two modes ~6 % apart by memory placement (0.455-0.48 | 0.50-0.51); the strided tile walk of round 6 "
                           "removed that (0.53-0.55 in every placement measured): 'slow' (< 0.49) would be a regression"}
            if ks_steady:
                s_med = float(np.median(ks_steady))
                out.update({"kernel_steady_ms": s_med, "kernel_steady_ms_range": [min(ks_steady), max(ks_steady)], "kernel_steady_launches": n_steady,
                            "frac_steady": frac_of(s_med), "frac_steady_range": [frac_of(max(ks_steady)), frac_of(min(ks_steady))],
                            "frac_steady_of_copy_ceiling": frac_of(s_med, COPY_CEILING_GBS)})
            return out
        finally:
            g.close()

    def assemble(m, alt, exchange_used, per_rank, pc, hbm=None):
        """(rank 0) the JSON line of one measurement"""
        times = m['times']
        dt_med, dt_min = float(np.median(times)), float(times.min())
        are = m['are']
        pic = kernel_picture(m, F)
        info = dict(fused=False, n_blocks=0) if dry else graph.info()
        its = args.steps / dt_med
        F_local, L_local = graph.F, graph.L
        fused = bool(info.get('fused'))
        plan = {} if dry else getattr(graph, 'engine', graph).plan_info()
        lay = layout_bytes(F_local, L_local, C, info.get('n_blocks', 0), fused, plan.get('table_rows') if plan.get('max_window') else None)
        ms_step = dt_med / args.steps * 1e3
        k_steady = k_med = k_min = 0.0
        n_steady = 0
        red_ms = None
        k_steady_only = None
        if pic['n'] and fused:
            # `kernel_avg_ms` is literally the average launch duration over the timed region: ALL K launches, relinearising ones
            # included (what rocprofv3 --stats averages, minus its share of the untimed first batch); the steady subset beside it
            allk = np.isfinite(pic['sweep'])
            sw = pic['sweep'][allk]
            k_steady, k_med, k_min, n_steady = float(sw.mean()), float(np.median(sw)), float(sw.min()), int(sw.size)
            k_steady_only = mean_ms(pic['sweep'], pic['ok'])
            red_ms = mean_ms(pic['reduce'], allk)
            k_src = ("device clock stamped by workgroup 0 of every kernel of one extra replay of the batch: kernel_avg_ms = sweep start -> "
                     "reduce start, the interval rocprofv3 reports as the kernel's duration (consecutive kernels tile the stream's timeline)")
        elif m['ev_ms'].size:                                    # general sweep: HIP events only
            ev_steady = pic['steady'][pic['ev_idx']] if pic['n'] else np.ones(m['ev_ms'].size, bool)
            ev_all = m['ev_ms'][:ev_steady.size]           # (more timed launches than stamped sweeps: the stamp ring holds 4096)
            ev = ev_all[ev_steady] if ev_steady.any() else ev_all
            k_steady, k_med, k_min, n_steady = float(ev.mean()), float(np.median(ev)), float(ev.min()), int(ev.size)
            k_src = f"HIP events around every {EVENT_EVERY}-th launch, one extra replay of the batch"
        else:
            k_src = "none"
        achieved = lay / (k_steady * 1e-3) / 1e9 if k_steady else 0.0
        traffic, traffic_src = measured_traffic() if (args.full and world == 1 and fused and F == 1_000_000 and not dry) else (None, None)
        lib_hash = None if (dry or not args.full) else library_fingerprint()
        roof = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                "frac_of_copy_ceiling": achieved / COPY_CEILING_GBS, "copy_ceiling": COPY_CEILING_GBS,
                "traffic": traffic, "kernel": m['k_name'], "bytes_per_launch": lay,
                "bytes_model": "engine layout, DESIGN.md section 4: F*(31 doubles + 8 B) + L*29 doubles + camera tables",
                "library_sha256_16": lib_hash,
                "kernel_avg_ms": k_steady, "kernel_median_ms": k_med, "kernel_min_ms": k_min,
                "kernel_launches_timed": n_steady, "kernel_timing": k_src,
                "kernel_steady_ms": k_steady_only, "kernel_steady_launches": int(pic['ok'].sum()) if pic['n'] else 0,
                "survey_equivalent_bytes": survey_bytes(F_local, L_local, C),
                "survey_equivalent_gbs": survey_bytes(F_local, L_local, C) / (k_steady * 1e-3) / 1e9 if k_steady else 0.0}
        if red_ms is not None:
            roof["reduce_kernel"] = "k_cam_reduce_rows" if plan.get('reduce_by_wave') else "k_cam_reduce_tree"
            roof["reduce_avg_ms"] = red_ms
            roof["step_ms_device"] = mean_ms(pic['step'])
            # a kernel cannot take longer than the step that contains it
            roof["consistent"] = bool(k_steady + red_ms <= ms_step * 1.03)
            if not roof["consistent"]:
                print(f"[bench] WARNING: kernel {k_steady:.4f} ms + reduce {red_ms:.4f} ms > step {ms_step:.4f} ms", file=sys.stderr)
        if m['ev_ms'].size and pic['n'] and fused:
            ev_steady = pic['steady'][pic['ev_idx']]
            if ev_steady.any():
                roof["kernel_event_ms"] = float(m['ev_ms'][:ev_steady.size][ev_steady].mean())
                roof["kernel_event_note"] = (f"HIP events around every {EVENT_EVERY}-th launch of the same replay: includes the dispatch latency behind the "
                                             "event's barrier packet, reported as a cross-check only")
        if not traffic and traffic_src:
            roof["traffic_note"] = traffic_src
        if traffic and k_steady:
            roof["traffic_source"] = f"profiles/{traffic_src}: committed rocprofv3 PMC passes of this command on this very binary, NOT measured by this run"
            roof["traffic_gbs"] = traffic / (k_steady * 1e-3) / 1e9
            roof["traffic_frac"] = roof["traffic_gbs"] / HBM_PEAK_GBS
        if pic['n'] and fused and (~pic['steady']).any():
            ns, relin = ~pic['steady'], m['relin']
            full = relin * 2 > F
            roof["relinearising_sweeps"] = {"count": int(ns.sum()), "kernel_avg_ms": mean_ms(pic['sweep'], ns),
                                            "kernel_max_ms": float(np.nanmax(pic['sweep'][ns])),
                                            "factors_per_sweep_mean": float(relin[ns].mean()), "factors_per_sweep_max": int(relin.max()),
                                            "extra_bytes_per_factor": 72}
            if full.any():
                roof["relinearising_sweeps"]["all_factors"] = {"count": int(full.sum()), "kernel_avg_ms": mean_ms(pic['sweep'], full)}
        par = "single GPU"
        if world > 1:
            how = {"rccl": "RCCL all-gather of camera partial sums per sweep", "peer": "peer-store exchange of camera partial sums per sweep (no collective)",
                   "python": "all_gather_into_tensor of camera partial sums per sweep"}.get(exchange_used, str(exchange_used))
            par = f"landmark-sharded x{world}, {how}"
        out = {
            "metric": "GBP iterations/sec (whole node), 1M-factor BA graph" if F == 1_000_000 else f"GBP iterations/sec, {F}-factor BA graph",
            "value": its, "unit": "iter/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_step, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f64", "data": "fixture file (tests/golden/data)" if args.bal else "synthetic",
            "config": {"workload": f"{workload} {C} cams x {L} landmarks x {F} reprojection factors "
                                   + ("" if args.bal else "(gbp_amd.synthetic.make_synthetic seed 0), ") + "ba.py defaults, loss=None",
                       "n_cams": C, "n_lmks": L, "n_factors": F,
                       "parallelism": par, "exchange": exchange_used if (world > 1 or args.sharded) else None,
                       "exchange_requested": args.exchange if (world > 1 or args.sharded) else None,
                       "exchange_fallback": getattr(graph, 'exchange_fallback', None),
                       "sweep": "fused" if fused else "general",
                       "topology": topology,
                       "camera_windows": {"widest": plan['max_window'], "table_rows": plan['table_rows']} if plan.get('max_window') else None,
                       "loop": ("python" if (args.python_loop or dry or not getattr(graph, 'library_loop', True)) else "in-library") if (world > 1 or args.sharded) else "gbp_ba_iterate"},
            "timing": {"protocol": ("state restored before every batch; W warm-up + K timed sweeps between barrier+synchronize; median over batches"
                                    if args.full else "one batch: W warm-up + K timed sweeps between barrier+synchronize"),
                       "batches": int(times.size), "timed_seconds": float(times.sum()),
                       "ms_per_step_median": ms_step, "ms_per_step_min": dt_min / args.steps * 1e3,
                       "ms_per_step_first": float(times[0]) / args.steps * 1e3},
        }
        if args.full:
            out["roofline"] = roof
            out["are_after"] = are
        if per_rank is not None:
            out["per_rank"] = per_rank
        if alt is not None:
            at = alt['times']
            out["other_exchange"] = {"exchange": alt.get('exchange'), "value": args.steps / float(np.median(at)), "ms_per_step": float(np.median(at)) / args.steps * 1e3,
                                     "batches": int(at.size), "camera_beliefs_match": alt.get('matches_rccl', alt.get('matches'))}
        if dry:
            out["dry_run"] = True
        if args.full and world == 1 and not args.no_cpu_baseline and not dry:
            out["cpu_baseline"] = cpu_baseline(problem, engine=graph)
            if args.bal and F <= 50_000:
                out["cpu_baseline_numpy"] = cpu_baseline_numpy(problem)
        if pc is not None:
            out["parity_check"] = pc
        if hbm is not None:
            roof["frac_hbm_bound"] = hbm["frac"]                 # the HONEST fraction of the HBM peak (median of five replays): `frac` above is cache-assisted
            roof["frac_hbm_bound_range"] = hbm["frac_range"]     # (the 1M graph's working set sits in the 256 MiB memory-side cache); min / max of the replays
            roof["frac_hbm_bound_mode"] = hbm["mode"]
            roof["frac_hbm_bound_of_copy_ceiling"] = hbm["frac_of_copy_ceiling"]
            roof["hbm_bound_size"] = hbm
        return out

    m = measure(graph)
    exchange_used = getattr(graph, 'exchange', None)
    # outside the timed region: the first ten sweeps once more, against the reference's own run of this graph (fixture G9b)
    pc = None if (dry or not args.full) else parity_check(graph, problem, dist, torch, side_dev, world, local_rank,
                                                          default_graph=args.window is None and not args.bal)
    per_rank = gather_per_rank(m)
    alt = None
    peer_unavailable = None
    if world > 1 and not dry and args.exchange == 'auto' and exchange_used == 'rccl':
        # The same job with the peer-store exchange (no collective call: reduce kernels store into the ranks' mailboxes over xGMI).
        # The RCCL result is complete at this point: should the newer path hang beyond its own time-outs, a watchdog prints that
        # line and ends the process -- the measurement cannot be lost to the comparison.
        import threading
        fallback = assemble(m, None, exchange_used, per_rank, pc) if rank == 0 else None

        def on_timeout():                                      # a THREAD: the main one may be stuck inside a native call
            if rank == 0:
                fallback["other_exchange"] = {"exchange": "peer", "error": "timed out (watchdog): the RCCL result stands"}
                os.write(json_fd, (json.dumps(fallback) + '\n').encode())
            os._exit(0)
        watchdog = threading.Timer(float(os.environ.get('GBP_BENCH_PEER_WATCHDOG_S', '240')), on_timeout)
        watchdog.daemon = True
        watchdog.start()
        alt = try_peer_exchange(args, problem, local_rank, dist, torch, measure, graph, side_dev, gather_per_rank)
        watchdog.cancel()
        if alt is not None and float(np.median(alt['times'])) < float(np.median(m['times'])) and alt.get('matches_rccl'):
            m, alt = alt, dict(m, exchange='rccl')
            exchange_used = 'peer'
            per_rank = m.pop('per_rank', per_rank)
        elif alt is not None:
            alt.pop('per_rank', None)
            alt = dict(alt, exchange='peer')
        else:
            peer_unavailable = PEER_NOTE.get('reason') or ("the peer-store exchange failed on another rank (its stderr has the reason); "
                                                           "the RCCL result stands")
    if args.dump_sweeps and rank == 0:
        np.savez(args.dump_sweeps, clk_us=m['clk'], event_ms=m['ev_ms'], relin=m['relin'], batch_s=m['times'])
    if args.dump_outputs and rank == 0:
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, a in m['outputs'].items():
            np.save(os.path.join(args.dump_outputs, name + '.npy'), a)

    # ---- N > 1: a stated model to judge the measurement against, and a workload that is NOT latency-bound ---------------------------
    # Both run after the headline measurement is complete, under a watchdog that prints that measurement should they hang.
    extras = {}
    if args.full and world > 1 and not dry:
        import threading
        base = assemble(m, alt, exchange_used, per_rank, pc) if rank == 0 else None
        if base is not None and peer_unavailable:
            base["other_exchange"] = {"exchange": "peer", "error": peer_unavailable}

        def extras_timeout():
            if rank == 0:
                base["extras_error"] = "prediction / secondary workload timed out (watchdog): the headline measurement above stands"
                os.write(json_fd, (json.dumps(base) + '\n').encode())
            os._exit(0)
        wd = threading.Timer(float(os.environ.get('GBP_BENCH_EXTRAS_WATCHDOG_S', '420')), extras_timeout)
        wd.daemon = True
        wd.start()

        def all_max(x):
            t = torch.tensor([float(x)], dtype=torch.float64, device=side_dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            return float(t.item())

        # (b) DESIGN.md section 6's model, from THIS binary on THESE devices: every rank runs its own shard alone through the sharded
        # loop with a one-rank peer-store exchange (reduce -> its own mailbox -> finish polling its own tags) -- everything a rank does per
        # sweep except waiting for the others -- on the timed batch schedule.  The slowest rank's solo step is the step the job would
        # have if links and skew cost nothing; measured minus predicted = what the exchange between devices really costs.
        solo_ms, solo_err = -1.0, None
        try:
            from gbp_amd.engine import BAEngine
            from gbp_amd.sharded import local_problem
            lo_l, hi_l = graph.lmk_range
            e1 = BAEngine.from_problem(local_problem(problem, lo_l, hi_l), device=local_rank, fused=False if args.no_fused else None)
            try:
                e1.peer_connect(0, [e1.peer_export(1)])
                e1.generate_priors_var(50.0); e1.update_beliefs_sharded(); e1.sync(); e1.snapshot_state()
                ts, t_end = [], time.perf_counter() + 1.0
                while len(ts) < 3 or (time.perf_counter() < t_end and len(ts) < 400):
                    e1.restore_snapshot(); e1.iterate_sharded(args.warmup); e1.sync()
                    t0 = time.perf_counter(); e1.iterate_sharded(args.steps); e1.sync()
                    ts.append((time.perf_counter() - t0) / max(args.steps, 1))
                solo_ms = float(np.median(ts)) * 1e3
            finally:
                e1.close()
        except Exception as e:                                   # noqa: BLE001
            solo_err = str(e)
            print(f"[bench] rank {rank}: solo-shard probe failed: {e}", file=sys.stderr)
        worst = all_max(solo_ms if solo_err is None else float('inf'))
        solo_all = [None] * world
        dist.all_gather_object(solo_all, solo_ms if solo_err is None else None)
        if np.isfinite(worst):
            measured = float(np.median(m['times'])) / args.steps * 1e3
            extras["prediction"] = {
                "predicted_step_ms": worst, "measured_step_ms": measured, "exchange_and_skew_ms": measured - worst,
                "solo_step_ms_per_rank": solo_all,
                "model": "slowest rank's own shard alone on its own device through the same sharded loop with a one-rank peer-store exchange "
                         "(DESIGN.md section 6, tools/shard_probe.py `peer1`), same batch schedule: the step of a job whose links and rank skew "
                         "cost nothing; one GPU's step / predicted_step_ms bounds the speed-up this problem size can show"}
        else:
            extras["prediction"] = {"error": solo_err or "the solo-shard probe failed on another rank"}

        # (c) SECONDARY workload, clearly not the headline: the same graph family with --secondary-lmks landmarks (8M factors by default:
        # 1M per rank at N = 8, the size at which one GPU's sweep is bandwidth-bound), every rank generating its own landmarks against
        # the shared cameras (make_synthetic(lmk_seed=rank), ShardedBA(local_shard=True)).  The 1M-factor headline graph is latency-bound
        # from four ranks on by the design's own numbers; this line shows what the sharded sweep does when it is not.
        if args.secondary_lmks > 0 and not args.bal and args.window is None and exchange_used in ('rccl', 'peer'):
            sec, sec_err = None, None
            try:
                from gbp_amd.synthetic import make_synthetic
                from gbp_amd.sharded import ShardedBA
                per = args.secondary_lmks // world
                mine = make_synthetic(n_cams=args.cams, n_lmks=per, obs_per_lmk=args.obs, seed=0, lmk_seed=1 + rank)
            except Exception as e:                               # noqa: BLE001
                sec_err, mine = str(e), None
            if all_max(0.0 if sec_err is None else 1.0) < 0.5:
                g2 = ShardedBA(mine, device=local_rank, fused=False if args.no_fused else None, local_shard=True, exchange=exchange_used)
                try:
                    m2 = measure(g2, min_timed_s=MIN_TIMED_S / 2, dump=False)
                    pr2 = gather_per_rank(m2, g2)
                    t2 = float(np.median(m2['times']))
                    sec = {"label": "SECONDARY (bandwidth-bound companion; not the BASELINE metric)",
                           "workload": f"synthetic BAL {C} cams x {g2.L_total} landmarks x {g2.F_total} reprojection factors, "
                                       f"{g2.F_total // world} per rank, every rank's landmarks generated on the rank (lmk_seed = 1 + rank)",
                           "n_factors": int(g2.F_total), "value": args.steps / t2, "unit": "iter/s", "ms_per_step": t2 / args.steps * 1e3,
                           "exchange": g2.exchange, "scaling_note": "weak within this entry: per-rank work is fixed as N grows",
                           "per_rank": pr2}
                finally:
                    g2.close()
            extras["secondary"] = sec if sec is not None else {"error": sec_err or "generation failed on another rank"}
        wd.cancel()

    hbm = None
    if args.full and world == 1 and not dry and not args.bal and not args.no_fused and not args.single_batch and not args.no_hbm_size and F == 1_000_000:
        try:
            hbm = hbm_bound_size()
        except Exception as e:                                   # noqa: BLE001
            print(f"[bench] HBM-bound size run failed: {e}", file=sys.stderr)
    if rank == 0:
        out = assemble(m, alt, exchange_used, per_rank, pc, hbm)
        if peer_unavailable:
            out["other_exchange"] = {"exchange": "peer", "error": peer_unavailable}
        if "prediction" in extras:
            out["predicted_step_ms"] = extras["prediction"].get("predicted_step_ms")
        out.update(extras)
        os.write(json_fd, (json.dumps(out) + '\n').encode())
    if dist is not None:
        dist.barrier()
        if hasattr(graph, 'close'):
            graph.close()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
