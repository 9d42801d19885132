"""Small, deterministic BA problems at the numerical edges of the sweep (test helper: tests/test_ba_conditioning_*.py).

Every problem has 4-8 cameras and at most 64 factors.  A camera is built from its axis-angle w and sits so that the world origin lies
at depth `depth` on its optical axis (t = (jx, jy, depth)): any rotation, near pi or near zero included, sees the landmark cloud around
the origin.  Initial estimates are the truth perturbed (cameras 1 %, landmarks 2 % of the scene size); measurements are the exact
projection plus `pix` px of Gaussian noise.  Each regime is (name, note, problem, engine keyword arguments, prior weakening factor,
float_impl) -- float_impl: the comparison runs through replay_ba's --float_implementation prior weakening.
"""
import dataclasses

import numpy as np

from gbp_amd.synthetic import BAProblem, FR1DESK_K, rodrigues


@dataclasses.dataclass
class Regime:
    name: str
    note: str
    problem: BAProblem
    kw: dict = dataclasses.field(default_factory=dict)      # BAEngine / HostBA keyword arguments (gauss_noise_std, loss, Nstds)
    wf: float = 50.0                                          # generate_priors_var(weaker_factor)
    float_impl: bool = False


def _project(K, w, t, y):
    p = (rodrigues(w[None])[0] @ y) + t
    return np.array([K[0] * p[0] / p[2] + K[2], K[1] * p[1] / p[2] + K[3]]), p[2]


def scene(seed, *, n_cams=6, n_lmks=16, degree=4, depth=5.0, ball=1.0, ws=None, pix=1.0, offset=0.0, near=None, outliers=(), seen=None):
    """A camera-major BAProblem.  degree: an int or one per landmark.  ws: the cameras' axis-angles (default: random axes, angles in
    [0.3, 2.5]).  offset: the whole scene translated by offset * ball along (1, -2, 3) / |.|.  near = (camera, z): landmark 0 is put at
    depth z in front of that camera.  outliers: (factor, sigmas) pairs -- that measurement moved by sigmas * pix px.  seen: the cameras of every landmark
    (default: `degree` random ones)."""
    rng = np.random.default_rng(seed)
    K = np.array(FR1DESK_K)
    if ws is None:
        ax = rng.normal(size=(n_cams, 3))
        ws = ax / np.linalg.norm(ax, axis=1, keepdims=True) * rng.uniform(0.3, 2.5, size=(n_cams, 1))
    ws = np.asarray(ws, dtype=np.float64)
    ts = np.concatenate([rng.uniform(-0.05, 0.05, size=(n_cams, 2)) * depth, np.full((n_cams, 1), depth)], axis=1)
    v = rng.normal(size=(n_lmks, 3))
    lmk = v / np.linalg.norm(v, axis=1, keepdims=True) * ball * rng.uniform(0.2, 1.0, size=(n_lmks, 1))
    if near is not None:
        c, zc = near
        lmk[0] = rodrigues(ws[c][None])[0].T @ (np.array([0.0, 0.0, zc]) - ts[c])
    deg = np.broadcast_to(np.asarray(degree), (n_lmks,))
    given, seen = seen, []
    for l in range(n_lmks):
        if given is not None:
            seen.append(np.asarray(given[l]))
            continue
        cams = rng.choice(n_cams, size=int(deg[l]), replace=False)
        if near is not None and l == 0 and near[0] not in cams:
            cams[0] = near[0]
        seen.append(cams)
    # translate the world: y -> y + T, t -> t - R T (a camera's view of the scene is unchanged)
    T = offset * ball * np.array([1.0, -2.0, 3.0]) / np.sqrt(14.0)
    R = rodrigues(ws)
    lmk_w = lmk + T
    ts_w = ts - np.einsum('cij,j->ci', R, T)
    rows = []
    for c in range(n_cams):
        for l in range(n_lmks):
            if c in seen[l]:
                uv, zc = _project(K, ws[c], ts[c], lmk[l])
                assert zc > 0
                rows.append((c, l, uv + rng.normal(scale=pix, size=2)))
    meas = np.array([r[2] for r in rows])
    for f, sig in outliers:
        meas[f] += sig * pix * np.array([0.6, 0.8])
    cam_means = np.concatenate([ts_w + rng.normal(scale=0.01 * ball, size=ts_w.shape),
                                ws + rng.normal(scale=0.002, size=ws.shape)], axis=1)
    lmk_means = lmk_w + rng.normal(scale=0.02 * ball, size=lmk_w.shape)
    if near is not None:
        lmk_means[0] = lmk_w[0] + rng.normal(scale=0.02 * near[1], size=3)
    return BAProblem(K=K, cam_means=cam_means, lmk_means=lmk_means, meas=meas, cam_idx=np.array([r[0] for r in rows], np.int32),
                     lmk_idx=np.array([r[1] for r in rows], np.int32))


# four landmarks of degree 1, six of degree 2; cameras 0-4 see three landmarks, camera 5 two
MINIMAL = [[0], [1], [2, 3], [3, 4], [4, 5], [5, 0], [1, 2], [0, 3], [2], [4, 1]]


def _axis(rng, n, angle):
    a = rng.normal(size=(n, 3))
    return a / np.linalg.norm(a, axis=1, keepdims=True) * np.asarray(angle, dtype=np.float64).reshape(-1, 1)


def regimes():
    rng = np.random.default_rng(2026)
    out = [
        Regime('baseline', 'control: 6 cameras, 16 landmarks of degree 4 at depth 5', scene(1)),
        Regime('weak_prior_1e2', 'priors 1e2 weaker than the factors (std)', scene(2), wf=1e2),
        Regime('weak_prior_1e4', 'priors 1e4 weaker: Lambda_prior / Lambda_f = 1e-8', scene(3), wf=1e4),
        Regime('weak_prior_1e6', 'priors 1e6 weaker: Lambda_prior / Lambda_f = 1e-12', scene(4), wf=1e6),
        Regime('float_impl', "ba.py --float_implementation: priors weakened 100x more over the burn-in", scene(5), float_impl=True),
        Regime('minimal_views', 'landmarks of degree 1 and 2; cameras see 2-3 landmarks', scene(6, n_lmks=10, seen=MINIMAL)),
        Regime('dominant_message', 'minimal views with priors 1e6 weaker: a degree-1 landmark\'s belief is its one message (W G ~ I)',
               scene(6, n_lmks=10, seen=MINIMAL), wf=1e6),
        Regime('low_parallax_1e2', 'landmarks at 1e2 x the cameras\' spread (depth 500)', scene(7, depth=500.0)),
        Regime('low_parallax_1e4', 'landmarks at 1e4 x the cameras\' spread (depth 5e4)', scene(8, depth=5e4)),
        Regime('far_1e3', 'whole scene translated by 1e3 x its size', scene(9, offset=1e3)),
        Regime('far_1e6', 'whole scene translated by 1e6 x its size', scene(10, offset=1e6)),
        Regime('noise_1e-3', 'gauss_noise_std = 1e-3 px (measurement noise likewise)', scene(11, pix=1e-3), kw=dict(gauss_noise_std=1e-3)),
        Regime('noise_1e3', 'gauss_noise_std = 1e3 px (the measurements keep 1 px noise)', scene(12), kw=dict(gauss_noise_std=1e3)),
        Regime('huber_outliers', 'huber, Nstds 3, outliers at 1e2 .. 1e4 sigma', scene(13, outliers=[(3, 1e2), (17, 1e3), (40, 1e4)]),
               kw=dict(loss='huber', Nstds=3.0)),
        Regime('constant_outliers', 'constant loss, Nstds 3, outliers at 1e2 .. 1e4 sigma', scene(14, outliers=[(5, 1e2), (22, 1e3), (51, 1e4)]),
               kw=dict(loss='constant', Nstds=3.0)),
        Regime('rot_near_pi', '|w| within 1e-6 of pi', scene(15, ws=_axis(rng, 6, np.pi - rng.uniform(1e-8, 1e-6, 6)))),
        Regime('rot_tiny', '|w| below 1e-6', scene(16, ws=_axis(rng, 6, rng.uniform(1e-8, 1e-6, 6)))),
        Regime('rot_above_2pi', '|w| above 2 pi (same rotations as |w| - 2 pi)', scene(17, ws=_axis(rng, 6, rng.uniform(2 * np.pi + 0.3, 2 * np.pi + 2.5, 6)))),
        Regime('near_plane', 'a landmark at depth 1e-3 in front of camera 0', scene(18, near=(0, 1e-3))),
    ]
    for r in out:
        p = r.problem
        assert 4 <= p.n_cams <= 8 and p.n_factors <= 64, r.name
        assert np.all(np.diff(p.cam_idx) >= 0)
    return out


# ---- one-step comparisons (tests/test_ba_conditioning_host.py and _gpu.py) ------------------------------------------------------------
# err(device, exact) <= min(C * err(yardstick, exact), CAP) + FLOOR, per quantity (rel_err_rows: max over rows of the relative Frobenius error)
C_RATIO = 8.0          # the device may lose 3 bits more than the reference's own dense float64 maths does from the same state: the
                       # covariance form reorders every sum, and a 2x2 Woodbury solve replaces the 6x6 / 3x3 inverses
FLOOR = 64 * np.finfo(float).eps     # where the yardstick is (nearly) exact -- one rounding of a short sum -- a few ulps of any row
CAP = 2e-8                           # a ceiling of its own against the exact sweep, for every regime: where the yardstick loses its digits
                                     # (weak priors: 1e-6 .. 1e6 relative) C x yardstick bounds nothing.  Worst unmodified sweep: 2.5e-9 on
                                     # the host core, 7.0e-9 on the MI355X (far_1e6, dense remainder, the yardstick as far off); J mu rounded
                                     # through float lands at 1.3e-7 .. 4.9e-7 in the weak-prior regimes.
MAHA_YARD, MAHA_DEV = 1e-8, 1e-6     # where the yardstick's mean is within 1e-8 sigma of the exact one, the device's must be within 1e-6 sigma
KINDS = ('damped', 'relin', 'xtra')  # the comparison sweep: ordinary damped / every factor relinearising / damped in that sweep (general only)
BURN = 8


def kind_kw(kind):
    """Graph parameters of a comparison kind: beta = 0 so that set_iters_since_relin(min_linear_iters) relinearises every factor;
    num_undamped_iters = 0 makes a factor damped in the sweep it relinearises in (the dense-remainder path)."""
    return dict(beta=0.0, num_undamped_iters=0 if kind == 'xtra' else 6, min_linear_iters=8)


def prepare(g, regime, kind, burn=BURN):
    """Priors, burn-in through replay_ba's schedule, then what the comparison sweep needs."""
    from oracle.oracle import replay_ba
    g.generate_priors_var(regime.wf)
    g.update_all_beliefs()
    replay_ba(g, burn, float_impl=regime.float_impl)
    if kind != 'damped':
        g.set_iters_since_relin(8)


QUANTITIES = ('cam_eta', 'cam_lam', 'lmk_eta', 'lmk_lam', 'msg_cam_eta', 'msg_cam_lam', 'msg_lmk_eta', 'msg_lmk_lam')


def one_step(state, nxt, regime, kind, rel_err_rows):
    """Exact and yardstick sweeps from `state` (taking the device's decisions: nxt['relin'], nxt['robust_flag']) against the device's
    next state `nxt` (the QUANTITIES + cam_mu / lmk_mu).  Returns {quantity: (err device, err yardstick)} and the Mahalanobis pair."""
    from oracle import exact_ba
    kw = dict(regime.kw)
    par = dict(sigma2=kw.get('gauss_noise_std', 2.0) ** 2, loss=kw.get('loss'), nstds=kw.get('Nstds', 3.0), **kind_kw(kind),
               relin=nxt['relin'], robust=nxt['robust_flag'])
    ex = exact_ba.sweep(state, dps=40, **par)
    yd = exact_ba.sweep(state, **par)
    assert np.array_equal(yd['relin'], nxt['relin'])
    errs = {q: (rel_err_rows(nxt[q], ex[q]), rel_err_rows(yd[q], ex[q])) for q in QUANTITIES}
    maha = {}
    for v in ('cam', 'lmk'):
        maha[v] = (exact_ba.mahalanobis(nxt[f'{v}_mu'], ex[f'{v}_mu'], ex[f'{v}_lam']),
                   exact_ba.mahalanobis(yd[f'{v}_mu'], ex[f'{v}_mu'], ex[f'{v}_lam']))
    return errs, maha


def check(errs, maha):
    """The criterion; returns the list of failures (empty: pass)."""
    bad = [f'{q}: device {d:.3g} > min({C_RATIO:g} x yardstick {y:.3g}, {CAP:g}) + floor' for q, (d, y) in errs.items()
           if not d <= min(C_RATIO * y, CAP) + FLOOR]
    bad += [f'{v} mean: device {d:.3g} sigma while the yardstick is at {y:.3g}' for v, (d, y) in maha.items() if y < MAHA_YARD and not d < MAHA_DEV]
    return bad


def worst(errs):
    """The largest device error against the exact sweep over the quantities."""
    return max(d for d, _ in errs.values())


def ratio(errs):
    """The worst device / yardstick ratio over the quantities (the floor added to both)."""
    return max((d + FLOOR) / (y + FLOOR) for d, y in errs.values())
